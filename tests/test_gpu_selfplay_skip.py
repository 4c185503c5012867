"""fs_step_skip_selfplay / k_step_skip_selfplay (FusedSelfPlayRollout.rollout_skipped,
PPOTrainer(self_play="decisions")): n agent decisions per arena in one launch, P1's actor asked once
per decision, P2's actor on every tick, the skipped ones included.

Bar 1, the simulation: P1's sampled index on a decision's first tick and 0 afterwards, P2's game input
of every tick (its index with Left and Right exchanged when mirrored), replayed through the CPU oracle's
masked steps, give each decision's last row, its float64 reward sum and the final state bit for bit;
the tick counts are checked against wrappers.is_skippable on the oracle's own observations.  Bar 2, the
actors: both match the host restatement (tests/policy_ref.py) at test_gpu_policy's unchanged bars
(MARGIN, LOGP_TOL), P1 per decision on the row before it, P2 per tick on the oracle's observation
before that tick, each with its documented counter.  Then the identities: max_ticks = 1 is
fs_step_n_selfplay, calls split anywhere, an arena's results do not depend on its wave."""
import ctypes as C
import functools

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd import wrappers as W
from footsies_gym_amd.rollout import swap_left_right
from tests import policy_ref
from tests.parity_utils import FINAL_KEYS, OBS_KEYS, assert_same, compare_outputs, compare_states, random_states
from tests.test_gpu_policy import LOGP_TOL, MARGIN  # the bars, unchanged
from tests.test_gpu_selfplay import mirrored

pytestmark = pytest.mark.gpu

CAP = _abi.FS_SKIP_DEFAULT_MAX_TICKS
# make_actor seeds of a pair that fights: the host restatement of both actors over the oracle ends about one
# round per arena in 32 decisions (3.9 ticks per decision), so 33 arenas meet terminal decisions too --
# test_gpu_selfplay's pair (9, 10) ends 24 rounds in 1057 arenas x 32 decisions
P1_ACTOR, P2_ACTOR = 13, 14
P1_SEED, P2_SEED, SIM_SEED = 0xC0FFEE, 0xBEEF, 21
AUTORESET = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}
FLOAT = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
PAIRS = ("guard", "move", "move_frame", "position")
SAMPLES = ("A1", "LP1", "ticks", "capped", "A2", "LP2")


def make(n, autoreset="same_step", float_mode="strict", dense=True, same=False, mirror=True, **kw):
    import torch
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    dev = torch.device("cuda", 0)
    sim = FootsiesSim(n, p2_mode="external", autoreset_mode=autoreset, float_mode=float_mode, dense_reward=dense,
                      seed=SIM_SEED, **kw)
    ro = FusedSelfPlayRollout(sim, make_actor(device=dev, seed=P1_ACTOR),
                              opponent=None if same else make_actor(device=dev, seed=P2_ACTOR), seed=P1_SEED,
                              opponent_seed=P1_SEED if same else P2_SEED, mirror=mirror)
    return sim, ro


def run(sim, ro, n, max_ticks=CAP):
    """One call: the trajectory by decision, P1's samples, ticks, capped, and P2's [n][max_ticks][N]
    samples pre-filled with 0xFF bytes (what no tick wrote stays)."""
    import torch
    traj = sim.alloc_trajectory(n)
    N, dev = sim.num_envs, sim.device
    a2 = torch.full((n, max_ticks, N), 0xFF, dtype=torch.uint8, device=dev)
    lp2 = torch.full((n, max_ticks, N), -1, dtype=torch.int32, device=dev).view(torch.float32)  # 0xFF bytes
    a1, lp1, ticks = ro.rollout_skipped(n, trajectory=traj, max_ticks=max_ticks, p2_actions=a2, p2_logp=lp2)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in traj.items()}
    res.update(A1=a1.cpu().numpy(), LP1=lp1.cpu().numpy(), ticks=ticks.cpu().numpy(),
               capped=ro.last_capped.cpu().numpy(), A2=a2.cpu().numpy(), LP2=lp2.cpu().numpy())
    return res


def row(res, d):
    return {k: res[k][d] for k in _abi.OUTPUT_SPEC}


def replay(ora, res, mirror, same_step, max_ticks, d0=0, before=None, obs_log=None):
    """Bar 1 for one call.  `ora` stands where the call began.  Returns flags of what the run met:
    (some decision ran more than one tick, some decision was terminal, some was capped).  `before`:
    the four observation pairs as they stand, kept up to date per arena with the oracle's ticks;
    `obs_log` (a list) receives (d, j, active, a copy of them before tick j) for bar 2."""
    n, N = res["A1"].shape
    ticks = res["ticks"].astype(np.int64)
    assert ticks.min() >= 1 and ticks.max() <= max_ticks
    # P2's arrays: written exactly where a tick ran
    ran = np.arange(max_ticks)[None, :, None] < ticks[:, None, :]
    assert (res["A2"][ran] < 8).all() and (res["A2"][~ran] == 0xFF).all()
    assert np.isfinite(res["LP2"][ran]).all()
    assert (res["LP2"][~ran].view(np.uint32) == 0xFFFFFFFF).all()
    for d in range(n):
        acc = np.zeros(N, np.float64)
        for j in range(int(ticks[d].max())):
            active = ticks[d] > j
            if obs_log is not None:
                obs_log.append((d0 + d, j, active.copy(), {k: before[k].copy() for k in PAIRS}))
            p1_in = res["A1"][d] if j == 0 else np.zeros(N, np.uint8)
            a2 = np.where(active, res["A2"][d, j], 0).astype(np.uint8)
            p2_in = swap_left_right(a2) if mirror else a2
            out = ora.step(p1_in, p2_in, active=active.astype(np.uint8))
            acc[active] += out["reward"][active]  # in tick order from 0.0
            over = out["terminated"].astype(bool) | out["truncated"].astype(bool)
            more = W.is_skippable(out) & ~over
            last = active & (ticks[d] == j + 1)
            inner = active & ~last
            assert more[inner].all(), (d0 + d, j, "a decision went on past a tick that was not skippable")
            closed = last & ~more
            capped = last & more
            assert (res["capped"][d][closed] == 0).all(), (d0 + d, j)
            assert (res["capped"][d][capped] == 1).all() and (ticks[d][capped] == max_ticks).all(), (d0 + d, j)
            if last.any():
                keys = OBS_KEYS + (FINAL_KEYS if same_step else ())
                exp = {k: np.asarray(out[k])[last] for k in keys}
                exp["reward"] = acc[last]
                compare_outputs(exp, {k: res[k][d][last] for k in keys}, step=d0 + d, same_step=same_step)
            if before is not None:
                for k in PAIRS:
                    before[k][active] = np.asarray(out[k])[active]
    return (ticks > 1).any(), res["terminated"].astype(bool).any(), res["capped"].any()


def check_draws(params, seed, feats, arena, counter, acts, logps):
    """test_gpu_policy's _check_policy over arbitrary (arena, counter) draws: feats [M][8], the rest [M]."""
    lg = policy_ref.logits(params, feats)
    u = policy_ref.policy_uniform(seed, arena, np.asarray(counter, dtype=np.uint64))
    act, logp, margin = policy_ref.sample(lg, u)
    ok = margin > MARGIN
    same = act == acts
    err = np.abs(logp[same] - logps[same])
    assert err.size and err.max() < LOGP_TOL, (err.max(), err.mean())
    assert ok.sum() > 0.9 * len(acts), ok.sum()  # 7 boundaries x 2 x MARGIN ~ 7% fall inside
    assert (act[ok] == acts[ok]).all(), "%d of %d actions differ away from CDF boundaries" % (
        (act[ok] != acts[ok]).sum(), ok.sum())
    return float(err.mean()), float(err.max())


CALLS = (24, 8)
CASES = {
    "33-same_step-strict": dict(n=33, autoreset="same_step", float_mode="strict"),
    "33-next_step-strict": dict(n=33, autoreset="next_step", float_mode="strict"),
    "1057-same_step-strict": dict(n=1057, autoreset="same_step", float_mode="strict"),
    "1057-next_step-double": dict(n=1057, autoreset="next_step", float_mode="double"),
    "1057-next_step-strict-sparse": dict(n=1057, autoreset="next_step", float_mode="strict", dense=False),
    "1057-same_step-strict-cap3": dict(n=1057, autoreset="same_step", float_mode="strict", max_ticks=3),
}


@functools.lru_cache(maxsize=None)
def played(oracle_lib, name):
    """Two consecutive mirrored calls replayed through the oracle, once per case and shared by the
    bars: (actors' parameters, per-call results, outputs before the first decision, the oracle's
    observation log, flags met, both final states, steps_taken after each call)."""
    cfg = dict(CASES[name])
    n, max_ticks = cfg.pop("n"), cfg.pop("max_ticks", CAP)
    sim, ro = make(n, **cfg)
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, autoreset_mode=AUTORESET[cfg["autoreset"]],
                            float_mode=FLOAT[cfg["float_mode"]], dense_reward=cfg.get("dense", True), base_seed=SIM_SEED)
    prev0 = sim.outputs_numpy()
    before = {k: np.array(prev0[k]) for k in PAIRS}
    runs, steps, log, met, d0 = [], [], [], np.zeros(3, bool), 0
    for m in CALLS:
        runs.append(run(sim, ro, m, max_ticks))
        met |= np.array(replay(ora, runs[-1], True, cfg["autoreset"] == "same_step", max_ticks, d0, before, log))
        d0 += m
        steps.append(sim.steps_taken)
    params = ([p.cpu().numpy() for p in ro.params], [p.cpu().numpy() for p in ro.params2])
    out = (params, runs, prev0, log, met, ora.state(), sim.get_state(), steps)
    ora.close()
    sim.close()
    return out


# -- 1. / 4. the simulation, exact (the replay itself runs inside played()) --------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_decisions_replay_through_the_oracle(oracle_lib, name):
    _, runs, _, _, met, exp_state, got_state, steps = played(oracle_lib, name)
    assert steps == [CALLS[0], sum(CALLS)]  # fs_steps_taken counts decisions
    compare_states(exp_state, got_state)
    ticks = np.concatenate([r["ticks"] for r in runs])
    term = np.concatenate([r["terminated"] for r in runs]).astype(bool)
    rew = np.concatenate([r["reward"] for r in runs])
    # the run reached the ground the kernel is about (else: a longer call, never a looser condition)
    assert met[0], "no decision ran more than one tick"
    assert met[1], "no terminal decision"
    if "next_step" in name:  # the decision after a terminal one is the reset burst alone
        after = term[:-1]
        assert after.any(), "no pending-burst decision"
        assert (ticks[1:][after] == 1).all() and (rew[1:][after] == 0.0).all()
    if "cap3" in name:
        capped = np.concatenate([r["capped"] for r in runs])
        assert capped.any() and (capped == 0).any() and ticks.max() == 3 and (ticks[capped == 1] == 3).all()
    else:
        assert not met[2] and ticks.max() < CAP


# -- 2. both actors against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["33-same_step-strict", "1057-same_step-strict", "1057-next_step-double"])
def test_both_actors_match_the_restatement(oracle_lib, name):
    (par1, par2), runs, prev0, log, _, _, _, _ = played(oracle_lib, name)
    n = CASES[name]["n"]
    A1 = np.concatenate([r["A1"] for r in runs])
    LP1 = np.concatenate([r["LP1"] for r in runs])
    allrows = [row(r, d) for r in runs for d in range(len(r["A1"]))]
    D = len(A1)
    # P1: decision d's draw on the row before it, counter d (fs_steps_taken started at 0)
    prev = [prev0] + allrows[:-1]
    f1 = np.concatenate([policy_ref.features(p) for p in prev])
    m1 = check_draws(par1, P1_SEED, f1, np.tile(np.arange(n), D), np.repeat(np.arange(D), n), A1.reshape(-1),
                     LP1.reshape(-1))
    # P2: tick j of decision d on the oracle's observation before that tick, mirrored, counter d + (j << 40)
    A2 = np.concatenate([r["A2"] for r in runs])
    LP2 = np.concatenate([r["LP2"] for r in runs])
    f2, ar, ctr, a2, lp2 = [], [], [], [], []
    for d, j, active, before in log:
        f2.append(policy_ref.features(mirrored(before))[active])
        ar.append(np.arange(n)[active])
        ctr.append(np.full(int(active.sum()), d + (j << 40), dtype=np.uint64))
        a2.append(A2[d, j][active])
        lp2.append(LP2[d, j][active])
    assert any(j > 0 for _, j, _, _ in log)  # draws on skipped ticks are part of what is checked
    m2 = check_draws(par2, P2_SEED, np.concatenate(f2), np.concatenate(ar), np.concatenate(ctr), np.concatenate(a2),
                     np.concatenate(lp2))
    print("N=%d: |d logp| vs the restatement P1 mean %.2e max %.3e, P2 mean %.2e max %.3e" % ((n,) + m1 + m2))
    if n == 1057:
        assert len(np.unique(A1)) == 8 and len(np.unique(np.concatenate(a2))) == 8


# -- 3. max_ticks = 1 is the per-tick kernel ------------------------------------------------------------------
@pytest.mark.parametrize("n,autoreset", [(33, "same_step"), (1057, "next_step")])
def test_max_ticks_1_equals_the_per_tick_kernel_bitwise(n, autoreset):
    import torch
    T = 40
    sim, ro = make(n, autoreset)
    traj = sim.alloc_trajectory(T)
    a1, lp1, a2, lp2 = ro.rollout(T, trajectory=traj)
    torch.cuda.synchronize()
    per_tick = {k: v.cpu().numpy() for k, v in traj.items()}
    sim2, ro2 = make(n, autoreset)
    res = run(sim2, ro2, T, max_ticks=1)
    for k in per_tick:
        assert_same(k, per_tick[k], res[k])
    assert_same("A1", a1.cpu().numpy(), res["A1"])
    assert_same("LP1", lp1.cpu().numpy(), res["LP1"])
    assert_same("A2", a2.cpu().numpy(), res["A2"][:, 0])
    assert_same("LP2", lp2.cpu().numpy(), res["LP2"][:, 0])
    compare_states(sim.get_state(), sim2.get_state())
    assert sim.steps_taken == sim2.steps_taken == T
    assert (res["ticks"] == 1).all()
    over = res["terminated"].astype(bool) | res["truncated"].astype(bool)
    exp = np.stack([W.is_skippable(row(res, d)) for d in range(T)]) & ~over
    assert_same("capped", exp.astype(np.uint8), res["capped"])
    assert exp.any() and not exp.all()


# -- 5. splits -----------------------------------------------------------------------------------------------
def test_split_calls_and_split_launches_give_one_call(monkeypatch):
    n, total = 33, 24
    sim, ro = make(n)
    whole = run(sim, ro, total, max_ticks=40)
    state = sim.get_state()
    sim.close()
    for parts, rows in (((16, 8), None), ((total,), 5 * n)):  # two calls | launches of 5 + 5 + 5 + 5 + 4 decisions
        if rows:
            monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(rows))
        sim, ro = make(n)
        got = [run(sim, ro, m, max_ticks=40) for m in parts]
        monkeypatch.delenv("FOOTSIES_MAX_LAUNCH_ROWS", raising=False)
        for k in tuple(_abi.OUTPUT_SPEC) + SAMPLES:
            assert_same(k, whole[k], np.concatenate([g[k] for g in got]), extra=str(parts))
        assert sim.steps_taken == total
        compare_states(state, sim.get_state())
        sim.close()
    assert whole["ticks"].max() > 1


# -- 6. wave independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [64, 45])
def test_an_arena_does_not_depend_on_its_wave(base):
    """Arena i of a 1057-arena handle is arena i - base of a handle created with arena_base = base and the
    same per-arena states.  base = 64 (two whole waves): every arena keeps its lane and its 31 wave mates
    and only the wave's index changes, which pins the keying of both draws by arena_base.  base = 45 (no
    multiple of 32): every arena sits on another lane pair, gathers its counter and features from other
    MFMA lanes and shares its wave with a different set of arenas, whose decisions close on other wave
    ticks -- and gets the same results."""
    n, D = 1057, 16
    sim, ro = make(n)
    state0 = sim.get_state()
    whole = run(sim, ro, D)
    sim.close()
    sub, ro2 = make(n - base, arena_base=base)
    sub.set_state(state0[base:])  # (the arenas' game RNG streams included)
    part = run(sub, ro2, D)
    for k in tuple(_abi.OUTPUT_SPEC) + SAMPLES:  # (the arena axis: 2 of P2's [n][max_ticks][N], else 1)
        assert_same(k, whole[k][:, :, base:] if k in ("A2", "LP2") else whole[k][:, base:], part[k])
    assert whole["ticks"].max() > 1
    sub.close()


def test_mirrored_p2_equals_p1_wherever_the_game_is_symmetric():
    """test_gpu_selfplay's mirror identity per decision: the same weights and seed, mirrored -- where the
    row before a decision is symmetric, P2's draw on the decision's first tick (counter + 0 << 40) is P1's."""
    n, D = 1057, 24
    sim, ro = make(n, same=True, mirror=True)
    prev0 = sim.outputs_numpy()
    res = run(sim, ro, D)
    prev = [prev0] + [row(res, d) for d in range(D - 1)]
    sym = np.stack([(r["position"][:, 0] == -r["position"][:, 1]) & (r["guard"][:, 0] == r["guard"][:, 1]) &
                    (r["move"][:, 0] == r["move"][:, 1]) & (r["move_frame"][:, 0] == r["move_frame"][:, 1])
                    for r in prev])
    assert sym[0].all(), "a fresh handle is symmetric"
    assert_same("p2_actions where symmetric", res["A1"][sym], res["A2"][:, 0][sym])
    assert_same("p2_logp where symmetric", res["LP1"][sym], res["LP2"][:, 0][sym])
    assert sym.sum() > n and len(np.unique(res["A1"][sym])) >= 4  # (not a degenerate agreement)
    sim.close()


# -- 7. general geometry -------------------------------------------------------------------------------------
def test_loaded_airborne_and_flipped_fighters(oracle_lib):
    n, D = 130, 16
    state = random_states(n, np.random.default_rng(3), p2="external", geom_frac=0.3)
    sim, ro = make(n)
    sim.set_state(state)
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, base_seed=SIM_SEED)
    ora.set_state(state)
    # the loaded states are what the general-geometry body is for (a launch-uniform branch on the handle's
    # flag, which set_state raises for any such fighter): airborne fighters and flipped facings, on either side
    f = state["f"]
    assert (f["position_y"] != 0).any(axis=0).all() and (f["facing_flipped"] != 0).any(axis=0).all()
    assert lib_name(sim) == b"fsk::selfplay::k_step_skip_selfplay<0>"
    res = run(sim, ro, D)
    replay(ora, res, True, True, CAP)
    compare_states(ora.state(), sim.get_state())
    ora.close()
    sim.close()


def lib_name(sim, n=8):
    from footsies_gym_amd._lib import lib
    return lib().fs_step_kernel(sim.handle, n, _abi.FS_KERNEL_SKIP_SELFPLAY)


# -- 8. the API ------------------------------------------------------------------------------------------------
def test_refusals_names_and_optional_outputs():
    import torch
    from footsies_gym_amd._lib import FootsiesError, lib
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    actor = make_actor(device=torch.device("cuda", 0), seed=1)

    def refused(sim, code):
        with pytest.raises(FootsiesError, match="fs_step_skip_selfplay") as e:
            FusedSelfPlayRollout(sim, actor).rollout_skipped(4)
        assert e.value.code == code

    # FS_E_UNSUPPORTED exactly where fs_step_n_selfplay returns it; no kernel is named there
    for kw in (dict(p2_mode="bot"), dict(p2_mode="noop"), dict(p2_mode="external", p1_mode="bot"),
               dict(p2_mode="external", frame_delay=2)):
        s = FootsiesSim(8, seed=4, **kw)
        refused(s, _abi.FS_E_UNSUPPORTED)
        assert lib_name(s) is None and s.steps_taken == 0
        s.close()
    sim = FootsiesSim(8, p2_mode="external", seed=4)
    assert lib_name(sim) == b"fsk::selfplay::k_step_skip_selfplay<0>" and lib_name(sim, 0) is None
    dbl = FootsiesSim(8, p2_mode="external", float_mode="double", seed=4)
    assert lib_name(dbl) == b"fsk::selfplay::k_step_skip_selfplay<1>"
    dbl.close()
    mask = np.zeros(8, np.uint8)
    mask[3] = 1
    sim.set_p2_mode("bot", mask)  # one arena's P2 switched to the bot
    refused(sim, _abi.FS_E_UNSUPPORTED)
    assert lib_name(sim) is None
    sim.set_p2_mode("external", mask)
    assert lib_name(sim) == b"fsk::selfplay::k_step_skip_selfplay<0>"

    # FS_E_INVALID: the arguments
    ro = FusedSelfPlayRollout(sim, actor)
    big = torch.zeros(16, dtype=torch.uint8, device=sim.device)  # (never written: the call is refused)

    def call(n=4, flags=_abi.FS_SELFPLAY_MIRROR, max_ticks=8, drop1=None, drop2=None, traj=None, p2_out=None):
        f = ["w1", "b1", "w2", "b2", "w3", "b3"]
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, ro.params)}, seed=1)
        p2 = _abi.fs_policy(**{k: (None if k == drop2 else t.data_ptr()) for k, t in zip(f, ro.params2)}, seed=2,
                            actions_out=p2_out)
        return lib().fs_step_skip_selfplay(sim.handle, n, C.byref(p1), C.byref(p2), flags, max_ticks,
                                           None if traj is None else C.byref(traj), None)

    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        assert call(drop1=k) == _abi.FS_E_INVALID and call(drop2=k) == _abi.FS_E_INVALID
    assert lib().fs_step_skip_selfplay(sim.handle, 4, None, None, 0, 8, None, None) == _abi.FS_E_INVALID
    assert call(n=0) == _abi.FS_E_INVALID and call(n=-1) == _abi.FS_E_INVALID
    assert call(max_ticks=0) == _abi.FS_E_INVALID
    assert call(max_ticks=_abi.FS_SKIP_POLICY_MAX_TICKS + 1) == _abi.FS_E_INVALID
    assert call(flags=2) == _abi.FS_E_INVALID and call(flags=3) == _abi.FS_E_INVALID
    # n * max_ticks * N past int32 with a P2 array: 2^17 * 4096 * 8 = 2^32 entries
    assert call(n=1 << 17, max_ticks=4096, p2_out=big.data_ptr()) == _abi.FS_E_INVALID
    t = sim.alloc_trajectory(4)
    ptrs = {k: t[k].data_ptr() for k in _abi.OUTPUT_SPEC if k in t}
    assert call(traj=_abi.fs_outputs(**{k: v for k, v in ptrs.items() if k != "reward"})) == _abi.FS_E_INVALID
    assert call(traj=_abi.fs_outputs(**{k: v for k, v in ptrs.items() if k != "final_move"})) == _abi.FS_E_INVALID
    assert sim.steps_taken == 0  # nothing ran
    assert call(traj=_abi.fs_outputs(**ptrs)) == 0 and call(flags=0) == 0 and call(max_ticks=1) == 0
    assert sim.steps_taken == 12
    with pytest.raises(ValueError):
        ro.rollout_skipped(0)
    with pytest.raises(ValueError):
        ro.rollout_skipped(4, max_ticks=0)
    sim.close()

    # every sample array is optional, and with traj = NULL the regular outputs hold the last decision
    a = FootsiesSim(256, p2_mode="external", seed=4)
    b = FootsiesSim(256, p2_mode="external", seed=4)
    ra, rb = FusedSelfPlayRollout(a, actor, seed=3), FusedSelfPlayRollout(b, actor, seed=3)
    got = ra.rollout_skipped(12, False, False, False, False)
    assert got == (False, False, False) and ra.last_capped is False and ra.last_p2 == (False, False)
    traj = b.alloc_trajectory(12)
    _, _, ticks = rb.rollout_skipped(12, trajectory=traj, p2_actions=None, p2_logp=None)
    torch.cuda.synchronize()
    assert rb.last_p2[0].shape == rb.last_p2[1].shape == (12, CAP, 256)
    assert rb.last_p2[0].dtype == torch.uint8 and rb.last_p2[1].dtype == torch.float32
    outs = a.outputs_numpy()
    compare_outputs({k: v[11].cpu().numpy() for k, v in traj.items()}, outs, same_step=True)
    compare_states(a.get_state(), b.get_state())
    assert int(ticks.max()) > 1
    a.close()
    b.close()


# -- 9. PPO ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", ["hip", "torch"])
def test_ppo_on_decisions_against_the_frozen_copy(learner):
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(64, p2_mode="external", seed=5)
    tr = PPOTrainer(sim, horizon=8, epochs=2, minibatches=4, lr=1e-2, seed=3, learner=learner, self_play="decisions",
                    opponent_refresh=2)
    assert tr.frame_skip and tr.self_play and tr.rollout.mirror
    ptrs = [p.data_ptr() for p in tr.rollout.params2]
    ages = []
    for _ in range(3):
        tr.iterate()
        for k in ("loss", "policy_loss", "value_loss", "entropy", "mean_reward", "ticks_per_decision", "capped",
                  "opponent_age"):
            assert bool(torch.isfinite(tr.stats[k].float()).all()), k
        assert float(tr.stats["ticks_per_decision"]) >= 1.0
        ages.append(int(tr.stats["opponent_age"]))
    assert ages == [1, 0, 1]
    assert [p.data_ptr() for p in tr.rollout.params2] == ptrs  # the opponent's buffers stay put
    assert sim.steps_taken == 3 * 8  # decisions
    sim.close()


def test_ppo_decisions_with_one_tick_collects_what_per_tick_self_play_collects():
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    a = FootsiesSim(64, p2_mode="external", seed=5)
    b = FootsiesSim(64, p2_mode="external", seed=5)
    ta = PPOTrainer(a, horizon=8, seed=3, self_play=True)
    tb = PPOTrainer(b, horizon=8, seed=3, self_play="decisions", max_skip_ticks=1)
    for x, y in zip(ta.collect(), tb.collect()):
        assert torch.equal(x, y)
    assert torch.equal(ta.logp, tb.logp) and bool((tb.ticks == 1).all())
    with pytest.raises(ValueError, match="self_play"):
        PPOTrainer(a, self_play="nonsense")
    with pytest.raises(ValueError, match="frame_skip"):
        PPOTrainer(a, self_play=True, frame_skip=True)
    a.close()
    b.close()
