"""fs_step_n_league / fs_step_skip_league (FusedSelfPlayRollout(pool=..., bots=...), PPOTrainer(opponent_bot=f)):
the pool launches on a handle where whole groups of 128 arenas are switched to the in-game bot, so that one
launch runs "P1's actor against the pool" in some blocks and "P1's actor against the scripted BattleAI" in others.

Every test here fails on the parent commit: the two entry points do not exist there.

The bars, none with a tolerance of its own:
1. groups against their twins, byte for byte -- a remote group is that group of the pool call on an unswitched
   handle (tests/test_gpu_selfplay_pool.py's cached runs), a bot group of the tick form is that group of
   fs_step_n_policy on a handle with the same arenas switched, under arbitrary P2 rows;
2. the CPU oracle with the same arenas switched replays the kernel's P1 actions everywhere and its P2 inputs in
   the remote groups, every output row and the whole final state equal (the bot, its never-Reset state across
   the reset burst and the game RNG included);
3. the same after fs_set_p2_mode re-assigns groups between two calls;
4. the actors against the host restatement at test_gpu_policy's unchanged MARGIN and LOGP_TOL;
5. refusals and kernel names; 6. the trainer.

P2's sample arrays are pre-filled with 0xFF bytes in every league run: a bot arena's entries must still hold
them afterwards.

Terminal rows in the oracle cases: the loaded random_states put 5% of the fighters at vital 0 and many more
mid-attack at close range, so rounds end from the first tick on and the fight goes on from the burst.  On the CPU
alone (a switched oracle of the 289 loaded arenas, bot / remote / bot, under hashed P1 and P2 actions, 64 ticks)
the bot groups held 37 terminal rows and the remote group 38 in same_step (19 and 14 of them within the first 16
ticks, 18 and 24 after), 37 and 37 in next_step, 32 and 32 with geom_frac = 0.3; remote / bot / remote held 35
and 37.  Each GPU case asserts at least one of either kind."""
import ctypes as C
import functools

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd.rollout import swap_left_right
from tests import policy_ref
from tests import test_gpu_selfplay as tick
from tests import test_gpu_selfplay_pool as P
from tests import test_gpu_selfplay_skip as skip
from tests.parity_utils import assert_same, compare_states, random_states
from tests.test_gpu_policy import LOGP_TOL, MARGIN  # noqa: F401 -- the bars, unchanged (skip.check_draws applies them)

pytestmark = pytest.mark.gpu

GROUP = _abi.FS_SELFPLAY_GROUP
N = P.N                        # 289: groups of 128, 128 and 33
P1_SEED, P2_SEED, SIM_SEED = P.P1_SEED, P.P2_SEED, P.SIM_SEED
CAP, CALLS, SLOTS = P.CAP, P.CALLS, P.SLOTS
SLOTS_OF = {289: SLOTS, 129: (0, 2), 128: (1,), 1: (1,)}
PATTERNS = [(289, (0, 1, 0)), (289, (1, 0, 1)), (129, (0, 1)), (1, (1,))]
SAMPLE_KEYS = ("A1", "LP1", "A2", "LP2", "ticks", "capped")  # (the arena axis is the last one)


def arena_mask(bots, n):
    return np.repeat(np.asarray(bots, dtype=bool), GROUP)[:n]


def make_league(n, bots, slots=None, mirror=True, **kw):
    """A remote-P2 sim, P's pool of three actors and the league rollout with `bots` groups on the in-game bot."""
    import torch
    from footsies_gym_amd.rollout import FusedPoolSelfPlayRollout, FusedSelfPlayRollout, OpponentPool
    sim = P._sim(n, **kw)
    pool = OpponentPool(sim, len(P.SLOT_ACTORS))
    for a in P.SLOT_ACTORS:
        pool.push(P._actor(a))
    ro = FusedSelfPlayRollout(sim, P._actor(P.P1_ACTOR), seed=P1_SEED, opponent_seed=P2_SEED, mirror=mirror, pool=pool,
                              bots=[bool(b) for b in bots])
    assert type(ro) is FusedPoolSelfPlayRollout
    slots = SLOTS_OF[n] if slots is None else slots
    return sim, P.Bound(ro, torch.tensor(slots, dtype=torch.uint8, device=sim.device)), pool


def run_tick(sim, ro, n):
    """tick.run with P2's sample arrays pre-filled with 0xFF bytes."""
    import torch
    traj = sim.alloc_trajectory(n)
    a2 = torch.full((n, sim.num_envs), 0xFF, dtype=torch.uint8, device=sim.device)
    lp2 = torch.full((n, sim.num_envs), -1, dtype=torch.int32, device=sim.device).view(torch.float32)
    a1, lp1, a2, lp2 = ro.rollout(n, p2_actions=a2, p2_logp=lp2, trajectory=traj)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in traj.items()}
    res.update(A1=a1.cpu().numpy(), LP1=lp1.cpu().numpy(), A2=a2.cpu().numpy(), LP2=lp2.cpu().numpy())
    return res


def play(sim, ro, form, calls, max_ticks=CAP):
    runs, steps = [], []
    for m in calls:
        runs.append(run_tick(sim, ro, m) if form == "tick" else skip.run(sim, ro, m, max_ticks))
        steps.append(sim.steps_taken)
    return runs, sim.get_state(), steps


@functools.lru_cache(maxsize=None)
def league(form, n, bots, max_ticks=CAP, calls=None):
    sim, ro, _ = make_league(n, bots)
    out = play(sim, ro, form, calls or CALLS[form], max_ticks)
    sim.close()
    return out


def untouched(res, cols):
    """P2's sample entries of the arenas `cols` still hold the 0xFF bytes written before the call."""
    assert (res["A2"][..., cols] == 0xFF).all()
    assert (res["LP2"][..., cols].view(np.uint32) == 0xFFFFFFFF).all()


def cut(res, k, sl):
    return res[k][..., sl] if k in SAMPLE_KEYS else res[k][:, sl]


# -- 1. groups against their twins ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tick", "skip"])
@pytest.mark.parametrize("n,bots", PATTERNS)
def test_remote_groups_equal_the_pool_launch_on_an_unswitched_handle(form, n, bots):
    runs, state, steps = league(form, n, bots)
    ref_runs, ref_state, ref_steps = P.pooled(form, n, SLOTS_OF[n])
    assert steps == ref_steps == list(np.cumsum(CALLS[form]))
    for g, sl in enumerate(P.groups(n)):
        for res, ref in zip(runs, ref_runs):
            if bots[g]:
                untouched(res, sl)
                continue
            assert sorted(res) == sorted(ref)
            for k in res:
                a, b = cut(res, k, sl), cut(ref, k, sl)
                assert a.shape == b.shape and a.size and a.tobytes() == b.tobytes(), (g, k)
        if not bots[g]:
            compare_states(ref_state[sl], state[sl])
    assert (state["p2_bot"] != 0).tolist() == arena_mask(bots, n).tolist()  # the header bit survives the launch


@functools.lru_cache(maxsize=None)
def policy_twin(n, bots):
    """fs_step_n_policy on a handle with the same arenas switched, under arbitrary P2 rows."""
    import torch
    from footsies_gym_amd.rollout import FusedPolicyRollout
    sim = P._sim(n)
    sim.set_p2_mode("bot", arena_mask(bots, n).astype(np.uint8))
    ro = FusedPolicyRollout(sim, P._actor(P.P1_ACTOR), seed=P1_SEED)
    gen = torch.Generator(device=sim.device)
    gen.manual_seed(5)
    runs = []
    for m in CALLS["tick"]:
        traj = sim.alloc_trajectory(m)
        rows = torch.randint(0, 8, (m, n), dtype=torch.uint8, device=sim.device, generator=gen)
        a1, lp1 = ro.rollout(m, p2_actions=rows, trajectory=traj)
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in traj.items()}
        res.update(A1=a1.cpu().numpy(), LP1=lp1.cpu().numpy())
        runs.append(res)
    out = runs, sim.get_state()
    sim.close()
    return out


@pytest.mark.parametrize("n,bots", PATTERNS)
def test_bot_groups_of_the_tick_form_equal_fs_step_n_policy_on_a_switched_twin(n, bots):
    """Every trajectory field, P1's actions and log-probs and the final state, the bot and RNG words included."""
    runs, state, _ = league("tick", n, bots)
    ref_runs, ref_state = policy_twin(n, bots)
    seen = 0
    for g, sl in enumerate(P.groups(n)):
        if not bots[g]:
            continue
        for res, ref in zip(runs, ref_runs):
            for k in ref:
                a, b = cut(res, k, sl), cut(ref, k, sl)
                assert a.shape == b.shape and a.size and a.tobytes() == b.tobytes(), (g, k)
        compare_states(ref_state[sl], state[sl])
        seen += 1
    assert seen == sum(bots)


def test_decision_form_with_max_ticks_1_equals_the_tick_form():
    bots = (0, 1, 0)
    runs, state, steps = league("tick", N, bots)
    runs1, state1, steps1 = league("skip", N, bots, 1, CALLS["tick"])
    assert steps == steps1
    for res, one in zip(runs, runs1):
        for k in res:
            got = one[k][:, 0] if k in ("A2", "LP2") else one[k]
            assert_same(k, res[k], got)
        assert (one["ticks"] == 1).all()
    compare_states(state, state1)


@pytest.mark.parametrize("form", ["tick", "skip"])
def test_with_no_group_switched_the_league_calls_are_the_pool_calls(form):
    runs, state, steps = league(form, N, (0, 0, 0))
    ref_runs, ref_state, ref_steps = P.pooled(form, N, SLOTS)
    assert steps == ref_steps
    for res, ref in zip(runs, ref_runs):
        assert sorted(res) == sorted(ref)
        for k in ref:
            assert res[k].tobytes() == ref[k].tobytes(), k
    compare_states(ref_state, state)


# -- 2. through the oracle --------------------------------------------------------------------------------
def loaded(n, bots, geom):
    st = random_states(n, np.random.default_rng(3), p2="external", geom_frac=geom)
    st["p2_bot"] = arena_mask(bots, n)
    return st


def make_oracle(oracle_lib, n, bots, autoreset="same_step", float_mode="strict", arena_base=0):
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, autoreset_mode=tick.AUTORESET[autoreset],
                            float_mode=tick.FLOAT[float_mode], base_seed=SIM_SEED, arena_base=arena_base)
    assert ora.set_p2_mode(_abi.FS_P2_BOT, arena_mask(bots, n).astype(np.uint8)) == 0
    return ora


def for_replay(res, bot):
    """`res` as the single-opponent replays read it: a bot arena's P2 entries, checked to be untouched, stand as
    input 0 (which the oracle ignores while the bot plays) where a tick ran."""
    untouched(res, bot)
    out = dict(res)
    out["A2"], out["LP2"] = res["A2"].copy(), res["LP2"].copy()
    if "ticks" in res:
        ran = np.arange(res["A2"].shape[1])[None, :, None] < res["ticks"][:, None, :]
        fill = ran & bot[None, None, :]
    else:
        fill = np.broadcast_to(bot[None, :], res["A2"].shape)
    out["A2"][fill] = 0
    out["LP2"][fill] = 0.0
    return out


def replay_calls(sim, ro, ora, form, bots, same_step, calls=None, between=None):
    """Consecutive calls replayed through `ora`; returns (terminal rows in bot arenas, in remote arenas)."""
    n = sim.num_envs
    bot = arena_mask(bots, n)
    at, ends = 0, np.zeros(2, np.int64)
    for c, m in enumerate(calls or CALLS[form]):
        if c and between:
            bot = between()
        if form == "tick":
            res = run_tick(sim, ro, m)
            tick.replay(ora, for_replay(res, bot), True, same_step, at)
        else:
            res = skip.run(sim, ro, m, CAP)
            skip.replay(ora, for_replay(res, bot), True, same_step, CAP, at)
        term = res["terminated"].astype(bool)
        ends += (term[:, bot].sum(), term[:, ~bot].sum())
        at += m
    compare_states(ora.state(), sim.get_state())
    return ends


ORACLE_CASES = [("same_step", "strict", 0.0, 0), ("next_step", "strict", 0.0, 0), ("same_step", "double", 0.0, 0),
                ("same_step", "strict", 0.3, 0), ("next_step", "double", 0.3, 0), ("same_step", "strict", 0.0, 256)]


@pytest.mark.parametrize("form", ["tick", "skip"])
@pytest.mark.parametrize("autoreset,float_mode,geom,arena_base", ORACLE_CASES)
def test_league_launch_replays_through_a_switched_oracle(oracle_lib, form, autoreset, float_mode, geom, arena_base):
    """Both auto-reset modes, both float models, airborne / flipped fighters (the general-geometry tick) and a
    non-zero arena_base; bot / remote / bot (partial) so that a reset burst meets the never-Reset bot."""
    bots = (1, 0, 1)
    state = loaded(N, bots, geom)
    sim, ro, _ = make_league(N, bots, autoreset=autoreset, float_mode=float_mode, arena_base=arena_base)
    ora = make_oracle(oracle_lib, N, bots, autoreset, float_mode, arena_base)
    sim.set_state(state)
    assert ora.set_state(state) == 0
    ends = replay_calls(sim, ro, ora, form, bots, autoreset == "same_step")
    print("terminal rows: %d in bot groups, %d in remote groups" % tuple(ends))
    assert ends[0] >= 1 and ends[1] >= 1
    sim.close()
    ora.close()


@pytest.mark.parametrize("form", ["tick", "skip"])
def test_split_launches_replay_the_same(oracle_lib, monkeypatch, form):
    monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(5 * N))  # 48 ticks: 9 launches of 5 and one of 3
    bots = (0, 1, 0)
    state = loaded(N, bots, 0.0)
    sim, ro, _ = make_league(N, bots)
    ora = make_oracle(oracle_lib, N, bots)
    sim.set_state(state)
    assert ora.set_state(state) == 0
    ends = replay_calls(sim, ro, ora, form, bots, True)
    assert ends[0] >= 1 and ends[1] >= 1
    sim.close()
    ora.close()


# -- 3. switching between calls ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tick", "skip"])
def test_groups_reassigned_between_calls(oracle_lib, form):
    """After the first call group 0 (remote) goes to the bot and group 1 (bot) back to the actor: the handle's
    P2 bit is the source of truth, and the oracle models the same switch."""
    bots, after = (0, 1, 0), (1, 0, 0)
    sim, ro, _ = make_league(N, bots)
    ora = make_oracle(oracle_lib, N, bots)
    state = loaded(N, bots, 0.0)
    sim.set_state(state)
    assert ora.set_state(state) == 0

    def between():
        to_bot = arena_mask((1, 0, 0), N).astype(np.uint8)
        to_remote = arena_mask((0, 1, 0), N).astype(np.uint8)
        sim.set_p2_mode("bot", to_bot)
        sim.set_p2_mode("external", to_remote)
        assert ora.set_p2_mode(_abi.FS_P2_BOT, to_bot) == 0 and ora.set_p2_mode(_abi.FS_P2_EXTERNAL, to_remote) == 0
        return arena_mask(after, N)

    replay_calls(sim, ro, ora, form, bots, True, between=between)
    assert (sim.get_state()["p2_bot"] != 0).tolist() == arena_mask(after, N).tolist()
    sim.close()
    ora.close()


# -- 4. the actors ----------------------------------------------------------------------------------------
def test_actors_match_the_restatement():
    bots = (0, 1, 0)
    bot = arena_mask(bots, N)
    sim, ro, pool = make_league(N, bots)
    prev0 = sim.outputs_numpy()
    T = 64
    res = run_tick(sim, ro, T)
    prev = [prev0] + [tick.rows(res, t) for t in range(T - 1)]
    f1 = np.stack([policy_ref.features(p) for p in prev])                  # [T][N][8]
    f2 = np.stack([policy_ref.features(tick.mirrored(p)) for p in prev])
    arena, counter = np.tile(np.arange(N), (T, 1)), np.repeat(np.arange(T), N).reshape(T, N)
    p1 = [p.cpu().numpy() for p in ro.params]
    for name, cols in (("bot groups", bot), ("remote groups", ~bot)):
        m1 = skip.check_draws(p1, P1_SEED, f1[:, cols].reshape(-1, 8), arena[:, cols].reshape(-1),
                              counter[:, cols].reshape(-1), res["A1"][:, cols].reshape(-1), res["LP1"][:, cols].reshape(-1))
        print("P1 in the %s: |d logp| mean %.2e max %.3e" % ((name,) + m1))
    for g, sl in enumerate(P.groups(N)):
        if bots[g]:
            untouched(res, sl)
            continue
        w = [p.cpu().numpy() for p in pool.params(SLOTS[g])]
        m2 = skip.check_draws(w, P2_SEED, f2[:, sl].reshape(-1, 8), arena[:, sl].reshape(-1), counter[:, sl].reshape(-1),
                              res["A2"][:, sl].reshape(-1), res["LP2"][:, sl].reshape(-1))
        print("group %d (slot %d): P2 |d logp| mean %.2e max %.3e" % ((g, SLOTS[g]) + m2))
    sim.close()


# -- 5. refusals and names --------------------------------------------------------------------------------
def test_refusals_and_kernel_names():
    import torch
    from footsies_gym_amd._lib import FootsiesError, lib
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, OpponentPool
    from footsies_gym_amd.simulator import FootsiesSim
    actor = P._actor(1)
    L = lib()
    name_n = lambda s, n=8: L.fs_step_kernel(s.handle, n, _abi.FS_KERNEL_LEAGUE)  # noqa: E731
    name_d = lambda s, n=8: L.fs_step_kernel(s.handle, n, _abi.FS_KERNEL_SKIP_LEAGUE)  # noqa: E731

    # the handle kinds every self-play call refuses
    for kw in (dict(p2_mode="bot"), dict(p2_mode="noop"), dict(p2_mode="external", p1_mode="bot"),
               dict(p2_mode="external", frame_delay=2)):
        s = FootsiesSim(8, seed=4, **kw)
        pool = OpponentPool(s, 2, actor)
        ro = FusedSelfPlayRollout(s, actor, pool=pool)
        ro.bots = np.zeros(1, bool)  # (the league calls, without the constructor's switch: these handles refuse it)
        slots = torch.zeros(1, dtype=torch.uint8, device=s.device)
        for call, match in ((lambda: ro.rollout(4, slots=slots), "fs_step_n_league"),
                            (lambda: ro.rollout_skipped(4, slots=slots), "fs_step_skip_league")):
            with pytest.raises(FootsiesError, match=match) as e:
                call()
            assert e.value.code == _abi.FS_E_UNSUPPORTED
        assert name_n(s) is None and name_d(s) is None and s.steps_taken == 0
        s.close()

    n = 289
    sim = FootsiesSim(n, p2_mode="external", seed=4)
    assert name_n(sim) == b"fsk::league::k_step_n_league<0>" and name_n(sim, 0) is None
    assert name_d(sim) == b"fsk::league::k_step_skip_league<0>" and name_d(sim, 0) is None
    dbl = FootsiesSim(8, p2_mode="external", float_mode="double", seed=4)
    assert name_n(dbl) == b"fsk::league::k_step_n_league<1>" and name_d(dbl) == b"fsk::league::k_step_skip_league<1>"
    dbl.close()
    pool = OpponentPool(sim, 3, actor)
    plain = FusedSelfPlayRollout(sim, actor, pool=pool)                       # the pool calls
    ro = FusedSelfPlayRollout(sim, actor, pool=pool, bots=[False, False, False])  # the league calls
    slots = torch.zeros(3, dtype=torch.uint8, device=sim.device)

    # one arena of group 1 switched: a mixed group, named; the four existing calls refuse the handle as before
    mask = np.zeros(n, np.uint8)
    mask[130] = 1
    sim.set_p2_mode("bot", mask)
    for call in (lambda: ro.rollout(4, slots=slots), lambda: ro.rollout_skipped(4, slots=slots)):
        with pytest.raises(FootsiesError, match=r"group 1 \(arenas 128 \.\. 255\)") as e:
            call()
        assert e.value.code == _abi.FS_E_UNSUPPORTED
    assert name_n(sim) is None and name_d(sim) is None
    single = FusedSelfPlayRollout(sim, actor, opponent=actor)
    mask[128:256] = 1
    sim.set_p2_mode("bot", mask)  # the whole group: the league calls take it, the others still refuse
    assert name_n(sim) is not None and name_d(sim) is not None
    for call, match in ((lambda: plain.rollout(4, slots=slots), "fs_step_n_selfplay_pool"),
                        (lambda: plain.rollout_skipped(4, slots=slots), "fs_step_skip_selfplay_pool"),
                        (lambda: single.rollout(4), "fs_step_n_selfplay:"),
                        (lambda: single.rollout_skipped(4), "fs_step_skip_selfplay:")):
        with pytest.raises(FootsiesError, match=match) as e:
            call()
        assert e.value.code == _abi.FS_E_UNSUPPORTED and "switched to the bot" in str(e.value)
    for flag in (_abi.FS_KERNEL_SELFPLAY, _abi.FS_KERNEL_SKIP_SELFPLAY, _abi.FS_KERNEL_SELFPLAY_POOL,
                 _abi.FS_KERNEL_SKIP_SELFPLAY_POOL):
        assert L.fs_step_kernel(sim.handle, 8, flag) is None
    # the last, partial group counts as a group
    mask[:] = 0
    mask[288] = 1
    sim.set_p2_mode("external", None)
    sim.set_p2_mode("bot", mask)
    with pytest.raises(FootsiesError, match=r"group 2 \(arenas 256 \.\. 288\)"):
        ro.rollout(4, slots=slots)
    assert sim.steps_taken == 0
    mask[256:] = 1
    sim.set_p2_mode("bot", mask)
    ro.rollout(4, slots=slots)
    assert sim.steps_taken == 4

    # FS_E_INVALID: the arguments, as for the pool calls
    f = ["w1", "b1", "w2", "b2", "w3", "b3"]

    def arg(n_slots=3, weights=True, slot=True):
        return _abi.fs_policy_pool(weights=pool.weights.data_ptr() if weights else None, n_slots=n_slots,
                                   slot=slots.data_ptr() if slot else None, seed=2)

    def call_n(n=4, flags=_abi.FS_SELFPLAY_MIRROR, drop1=None, p=None, null_pool=False):
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, ro.params)}, seed=1)
        return L.fs_step_n_league(sim.handle, n, C.byref(p1), None if null_pool else C.byref(p or arg()), flags, None)

    def call_d(n=4, flags=_abi.FS_SELFPLAY_MIRROR, max_ticks=8, drop1=None, p=None, null_pool=False):
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, ro.params)}, seed=1)
        return L.fs_step_skip_league(sim.handle, n, C.byref(p1), None if null_pool else C.byref(p or arg()), flags,
                                     max_ticks, None, None)

    for call in (call_n, call_d):
        assert call(null_pool=True) == _abi.FS_E_INVALID
        assert call(p=arg(weights=False)) == _abi.FS_E_INVALID and call(p=arg(slot=False)) == _abi.FS_E_INVALID
        assert call(p=arg(n_slots=0)) == _abi.FS_E_INVALID and call(p=arg(n_slots=257)) == _abi.FS_E_INVALID
        for k in f:
            assert call(drop1=k) == _abi.FS_E_INVALID
        assert call(n=0) == _abi.FS_E_INVALID and call(n=-1) == _abi.FS_E_INVALID
        assert call(flags=2) == _abi.FS_E_INVALID and call(flags=3) == _abi.FS_E_INVALID
    assert L.fs_step_n_league(sim.handle, 4, None, C.byref(arg()), 0, None) == _abi.FS_E_INVALID
    assert call_d(max_ticks=0) == _abi.FS_E_INVALID and call_d(max_ticks=_abi.FS_SKIP_POLICY_MAX_TICKS + 1) == _abi.FS_E_INVALID
    assert sim.steps_taken == 4  # nothing more ran
    assert call_n(flags=0) == 0 and call_d(flags=0) == 0
    assert sim.steps_taken == 12
    sim.close()


# -- 6. the trainer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,iterations", [(True, 3), ("decisions", 2)])
def test_ppo_plays_the_league(mode, iterations):
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.rollout import bot_groups
    from footsies_gym_amd.simulator import FootsiesSim
    n, seed = 384, 3
    bots = bot_groups(seed, 0, 3, 0.5)
    assert 0 < bots.sum() < 3  # (this seed draws both kinds)
    sim = FootsiesSim(n, p2_mode="external", seed=5)
    tr = PPOTrainer(sim, horizon=16, epochs=2, minibatches=4, lr=1e-2, seed=seed, learner="hip", self_play=mode,
                    opponent_pool=3, opponent_bot=0.5)
    assert tr.bots.tolist() == bots.tolist()
    bot = torch.from_numpy(arena_mask(bots, n)).to(sim.device)
    assert (sim.get_state()["p2_bot"] != 0).tolist() == arena_mask(bots, n).tolist()
    for it in range(iterations):
        tr.iterate()
        for k, v in tr.stats.items():
            assert bool(torch.isfinite(v.float()).all()), k
        term = tr.traj["terminated"] != 0
        won = term & (tr.traj["reward"] > 0)
        ep, wins = tr.stats["pool_episodes"], tr.stats["pool_wins"]
        assert ep.shape == wins.shape == (3,)
        assert int(ep.sum()) == int(term[:, ~bot].sum()) and int(wins.sum()) == int(won[:, ~bot].sum())
        assert tr.stats["bot_episodes"].dtype == tr.stats["bot_wins"].dtype == torch.int64
        assert int(tr.stats["bot_episodes"]) == int(term[:, bot].sum())
        assert int(tr.stats["bot_wins"]) == int(won[:, bot].sum())
    assert sim.steps_taken == iterations * 16
    assert (sim.get_state()["p2_bot"] != 0).tolist() == arena_mask(bots, n).tolist()
    sim.close()
    # without opponent_pool: the single frozen copy as a one-slot pool
    sim = FootsiesSim(n, p2_mode="external", seed=5)
    tr = PPOTrainer(sim, horizon=8, seed=seed, learner="hip", self_play=mode, opponent_bot=0.5)
    tr.iterate()
    assert tr.pool.capacity == 1 and tr.stats["pool_episodes"].shape == (1,) and "bot_wins" in tr.stats
    assert bool(torch.isfinite(tr.stats["loss"]))
    sim.close()


def test_ppo_without_opponent_bot_is_unchanged():
    """opponent_bot=None: stats and weights after two iterations byte-identical to a trainer built without it."""
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    out = []
    for kw in ({}, {"opponent_bot": None}):
        sim = FootsiesSim(384, p2_mode="external", seed=5)
        tr = PPOTrainer(sim, horizon=16, epochs=2, minibatches=4, lr=1e-2, seed=3, learner="hip", self_play=True,
                        opponent_pool=3, **kw)
        for _ in range(2):
            tr.iterate()
        torch.cuda.synchronize()
        assert tr.bots is None and "bot_episodes" not in tr.stats
        out.append(({k: v.cpu().numpy().tobytes() for k, v in tr.stats.items()},
                    [p.detach().cpu().numpy().tobytes() for p in list(tr.actor.parameters()) + list(tr.critic.parameters())]))
        sim.close()
    assert out[0] == out[1]
