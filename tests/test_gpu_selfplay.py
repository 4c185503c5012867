"""fs_step_n_selfplay / k_step_n_selfplay (FusedSelfPlayRollout, PPOTrainer(self_play=True)): both
fighters sampled by in-kernel actors, one launch per block of ticks.

Bar 1, the simulation: P1's sampled indices and P2's game inputs (its indices with Left and Right
exchanged when mirrored), replayed through the CPU oracle with a remote P2, give the same outputs
on every tick and the same final state.  Bar 2, the actors: each matches the host restatement
(tests/policy_ref.py) under test_gpu_policy's unchanged bars (_check_policy: MARGIN, LOGP_TOL), P2 on
the mirrored rows with its own weights and seed.  Then two derivable identities, both bitwise: an
unmirrored P2 with P1's weights and seed is the same actor twice, and a mirrored one is wherever
the game is symmetric."""
import ctypes as C

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd.rollout import swap_left_right
from tests import policy_ref
from tests.parity_utils import assert_same, compare_outputs, compare_states, random_states
from tests.test_gpu_policy import LOGP_TOL, MARGIN, _check_policy  # noqa: F401 -- the bars, unchanged

pytestmark = pytest.mark.gpu

P1_ACTOR, P2_ACTOR = 9, 10
P1_SEED, P2_SEED, SIM_SEED = 0xC0FFEE, 0xBEEF, 21
AUTORESET = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}
FLOAT = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
PAIRS = ("guard", "move", "move_frame", "position")  # the [N, 2] fields the actors' features come from


def make(n, autoreset="same_step", float_mode="strict", same=False, mirror=True, **kw):
    """A remote-P2 sim and its self-play rollout: two different actors and seeds, or (`same`) P2 with
    P1's weights and P1's seed."""
    import torch
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    dev = torch.device("cuda", 0)
    sim = FootsiesSim(n, p2_mode="external", autoreset_mode=autoreset, float_mode=float_mode, seed=SIM_SEED, **kw)
    ro = FusedSelfPlayRollout(sim, make_actor(device=dev, seed=P1_ACTOR),
                              opponent=None if same else make_actor(device=dev, seed=P2_ACTOR), seed=P1_SEED,
                              opponent_seed=P1_SEED if same else P2_SEED, mirror=mirror)
    return sim, ro


def run(sim, ro, n):
    """One call: the trajectory and the four sample arrays on the host."""
    import torch
    traj = sim.alloc_trajectory(n)
    a1, lp1, a2, lp2 = ro.rollout(n, trajectory=traj)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in traj.items()}
    res.update(A1=a1.cpu().numpy(), LP1=lp1.cpu().numpy(), A2=a2.cpu().numpy(), LP2=lp2.cpu().numpy())
    return res


def rows(res, t):
    return {k: res[k][t] for k in _abi.OUTPUT_SPEC}


def replay(ora, res, mirror, same_step, t0=0):
    """Bar 1 for one call's rows: the oracle on P1's indices and P2's game inputs."""
    for t in range(len(res["A1"])):
        p2_in = swap_left_right(res["A2"][t]) if mirror else res["A2"][t]
        compare_outputs(ora.step(res["A1"][t], p2_in), rows(res, t), step=t0 + t, same_step=same_step)


def mirrored(row):
    """An output row as P2 sees it: the four pair fields column-swapped, the position negated -- whose
    policy_ref.features are exactly the mirrored feature vector (negation commutes with the f32
    scale and the bf16 rounding)."""
    out = {k: np.asarray(row[k])[:, ::-1] for k in PAIRS}
    out["position"] = -out["position"]
    return out


def check_actors(ro, prev, res, t0, n):
    """Bar 2: P1 on the rows as they are, P2 on the mirrored rows with its own weights and seed."""
    p1 = _check_policy([p.cpu().numpy() for p in ro.params], ro.seed, prev, res["A1"], res["LP1"], t0, n)
    prev2 = [mirrored(r) for r in prev] if ro.mirror else prev
    p2 = _check_policy([p.cpu().numpy() for p in ro.params2], ro.opponent_seed, prev2, res["A2"], res["LP2"], t0, n)
    return p1, p2


_played = {}


def played(oracle_lib, n, autoreset="same_step", float_mode="strict"):
    """Two consecutive mirrored calls (48 + 16 ticks, so t0 carries) replayed through the oracle, once
    per case and shared by bars 1 and 2: (rollout, outputs before tick 0, the 64 rows, final states, steps)."""
    key = (n, autoreset, float_mode)
    if key not in _played:
        sim, ro = make(n, autoreset, float_mode)
        ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, autoreset_mode=AUTORESET[autoreset],
                                float_mode=FLOAT[float_mode], base_seed=SIM_SEED)
        prev0 = sim.outputs_numpy()
        parts, t0, steps = [], 0, []
        for T in (48, 16):
            parts.append(run(sim, ro, T))
            replay(ora, parts[-1], True, autoreset == "same_step", t0)
            t0 += T
            steps.append(sim.steps_taken)
        res = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        _played[key] = (ro, prev0, res, ora.state(), sim.get_state(), steps)
        sim.close()
    return _played[key]


# -- 1. the simulation, exact -----------------------------------------------------------------------------
@pytest.mark.parametrize("n,autoreset,float_mode", [(33, "same_step", "strict"), (33, "next_step", "strict"),
                                                    (1025, "same_step", "strict"), (1025, "next_step", "strict"),
                                                    (1025, "same_step", "double")])
def test_simulation_replays_through_the_oracle(oracle_lib, n, autoreset, float_mode):
    """33 arenas put two live lanes in a second wave; every tick's outputs are compared inside played()."""
    ro, prev0, res, exp_state, got_state, steps = played(oracle_lib, n, autoreset, float_mode)
    assert steps == [48, 64]
    compare_states(exp_state, got_state)
    assert res["A1"].shape == res["A2"].shape == (64, n) and res["A1"].max() < 8 and res["A2"].max() < 8


# -- 2. both actors against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 1025])
def test_both_actors_match_the_restatement(oracle_lib, n):
    ro, prev0, res, _, _, _ = played(oracle_lib, n)
    prev = [prev0] + [rows(res, t) for t in range(63)]
    (m1, w1), (m2, w2) = check_actors(ro, prev, res, 0, n)
    print("N=%d x 64: |d logp| vs the restatement P1 mean %.2e max %.3e, P2 mean %.2e max %.3e" % (n, m1, w1, m2, w2))
    if n == 1025:
        assert len(np.unique(res["A1"])) == 8 and len(np.unique(res["A2"])) == 8


# -- 3. flags = 0: the same actor twice --------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 33])
def test_unmirrored_p2_with_p1s_weights_and_seed_is_p1_bitwise(n):
    """Identical inputs, the same function, -ffp-contract=off and no reduction-order freedom: P2's
    fragments read from LDS hold the bits of P1's in registers, so every sample and log-probability
    is equal bit for bit."""
    sim, ro = make(n, same=True, mirror=False)
    res = run(sim, ro, 40)
    assert_same("p2_actions", res["A1"], res["A2"])
    assert_same("p2_logp", res["LP1"], res["LP2"])
    assert np.isfinite(res["LP1"]).all() and sim.steps_taken == 40


# -- 4. mirror symmetry ------------------------------------------------------------------------------------
def test_mirrored_p2_equals_p1_wherever_the_game_is_symmetric():
    """The same weights and the same seed, mirrored: where the row before a tick is symmetric
    (position[:, 0] == -position[:, 1], guard, move and move_frame equal across the pair) both
    actors see the same features and draw with the same uniform."""
    n, T = 1025, 64
    sim, ro = make(n, same=True, mirror=True)
    prev0 = sim.outputs_numpy()
    res = run(sim, ro, T)
    prev = [prev0] + [rows(res, t) for t in range(T - 1)]
    sym = np.stack([(r["position"][:, 0] == -r["position"][:, 1]) & (r["guard"][:, 0] == r["guard"][:, 1]) &
                    (r["move"][:, 0] == r["move"][:, 1]) & (r["move_frame"][:, 0] == r["move_frame"][:, 1])
                    for r in prev])
    assert sym[0].all(), "a fresh handle is symmetric"
    whole = int(sym.all(axis=1).sum())
    print("mirror symmetry: %d of %d rows symmetric in every arena, %d of %d arena-ticks" % (whole, T, sym.sum(), sym.size))
    assert_same("p2_actions where symmetric", res["A1"][sym], res["A2"][sym])
    assert_same("p2_logp where symmetric", res["LP1"][sym], res["LP2"][sym])
    assert len(np.unique(res["A1"][sym])) == 8  # (not a degenerate agreement)


# -- 5. full size: two waves share a SIMD ------------------------------------------------------------------
def test_full_size_once(oracle_lib):
    n, T = 65536, 16
    sim, ro = make(n)
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, base_seed=SIM_SEED)
    prev0 = sim.outputs_numpy()
    res = run(sim, ro, T)
    replay(ora, res, True, True)
    compare_states(ora.state(), sim.get_state())
    assert sim.steps_taken == T
    prev = [prev0] + [rows(res, t) for t in range(T - 1)]
    (m1, w1), (m2, w2) = check_actors(ro, prev, res, 0, n)
    print("N=65536 x 16: |d logp| vs the restatement P1 mean %.2e max %.3e, P2 mean %.2e max %.3e" % (m1, w1, m2, w2))


# -- 6. split launches --------------------------------------------------------------------------------------
def test_split_launches_equal_the_unsplit_call(monkeypatch):
    n, T = 33, 24
    sim, ro = make(n)
    whole = run(sim, ro, T)
    whole_state = sim.get_state()
    monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(7 * n))  # 7 + 7 + 7 + 3 ticks
    sim2, ro2 = make(n)
    parts = run(sim2, ro2, T)
    assert sim2.steps_taken == T
    for k in whole:
        assert whole[k].tobytes() == parts[k].tobytes(), k
    compare_states(whole_state, sim2.get_state())


# -- 7. general geometry -----------------------------------------------------------------------------------
def test_loaded_airborne_and_flipped_fighters(oracle_lib):
    n, T = 130, 30
    state = random_states(n, np.random.default_rng(3), p2="external", geom_frac=0.3)
    sim, ro = make(n)
    sim.set_state(state)
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, base_seed=SIM_SEED)
    ora.set_state(state)
    res = run(sim, ro, T)
    replay(ora, res, True, True)
    compare_states(ora.state(), sim.get_state())


# -- 8. refusals and optional outputs ----------------------------------------------------------------------
def test_refusals_and_optional_outputs():
    import torch
    from footsies_gym_amd._lib import FootsiesError, lib
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    actor = make_actor(device=torch.device("cuda", 0), seed=1)
    name = lambda s, n=8: lib().fs_step_kernel(s.handle, n, _abi.FS_KERNEL_SELFPLAY)  # noqa: E731

    def refused(sim, code, **kw):
        with pytest.raises(FootsiesError, match="fs_step_n_selfplay") as e:
            FusedSelfPlayRollout(sim, actor, **kw).rollout(4)
        assert e.value.code == code
        return e

    # FS_E_UNSUPPORTED: the handle's kind; no kernel is named for it
    for kw in (dict(p2_mode="bot"), dict(p2_mode="noop"), dict(p2_mode="external", p1_mode="bot"),
               dict(p2_mode="external", frame_delay=2)):
        s = FootsiesSim(8, seed=4, **kw)
        refused(s, _abi.FS_E_UNSUPPORTED)
        assert name(s) is None and s.steps_taken == 0
        s.close()
    sim = FootsiesSim(8, p2_mode="external", seed=4)
    assert name(sim) == b"fsk::selfplay::k_step_n_selfplay<0>" and name(sim, 0) is None
    dbl = FootsiesSim(8, p2_mode="external", float_mode="double", seed=4)
    assert name(dbl) == b"fsk::selfplay::k_step_n_selfplay<1>"
    dbl.close()
    mask = np.zeros(8, np.uint8)
    mask[3] = 1
    sim.set_p2_mode("bot", mask)  # one arena's P2 switched to the bot
    refused(sim, _abi.FS_E_UNSUPPORTED)
    assert name(sim) is None
    sim.set_p2_mode("external", mask)
    assert name(sim) == b"fsk::selfplay::k_step_n_selfplay<0>"

    # FS_E_INVALID: the arguments
    ro = FusedSelfPlayRollout(sim, actor)
    w = ro.params

    def call(n=4, flags=_abi.FS_SELFPLAY_MIRROR, drop1=None, drop2=None, traj=None):
        f = ["w1", "b1", "w2", "b2", "w3", "b3"]
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, w)}, seed=1)
        p2 = _abi.fs_policy(**{k: (None if k == drop2 else t.data_ptr()) for k, t in zip(f, ro.params2)}, seed=2)
        return lib().fs_step_n_selfplay(sim.handle, n, C.byref(p1), C.byref(p2), flags, None if traj is None else C.byref(traj))

    for k in ("w1", "b1", "w2", "b2", "w3", "b3"):
        assert call(drop1=k) == _abi.FS_E_INVALID and call(drop2=k) == _abi.FS_E_INVALID
    assert lib().fs_step_n_selfplay(sim.handle, 4, None, None, 0, None) == _abi.FS_E_INVALID
    assert call(n=0) == _abi.FS_E_INVALID and call(n=-1) == _abi.FS_E_INVALID
    assert call(flags=2) == _abi.FS_E_INVALID and call(flags=3) == _abi.FS_E_INVALID
    t = sim.alloc_trajectory(4)
    ptrs = {k: t[k].data_ptr() for k in _abi.OUTPUT_SPEC if k in t}
    assert call(traj=_abi.fs_outputs(**{k: v for k, v in ptrs.items() if k != "reward"})) == _abi.FS_E_INVALID
    assert call(traj=_abi.fs_outputs(**{k: v for k, v in ptrs.items() if k != "final_move"})) == _abi.FS_E_INVALID  # same-step
    assert sim.steps_taken == 0  # nothing ran
    assert call(traj=_abi.fs_outputs(**ptrs)) == 0 and call(flags=0) == 0
    assert sim.steps_taken == 8

    # all four sample arrays are optional: the same game with and without them
    a = FootsiesSim(256, p2_mode="external", seed=4)
    b = FootsiesSim(256, p2_mode="external", seed=4)
    got = FusedSelfPlayRollout(a, actor, seed=3).rollout(30, False, False, False, False)
    assert got == (False, False, False, False)
    FusedSelfPlayRollout(b, actor, seed=3).rollout(30)
    torch.cuda.synchronize()
    for k, v in a.outputs_numpy().items():
        assert np.array_equal(v, b.outputs_numpy()[k]), k
    compare_states(a.get_state(), b.get_state())
    # derived opponent seed: never the actor's; a wrong actor shape is refused for either side
    r = FusedSelfPlayRollout(a, actor, seed=3)
    assert r.opponent_seed != r.seed and FusedSelfPlayRollout(a, actor, seed=3, opponent_seed=3).opponent_seed == 3
    with pytest.raises(ValueError):
        FusedSelfPlayRollout(a, actor, opponent=make_actor(hidden=32, device=torch.device("cuda", 0)))


# -- 9. PPO ------------------------------------------------------------------------------------------------
def test_ppo_self_play_refreshes_the_opponent_every_second_update():
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(256, p2_mode="external", seed=5)
    tr = PPOTrainer(sim, horizon=16, epochs=2, minibatches=4, lr=1e-2, seed=3, learner="hip", self_play=True,
                    opponent_refresh=2)
    initial = [p.detach().clone() for p in tr.actor.parameters()]
    current = lambda: [p.detach() for p in tr.actor.parameters()]  # noqa: E731
    same = lambda xs, ys: all(torch.equal(x, y) for x, y in zip(xs, ys))  # noqa: E731
    assert same(tr.rollout.params2, initial) and tr.rollout.mirror
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(tr.rollout.params, tr.rollout.params2))
    ptrs = [p.data_ptr() for p in tr.rollout.params2]
    ages = []
    for it in range(3):
        tr.iterate()
        for v in tr.stats.values():
            assert bool(torch.isfinite(v.float()).all())
        ages.append(int(tr.stats["opponent_age"]))
        assert same(tr.rollout.params, current())  # P1 always plays the latest policy
        if it == 0:  # the opponent is still the initial actor, which the learner has left
            assert same(tr.rollout.params2, initial) and not same(tr.rollout.params2, current())
        if it == 1:
            assert same(tr.rollout.params2, current()) and not same(tr.rollout.params2, initial)
            second = [p.clone() for p in tr.rollout.params2]
        if it == 2:
            assert same(tr.rollout.params2, second) and not same(tr.rollout.params2, current())
    assert ages == [1, 0, 1]
    assert [p.data_ptr() for p in tr.rollout.params2] == ptrs  # the buffers stay put
    assert sim.steps_taken == 3 * 16
    bot = FootsiesSim(8, p2_mode="bot", seed=5)
    with pytest.raises(ValueError, match="external"):
        PPOTrainer(bot, self_play=True)
    with pytest.raises(ValueError, match="frame_skip"):
        PPOTrainer(sim, self_play=True, frame_skip=True)
    with pytest.raises(ValueError, match="opponent_refresh"):
        PPOTrainer(sim, self_play=True, opponent_refresh=0)
