"""fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool (OpponentPool, FusedSelfPlayRollout(pool=...),
PPOTrainer(opponent_pool=K)): self-play against a pool of snapshots in one launch, P2's weights chosen
per group of 128 consecutive arenas.

The contract is an identity: arena i's results are bit for bit those of the single-opponent call with
the weights of slot[i / 128].  So the main bar compares one pool launch, group by group and byte for
byte, against one single-opponent run per slot (every trajectory field, the four sample arrays, the final
state).  Beside it the bars of the calls it extends, on the pool launch itself: the oracle replays P1's
indices and P2's game inputs, and both actors match the host restatement (tests/policy_ref.py) at
test_gpu_policy's unchanged MARGIN and LOGP_TOL, P2 per group with that group's slot weights.

The main shape is N = 289: two full groups and a 33-arena one whose second wave is part-filled."""
import ctypes as C
import functools

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests import policy_ref
from tests import test_gpu_selfplay as tick
from tests import test_gpu_selfplay_skip as skip
from tests.parity_utils import assert_same, compare_states, random_states
from tests.test_gpu_policy import LOGP_TOL, MARGIN  # noqa: F401 -- the bars, unchanged (skip.check_draws applies them)

pytestmark = pytest.mark.gpu

GROUP = _abi.FS_SELFPLAY_GROUP
N = 289
P1_ACTOR = 13                 # (test_gpu_selfplay_skip's pair 13 / 14 fights: rounds end within a test's ticks)
SLOT_ACTORS = (14, 10, 9)     # make_actor seeds of slots 0, 1, 2
SLOTS = (2, 0, 1)
P1_SEED, P2_SEED, SIM_SEED = tick.P1_SEED, tick.P2_SEED, tick.SIM_SEED
AUTORESET, FLOAT = tick.AUTORESET, tick.FLOAT
CAP = skip.CAP


def groups(n):
    return [slice(g * GROUP, min((g + 1) * GROUP, n)) for g in range((n + GROUP - 1) // GROUP)]


class Bound:
    """A pool rollout with its `slots` bound, so that the run() helpers of the single-opponent tests drive it."""

    def __init__(self, ro, slots):
        self.ro, self.slots = ro, slots

    def rollout(self, *a, **kw):
        return self.ro.rollout(*a, slots=self.slots, **kw)

    def rollout_skipped(self, *a, **kw):
        return self.ro.rollout_skipped(*a, slots=self.slots, **kw)

    def __getattr__(self, name):
        return getattr(self.ro, name)


def _sim(n, autoreset="same_step", float_mode="strict", **kw):
    from footsies_gym_amd.simulator import FootsiesSim
    return FootsiesSim(n, p2_mode="external", autoreset_mode=autoreset, float_mode=float_mode, seed=SIM_SEED, **kw)


def _actor(seed):
    import torch
    from footsies_gym_amd.rollout import make_actor
    return make_actor(device=torch.device("cuda", 0), seed=seed)


def make_pool(n, slots, actors=SLOT_ACTORS, mirror=True, **kw):
    """A remote-P2 sim, a pool holding `actors` and the rollout against it under `slots`."""
    import torch
    from footsies_gym_amd.rollout import FusedPoolSelfPlayRollout, FusedSelfPlayRollout, OpponentPool
    sim = _sim(n, **kw)
    pool = OpponentPool(sim, len(actors))
    for i, a in enumerate(actors):
        assert pool.push(_actor(a)) == i
    ro = FusedSelfPlayRollout(sim, _actor(P1_ACTOR), seed=P1_SEED, opponent_seed=P2_SEED, mirror=mirror, pool=pool)
    assert type(ro) is FusedPoolSelfPlayRollout
    return sim, Bound(ro, torch.tensor(slots, dtype=torch.uint8, device=sim.device)), pool


def make_single(n, actor, mirror=True, **kw):
    from footsies_gym_amd.rollout import FusedSelfPlayRollout
    sim = _sim(n, **kw)
    return sim, FusedSelfPlayRollout(sim, _actor(P1_ACTOR), opponent=_actor(actor), seed=P1_SEED, opponent_seed=P2_SEED,
                                     mirror=mirror)


def play(sim, ro, form, calls, max_ticks=CAP):
    """Consecutive calls (so the counters carry): per-call results, the final state, steps_taken per call."""
    runs, steps = [], []
    for m in calls:
        runs.append(tick.run(sim, ro, m) if form == "tick" else skip.run(sim, ro, m, max_ticks))
        steps.append(sim.steps_taken)
    return runs, sim.get_state(), steps


CALLS = {"tick": (48, 16), "skip": (12, 4)}


@functools.lru_cache(maxsize=None)
def single(form, n, actor, mirror=True, max_ticks=CAP):
    """The reference of the identity: one single-opponent run per (shape, opponent), shared and left unchanged."""
    sim, ro = make_single(n, actor, mirror)
    out = play(sim, ro, form, CALLS[form], max_ticks)
    sim.close()
    return out


@functools.lru_cache(maxsize=None)
def pooled(form, n, slots, mirror=True, max_ticks=CAP, actors=SLOT_ACTORS):
    sim, ro, _ = make_pool(n, list(slots), actors, mirror)
    out = play(sim, ro, form, CALLS[form], max_ticks)
    sim.close()
    return out


def assert_groups_equal(form, n, slots, mirror=True, max_ticks=CAP, actors=SLOT_ACTORS, got=None):
    """Every group of the pool run against the single run with its slot's weights, byte for byte."""
    runs, state, steps = got if got is not None else pooled(form, n, tuple(slots), mirror, max_ticks, actors)
    assert steps == list(np.cumsum(CALLS[form]))
    for g, sl in enumerate(groups(n)):
        s = min(slots[g], len(actors) - 1)
        ref_runs, ref_state, ref_steps = single(form, n, actors[s], mirror, max_ticks)
        assert ref_steps == steps
        for c, (res, ref) in enumerate(zip(runs, ref_runs)):
            assert sorted(res) == sorted(ref)
            for k in res:  # the arena axis is the last of the sample arrays, the second of the [rows][N](, 2) fields
                a, b = (res[k][..., sl], ref[k][..., sl]) if k in ("A1", "LP1", "A2", "LP2", "ticks", "capped") else (
                    res[k][:, sl], ref[k][:, sl])
                assert a.shape == b.shape and a.size and a.tobytes() == b.tobytes(), (g, c, k)
        compare_states(ref_state[sl], state[sl])


# -- 1. bitwise identity, per tick -------------------------------------------------------------------------
@pytest.mark.parametrize("n,slots,mirror", [(N, SLOTS, True), (N, SLOTS, False), (1, (1,), True)])
def test_tick_launch_equals_the_single_opponent_launches_group_by_group(n, slots, mirror):
    assert_groups_equal("tick", n, slots, mirror)
    runs, _, _ = pooled("tick", n, tuple(slots), mirror)
    assert runs[0]["A2"].shape == (48, n) and runs[1]["A2"].shape == (16, n)


# -- 2. bitwise identity, per decision ---------------------------------------------------------------------
@pytest.mark.parametrize("n,slots,max_ticks", [(N, SLOTS, CAP), (N, SLOTS, 3), (1, (1,), CAP)])
def test_decision_launch_equals_the_single_opponent_launches_group_by_group(n, slots, max_ticks):
    """Also `ticks`, `capped` and P2's [n][max_ticks][N] arrays: pre-filled with 0xFF bytes in every run, so
    equal bytes say the same entries were written with the same values."""
    assert_groups_equal("skip", n, slots, True, max_ticks)
    runs, _, _ = pooled("skip", n, tuple(slots), True, max_ticks)
    assert runs[0]["A2"].shape == (12, max_ticks, n)
    if max_ticks == 3 and n == N:
        assert any(r["capped"].any() for r in runs)
    if n == N:
        assert any((r["ticks"] > 1).any() for r in runs)


# -- 3. the oracle replays the pool launches ---------------------------------------------------------------
@pytest.mark.parametrize("autoreset,float_mode", [("same_step", "strict"), ("next_step", "strict"), ("same_step", "double")])
def test_tick_launch_replays_through_the_oracle(oracle_lib, autoreset, float_mode):
    sim, ro, _ = make_pool(N, SLOTS, autoreset=autoreset, float_mode=float_mode)
    ora = oracle_lib.Oracle(N, p2_mode=_abi.FS_P2_EXTERNAL, autoreset_mode=AUTORESET[autoreset],
                            float_mode=FLOAT[float_mode], base_seed=SIM_SEED)
    t0 = 0
    for T in CALLS["tick"]:
        tick.replay(ora, tick.run(sim, ro, T), True, autoreset == "same_step", t0)
        t0 += T
    compare_states(ora.state(), sim.get_state())
    assert sim.steps_taken == 64


@pytest.mark.parametrize("autoreset,float_mode", [("same_step", "strict"), ("next_step", "strict"), ("same_step", "double")])
def test_decision_launch_replays_through_masked_oracle_steps(oracle_lib, autoreset, float_mode):
    sim, ro, _ = make_pool(N, SLOTS, autoreset=autoreset, float_mode=float_mode)
    ora = oracle_lib.Oracle(N, p2_mode=_abi.FS_P2_EXTERNAL, autoreset_mode=AUTORESET[autoreset],
                            float_mode=FLOAT[float_mode], base_seed=SIM_SEED)
    d0 = 0
    for m in CALLS["skip"]:
        skip.replay(ora, skip.run(sim, ro, m, CAP), True, autoreset == "same_step", CAP, d0)
        d0 += m
    compare_states(ora.state(), sim.get_state())
    assert sim.steps_taken == 16


# -- 4. the actors against the restatement, P2 per group ---------------------------------------------------
def test_actors_match_the_restatement_with_each_groups_slot_weights():
    sim, ro, pool = make_pool(N, SLOTS)
    prev0 = sim.outputs_numpy()
    res = tick.run(sim, ro, 64)
    T = 64
    prev = [prev0] + [tick.rows(res, t) for t in range(T - 1)]
    f1 = np.stack([policy_ref.features(p) for p in prev])                  # [T][N][8]
    f2 = np.stack([policy_ref.features(tick.mirrored(p)) for p in prev])
    arena, counter = np.tile(np.arange(N), (T, 1)), np.repeat(np.arange(T), N).reshape(T, N)
    p1 = [p.cpu().numpy() for p in ro.params]
    m1 = skip.check_draws(p1, P1_SEED, f1.reshape(-1, 8), arena.reshape(-1), counter.reshape(-1), res["A1"].reshape(-1),
                          res["LP1"].reshape(-1))
    print("P1 |d logp| mean %.2e max %.3e" % m1)
    per_slot = {}
    for g, sl in enumerate(groups(N)):
        w = [p.cpu().numpy() for p in pool.params(SLOTS[g])]
        m2 = skip.check_draws(w, P2_SEED, f2[:, sl].reshape(-1, 8), arena[:, sl].reshape(-1), counter[:, sl].reshape(-1),
                              res["A2"][:, sl].reshape(-1), res["LP2"][:, sl].reshape(-1))
        print("group %d (slot %d): P2 |d logp| mean %.2e max %.3e" % ((g, SLOTS[g]) + m2))
        per_slot[SLOTS[g]] = w
    sim.close()
    # the three slots are three different opponents: on the same rows and the same uniforms the restatement
    # draws differently with each, and so did the device in the single-opponent runs of bar 1 (tick 0 starts
    # from the same state in all three)
    draws = []
    for s in range(3):
        lg = policy_ref.logits(per_slot[s], f2.reshape(-1, 8))
        u = policy_ref.policy_uniform(P2_SEED, arena.reshape(-1), counter.reshape(-1).astype(np.uint64))
        draws.append(policy_ref.sample(lg, u)[0])
    assert (draws[0] != draws[1]).any() and (draws[1] != draws[2]).any() and (draws[0] != draws[2]).any()
    a2 = [single("tick", N, a)[0][0]["A2"][0] for a in SLOT_ACTORS]
    assert (a2[0] != a2[1]).any() and (a2[1] != a2[2]).any() and (a2[0] != a2[2]).any()


# -- 5. assignment edge cases ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tick", "skip"])
def test_a_pool_of_one_equals_the_single_opponent_call(form):
    assert_groups_equal(form, N, (0, 0, 0), actors=(SLOT_ACTORS[0],))


@pytest.mark.parametrize("form", ["tick", "skip"])
def test_a_slot_past_the_pool_plays_the_last_slot(form):
    assert_groups_equal(form, N, (200, 3, 255))  # n_slots = 3: all three clamp to slot 2


def test_one_slot_everywhere_equals_the_single_run():
    assert_groups_equal("tick", N, (1, 1, 1))


@pytest.mark.parametrize("n,slots", [(128, (1,)), (129, (0, 2))])
def test_the_group_boundary(n, slots):
    """128 arenas are one full group (one slot byte); 129 put one arena alone in a second group."""
    assert len(groups(n)) == len(slots)
    assert_groups_equal("tick", n, slots)
    assert_groups_equal("skip", n, slots)


# -- 6. splits and geometry --------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["tick", "skip"])
def test_split_launches_change_nothing(monkeypatch, form):
    """The sample arrays are offset per launch, the slot array is not."""
    monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(5 * N))  # 48 ticks: 9 launches of 5 and one of 3
    sim, ro, _ = make_pool(N, SLOTS)
    got = play(sim, ro, form, CALLS[form])
    sim.close()
    monkeypatch.delenv("FOOTSIES_MAX_LAUNCH_ROWS")
    whole = pooled(form, N, SLOTS)
    for res, ref in zip(got[0], whole[0]):
        for k in ref:
            assert res[k].tobytes() == ref[k].tobytes(), k
    compare_states(whole[1], got[1])
    assert got[2] == whole[2]


@pytest.mark.parametrize("form", ["tick", "skip"])
def test_loaded_airborne_and_flipped_fighters(oracle_lib, form):
    n = 130
    state = random_states(n, np.random.default_rng(3), p2="external", geom_frac=0.3)
    sim, ro, _ = make_pool(n, (1, 2))
    sim.set_state(state)
    ora = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_EXTERNAL, base_seed=SIM_SEED)
    ora.set_state(state)
    if form == "tick":
        tick.replay(ora, tick.run(sim, ro, 30), True, True)
    else:
        skip.replay(ora, skip.run(sim, ro, 10, CAP), True, True, CAP)
    compare_states(ora.state(), sim.get_state())
    sim.close()


# -- 7. refusals and kernel names --------------------------------------------------------------------------
def test_refusals_and_kernel_names():
    import torch
    from footsies_gym_amd._lib import FootsiesError, lib
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, OpponentPool
    from footsies_gym_amd.simulator import FootsiesSim
    actor = _actor(1)
    L = lib()
    name_n = lambda s, n=8: L.fs_step_kernel(s.handle, n, _abi.FS_KERNEL_SELFPLAY_POOL)  # noqa: E731
    name_d = lambda s, n=8: L.fs_step_kernel(s.handle, n, _abi.FS_KERNEL_SKIP_SELFPLAY_POOL)  # noqa: E731

    # FS_E_UNSUPPORTED: the handle kinds the single-opponent calls refuse; no kernel is named for them
    for kw in (dict(p2_mode="bot"), dict(p2_mode="noop"), dict(p2_mode="external", p1_mode="bot"),
               dict(p2_mode="external", frame_delay=2)):
        s = FootsiesSim(8, seed=4, **kw)
        ro = FusedSelfPlayRollout(s, actor, pool=OpponentPool(s, 2, actor))
        slots = torch.zeros(1, dtype=torch.uint8, device=s.device)
        for call, match in ((lambda: ro.rollout(4, slots=slots), "fs_step_n_selfplay_pool"),
                            (lambda: ro.rollout_skipped(4, slots=slots), "fs_step_skip_selfplay_pool")):
            with pytest.raises(FootsiesError, match=match) as e:
                call()
            assert e.value.code == _abi.FS_E_UNSUPPORTED
        assert name_n(s) is None and name_d(s) is None and s.steps_taken == 0
        s.close()
    sim = FootsiesSim(8, p2_mode="external", seed=4)
    assert name_n(sim) == b"fsk::selfplay::k_step_n_selfplay_pool<0>" and name_n(sim, 0) is None
    assert name_d(sim) == b"fsk::selfplay::k_step_skip_pool_selfplay<0>" and name_d(sim, 0) is None
    dbl = FootsiesSim(8, p2_mode="external", float_mode="double", seed=4)
    assert name_n(dbl) == b"fsk::selfplay::k_step_n_selfplay_pool<1>"
    assert name_d(dbl) == b"fsk::selfplay::k_step_skip_pool_selfplay<1>"
    dbl.close()
    mask = np.zeros(8, np.uint8)
    mask[3] = 1
    sim.set_p2_mode("bot", mask)  # one arena's P2 switched to the bot
    assert name_n(sim) is None and name_d(sim) is None
    sim.set_p2_mode("external", mask)
    assert name_n(sim) is not None and name_d(sim) is not None

    # FS_E_INVALID: the arguments
    pool = OpponentPool(sim, 3, actor)
    ro = FusedSelfPlayRollout(sim, actor, pool=pool)
    slots = torch.zeros(1, dtype=torch.uint8, device=sim.device)
    small = torch.zeros(64, dtype=torch.uint8, device=sim.device)
    f = ["w1", "b1", "w2", "b2", "w3", "b3"]

    def arg(n_slots=3, weights=True, slot=True, actions_out=None):
        return _abi.fs_policy_pool(weights=pool.weights.data_ptr() if weights else None, n_slots=n_slots,
                                   slot=slots.data_ptr() if slot else None, seed=2, actions_out=actions_out)

    def call_n(n=4, flags=_abi.FS_SELFPLAY_MIRROR, drop1=None, p=None, null_pool=False):
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, ro.params)}, seed=1)
        return L.fs_step_n_selfplay_pool(sim.handle, n, C.byref(p1), None if null_pool else C.byref(p or arg()), flags, None)

    def call_d(n=4, flags=_abi.FS_SELFPLAY_MIRROR, max_ticks=8, drop1=None, p=None, null_pool=False):
        p1 = _abi.fs_policy(**{k: (None if k == drop1 else t.data_ptr()) for k, t in zip(f, ro.params)}, seed=1)
        return L.fs_step_skip_selfplay_pool(sim.handle, n, C.byref(p1), None if null_pool else C.byref(p or arg()), flags,
                                            max_ticks, None, None)

    for call in (call_n, call_d):
        assert call(null_pool=True) == _abi.FS_E_INVALID
        assert call(p=arg(weights=False)) == _abi.FS_E_INVALID and call(p=arg(slot=False)) == _abi.FS_E_INVALID
        assert call(p=arg(n_slots=0)) == _abi.FS_E_INVALID and call(p=arg(n_slots=257)) == _abi.FS_E_INVALID
        assert call(p=arg(n_slots=-1)) == _abi.FS_E_INVALID
        for k in f:
            assert call(drop1=k) == _abi.FS_E_INVALID
        assert call(n=0) == _abi.FS_E_INVALID and call(n=-1) == _abi.FS_E_INVALID
        assert call(flags=2) == _abi.FS_E_INVALID and call(flags=3) == _abi.FS_E_INVALID
    assert L.fs_step_n_selfplay_pool(sim.handle, 4, None, C.byref(arg()), 0, None) == _abi.FS_E_INVALID
    assert call_d(max_ticks=0) == _abi.FS_E_INVALID and call_d(max_ticks=_abi.FS_SKIP_POLICY_MAX_TICKS + 1) == _abi.FS_E_INVALID
    # n * max_ticks * N entries of P2's arrays past int32 (refused before anything is written)
    assert call_d(n=2**17, max_ticks=4096, p=arg(actions_out=small.data_ptr())) == _abi.FS_E_INVALID
    assert sim.steps_taken == 0  # nothing ran
    # the bounds of n_slots are accepted (pool.weights holds 3 slots: slot bytes are 0)
    assert call_n(p=arg(n_slots=1)) == 0 and call_d(p=arg(n_slots=1)) == 0
    assert call_n(flags=0) == 0 and call_d(flags=0) == 0
    assert sim.steps_taken == 16
    # the Python side: slots are required and checked, one opponent or a pool
    with pytest.raises(ValueError, match="slots"):
        ro.rollout(4)
    with pytest.raises(ValueError, match="slots"):
        ro.rollout(4, slots=torch.zeros(2, dtype=torch.uint8, device=sim.device))
    with pytest.raises(ValueError, match="slots"):
        ro.rollout_skipped(4, slots=torch.zeros(1, dtype=torch.int32, device=sim.device))
    with pytest.raises(ValueError, match="not both"):
        FusedSelfPlayRollout(sim, actor, opponent=actor, pool=pool)
    with pytest.raises(ValueError, match="push"):
        ro.refresh_opponent(actor)
    with pytest.raises(ValueError, match="capacity"):
        OpponentPool(sim, 257)
    assert sim.steps_taken == 16
    sim.close()


# -- 8. PPO ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,iterations", [(True, 4), ("decisions", 2)])
def test_ppo_plays_the_pool(mode, iterations):
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(256, p2_mode="external", seed=5)
    tr = PPOTrainer(sim, horizon=16, epochs=2, minibatches=4, lr=1e-2, seed=3, learner="hip", self_play=mode,
                    opponent_pool=3, opponent_refresh=1)
    current = lambda: [p.detach() for p in tr.actor.parameters()]  # noqa: E731
    same = lambda xs, ys: all(torch.equal(x, y) for x, y in zip(xs, ys))  # noqa: E731
    pool = tr.pool
    ptr = pool.weights.data_ptr()
    assert pool.capacity == 3 and pool.filled == 1 and pool.newest == 0 and same(pool.params(0), current())
    initial = [p.clone() for p in pool.params(0)]
    filled, newest, seen = [], [], []
    for it in range(iterations):
        tr.iterate()
        for k, v in tr.stats.items():
            assert bool(torch.isfinite(v.float()).all()), k
        filled.append(int(tr.stats["pool_filled"]))
        newest.append(pool.newest)
        seen.append(tr.slots.cpu().numpy())
        assert seen[-1].shape == (2,) and (seen[-1] < min(it + 1, 3)).all()  # drawn from what was filled before the push
        assert same(pool.params(pool.newest), current())  # the learner was pushed
        assert int(tr.stats["opponent_age"]) == 0
        ep, wins = tr.stats["pool_episodes"], tr.stats["pool_wins"]
        assert ep.shape == wins.shape == (3,) and ep.dtype == wins.dtype == torch.int64
        term = tr.traj["terminated"] != 0
        assert int(ep.sum()) == int(term.sum())
        assert bool((wins <= ep).all()) and bool((wins >= 0).all())
        assert int(wins.sum()) == int((term & (tr.traj["reward"] > 0)).sum())
        if it == 0:
            assert same(pool.params(0), initial) and not same(pool.params(1), initial)
        if it == 2:  # the pool was full: the oldest snapshot, the initial actor in slot 0, is overwritten
            assert not same(pool.params(0), initial)
    assert filled == [2, 3, 3, 3][:iterations] and newest == [1, 2, 0, 1][:iterations]
    assert pool.weights.data_ptr() == ptr and tr.rollout.pool is pool  # the buffer stays put
    assert sim.steps_taken == iterations * 16
    sim.close()


def test_ppo_without_a_pool_is_unchanged():
    """opponent_pool=None: stats and weights byte-identical to a trainer built without the argument."""
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.simulator import FootsiesSim
    out = []
    for kw in ({}, {"opponent_pool": None, "opponent_latest": 0.25}):
        sim = FootsiesSim(256, p2_mode="external", seed=5)
        tr = PPOTrainer(sim, horizon=16, epochs=2, minibatches=4, lr=1e-2, seed=3, learner="hip", self_play=True, **kw)
        for _ in range(2):
            tr.iterate()
        torch.cuda.synchronize()
        assert tr.pool is None and "pool_filled" not in tr.stats
        out.append(({k: v.cpu().numpy().tobytes() for k, v in tr.stats.items()},
                    [p.detach().cpu().numpy().tobytes() for p in list(tr.actor.parameters()) + list(tr.critic.parameters())]))
        sim.close()
    assert out[0] == out[1]
