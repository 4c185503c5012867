"""Every in-kernel draw site and action stream with the step counter, the arena index and the seeds past 2^31,
2^32 and 2^40: the ABI carries them as uint64, and a truncation to 32 bits at any site (StepParams::t0, the tick
loops, policy_act_arena's two-halves lane read, k_hash_actions, the split-launch carry of fs_api.cpp, a ctypes
signature) would repeat or shift the sampling streams after some hours of training.

fs_steps_taken starts at S through the test hook FOOTSIES_STEPS_START.  The draws are held to
tests/sampler_ref.exact_draw with test_gpu_sampler_exact's constant-logit actors and its check() -- no margin,
sentinels in what a call leaves unwritten, its LOGP_BAR unchanged -- at counter S + k (P2 per decision:
(S + d) + (j << 40)) and arena arena_base + i; tests/test_wide_ranges.py holds those references to Python integers
at these very values.  The sampled actions, replayed through an oracle created with the same arena_base (the
replays of test_gpu_policy, test_gpu_selfplay, test_gpu_selfplay_skip and test_gpu_league), give every output row
and the final state bit for bit.

Two calls on one handle, 32 + 16 ticks or 12 + 12 decisions: from S = 2^31 - 20 and 2^32 - 20 step 20 is the first
past the boundary -- inside a launch, or (FOOTSIES_MAX_LAUNCH_ROWS) with a launch starting exactly there ("on") or
one step earlier ("before"), the other call split as well so that the wide counter is carried from launch to
launch.  From S = 2^40 - 80 a third call takes the calls without a bound across 2^40; the per-decision self-play,
pool and league calls are held to their bound there: fs_steps_taken + n < 2^40."""
import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests import sampler_ref as S
from tests import test_gpu_league as league
from tests import test_gpu_sampler_exact as X
from tests import test_gpu_selfplay as tick
from tests import test_gpu_selfplay_skip as skip
from tests.parity_utils import assert_same, compare_outputs, compare_states

pytestmark = pytest.mark.gpu

N, MAX_TICKS = X.N, X.MAX_TICKS
STARTS = {"2^31-20": 2**31 - 20, "2^32-20": 2**32 - 20, "2^40-80": 2**40 - 80, "2^40+2^33": 2**40 + 2**33}
BASES = {"2^32+45": 2**32 + 45, "2^63+128": 2**63 + 128}
BOUNDARY = 20  # steps from the first two starts to the boundary
# ticks (or decisions) per launch of each of the two calls: a launch starts at step 20 / at step 19
SPLITS = {"tick": {"on": (10, 10), "before": (19, 7)}, "decision": {"on": (4, 4), "before": (7, 7)}}
CALLS = {"tick": (32, 16), "decision": (12, 12)}
ACROSS_2_40 = {"tick": 40, "decision": 60}  # the third call from 2^40 - 80: 48 + 40 and 24 + 60 pass step 80
ROUNDS = (10, 14)  # sampler_ref.LIVE_SETS: all eight actions live (a wrong uniform shows in 7 draws of 8), a mixed set
# (start, arena_base, split): every start with both bases inside a launch, each split kind at both boundaries
CASES = [(s, b, None) for s in STARTS for b in BASES] + [
    ("2^31-20", "2^63+128", "on"), ("2^31-20", "2^32+45", "before"), ("2^32-20", "2^32+45", "on"),
    ("2^32-20", "2^63+128", "before")]
BOUNDED = [c for c in CASES if c[0] != "2^40+2^33"]  # what the per-decision self-play forms accept
IDS = lambda cases: ["%s-%s-%s" % (s, b, k or "whole") for s, b, k in cases]  # noqa: E731
P2 = {"bot": _abi.FS_P2_BOT, "external": _abi.FS_P2_EXTERNAL}


def _started(monkeypatch, p2, start, base, autoreset="same_step"):
    """A handle whose fs_steps_taken starts at `start`, its oracle with the same arena_base, the arenas' indices."""
    from footsies_gym_amd.simulator import FootsiesSim
    from oracle import binding
    monkeypatch.setenv("FOOTSIES_STEPS_START", ("0x%x" if start >> 40 else "%d") % start)  # (both spellings)
    sim = FootsiesSim(N, p2_mode=p2, seed=X.SIM_SEED, arena_base=base, autoreset_mode=autoreset)
    monkeypatch.delenv("FOOTSIES_STEPS_START")
    assert sim.steps_taken == start
    ora = binding.Oracle(N, p2_mode=P2[p2], base_seed=X.SIM_SEED, arena_base=base, autoreset_mode=tick.AUTORESET[autoreset])
    compare_states(ora.state(), sim.get_state())
    return sim, ora, np.uint64(base) + np.arange(N, dtype=np.uint64)


def _calls(kind, start, split):
    """((steps, launch limit in steps or None) per call).  A split case splits both calls, and one of its launches
    starts on the boundary ("on"), or one step before it and none on it ("before")."""
    calls = CALLS[kind] + ((ACROSS_2_40[kind],) if start == "2^40-80" else ())
    if not split:
        return tuple((n, None) for n in calls)
    limits = SPLITS[kind][split]
    first = np.cumsum((0,) + calls)
    starts = [int(at) + j for at, n, lim in zip(first, calls, limits) for j in range(0, n, lim)]
    assert all(n > lim for n, lim in zip(calls, limits))
    assert (BOUNDARY in starts) if split == "on" else (BOUNDARY - 1 in starts and BOUNDARY not in starts)
    return tuple(zip(calls, limits))


def _limit(monkeypatch, sim, steps):
    if steps:
        monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(steps * sim.num_envs))
    else:
        monkeypatch.delenv("FOOTSIES_MAX_LAUNCH_ROWS", raising=False)


def _host(traj, **samples):
    res = {k: v for k, v in zip(traj, X._np(*traj.values()))}
    res.update(zip(samples, X._np(*samples.values())))
    return res


def _decision_tick_counters(t0, n):
    """[n][MAX_TICKS][1]: P2's counter of tick j of decision d, (t0 + d) + (j << 40)."""
    d = np.uint64(t0) + np.arange(n, dtype=np.uint64)
    return (d[:, None] + (np.arange(MAX_TICKS, dtype=np.uint64)[None, :] << np.uint64(40)))[:, :, None]


def _decision_arrays(n):
    import torch
    return (torch.full((n, N), -1, dtype=torch.int32, device=X._dev()),
            torch.full((n, N), 0xFF, dtype=torch.uint8, device=X._dev()))


def _crossed(start, total):
    """The calls of a case took the counter over the boundary its start is named for."""
    s = STARTS[start]
    if start != "2^40+2^33":
        bound = {"2^31-20": 2**31, "2^32-20": 2**32, "2^40-80": 2**40}[start]
        assert s < bound <= s + total - 1, (start, total)


# -- P1's actor alone: fs_step_n_policy, fs_step_skip_policy ------------------------------------------------------
@pytest.mark.parametrize("start,base,split", CASES, ids=IDS(CASES))
def test_policy_per_tick(monkeypatch, start, base, split):
    from footsies_gym_amd.rollout import FusedPolicyRollout
    sim, ora, arena = _started(monkeypatch, "bot", STARTS[start], BASES[base])
    fig, calls, at = X.Figure(), _calls("tick", start, split), STARTS[start]
    for r, i in enumerate(ROUNDS):
        live = S.LIVE_SETS[i]
        ro = FusedPolicyRollout(sim, X._actor(live, 100 + i), seed=X.P1_SEED + i)
        for T, lim in (calls if r == 0 else calls[:1]):
            _limit(monkeypatch, sim, lim)
            traj, (a, lp) = sim.alloc_trajectory(T), X._sentinels(T, N)
            ro.rollout(T, actions=a, logp=lp, trajectory=traj)
            res = _host(traj, A1=a, LP1=lp)
            X.check(fig, "fs_step_n_policy t0=%d" % at, live, X.P1_SEED + i, X._tick_counters(at, T), res["A1"],
                    res["LP1"], arena=arena)
            for t in range(T):
                compare_outputs(ora.step(res["A1"][t]), tick.rows(res, t), step=t)
            at += T
            assert sim.steps_taken == at
    _crossed(start, sum(T for T, _ in calls))
    compare_states(ora.state(), sim.get_state())
    fig.report("fs_step_n_policy from %s, arena_base %s, split %s" % (start, base, split))
    sim.close()


@pytest.mark.parametrize("start,base,split", CASES, ids=IDS(CASES))
def test_policy_per_decision(monkeypatch, start, base, split):
    from footsies_gym_amd.rollout import FusedPolicyRollout
    sim, ora, arena = _started(monkeypatch, "bot", STARTS[start], BASES[base])
    fig, calls, at = X.Figure(), _calls("decision", start, split), STARTS[start]
    for r, i in enumerate(ROUNDS):
        live = S.LIVE_SETS[i]
        ro = FusedPolicyRollout(sim, X._actor(live, 200 + i), seed=X.P1_SEED + i)
        for D, lim in (calls if r == 0 else calls[:1]):
            _limit(monkeypatch, sim, lim)
            traj, (a, lp), (tk, cp) = sim.alloc_trajectory(D), X._sentinels(D, N), _decision_arrays(D)
            ro.rollout_skipped(D, actions=a, logp=lp, ticks=tk, capped=cp, trajectory=traj, max_ticks=MAX_TICKS)
            res = _host(traj, A1=a, LP1=lp, ticks=tk, capped=cp)
            X.check(fig, "fs_step_skip_policy t0=%d" % at, live, X.P1_SEED + i, X._tick_counters(at, D), res["A1"],
                    res["LP1"], arena=arena)
            ran = X._ticks_and_capped(res["ticks"], res["capped"])
            # the bot plays P2: the self-play replay with an input the oracle ignores on every tick that ran
            res["A2"] = np.where(ran, 0, 0xFF).astype(np.uint8)
            res["LP2"] = np.where(ran, 0, 0xFFFFFFFF).astype(np.uint32).view(np.float32)
            skip.replay(ora, res, False, True, MAX_TICKS)
            at += D
            assert sim.steps_taken == at
    _crossed(start, sum(D for D, _ in calls))
    compare_states(ora.state(), sim.get_state())
    fig.report("fs_step_skip_policy from %s, arena_base %s, split %s" % (start, base, split))
    sim.close()


# -- both actors: one opponent, a pool, a league (mirror on and off) ----------------------------------------------
FORMS = [("selfplay", True), ("selfplay_pool", True), ("league", False), ("league", True)]
FORM_IDS = ["%s-mirror%d" % f for f in FORMS]
BOTS = (0, 1, 0)  # test_gpu_sampler_exact's league: the middle group plays the in-game bot


def _league_oracle(ora, form):
    bot = league.arena_mask(BOTS if form == "league" else (0, 0, 0), N)
    if form == "league":
        assert ora.set_p2_mode(_abi.FS_P2_BOT, bot.astype(np.uint8)) == 0
    return bot


@pytest.mark.parametrize("start,base,split", CASES, ids=IDS(CASES))
@pytest.mark.parametrize("form,mirror", FORMS, ids=FORM_IDS)
def test_selfplay_per_tick(monkeypatch, form, mirror, start, base, split):
    sim, ora, arena = _started(monkeypatch, "external", STARTS[start], BASES[base])
    bot = _league_oracle(ora, form)
    fig, calls, at = X.Figure(), _calls("tick", start, split), STARTS[start]
    for r, i in enumerate(ROUNDS):
        live = S.LIVE_SETS[i]
        ro, lives2, bot_groups, kw = X._opponents(sim, form, i, X._actor(live, 300 + i), mirror)
        for T, lim in (calls if r == 0 else calls[:1]):
            _limit(monkeypatch, sim, lim)
            traj, (a, lp), (a2, lp2) = sim.alloc_trajectory(T), X._sentinels(T, N), X._sentinels(T, N)
            ro.rollout(T, actions=a, logp=lp, p2_actions=a2, p2_logp=lp2, trajectory=traj, **kw)
            res = _host(traj, A1=a, LP1=lp, A2=a2, LP2=lp2)
            what, ctr = "fs_step_n_%s mirror=%d t0=%d" % (form, mirror, at), X._tick_counters(at, T)
            X.check(fig, what + ", P1", live, X.P1_SEED + i, ctr, res["A1"], res["LP1"], arena=arena)
            X._check_p2(fig, what, lives2, bot_groups, X.P2_SEED + i, ctr, res["A2"], res["LP2"], arena=arena)
            tick.replay(ora, league.for_replay(res, bot), mirror, True)
            at += T
            assert sim.steps_taken == at
    _crossed(start, sum(T for T, _ in calls))
    compare_states(ora.state(), sim.get_state())
    fig.report("fs_step_n_%s mirror=%d from %s, arena_base %s, split %s" % (form, mirror, start, base, split))
    sim.close()


def _skip_call(sim, ro, kw, D):
    traj, (a, lp), (a2, lp2), (tk, cp) = (sim.alloc_trajectory(D), X._sentinels(D, N), X._sentinels(D, MAX_TICKS, N),
                                          _decision_arrays(D))
    ro.rollout_skipped(D, actions=a, logp=lp, ticks=tk, capped=cp, p2_actions=a2, p2_logp=lp2, trajectory=traj,
                       max_ticks=MAX_TICKS, **kw)
    return _host(traj, A1=a, LP1=lp, A2=a2, LP2=lp2, ticks=tk, capped=cp)


def _check_skip_call(fig, what, res, at, i, live, lives2, bot_groups, arena):
    D = len(res["A1"])
    X.check(fig, what + ", P1", live, X.P1_SEED + i, X._tick_counters(at, D), res["A1"], res["LP1"], arena=arena)
    ran = X._ticks_and_capped(res["ticks"], res["capped"])
    X._check_p2(fig, what, lives2, bot_groups, X.P2_SEED + i, _decision_tick_counters(at, D), res["A2"], res["LP2"], ran,
                arena=arena)
    return ran


@pytest.mark.parametrize("start,base,split", BOUNDED, ids=IDS(BOUNDED))
@pytest.mark.parametrize("form,mirror", FORMS, ids=FORM_IDS)
def test_selfplay_per_decision(monkeypatch, form, mirror, start, base, split):
    sim, ora, arena = _started(monkeypatch, "external", STARTS[start], BASES[base])
    bot = _league_oracle(ora, form)
    fig, at, later = X.Figure(), STARTS[start], False
    calls = _calls("decision", start, split)[:2]  # (no third call: these forms stop at 2^40)
    for r, i in enumerate(ROUNDS):
        live = S.LIVE_SETS[i]
        ro, lives2, bot_groups, kw = X._opponents(sim, form, i, X._actor(live, 300 + i), mirror)
        for D, lim in (calls if r == 0 else calls[:1]):
            _limit(monkeypatch, sim, lim)
            res = _skip_call(sim, ro, kw, D)
            what = "fs_step_skip_%s mirror=%d t0=%d" % (form, mirror, at)
            ran = _check_skip_call(fig, what, res, at, i, live, lives2, bot_groups, arena)
            later |= bool(ran[:, 1:][..., ~bot].any())
            skip.replay(ora, league.for_replay(res, bot), mirror, True, MAX_TICKS)
            at += D
            assert sim.steps_taken == at
    assert later, "no remote P2 drew past a decision's first tick: the (j << 40) of its counter went unseen"
    if start != "2^40-80":
        _crossed(start, sum(CALLS["decision"]))
    compare_states(ora.state(), sim.get_state())
    fig.report("fs_step_skip_%s mirror=%d from %s, arena_base %s, split %s" % (form, mirror, start, base, split))
    sim.close()


# -- the bound of the per-decision self-play, pool and league calls: fs_steps_taken + n < 2^40 ---------------------
CALL_NAME = {"selfplay": "fs_step_skip_selfplay", "selfplay_pool": "fs_step_skip_selfplay_pool",
             "league": "fs_step_skip_league"}


def _refused(sim, ro, kw, n, call):
    from footsies_gym_amd._lib import FootsiesError
    before, state = sim.steps_taken, sim.get_state()
    with pytest.raises(FootsiesError) as e:
        ro.rollout_skipped(n, max_ticks=MAX_TICKS, **kw)
    assert e.value.code == _abi.FS_E_INVALID
    assert str(e.value).endswith("%s: fs_steps_taken + n must stay below 2^40" % call), str(e.value)
    assert sim.steps_taken == before
    compare_states(state, sim.get_state())


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("form", sorted(CALL_NAME))
def test_per_decision_selfplay_stops_at_2_40(monkeypatch, form, mirror):
    """From 2^40 - 80: 80 decisions are refused and leave the handle as it was, 79 run with every draw exact --
    the last decision's counter is 2^40 - 1, P2's ((2^40 - 1) + (j << 40)) -- and then not one more is taken."""
    i, base = ROUNDS[0], BASES["2^32+45"] if mirror else BASES["2^63+128"]
    live, at = S.LIVE_SETS[i], STARTS["2^40-80"]
    sim, ora, arena = _started(monkeypatch, "external", at, base)
    bot = _league_oracle(ora, form)
    ro, lives2, bot_groups, kw = X._opponents(sim, form, i, X._actor(live, 300 + i), mirror)
    _refused(sim, ro, kw, 80, CALL_NAME[form])
    fig = X.Figure()
    res = _skip_call(sim, ro, kw, 79)
    ran = _check_skip_call(fig, "%s mirror=%d, 79 decisions to 2^40 - 1" % (CALL_NAME[form], mirror), res, at, i, live,
                           lives2, bot_groups, arena)
    assert ran[78, 1:][..., ~bot].any()  # the last decision's later ticks drew
    skip.replay(ora, league.for_replay(res, bot), mirror, True, MAX_TICKS)
    assert sim.steps_taken == 2**40 - 1
    compare_states(ora.state(), sim.get_state())
    _refused(sim, ro, kw, 1, CALL_NAME[form])
    fig.report("%s mirror=%d up to 2^40 - 1" % (CALL_NAME[form], mirror))
    sim.close()


@pytest.mark.parametrize("form", sorted(CALL_NAME))
def test_per_decision_selfplay_is_refused_past_2_40(monkeypatch, form):
    i = ROUNDS[0]
    sim, ora, _ = _started(monkeypatch, "external", STARTS["2^40+2^33"], BASES["2^32+45"])
    ro, _, _, kw = X._opponents(sim, form, i, X._actor(S.LIVE_SETS[i], 300 + i), True)
    _refused(sim, ro, kw, 1, CALL_NAME[form])
    _refused(sim, ro, kw, 12, CALL_NAME[form])
    sim.close()


# -- the synthetic action stream: fs_step_n without rows, fs_hash_actions + fs_step_n_packed ----------------------
HASH_SEED = 0x5EED


def _hashed_rows(binding, at, T, base):
    return [np.stack([binding.hash_actions(HASH_SEED, N, at + k, p, env0=base) for k in range(T)]) for p in (0, 1)]


@pytest.mark.parametrize("start,base,split", CASES, ids=IDS(CASES))
@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
def test_step_n_hashes_its_actions_at_the_wide_counter(monkeypatch, oracle_lib, autoreset, start, base, split):
    """fs_step_n with p1 = p2 = NULL: the in-kernel hash of t = S + k, env = arena_base + i."""
    sim, ora, _ = _started(monkeypatch, "external", STARTS[start], BASES[base], autoreset)
    calls, at = _calls("tick", start, split), STARTS[start]
    for T, lim in calls:
        _limit(monkeypatch, sim, lim)
        traj = sim.step_n(T, action_seed=HASH_SEED, trajectory=sim.alloc_trajectory(T))
        res = _host(traj)
        h1, h2 = _hashed_rows(oracle_lib, at, T, BASES[base])
        for t in range(T):
            compare_outputs(ora.step(h1[t], h2[t]), tick.rows(res, t), step=t, same_step=autoreset == "same_step")
        at += T
        assert sim.steps_taken == at
    _crossed(start, sum(T for T, _ in calls))
    compare_states(ora.state(), sim.get_state())
    sim.close()


@pytest.mark.parametrize("start,base,split", CASES, ids=IDS(CASES))
@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
def test_hash_actions_and_step_n_packed_at_the_wide_counter(monkeypatch, oracle_lib, autoreset, start, base, split):
    """fs_hash_actions(t0 = S + ...) gives the numpy rows, and fs_step_n_packed over them the oracle's game."""
    from footsies_gym_amd.simulator import unpack_trajectory
    sim, ora, _ = _started(monkeypatch, "external", STARTS[start], BASES[base], autoreset)
    calls, at = _calls("tick", start, split), STARTS[start]
    for T, lim in calls:
        _limit(monkeypatch, sim, lim)
        p1, p2 = sim.hash_actions(T, seed=HASH_SEED, t0=at)
        h1, h2 = _hashed_rows(oracle_lib, at, T, BASES[base])
        g1, g2 = X._np(p1, p2)
        assert_same("fs_hash_actions p1", h1, g1)
        assert_same("fs_hash_actions p2", h2, g2)
        traj = sim.step_n_packed(T, p1, p2)
        fields = unpack_trajectory(traj)
        res = dict(zip(fields, X._np(*fields.values())))
        for t in range(T):
            compare_outputs(ora.step(h1[t], h2[t]), {k: v[t] for k, v in res.items()}, step=t,
                            same_step=autoreset == "same_step")
        at += T
        assert sim.steps_taken == at
    compare_states(ora.state(), sim.get_state())
    sim.close()


@pytest.mark.parametrize("base", sorted(BASES))
def test_hash_actions_at_2_62(oracle_lib, base):
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(N, p2_mode="external", seed=X.SIM_SEED, arena_base=BASES[base])
    T, t0 = 40, 2**62
    g1, g2 = X._np(*sim.hash_actions(T, seed=HASH_SEED, t0=t0))
    h1, h2 = _hashed_rows(oracle_lib, t0, T, BASES[base])
    assert_same("fs_hash_actions p1", h1, g1)
    assert_same("fs_hash_actions p2", h2, g2)
    assert len(np.unique(g1)) == 8 and len(np.unique(g2)) == 8
    g = X._np(sim.hash_actions(T, seed=HASH_SEED, t0=t0, p2=False)[0])[0]
    assert_same("fs_hash_actions p1 alone", h1, g)
    sim.close()


# -- seeds --------------------------------------------------------------------------------------------------------
WIDE_SEEDS = [2**31, 2**32 - 1, 2**32, 2**32 + 5, 2**63, 2**64 - 1, 5, 0]
BOT_TICKS = 60


def _bot_ticks(sim, ora):
    """BOT_TICKS ticks of an idle P1 against the in-game bot, which consumes the arena's RNG."""
    import torch
    n = sim.num_envs
    idle = torch.zeros((BOT_TICKS, n), dtype=torch.uint8, device=sim.device)
    res = _host(sim.step_n(BOT_TICKS, p1=idle, trajectory=sim.alloc_trajectory(BOT_TICKS)))
    before = ora.state()["rng"].copy()
    for t in range(BOT_TICKS):
        compare_outputs(ora.step(np.zeros(n, np.uint8)), tick.rows(res, t), step=t)
    compare_states(ora.state(), sim.get_state())
    assert (ora.state()["rng"] != before).any()  # the bots drew


def test_base_seed_plus_arena_index_folds_to_32_bits(oracle_lib):
    from footsies_gym_amd.simulator import FootsiesSim
    seed, base = 2**31 + 7, 2**33 + 64
    sim = FootsiesSim(N, p2_mode="bot", seed=seed, arena_base=base)
    ora = oracle_lib.Oracle(N, p2_mode=_abi.FS_P2_BOT, base_seed=seed, arena_base=base)
    compare_states(ora.state(), sim.get_state())
    compare_outputs(ora.outputs(), sim.outputs_numpy())
    _bot_ticks(sim, ora)
    sim.close()


def test_reset_takes_the_low_32_bits_of_a_seed(oracle_lib):
    from footsies_gym_amd.simulator import FootsiesSim
    seeds = np.resize(np.array(WIDE_SEEDS, dtype=np.uint64), N)
    sim = FootsiesSim(N, p2_mode="bot", seed=3, arena_base=BASES["2^32+45"])
    ora = oracle_lib.Oracle(N, p2_mode=_abi.FS_P2_BOT, base_seed=3, arena_base=BASES["2^32+45"])
    sim.reset(seeds=seeds)
    compare_outputs(ora.reset(seeds=seeds), sim.outputs_numpy())
    compare_states(ora.state(), sim.get_state())
    rng = sim.get_state()["rng"]
    assert len({tuple(r) for r in rng.tolist()}) == 4 and np.array_equal(rng[2], rng[7])  # (2^32 is 0)
    _bot_ticks(sim, ora)
    sim.close()
