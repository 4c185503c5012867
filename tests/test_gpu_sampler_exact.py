"""The in-kernel sampler (policy_act_side, csrc/fs_policy.h) held to an exact restatement at every call site.

With W3 = 0 an actor's logits are its last bias whatever the game and the hidden layers do
(tests/sampler_ref.py), so a draw is a function of (seed, arena, counter) alone and a few lines of numpy float32
give it bit for bit: logits 0 on a live set and -200 elsewhere make every softmax weight exactly 1 or 0.  Checked
here with no margin and no draw left out, which test_gpu_policy's bars (MARGIN, LOGP_TOL: right for a bf16 MLP)
cannot do: the selection's branches on every boundary, the exchange between the lane halves, the pair-to-MFMA lane
gather, the keying by arena_base + arena, and every call site's counter -- the tick, the decision, P2's
decision + (tick << 40) -- across calls on one handle.  300 arenas from arena_base 45: three pool groups (128, 128,
44), a part-filled last wave, no arena on the lane it has from base 0.

Log-probabilities: -ln K for K live actions, float64.  K = 1 must give exactly 0.0 (log 1 and 0 - 0 are exact;
the GPU does).  For K > 1 the largest |logp + ln K| over all draws of the call-site tests was measured on an MI355X
at LOGP_MEASURED (v_log_f32 and one float32 product by ln 2); the bar is FACTOR = 4 times that.

Draws on a boundary: a random uniform puts the target exactly on a threshold once in 2^24 draws, so those are
pinned (sampler_ref.BOUNDARY_PINS: u = k / 8 with all eight live): `target < c` must be strict at every threshold.

Zero-weight draws: for sampler_ref.zero_weight_cases() -- logits whose upper-half thresholds round below the
softmax total although action 7's weight is exactly 0 -- the arena whose uniform is 1 - 2^-24 or 1 - 2^-23 must
draw an action of non-zero weight with a log-probability above -20, as P1 of fs_step_n_policy, as P2 of
fs_step_n_selfplay (plain and mirrored) and as P2 of fs_step_skip_selfplay on a decision's second or third tick.
Every other draw of those launches matches the bf16 restatement at test_gpu_policy's bars."""
import numpy as np
import pytest

from tests import policy_ref
from tests import sampler_ref as S
from tests.test_gpu_policy import LOGP_TOL, MARGIN  # the bars of the bf16 restatement, unchanged

pytestmark = pytest.mark.gpu

N, BASE = 300, 45
TICKS = (32, 16)              # two per-tick calls on one handle: the second one's counters start at 32
DECISIONS, MAX_TICKS = 12, 8  # the per-decision calls; an attack outlasts 8 ticks, so some decisions cap
P1_SEED, P2_SEED, SIM_SEED = 0x5A3D1E5, 0x0DDBA11, 21
SLOT_BYTES = (1, 200, 0)      # per group; 200 clamps to the pool's last slot
SLOT_OF_GROUP = (1, 2, 0)
FACTOR = 4.0
LOGP_MEASURED = 9.747e-8      # max |logp + ln K| over every K > 1 draw of the call-site tests, on an MI355X
LOGP_BAR = FACTOR * LOGP_MEASURED
ARENA = np.arange(BASE, BASE + N, dtype=np.uint64)
GROUPS = (slice(0, 128), slice(128, 256), slice(256, N))


def _dev():
    import torch
    return torch.device("cuda", 0)


def _sim(p2, n=N, base=BASE):
    from footsies_gym_amd.simulator import FootsiesSim
    return FootsiesSim(n, p2_mode=p2, seed=SIM_SEED, arena_base=base)


def _actor(live, hidden_seed, scale=1):
    return S.constant_logit_actor(S.live_logits(live), hidden_seed, scale, device=_dev())


def _sentinels(*shape):
    """(actions, logp) device arrays of `shape` filled with 0xFF bytes: what no draw writes."""
    import torch
    return (torch.full(shape, 0xFF, dtype=torch.uint8, device=_dev()),
            torch.full(shape, -1, dtype=torch.int32, device=_dev()).view(torch.float32))


def _np(*tensors):
    import torch
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in tensors]


class Figure:
    """The largest |logp + ln K| a test met, per K = 1 and K > 1."""

    def __init__(self):
        self.one = self.many = 0.0
        self.draws = 0

    def report(self, what):
        print("%s: %d draws exact; max |logp + ln K| %.3e (K > 1), %.1e (K = 1)" % (what, self.draws, self.many, self.one))


def check(fig, what, live, seed, counter, acts, logps, written=None, arena=ARENA):
    """`acts` / `logps` against exact_draw(live, seed, arena, counter) -- `counter` broadcasts against the arena
    axis (the last) -- at every entry of `written` (all by default); the others must hold the sentinel."""
    exp, ref, _ = S.exact_draw(live, seed, arena, counter)
    assert exp.shape == acts.shape == logps.shape, (what, exp.shape, acts.shape)
    if written is None:
        written = np.ones(acts.shape, dtype=bool)
    assert (acts[~written] == 0xFF).all() and (logps[~written].view(np.uint32) == 0xFFFFFFFF).all(), \
        "%s, live %s: an entry the call leaves untouched was written" % (what, live)
    bad = written & (acts != exp)
    if bad.any():
        at = tuple(int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s, live %s: %d of %d draws differ from exact_draw; first at %s: drew %d, exact %d" % (
            what, live, bad.sum(), written.sum(), at, acts[at], exp[at]))
    err = float(np.abs(logps[written].astype(np.float64) - ref).max()) if written.any() else 0.0
    fig.draws += int(written.sum())
    if len(live) == 1:
        fig.one = max(fig.one, err)
        assert err == 0.0, "%s, live %s: log-probability of a certain action off 0.0 by %.3e" % (what, live, err)
    else:
        fig.many = max(fig.many, err)
        assert err <= LOGP_BAR, "%s, live %s: |logp + ln %d| = %.3e above %.1e" % (what, live, len(live), err, LOGP_BAR)


def _tick_counters(t0, n):
    return (np.uint64(t0) + np.arange(n, dtype=np.uint64))[:, None]


def _decision_tick_counters(t0):
    """[DECISIONS][MAX_TICKS][1]: P2's counter of tick j of decision d, (t0 + d) + (j << 40)."""
    d = np.uint64(t0) + np.arange(DECISIONS, dtype=np.uint64)
    return (d[:, None] + (np.arange(MAX_TICKS, dtype=np.uint64)[None, :] << np.uint64(40)))[:, :, None]


def _ticks_and_capped(ticks, capped):
    assert ticks.min() >= 1 and ticks.max() <= MAX_TICKS and np.isin(capped, (0, 1)).all()
    assert (ticks[capped == 1] == MAX_TICKS).all(), "a capped decision ran fewer than max_ticks ticks"
    return np.arange(MAX_TICKS)[None, :, None] < ticks[:, None, :]  # [d][j][i]: tick j of decision d ran


def _live2(i, k=0):
    """P2's live set of round i (slot k of a pool): never P1's."""
    return S.LIVE_SETS[(i + 7 + 5 * k) % len(S.LIVE_SETS)]


# -- fs_step_n_policy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1, 8])
def test_policy_per_tick(scale):
    """P1 of fs_step_n_policy, the hidden layers at their init scale and x 8 (most units saturated): they do
    not reach the logits."""
    from footsies_gym_amd.rollout import FusedPolicyRollout
    sim, fig = _sim("bot"), Figure()
    for i, live in enumerate(S.LIVE_SETS):
        ro = FusedPolicyRollout(sim, _actor(live, 100 + i, scale), seed=P1_SEED + i)
        for T in TICKS:
            t0 = sim.steps_taken
            a, lp = _sentinels(T, N)
            ro.rollout(T, actions=a, logp=lp)
            a, lp = _np(a, lp)
            check(fig, "fs_step_n_policy x%d t0=%d" % (scale, t0), live, P1_SEED + i, _tick_counters(t0, T), a, lp)
            assert sim.steps_taken == t0 + T
    fig.report("fs_step_n_policy, hidden x%d" % scale)
    sim.close()


# -- fs_step_skip_policy ---------------------------------------------------------------------------------------
def test_policy_per_decision():
    """P1 of fs_step_skip_policy: the counter is the decision."""
    from footsies_gym_amd.rollout import FusedPolicyRollout
    import torch
    sim, fig, caps = _sim("bot"), Figure(), []
    for i, live in enumerate(S.LIVE_SETS):
        ro = FusedPolicyRollout(sim, _actor(live, 200 + i), seed=P1_SEED + i)
        t0 = sim.steps_taken
        a, lp = _sentinels(DECISIONS, N)
        tk = torch.full((DECISIONS, N), -1, dtype=torch.int32, device=_dev())
        cp = torch.full((DECISIONS, N), 0xFF, dtype=torch.uint8, device=_dev())
        ro.rollout_skipped(DECISIONS, actions=a, logp=lp, ticks=tk, capped=cp, max_ticks=MAX_TICKS)
        a, lp, tk, cp = _np(a, lp, tk, cp)
        check(fig, "fs_step_skip_policy t0=%d" % t0, live, P1_SEED + i, _tick_counters(t0, DECISIONS), a, lp)
        _ticks_and_capped(tk, cp)
        caps.append(cp)
        assert sim.steps_taken == t0 + DECISIONS
    caps = np.concatenate(caps)
    assert (caps == 1).any() and (caps == 0).any()
    fig.report("fs_step_skip_policy")
    sim.close()


# -- the self-play calls: one opponent, a pool, a league -------------------------------------------------------
def _opponents(sim, form, i, actor1, mirror):
    """(rollout, P2's live set per arena group, the groups the bot plays, extra keyword arguments of its calls)"""
    import torch
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, OpponentPool
    seeds = dict(seed=P1_SEED + i, opponent_seed=P2_SEED + i, mirror=mirror)
    if form == "selfplay":
        live2 = _live2(i)
        return FusedSelfPlayRollout(sim, actor1, opponent=_actor(live2, 400 + i), **seeds), (live2,) * 3, (), {}
    pool = OpponentPool(sim, 3)
    for k in range(3):
        assert pool.push(_actor(_live2(i, k), 500 + 3 * i + k)) == k
    assert len({_live2(i, k) for k in range(3)}) == 3
    bots = [False, True, False] if form == "league" else None
    ro = FusedSelfPlayRollout(sim, actor1, pool=pool, bots=bots, **seeds)
    slots = torch.tensor(SLOT_BYTES, dtype=torch.uint8, device=_dev())
    return ro, tuple(_live2(i, k) for k in SLOT_OF_GROUP), ((1,) if bots else ()), dict(slots=slots)


def _check_p2(fig, what, lives2, bot_groups, seed, counter, a2, lp2, written=None, arena=ARENA):
    for g, sl in enumerate(GROUPS):
        w = None if written is None else written[..., sl]
        if g in bot_groups:  # the bot plays here: nothing of P2's arrays is written
            w = np.zeros(a2[..., sl].shape, dtype=bool)
        check(fig, "%s, P2 group %d" % (what, g), lives2[g], seed, counter, a2[..., sl], lp2[..., sl], w, arena[sl])


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("form", ["selfplay", "selfplay_pool", "league"])
def test_selfplay_per_tick(form, mirror):
    """fs_step_n_selfplay / _pool / fs_step_n_league: both actors on the tick's counter, each with its own seed
    and live set; P2's stored index is the sampled one (before the Left / Right exchange of a mirrored P2)."""
    sim, fig = _sim("external"), Figure()
    for i, live in enumerate(S.LIVE_SETS):
        ro, lives2, bot_groups, kw = _opponents(sim, form, i, _actor(live, 300 + i), mirror)
        for T in TICKS:
            t0 = sim.steps_taken
            (a, lp), (a2, lp2) = _sentinels(T, N), _sentinels(T, N)
            ro.rollout(T, actions=a, logp=lp, p2_actions=a2, p2_logp=lp2, **kw)
            a, lp, a2, lp2 = _np(a, lp, a2, lp2)
            what = "fs_step_n_%s mirror=%d t0=%d" % (form, mirror, t0)
            check(fig, what + ", P1", live, P1_SEED + i, _tick_counters(t0, T), a, lp)
            _check_p2(fig, what, lives2, bot_groups, P2_SEED + i, _tick_counters(t0, T), a2, lp2)
            assert sim.steps_taken == t0 + T
    fig.report("fs_step_n_%s, mirror=%d" % (form, mirror))
    sim.close()


@pytest.mark.parametrize("mirror", [False, True])
@pytest.mark.parametrize("form", ["selfplay", "selfplay_pool", "league"])
def test_selfplay_per_decision(form, mirror):
    """fs_step_skip_selfplay / _pool / fs_step_skip_league: P1 on the decision's counter; P2 on every tick j of
    every decision with counter + (j << 40), written for exactly the ticks[d][i] ticks that ran."""
    import torch
    sim, fig, caps = _sim("external"), Figure(), []
    for i, live in enumerate(S.LIVE_SETS):
        ro, lives2, bot_groups, kw = _opponents(sim, form, i, _actor(live, 300 + i), mirror)
        t0 = sim.steps_taken
        (a, lp), (a2, lp2) = _sentinels(DECISIONS, N), _sentinels(DECISIONS, MAX_TICKS, N)
        tk = torch.full((DECISIONS, N), -1, dtype=torch.int32, device=_dev())
        cp = torch.full((DECISIONS, N), 0xFF, dtype=torch.uint8, device=_dev())
        ro.rollout_skipped(DECISIONS, actions=a, logp=lp, ticks=tk, capped=cp, p2_actions=a2, p2_logp=lp2,
                           max_ticks=MAX_TICKS, **kw)
        a, lp, a2, lp2, tk, cp = _np(a, lp, a2, lp2, tk, cp)
        what = "fs_step_skip_%s mirror=%d t0=%d" % (form, mirror, t0)
        check(fig, what + ", P1", live, P1_SEED + i, _tick_counters(t0, DECISIONS), a, lp)
        ran = _ticks_and_capped(tk, cp)
        _check_p2(fig, what, lives2, bot_groups, P2_SEED + i, _decision_tick_counters(t0), a2, lp2, ran)
        caps.append(cp)
        assert sim.steps_taken == t0 + DECISIONS
    caps = np.concatenate(caps)
    assert (caps == 1).any() and (caps == 0).any()
    fig.report("fs_step_skip_%s, mirror=%d" % (form, mirror))
    sim.close()


# -- draws on a boundary ---------------------------------------------------------------------------------------
ALL_LIVE, ATTACK = tuple(range(8)), (4,)


@pytest.mark.parametrize("site", ["policy", "skip_policy", "selfplay", "skip_selfplay"])
def test_a_target_on_a_threshold_draws_the_action_above_it(site):
    """All eight actions live and u = k / 8: target = k, exactly the threshold between actions k - 1 and k, for
    k = 0 .. 7 (sampler_ref.BOUNDARY_PINS) -- every comparison of the selection at equality, in both halves.  As
    P1 per tick and per decision, and as a mirrored P2 per tick and on the per-arena counter path."""
    from footsies_gym_amd.rollout import FusedPolicyRollout, FusedSelfPlayRollout
    n, fig = S.BOUNDARY_N, Figure()
    for k, (seed, base, local, counter) in enumerate(S.BOUNDARY_PINS):
        arena = np.arange(base, base + n, dtype=np.uint64)
        T = counter + 1
        assert S.exact_draw(ALL_LIVE, seed, arena[local], np.uint64(counter))[2] == np.float32(k)
        if site in ("policy", "skip_policy"):
            sim = _sim("bot", n, base)
            ro = FusedPolicyRollout(sim, _actor(ALL_LIVE, 600 + k), seed=seed)
            a, lp = _sentinels(T, n)
            if site == "policy":
                ro.rollout(T, actions=a, logp=lp)
            else:
                ro.rollout_skipped(T, actions=a, logp=lp, max_ticks=MAX_TICKS)
            a, lp = _np(a, lp)
            ctr, at, written = _tick_counters(0, T), (counter, local), None
        else:
            sim = _sim("external", n, base)
            ro = FusedSelfPlayRollout(sim, _actor(ATTACK, 8), opponent=_actor(ALL_LIVE, 600 + k), seed=seed ^ 0x55,
                                      opponent_seed=seed, mirror=True)
            if site == "selfplay":
                a, lp = _sentinels(T, n)
                ro.rollout(T, p2_actions=a, p2_logp=lp)
                a, lp = _np(a, lp)
                ctr, at, written = _tick_counters(0, T), (counter, local), None
            else:
                a, lp = _sentinels(T, MAX_TICKS, n)
                _, _, ticks = ro.rollout_skipped(T, p2_actions=a, p2_logp=lp, max_ticks=MAX_TICKS)
                a, lp, ticks = _np(a, lp, ticks)
                ctr = (np.arange(T, dtype=np.uint64)[:, None] +
                       (np.arange(MAX_TICKS, dtype=np.uint64)[None, :] << np.uint64(40)))[:, :, None]
                at, written = (counter, 0, local), np.arange(MAX_TICKS)[None, :, None] < ticks[:, None, :]
        assert a[at] == k, "%s: target = %d drew action %d" % (site, k, a[at])
        check(fig, "%s, u = %d/8" % (site, k), ALL_LIVE, seed, ctr, a, lp, written, arena)
        sim.close()
    fig.report("boundaries, %s" % site)


# -- zero-weight draws -----------------------------------------------------------------------------------------
ZERO = S.zero_weight_cases()


def _others_match_the_restatement(params, seed, base, counter, acts, logps, skip):
    """Every written draw but `skip` against the bf16 restatement at test_gpu_policy's bars.  `counter`
    broadcasts against the arena axis; entries still holding the sentinel did not run."""
    lg = policy_ref.logits(params, np.zeros((1, 8), dtype=np.float32))
    assert np.array_equal(lg[0], S.kernel_logits(params[5]))  # W3 = 0: the features do not matter
    arena = np.arange(base, base + acts.shape[-1], dtype=np.uint64)
    u = np.broadcast_to(policy_ref.policy_uniform(seed, arena, counter), acts.shape).reshape(-1)
    act, logp, margin = policy_ref.sample(np.repeat(lg, u.size, axis=0), u)
    got, got_lp = acts.reshape(-1), logps.reshape(-1)
    keep = got != 0xFF
    keep[np.ravel_multi_index(skip, acts.shape)] = False
    assert keep.sum() >= acts.shape[-1] - 1
    ok = keep & (margin > MARGIN)
    assert (act[ok] == got[ok]).all(), "%d of %d draws differ away from CDF boundaries" % ((act[ok] != got[ok]).sum(), ok.sum())
    same = keep & (act == got)
    assert np.abs(logp[same] - got_lp[same]).max() < LOGP_TOL


def _zero_weight_launch(case, kind):
    """One launch with `case`'s logits on the side under test.  Returns (that actor's parameters, its seed,
    arena_base, the counters, its actions, its log-probabilities, the pinned entry's index)."""
    from footsies_gym_amd.rollout import FusedPolicyRollout, FusedSelfPlayRollout
    seed, base, local, counter, _ = case["skip" if kind == "skip" else "tick"]
    n = S.ZERO_WEIGHT_N
    zero = S.constant_logit_actor(case["b3"], 7, device=_dev())
    if kind == "policy":
        sim, T = _sim("bot", n, base), counter + 2
        ro = FusedPolicyRollout(sim, zero, seed=seed)
        a, lp = _sentinels(T, n)
        ro.rollout(T, actions=a, logp=lp)
        out = (ro.params, _tick_counters(0, T)) + tuple(_np(a, lp)) + ((counter, local),)
    elif kind == "skip":
        # P1 always attacks, so its second decision runs on for ticks in which P2 keeps drawing
        sim, d, j = _sim("external", n, base), counter & ((1 << 40) - 1), counter >> 40
        ro = FusedSelfPlayRollout(sim, _actor(ATTACK, 8), opponent=zero, seed=seed ^ 0x55, opponent_seed=seed, mirror=True)
        a2, lp2 = _sentinels(d + 1, MAX_TICKS, n)
        _, _, ticks = ro.rollout_skipped(d + 1, p2_actions=a2, p2_logp=lp2, max_ticks=MAX_TICKS)
        assert int(ticks[d, local]) > j, "the pinned arena's decision ended before tick %d" % j
        ctr = (np.arange(d + 1, dtype=np.uint64)[:, None] +
               (np.arange(MAX_TICKS, dtype=np.uint64)[None, :] << np.uint64(40)))[:, :, None]
        out = (ro.params2, ctr) + tuple(_np(a2, lp2)) + ((d, j, local),)
    else:
        sim, T = _sim("external", n, base), counter + 2
        ro = FusedSelfPlayRollout(sim, _actor(ALL_LIVE, 8), opponent=zero, seed=seed ^ 0x55, opponent_seed=seed,
                                  mirror=kind == "selfplay-mirror")
        a2, lp2 = _sentinels(T, n)
        ro.rollout(T, p2_actions=a2, p2_logp=lp2)
        out = (ro.params2, _tick_counters(0, T)) + tuple(_np(a2, lp2)) + ((counter, local),)
    sim.close()
    return ([p.cpu().numpy() for p in out[0]], seed, base) + out[1:]


@pytest.mark.parametrize("kind", ["policy", "selfplay", "selfplay-mirror", "skip"])
@pytest.mark.parametrize("case", ZERO, ids=[c["name"] for c in ZERO])
def test_no_zero_weight_action_is_drawn(case, kind):
    params, seed, base, counter, acts, logps, at = _zero_weight_launch(case, kind)
    u = policy_ref.policy_uniform(seed, np.array([base + at[-1]]), np.broadcast_to(counter, acts.shape[:-1] + (1,))[at[:-1]])
    assert u[0] >= np.float32(1) - np.float32(2.0 ** -23)  # the pinned draw is the one looked at
    print("%s %s: u = 1 - %g, drew %d with logp %.3f" % (case["name"], kind, 1.0 - float(u[0]), acts[at], logps[at]))
    assert acts[at] in case["allowed"], "action %d has weight 0 (non-zero: %s), logp %.1f" % (
        acts[at], case["allowed"], logps[at])
    assert logps[at] > -20.0, logps[at]
    _others_match_the_restatement(params, seed, base, counter, acts, logps, at)
