"""tests/sampler_ref.py on the host: the pinned uniforms, exact_draw's range, its agreement with
policy_ref.sample away from CDF boundaries, and the zero-weight draw -- an fp32 emulation of the selection as
it associated before the rule draws action 7 (weight exactly 0) in every zero_weight_cases() case; the rule
"a half's fall-through is its last action of non-zero weight" does not."""
import numpy as np
import pytest

from tests import policy_ref
from tests import sampler_ref as S

F = np.float32
CASES = S.zero_weight_cases()
DEAD_GAP = F(-150.0)  # a dead action of the random rows: its weight underflows to 0 unless the row's maximum is below -60


def test_pinned_triples_give_the_stated_uniforms():
    for seed, arena, bits in ((3747935, 0, S.TOP), (5374434, 1, S.TOP), (1806949, 37, S.SECOND), (6245250, 63, S.SECOND)):
        assert policy_ref.policy_uniform(seed, arena, 0) == F(bits) / F(2 ** 24)
    assert F(S.TOP) / F(2 ** 24) == F(1) - F(2.0 ** -24) and F(S.SECOND) / F(2 ** 24) == F(1) - F(2.0 ** -23)
    for seed, base, local, counter, bits in S.TICK_PINS + S.SKIP_PINS:
        u = policy_ref.policy_uniform(seed, np.array([base + local]), np.uint64(counter))
        assert u.dtype == F and u[0] == F(bits) / F(2 ** 24), (seed, base, local, counter)
        assert local < S.ZERO_WEIGHT_N
    # P2's decision-tick counters name a tick after a decision's first; both bases and both uniforms occur
    assert all(counter >> 40 in (1, 2) and counter & ((1 << 40) - 1) == 1 for _, _, _, counter, _ in S.SKIP_PINS)
    for pins in (S.TICK_PINS, S.SKIP_PINS):
        assert {b for _, b, _, _, _ in pins} == {0, 45} and {bits for _, _, _, _, bits in pins} == {S.TOP, S.SECOND}
    assert len(CASES) == 8 and len({c["tick"] for c in CASES}) == 8 and len({c["skip"] for c in CASES}) == 4


def test_exact_draw_stays_below_k_at_the_top_uniform():
    seed, arena = 3747935, 0  # u = 1 - 2^-24, the largest value policy_uniform has
    for k in range(1, 9):
        live = tuple(range(8 - k, 8))
        act, logp, target = S.exact_draw(live, seed, arena, 0)
        assert target.dtype == F and target < F(k) and act == 7
        assert logp == -np.log(np.float64(k))
        # ... and so does the kernel's own arithmetic on those logits, under either rule
        for rule in ("parent", "fixed"):
            a, e, t, total = S.kernel_draw(S.live_logits(live)[None], policy_ref.policy_uniform(seed, [arena], 0), rule)
            assert total[0] == F(k) and t[0] == target and a[0] == 7
            assert sorted(e[0]) == [0.0] * (8 - k) + [1.0] * k


def test_exact_draw_is_the_kernel_arithmetic_and_the_float64_sampler_away_from_boundaries():
    arena = np.arange(45, 345, dtype=np.uint64)[None, :]
    counter = (np.arange(24, dtype=np.uint64) + (np.arange(24, dtype=np.uint64) % np.uint64(3) << np.uint64(40)))[:, None]
    for i, live in enumerate(S.LIVE_SETS):
        seed = 0xABCDE + i
        act, logp, _ = S.exact_draw(live, seed, arena, counter)
        assert act.shape == (24, 300) and np.isin(act, live).all()
        u = policy_ref.policy_uniform(seed, arena, counter).reshape(-1)
        lg = np.repeat(S.live_logits(live)[None], u.size, axis=0)
        assert np.array_equal(S.kernel_logits(S.live_logits(live)), S.live_logits(live))
        for rule in ("parent", "fixed"):  # exactly, every draw
            assert np.array_equal(S.kernel_draw(lg, u, rule)[0], act.reshape(-1)), (live, rule)
        a64, lp64, margin = policy_ref.sample(lg, u)
        # (target = u * K is rounded to float32, half an ulp of at most 2^-22 below 8, 2^-22 / K in probability:
        # only a uniform that close to a boundary may round across it)
        ok = margin > 2.0 ** -22
        assert ok.sum() >= u.size - 8
        assert np.array_equal(a64[ok], act.reshape(-1)[ok]), live
        assert np.abs(lp64[ok] - logp).max() < 1e-6  # (policy_ref.sample returns float32)
        if len(live) > 1:
            assert len(np.unique(act)) == len(live)


def test_boundary_pins_sit_on_every_threshold():
    live = tuple(range(8))
    for k, (seed, base, local, counter) in enumerate(S.BOUNDARY_PINS):
        assert local < S.BOUNDARY_N
        act, _, target = S.exact_draw(live, seed, np.array([base + local]), np.uint64(counter))
        assert target[0] == F(k) and act[0] == k  # on the threshold below action k: k is drawn, not k - 1
        u = policy_ref.policy_uniform(seed, np.array([base + local]), np.uint64(counter))
        for rule in ("parent", "fixed"):
            assert S.kernel_draw(S.live_logits(live)[None], u, rule)[0][0] == k


def test_live_sets_are_the_nineteen():
    assert len(S.LIVE_SETS) == 19 == len(set(S.LIVE_SETS))
    assert all(tuple(sorted(s)) == s and 0 <= min(s) and max(s) < 8 for s in S.LIVE_SETS)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_parent_association_draws_the_zero_weight_action_and_the_rule_does_not(case):
    lg = S.kernel_logits(case["b3"])[None]
    for seed, base, local, counter, bits in (case["tick"], case["skip"]):
        u = policy_ref.policy_uniform(seed, np.array([base + local]), np.uint64(counter))
        assert u[0] == F(bits) / F(2 ** 24)
        act, e, target, total = S.kernel_draw(lg, u, "parent")
        assert e[0, 7] == 0.0 and act[0] == 7, (act, e, target, total)  # the defect: an action of probability zero
        assert total[0] == F(1) + F(2.0 ** -23) and target[0] == F(1)
        assert set(np.nonzero(e[0])[0]) == set(case["allowed"])
        fixed = S.kernel_draw(lg, u, "fixed")[0]
        assert fixed[0] == max(case["allowed"])
    # the construction does not lean on v_exp_f32 being correctly rounded: the small weights may move by an ulp
    small = S.fast_exp(lg - lg.max())[0, 4]
    lo, hi = (2.0 ** -25.58, 2.0 ** -24) if len(case["allowed"]) == 4 else (2.0 ** -25, 2.0 ** -24)
    assert lo * (1 + 2e-7) < small < hi * (1 - 2e-7)


def test_the_rule_changes_no_draw_of_non_zero_weight():
    """Random peaked logits with dead actions: "fixed" differs from "parent" only where parent's action has
    weight 0, and never returns such an action."""
    rng = np.random.default_rng(5)
    M = 200000
    lg = (rng.standard_normal((M, 8)) * 12).astype(F)
    lg[rng.random((M, 8)) < 0.3] = DEAD_GAP
    u = np.concatenate([F(1) - np.arange(1, 5, dtype=F) * F(2.0 ** -24)] * (M // 4))
    a_par, e, _, _ = S.kernel_draw(lg, u, "parent")
    a_fix = S.kernel_draw(lg, u, "fixed")[0]
    rows = np.arange(M)
    assert (e[rows, a_fix] > 0).all()
    differ = a_par != a_fix
    assert differ.any() and (e[rows, a_par][differ] == 0).all()
    assert (e[rows, a_par] == 0).sum() == differ.sum()

