"""tests/ppo_ref.py on the CPU: the float64 reference is finite at every scale, and the edge rows
keep the edges the GPU tests (tests/test_gpu_learn_edges.py) rely on -- asserted here from the
float64 reference alone, on the very tables those tests run (edge_rows draws on the CPU), so an
edge cannot silently vanish.  Measured with actor seed 3 (ppo_ref.EDGE_SEED) at scale 8, n = 5000:
largest |layer-2 pre-activation| 74.7 (2^(2.885 x 74.7) is inf in fp32), smallest log p -108.7
(e^-104 is below fp32's smallest denormal), smallest taken log p -87.8 (e^-87.4 is fp32's smallest
normal); at scale 3: 20.6, -35.1, -28.6; at scale 1: 4.5, -9.2, -7.9."""
import pytest

from tests import ppo_ref

SCALES = (1, 3, 8)
MARGINS = (1e-3, 0.02)


def _forward64(actor, table):
    import torch
    a64 = ppo_ref.copy.deepcopy(actor).double()
    x = table[:, :8].double()
    with torch.no_grad():
        z2 = a64[2](torch.tanh(a64[0](x)))
        return z2, torch.log_softmax(a64(x), dim=1)


@pytest.mark.parametrize("n", [5000, 33])
@pytest.mark.parametrize("scale", SCALES)
def test_ref64_is_finite_and_ratios_keep_their_margin(scale, n):
    import torch
    for margin in MARGINS:
        actor, critic, table, (grads, losses, lp, values) = ppo_ref.edge_case(scale, n, margin)
        assert table.dtype == torch.float32 and tuple(table.shape) == (n, 12) and bool(torch.isfinite(table).all())
        for name, g, p in zip(ppo_ref.NAMES, grads, list(actor.parameters()) + list(critic.parameters())):
            assert g.dtype == torch.float64 and g.shape == p.shape and bool(torch.isfinite(g).all()), name
        for t in (losses, lp, values):
            assert t.dtype == torch.float64 and bool(torch.isfinite(t).all())
        assert lp.shape == (n,) and values.shape == (n,) and float(lp.max()) <= 0.0
        # the log-probs are the float64 policy's of the table's own actions
        _, lp_all = _forward64(actor, table)
        assert torch.equal(lp, lp_all.gather(1, table[:, 8].long()[:, None])[:, 0])
        ratio = torch.exp(lp - table[:, 9].double())
        for edge in (1 - ppo_ref.CLIP, 1 + ppo_ref.CLIP):
            assert float((ratio - edge).abs().min()) >= margin, (margin, edge)
        assert bool((table[::5, :2] == 0).all()) and bool((table[::17, 10] == 0).all())
        e = ratio[3::ppo_ref.EDGE_STRIDE].log()
        want = torch.full_like(e, ppo_ref.EDGE_LOG_RATIO)
        want[1::2] = -ppo_ref.EDGE_LOG_RATIO
        assert torch.allclose(e, want, rtol=0, atol=1e-4)  # (old is stored in float32: |old| 2^-24)


@pytest.mark.parametrize("scale", SCALES)
def test_margin_moves_old_log_probs_only(scale):
    """The margin moves rows, it does not redraw them: everything but the old log-probs of the rows
    that sat near an edge is the same table."""
    import torch
    _, _, t0, _ = ppo_ref.edge_case(scale, 5000, MARGINS[0])
    _, _, t1, _ = ppo_ref.edge_case(scale, 5000, MARGINS[1])
    keep = [c for c in range(12) if c != 9]
    assert torch.equal(t0[:, keep], t1[:, keep])
    moved = t0[:, 9] != t1[:, 9]
    assert 0 < int(moved.sum()) < 0.2 * 5000


@pytest.mark.parametrize("scale", SCALES)
def test_edge_rows_cover_the_clip_range(scale):
    import torch
    for margin in MARGINS:
        _, _, table, (_, _, lp, _) = ppo_ref.edge_case(scale, 5000, margin)
        ratio = torch.exp(lp - table[:, 9].double())
        lo, hi = 1 - ppo_ref.CLIP, 1 + ppo_ref.CLIP
        for part in (ratio < lo, (ratio > lo) & (ratio < hi), ratio > hi):
            assert int(part.sum()) > 500
        clipped, active = ppo_ref.edge_ratio_kinds(table, lp)
        adv = table[:, 10]
        for kind in (clipped, active):  # e^+8 and e^-8 rows of either kind: advantages of both signs
            assert int((kind & (ratio > hi)).sum()) >= 5 and int((kind & (ratio < lo)).sum()) >= 5
            assert bool((adv[kind] > 0).any()) and bool((adv[kind] < 0).any())
        assert len(torch.unique(table[1::2, 8])) == 8  # the uniform rows take every action


def test_scale_8_rows_reach_the_saturated_and_underflowing_paths():
    import torch
    actor, _, table, (_, _, lp, _) = ppo_ref.edge_case(8, 5000)
    z2, lp_all = _forward64(actor, table)
    assert float(z2.abs().max()) > 45     # 2^(2 log2(e) x 45) overflows fp32: exp2 -> inf in tanh_hw
    assert float(lp_all.min()) < -104     # p underflows to 0 in fp32: the entropy's p lp with p = 0
    assert float(lp.min()) < -87          # a taken action below fp32's smallest normal probability
    h1 = torch.tanh(ppo_ref.copy.deepcopy(actor).double()[0](table[:, :8].double()))
    assert float((h1.abs() > 0.999).double().mean()) > 0.3 and float((torch.tanh(z2).abs() > 0.999).double().mean()) > 0.7


def test_scaled_nets_scale_every_parameter():
    import torch
    a1, c1 = ppo_ref.nets(3)
    a8, c8 = ppo_ref.scaled_nets(3, 8)
    for p, q in zip(list(a1.parameters()) + list(c1.parameters()), list(a8.parameters()) + list(c8.parameters())):
        assert torch.equal(p * 8, q)
