"""fs_ppo_eval / fs_ppo_grad / fs_ppo_grad_runs (csrc/fs_learn.hip) at trained-scale weights, against
float64 autograd (tests/ppo_ref.ref64), in both learner precisions.

tests/test_gpu_learn.py holds the kernels to torch fp32 autograd on freshly initialised nets, where
no tanh saturates and no probability underflows.  Here every parameter is multiplied by 3 and by 8
(ppo_ref.scaled_nets; tests/test_ppo_ref.py asserts what the rows then reach: at scale 8 half of h1
and 83 % of h2 saturated, layer-2 pre-activations of 74 -- exp2 of 2.885 x 74 is inf --, log-probs
of -108 and a taken action at -87.8), on ppo_ref.edge_rows: rare actions taken, exact-zero
features, ratios of e^+-8 with advantages of both signs, zero advantages.  n = 5000 and n = 33 (one
32-sample tile and one row).  fp32 autograd is itself too coarse a reference here (3e-6 .. 4e-5 of a
gradient tensor's largest entry), hence float64.

Every bound is 4 x a figure measured on an MI355X by `tools/split_error.py --edge-rows` and kept
in profiles/r13a_learn_edges.json (MEASURED below: per (scale, precision) the larger of the
n = 5000 and n = 33 figures).  Gradients are compared per tensor as max |d| / max |reference|,
against the largest such figure of the tensor's network; loss means as |d| / max(1, |reference|).

  scale precision   |d value|  |d log p|  margin  grad actor  grad critic  losses (policy, value, entropy)
  3     fp32        1.45e-6    1.17e-5    1e-3    3.15e-6     2.13e-7      8.1e-7  1.3e-7  1.1e-7
  3     split_bf16  4.29e-5    2.93e-4    1.2e-3  1.54e-4     6.30e-6      1.3e-4  1.5e-6  7.1e-7
  8     fp32        7.33e-6    4.81e-5    1e-3    7.95e-6     3.07e-7      5.1e-6  4.7e-8  1.6e-7
  8     split_bf16  1.89e-4    1.70e-3    6.8e-3  6.93e-4     1.55e-5      5.2e-4  7.6e-7  4.6e-6

torch fp32 on the same rows: |d value| 1.8e-6 / 6.0e-6, |d log p| 9.2e-6 / 6.4e-5, gradients 4.4e-6
/ 4.1e-5 (scale 3 / 8): the fp32 kernel is as close to float64 as torch fp32 is (0.2 x .. 1.3 x).
split_bf16 is 20 - 30 x farther and grows with the scale: each 64-wide product carries 2^-16 of
its magnitude, which grows with the weights, and the output layer multiplies what the unsaturated
units pass on by the weights again -- a property of the split, not of the tanh or softmax paths,
which stay finite.

Clip-edge margin: rows are kept max(1e-3, 4 x the measured forward |d log p|) from both clip edges
(moved, not left out: ppo_ref.edge_rows), so a rounding difference in the forward pass cannot
switch a row's policy term on or off."""
import copy

import pytest

from tests import ppo_ref

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp32", "split_bf16")
SCALES = (3, 8)
FACTOR = 4.0
# profiles/r13a_learn_edges.json, the larger of n = 5000 and n = 33 (rounded up in the last digit)
MEASURED = {
    (3, "fp32"): dict(values=1.451e-06, logp=1.170e-05, margin=1e-3, actor=3.150e-06, critic=2.130e-07,
                      loss=(8.115e-07, 1.312e-07, 1.117e-07)),
    (3, "split_bf16"): dict(values=4.292e-05, logp=2.928e-04, margin=0.0012, actor=1.539e-04, critic=6.300e-06,
                            loss=(1.318e-04, 1.540e-06, 7.056e-07)),
    (8, "fp32"): dict(values=7.333e-06, logp=4.809e-05, margin=1e-3, actor=7.955e-06, critic=3.075e-07,
                      loss=(5.146e-06, 4.657e-08, 1.576e-07)),
    (8, "split_bf16"): dict(values=1.888e-04, logp=1.698e-03, margin=0.0068, actor=6.930e-04, critic=1.553e-05,
                            loss=(5.171e-04, 7.630e-07, 4.611e-06)),
}
CLIP, VF_COEF, ENT_COEF = ppo_ref.CLIP, ppo_ref.VF_COEF, ppo_ref.ENT_COEF


def _on_gpu(actor, critic, table):
    """Copies on cuda:0 (the shared CPU case stays as it is; PPOGrad attaches .grad to what it is given)."""
    import torch
    dev = torch.device("cuda", 0)
    return copy.deepcopy(actor).to(dev), copy.deepcopy(critic).to(dev), table.to(dev)


def _rel(got, ref):
    """max |got - ref| / max |ref| per tensor, in float64 on the CPU."""
    return [float((g.double().cpu() - e).abs().max() / e.abs().max()) for g, e in zip(got, ref)]


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scale", SCALES)
def test_margins_follow_the_measured_forward_error(scale, precision):
    m = MEASURED[scale, precision]
    assert max(1e-3, FACTOR * m["logp"]) <= m["margin"] <= 0.05  # (the inside band is 0.4 wide)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [5000, 33])
@pytest.mark.parametrize("scale", SCALES)
def test_eval_matches_float64_at_scale(scale, n, precision):
    """PPOGrad.evaluate: the critic's values and the taken actions' log-probs against float64; all
    finite, no log-prob above 0 (a saturated softmax gives exactly 0)."""
    import torch
    from footsies_gym_amd.ppo import PPOGrad
    m = MEASURED[scale, precision]
    actor, critic, table, (_, _, ref_lp, ref_v) = ppo_ref.edge_case(scale, n)
    a, c, t = _on_gpu(actor, critic, table)
    x, act = t[:, :8].contiguous(), t[:, 8].to(torch.uint8).contiguous()
    v, lp = PPOGrad(a, c, precision=precision).evaluate(x, act, n)
    torch.cuda.synchronize()
    assert v.shape == (n,) and lp.shape == (n,)
    assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(lp).all())
    assert float(lp.max()) <= 0.0
    dv, dlp = float((v.double().cpu() - ref_v).abs().max()), float((lp.double().cpu() - ref_lp).abs().max())
    print("scale %d %s n=%d: max |d value| %.3e, max |d log p| %.3e" % (scale, precision, n, dv, dlp))
    assert dv <= FACTOR * m["values"], (dv, m["values"])
    assert dlp <= FACTOR * m["logp"], (dlp, m["logp"])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("n", [5000, 33])
@pytest.mark.parametrize("scale", SCALES)
def test_grad_matches_float64_at_scale(scale, n, precision):
    import torch
    from footsies_gym_amd.ppo import PPOGrad
    m = MEASURED[scale, precision]
    actor, critic, table, (ref, ref_loss, ref_lp, _) = ppo_ref.edge_case(scale, n, m["margin"])
    a, c, t = _on_gpu(actor, critic, table)
    pg = PPOGrad(a, c, precision=precision)
    loss = pg(t, CLIP, VF_COEF, ENT_COEF).clone()
    got = [p.grad.detach().clone() for p in pg.params]
    _, lp = pg.evaluate(t[:, :8].contiguous(), t[:, 8].to(torch.uint8).contiguous(), n)
    torch.cuda.synchronize()
    # no tolerance: finite, the reference's shapes
    assert bool(torch.isfinite(loss).all()) and loss.shape == (3,)
    for name, g, e in zip(ppo_ref.NAMES, got, ref):
        assert g.shape == e.shape and bool(torch.isfinite(g).all()), name
    # the rows the kernel kept (by its own log-probs): every part of the clip range, none moved across
    # an edge against the reference, and e^+-8 rows on both sides
    old = table[:, 9].double()
    ratio, ratio_ref = torch.exp(lp.double().cpu() - old), torch.exp(ref_lp - old)
    lo, hi = 1 - CLIP, 1 + CLIP
    assert torch.equal(ratio < lo, ratio_ref < lo) and torch.equal(ratio > hi, ratio_ref > hi)
    if n == 5000:
        for part in (ratio < lo, (ratio > lo) & (ratio < hi), ratio > hi):
            assert int(part.sum()) > 500
        far = ratio[3::ppo_ref.EDGE_STRIDE]
        assert int((far > 1000).sum()) >= 20 and int((far < 1e-3).sum()) >= 20
    rel = _rel(got, ref)
    dl = [float(abs(g - e) / max(1.0, abs(e))) for g, e in zip(loss.double().cpu(), ref_loss)]
    print("scale %d %s n=%d: gradient max |d| / max |ref| actor %.3e critic %.3e, losses %s" % (
        scale, precision, n, max(rel[:6]), max(rel[6:]), " ".join("%.2e" % d for d in dl)))
    for name, r in zip(ppo_ref.NAMES, rel):
        bound = FACTOR * m[name.split(".")[0]]
        assert r <= bound, (name, r, bound)
    for name, d, b in zip(("policy", "value", "entropy"), dl, m["loss"]):
        assert d <= FACTOR * b, (name, d, b)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scale", SCALES)
def test_clipped_far_rows_add_what_padding_adds(scale, precision):
    """wsel: an e^+8 row with a positive advantage and an e^-8 row with a negative one are clipped
    against their advantage -- min() takes the clamped term, whose gradient is zero.  With no
    entropy term, the actor's gradient with those rows as they are equals the gradient with their
    advantage set to 0 and their old log-prob to the current one (ratio 1, nothing to weigh),
    within the gradient bound above.  The e^+-8 rows of the other sign are not clipped: the same
    edit of those moves the gradient by far more than the bound (e^8 x adv / n per row)."""
    import torch
    from footsies_gym_amd.ppo import PPOGrad
    m = MEASURED[scale, precision]
    n = 5000
    actor, critic, table, (ref, _, ref_lp, _) = ppo_ref.edge_case(scale, n, m["margin"], 0.0)
    clipped, active = ppo_ref.edge_ratio_kinds(table, ref_lp)
    assert int(clipped.sum()) >= 20 and int(active.sum()) >= 20
    a, c, t = _on_gpu(actor, critic, table)
    pg = PPOGrad(a, c, precision=precision)

    def actor_grads(tbl):
        pg(tbl, CLIP, VF_COEF, 0.0)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(pg.grad).all())
        return [p.grad.detach().double().cpu() for p in pg.params[:6]]

    def neutral(kind):
        tbl = table.clone()
        tbl[kind, 9] = ref_lp[kind].float()
        tbl[kind, 10] = 0.0
        return tbl.to(t.device)

    as_is = actor_grads(t)
    scales = [float(e.abs().max()) for e in ref[:6]]
    bound = FACTOR * m["actor"]
    gap = [float((g - h).abs().max()) / s for g, h, s in zip(as_is, actor_grads(neutral(clipped)), scales)]
    moved = [float((g - h).abs().max()) / s for g, h, s in zip(as_is, actor_grads(neutral(active)), scales)]
    print("scale %d %s: clipped e^+-8 rows neutralised: %.3e of the largest entry; active ones: %.3e" % (
        scale, precision, max(gap), max(moved)))
    assert max(gap) <= bound, (gap, bound)
    assert min(moved) > 100 * bound, (moved, bound)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_grad_over_runs_equals_gathered_edge_rows(precision):
    """fs_ppo_grad_runs at scale 8 on the edge rows: 37 shuffled runs of 16 rows out of 4096, read in
    place, against the same rows gathered into a table first -- gradient and loss means bit for bit
    (tests/test_gpu_learn.py test_ppo_grad_over_runs_equals_gathered_rows, where it matters)."""
    import torch
    from footsies_gym_amd.ppo import PPOGrad
    total, run_len, n_runs = 4096, 16, 37
    actor, critic, table, _ = ppo_ref.edge_case(8, total, MEASURED[8, precision]["margin"])
    a, c, t = _on_gpu(actor, critic, table)
    g = torch.Generator(device="cuda").manual_seed(run_len + n_runs)
    runs = torch.randperm(total // run_len, generator=g, device="cuda")[:n_runs].contiguous()
    pg = PPOGrad(a, c, precision=precision)
    gathered = t.view(-1, run_len, 12)[runs].reshape(-1, 12).contiguous()
    loss_g = pg(gathered, CLIP, VF_COEF, ENT_COEF).clone()
    grad_g = pg.grad.clone()
    loss_r = pg(t, CLIP, VF_COEF, ENT_COEF, runs=runs, run_len=run_len).clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(grad_g).all()) and bool(grad_g.abs().max() > 0)
    assert torch.equal(grad_g, pg.grad) and torch.equal(loss_g, loss_r)
