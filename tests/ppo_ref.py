"""Shared pieces of the learner's tests (fs_ppo_grad / fs_ppo_eval, csrc/fs_learn.hip): the nets, the
sample tables and the references the kernels are held to.

- `nets` / `scaled_nets`: make_actor / make_critic, as drawn (weights ~ N(0, 0.3^2): no saturated
  tanh, log-probs above -9) or with every parameter multiplied by `scale`, which is where PPO takes
  them (at scale 8 most hidden units sit at +-1 and log-probs reach -110).
- `rows`: the [n, 12] table of tests/test_gpu_learn.py; `edge_rows`: the same table built from the
  float64 policy with the edges a trained policy has (rare actions taken, exact-zero features,
  ratios of e^+-8, zero advantages), always drawn on the CPU so the CPU test of this module
  (tests/test_ppo_ref.py) asserts the edges of the very rows the GPU tests run.
- `torch_reference`: ppo.py's minibatch loss through autograd in the nets' own dtype;
  `ref64`: the same on float64 copies, with the per-row log-probs and values: the reference.
"""
import copy
import functools

NAMES = ["actor.w1", "actor.b1", "actor.w2", "actor.b2", "actor.w3", "actor.b3",
         "critic.w1", "critic.b1", "critic.w2", "critic.b2", "critic.w3", "critic.b3"]
EDGE_SEED = 3       # the actor seed whose scale-8 rows reach the edges test_ppo_ref.py asserts
EDGE_STRIDE = 101   # rows [3::101] of edge_rows carry ratios of e^+-8
EDGE_LOG_RATIO = 8.0


def nets(seed, device=None):
    from footsies_gym_amd.ppo import make_critic
    from footsies_gym_amd.rollout import make_actor
    return make_actor(device=device, seed=seed), make_critic(device=device, seed=seed + 1)


def scaled_nets(seed, scale, device=None):
    """make_actor(seed) and make_critic(seed + 1) with every parameter multiplied by `scale`."""
    import torch
    actor, critic = nets(seed)
    with torch.no_grad():
        for p in list(actor.parameters()) + list(critic.parameters()):
            p.mul_(scale)
    return actor.to(device), critic.to(device)


def rows(actor, n, seed, margin=1e-3, clip=0.2):
    """[n, 12] rows whose old log-probs put ratios below, inside and above the clip range, none
    within `margin` of a clip edge: there the clipped loss's gradient jumps (the sample's policy
    term switches on or off), so any rounding difference in the forward pass can flip a sample
    and move the minibatch gradient by ~1/sqrt(n) relative -- a property of the loss, not of
    the kernel (measured with the float64 reference: tools/split_error.py)."""
    import torch
    dev = next(actor.parameters()).device
    g = torch.Generator(device=dev).manual_seed(seed)
    x = torch.rand((n, 8), generator=g, device=dev) * 2 - 0.5
    a = torch.randint(0, 8, (n,), generator=g, device=dev)
    with torch.no_grad():
        lp = torch.log_softmax(actor(x), dim=1).gather(1, a[:, None])[:, 0]
    old = lp + torch.randn(n, generator=g, device=dev) * 0.3
    for edge in (1 - clip, 1 + clip):  # ratio = exp(lp - old): move old so it sits 2 margins away
        near = (torch.exp(lp - old) - edge).abs() < margin
        old = torch.where(near, lp - torch.log(torch.full_like(old, edge + 2 * margin)), old)
    adv = torch.randn(n, generator=g, device=dev)
    adv[::17] = 0.0  # s1 == s2 == 0: torch.min's tie
    ret = torch.randn(n, generator=g, device=dev)
    return torch.cat([x, a[:, None].float(), old[:, None], adv[:, None], ret[:, None]], dim=1).contiguous()


def _loss(actor, critic, table, clip):
    import torch
    xb, ab = table[:, :8], table[:, 8].long()
    oldb, advb, retb = table[:, 9], table[:, 10], table[:, 11]
    lp_all = torch.log_softmax(actor(xb), dim=1)
    lp = lp_all.gather(1, ab[:, None])[:, 0]
    ratio = torch.exp(lp - oldb)
    pg = -torch.min(ratio * advb, torch.clamp(ratio, 1 - clip, 1 + clip) * advb).mean()
    values = critic(xb).squeeze(-1)
    vf = (values - retb).pow(2).mean()
    ent = -(lp_all.exp() * lp_all).sum(1).mean()
    return pg, vf, ent, lp, values


def torch_reference(actor, critic, table, clip, vf_coef, ent_coef, forward=False):
    """ppo.py's update loss on one minibatch, through autograd (the learner="torch" path), in the
    nets' own dtype: (grads, the three loss means), and with `forward` also the per-row log-probs
    of the taken action and the values."""
    import torch
    params = list(actor.parameters()) + list(critic.parameters())
    for p in params:
        p.grad = None
    pg, vf, ent, lp, values = _loss(actor, critic, table, clip)
    (pg + vf_coef * vf - ent_coef * ent).backward()
    grads = [p.grad.detach().clone() for p in params]
    for p in params:
        p.grad = None
    losses = torch.stack([pg, vf, ent]).detach()
    return (grads, losses, lp.detach(), values.detach()) if forward else (grads, losses)


def ref64(actor, critic, table, clip, vf_coef, ent_coef):
    """The reference: float64 deep copies of the nets, the same loss through autograd on the table
    in float64.  Returns (grads, loss means [3], log-probs of the taken actions [n], values [n])."""
    a64, c64 = copy.deepcopy(actor).double(), copy.deepcopy(critic).double()
    return torch_reference(a64, c64, table.double(), clip, vf_coef, ent_coef, forward=True)


def edge_rows(actor64, n, seed, margin, clip=0.2, scale=1.0):
    """`rows`' table with a trained policy's edges, from the float64 actor, drawn on the CPU
    (returned there, float32):
    - actions from the float64 policy on even rows (so the peaked policy's ratios are realistic)
      and uniform on odd rows (so actions of probability e^-90 are taken);
    - exact-zero features, the real observations' guard = 0 and move = 0 (x[::5, :2] = 0);
    - old = lp64 + 0.3 randn, pushed off both clip edges by `margin` as in `rows`;
    - rows [3::101]: old = lp64 -+ 8 alternately (ratios e^+8, e^-8), advantages of both signs;
    - adv[::17] = 0; returns ~ N(0, scale^2).
    Every random draw precedes the use of `margin`: two margins give the same x, actions,
    advantages and returns, and differ only in the old log-probs that were near an edge."""
    import torch
    a64 = copy.deepcopy(actor64).double().cpu()
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 8), generator=g) * 2 - 0.5
    x[::5, :2] = 0.0
    with torch.no_grad():
        lp_all = torch.log_softmax(a64(x.double()), dim=1)
    drawn = torch.multinomial(lp_all.exp(), 1, generator=g)[:, 0]
    a = torch.randint(0, 8, (n,), generator=g)
    a[::2] = drawn[::2]
    noise = torch.randn(n, generator=g, dtype=torch.float64) * 0.3
    adv = torch.randn(n, generator=g)
    ret = torch.randn(n, generator=g) * scale
    lp = lp_all.gather(1, a[:, None])[:, 0]
    old = lp + noise
    for edge in (1 - clip, 1 + clip):  # two margins away from the edge; float32 rounding of old
        near = (torch.exp(lp - old) - edge).abs() < margin  # (|old| 2^-24) stays far inside one
        old = torch.where(near, lp - torch.log(torch.full_like(old, edge + 2 * margin)), old)
    sign = torch.ones(len(old[3::EDGE_STRIDE]), dtype=torch.float64)
    sign[1::2] = -1.0
    old[3::EDGE_STRIDE] = lp[3::EDGE_STRIDE] - EDGE_LOG_RATIO * sign
    adv[::17] = 0.0
    return torch.cat([x, a[:, None].float(), old.float()[:, None], adv[:, None], ret[:, None]], dim=1).contiguous()


CLIP, VF_COEF, ENT_COEF = 0.2, 0.5, 0.01


@functools.lru_cache(maxsize=None)
def edge_case(scale, n, margin=1e-3, ent_coef=ENT_COEF):
    """One edge case, computed once per session and shared (leave it unchanged): the CPU fp32 nets
    scaled_nets(EDGE_SEED, scale), their edge_rows table (seed n) and its ref64."""
    actor, critic = scaled_nets(EDGE_SEED, scale)
    table = edge_rows(actor, n, seed=n, margin=margin, scale=scale)
    return actor, critic, table, ref64(actor, critic, table, CLIP, VF_COEF, ent_coef)


def edge_ratio_kinds(table, lp64, clip=0.2):
    """Of edge_rows' e^+-8 rows (by the float64 log-probs `lp64`): the boolean masks (clipped,
    active) over all rows.  Clipped: the clamp holds the ratio against the advantage's sign (ratio
    above the range with adv > 0, below it with adv < 0), so min() takes the clamped term and the
    row's policy gradient is zero; active: the other sign (the unclipped term is the smaller)."""
    import torch
    edge = torch.zeros(table.shape[0], dtype=torch.bool, device=table.device)
    edge[3::EDGE_STRIDE] = True
    ratio = torch.exp(lp64.double() - table[:, 9].double())
    adv = table[:, 10]
    clipped = edge & (((ratio > 1 + clip) & (adv > 0)) | ((ratio < 1 - clip) & (adv < 0)))
    active = edge & (((ratio > 1 + clip) & (adv < 0)) | ((ratio < 1 - clip) & (adv > 0)))
    return clipped, active
