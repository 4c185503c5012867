"""A small PPO learner over fused rollouts (BASELINE config C5: "65 536 envs driving a small
PPO actor (PyTorch-ROCm), end-to-end steps/sec with policy in the loop").

One iteration:
1. `horizon` policy-driven ticks of every arena in one kernel launch (fs_step_n_policy).
   P1's actions are sampled by the bf16 actor inside the tick loop, and every tick's
   outputs land in a [horizon][N] trajectory in HBM.
2. Features of the horizon + 1 observations, critic values, and GAE advantages, in torch on
   the same device. The observation before tick t is the output of tick t - 1 (after a
   same-step auto-reset that is the fresh round's state, so a terminal tick's successor is
   never bootstrapped through: done masks it).
3. `epochs` x `minibatches` clipped-surrogate updates of the actor and critic (fp32 Adam; the
   gradients' 64x64 hidden layer on split-bf16 MFMAs by default since round 4,
   `learner_precision="fp32"` for fp32 FMAs).  With
   `learner="hip"` (the default) each minibatch's loss and gradient come from one fused
   forward + backward kernel per network (fs_ppo_grad, csrc/fs_learn.hip) straight into the
   parameters' .grad; `learner="torch"` runs the same loss through torch autograd (the
   definition the kernel is tested against, tests/test_gpu_learn.py).  Adam is torch's.
   The importance ratio's old log-probabilities are the behaviour policy's: the log-probs the
   bf16 kernel actor sampled with (`old_logp="behaviour"`, the default), or the same network
   recomputed in fp32 (`old_logp="fp32"`, first ratio exactly 1).  Either way the iteration
   reports how far the two are apart: `kl_behaviour_fp32`, the sample estimate
   E_a~behaviour[log p_bf16(a) - log p_fp32(a)] of KL(bf16 actor || fp32 actor), and
   `logp_abs_diff`, the mean |log p_bf16(a) - log p_fp32(a)|.  The fp32 log-probs come from
   fs_ppo_eval at fp32 FMAs (FS_PPO_FP32) whatever the learner's precision; the critic values and
   the gradients use `learner_precision`, whatever `old_logp` is (`PPOTrainer.prepare`).
4. The new actor weights are copied into the rollout's device buffers (no reallocation).

Nothing leaves the GPU inside an iteration, and the simulator never waits on the host.
"""
import ctypes as C
import time

from . import _abi
from ._lib import check, lib
from .rollout import (N_ACTIONS, N_FEATURES, FusedPolicyRollout, FusedSelfPlayRollout, OpponentPool, bot_groups,
                      make_actor, mirror_features, obs_features, pool_groups)


def _torch():
    import torch
    return torch


def make_critic(hidden=64, device=None, seed=1):
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(N_FEATURES, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                        nn.Linear(hidden, 1))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    return net.to(device)


_WGRAD_CHUNK = 8192
_SHUFFLE_CHUNK = 2048  # minibatches are drawn as shuffled runs of this many consecutive samples


def _weight_grad(g, x):
    """g^T x for tall, skinny g [M, out] and x [M, in] (M ~ 2M samples, out/in <= 64): one
    batched GEMM over row chunks, then a sum over the chunks.  A single GEMM with a reduction
    dimension of millions and a 64 x 64 result leaves hipBLASLt a handful of output tiles to
    split; the batched form runs ~13x faster on MI355X (fp32, 2.1M x 64: 0.2 ms vs 2.6 ms)."""
    torch = _torch()
    M = g.shape[0]
    full = (M // _WGRAD_CHUNK) * _WGRAD_CHUNK
    out = torch.zeros((g.shape[1], x.shape[1]), dtype=g.dtype, device=g.device)
    if full:
        gc = g[:full].reshape(-1, _WGRAD_CHUNK, g.shape[1])
        xc = x[:full].reshape(-1, _WGRAD_CHUNK, x.shape[1])
        out += torch.bmm(gc.transpose(1, 2), xc).sum(0)
    if full < M:
        out += g[full:].t() @ x[full:]
    return out


def _linear_fn():
    torch = _torch()

    class SkinnyLinear(torch.autograd.Function):
        """y = x W^T + b with the weight gradient formed by `_weight_grad`."""

        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return torch.addmm(b, x, w.t())

        @staticmethod
        def backward(ctx, gy):
            x, w = ctx.saved_tensors
            gy = gy.contiguous()
            gx = gy @ w if ctx.needs_input_grad[0] else None  # (the first layer's input is data)
            return gx, _weight_grad(gy, x.contiguous()), gy.sum(0)

    return SkinnyLinear


_SKINNY = None


def mlp(net, x):
    """net(x) for an nn.Sequential of Linear / activation layers, with every Linear through
    SkinnyLinear (same values; the weight gradients take the batched path)."""
    global _SKINNY
    torch = _torch()
    if _SKINNY is None:
        _SKINNY = _linear_fn()
    for m in net:
        x = _SKINNY.apply(x, m.weight, m.bias) if isinstance(m, torch.nn.Linear) else m(x)
    return x


class PPOGrad:
    """fs_ppo_grad for an actor (8-64-64-8) and a critic (8-64-64-1): each call writes the
    minibatch gradient of PPO's loss into one flat device buffer whose views are the
    parameters' ``.grad`` (set once here), and returns the device [3] of (policy, value,
    entropy) loss means.

    precision: "fp32" (default) runs the 64x64 hidden layer on fp32 FMAs; "split_bf16"
    (FS_PPO_SPLIT_BF16) runs it on bf16 MFMAs with each fp32 operand split into a bf16 high
    and low part (hi*hi + hi*lo + lo*hi, fp32 accumulation: ~2^-16 relative per product) --
    same results to ~1e-5 relative, not bit-identical to the fp32 path."""

    PRECISIONS = {"fp32": _abi.FS_PPO_FP32, "split_bf16": _abi.FS_PPO_SPLIT_BF16}

    def __init__(self, actor, critic, precision="fp32"):
        torch = _torch()
        if precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(self.PRECISIONS))
        self.precision = precision
        self._prec = self.PRECISIONS[precision]
        self._modules = (actor, critic)
        nets = self._collect()
        dev = nets[0][0].device
        self.device = dev
        self._nets = nets
        self.params = nets[0] + nets[1]
        self._validate(self.params)
        self.grad = torch.zeros(_abi.FS_PPO_ACTOR_PARAMS + _abi.FS_PPO_CRITIC_PARAMS, dtype=torch.float32, device=dev)
        off = 0
        for p in self.params:
            p.grad = self.grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        assert off == self.grad.numel()
        self.loss = torch.zeros(3, dtype=torch.float32, device=dev)
        self.workspace = torch.empty(lib().fs_ppo_workspace_bytes(), dtype=torch.uint8, device=dev)
        self._bind()

    def _collect(self):
        """The parameters as the modules hold them now: [weight, bias] x 3 per network (a module
        whose weight was replaced -- load_state_dict(assign=True), m.weight = nn.Parameter(...) --
        yields the new tensor)."""
        torch = _torch()
        nets = []
        for net, out in zip(self._modules, (N_ACTIONS, 1)):
            lin = [m for m in net if isinstance(m, torch.nn.Linear)]
            acts = [m for m in net if not isinstance(m, torch.nn.Linear)]
            shapes = [tuple(m.weight.shape) for m in lin]
            if shapes != [(64, N_FEATURES), (64, 64), (out, 64)] or not all(isinstance(m, torch.nn.Tanh) for m in acts):
                raise ValueError("the fused learner takes 8-64-64-%d tanh MLPs; got %s" % (out, shapes))
            if any(m.bias is None for m in lin):
                raise ValueError("the fused learner needs every Linear to have a bias")
            nets.append([t for m in lin for t in (m.weight, m.bias)])
        return nets

    def _validate(self, params):
        torch = _torch()
        for t in params:
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError("the fused learner needs contiguous fp32 device parameters")
            if t.device != self.device:
                raise ValueError("parameter on %s, but the fused learner was built on %s" % (t.device, self.device))

    def _bind(self):
        """The kernels' view of the parameters: raw device pointers of every weight and bias."""
        self._mlps = [_abi.fs_mlp(*[t.data_ptr() for t in params]) for params in self._nets]
        self._ptrs = [p.data_ptr() for p in self.params]

    def _check_bindings(self):
        """Before a launch: the parameters are re-collected from the modules (a module whose weight
        or bias was replaced by a new tensor is seen), each must still be a contiguous fp32 tensor
        on this learner's device, every .grad must still be its view of the flat buffer the kernel
        writes (an optimizer's zero_grad(set_to_none=True) drops it; it is re-attached -- the
        kernel overwrites the whole buffer), and the kernel's pointers are re-read when any
        parameter moved (param.data = ..., a new Parameter)."""
        nets = self._collect()
        params = nets[0] + nets[1]
        moved = [p.data_ptr() for p in params] != self._ptrs or any(a is not b for a, b in zip(params, self.params))
        if moved:
            self._validate(params)
            self._nets, self.params = nets, params
        off = 0
        base = self.grad.data_ptr()
        for p in self.params:
            if p.grad is None or p.grad.data_ptr() != base + 4 * off or p.grad.shape != p.shape:
                p.grad = self.grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        if moved:
            self._bind()

    def evaluate(self, x, actions=None, n_logp=0, precision=None, values=True):
        """fs_ppo_eval: (critic(x) [n], log_softmax(actor(x[:n_logp]))[actions] [n_logp] or None),
        without gradient; x: device [n, 8] fp32, actions: device uint8 [n_logp].  `precision`:
        "fp32" or "split_bf16" for this call (default: the learner's own); values=False: the
        log-probs only (the critic is not run, the first result is None)."""
        torch = _torch()
        if precision is not None and precision not in self.PRECISIONS:
            raise ValueError("precision must be one of %s" % sorted(self.PRECISIONS))
        prec = self._prec if precision is None else self.PRECISIONS[precision]
        if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] != N_FEATURES or not x.is_contiguous():
            raise ValueError("x must be a contiguous [n, 8] float32 tensor")
        n = x.shape[0]
        want_values = values
        values = torch.empty(n, dtype=torch.float32, device=x.device) if want_values else None
        logp = None
        if n_logp:
            if actions is None or actions.dtype != torch.uint8 or actions.numel() < n_logp or not actions.is_contiguous():
                raise ValueError("actions must be a contiguous uint8 tensor of at least n_logp entries")
            logp = torch.empty(n_logp, dtype=torch.float32, device=x.device)
        self._check_bindings()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().fs_ppo_eval_ex(C.c_void_p(x.data_ptr()), n, C.c_void_p(actions.data_ptr() if n_logp else None),
                                   n_logp, C.byref(self._mlps[0]), C.byref(self._mlps[1]),
                                   C.c_void_p(values.data_ptr() if want_values else None),
                                   C.c_void_p(logp.data_ptr() if n_logp else None),
                                   C.c_void_p(self.workspace.data_ptr()), self.workspace.numel(), C.c_void_p(stream),
                                   prec))
        return values, logp

    def __call__(self, rows, clip, vf_coef, ent_coef, runs=None, run_len=1):
        """rows: device [n][12] fp32 (features, action, old log-prob, advantage, return).  With
        `runs` (device int64 [k]) the minibatch is the k runs rows[runs[j] * run_len :
        (runs[j] + 1) * run_len] in that order, read in place (fs_ppo_grad_runs; run_len a power
        of two): the same gradient, bit for bit, as on ``rows.view(-1, run_len, 12)[runs]``."""
        torch = _torch()
        if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 12 or not rows.is_contiguous():
            raise ValueError("rows must be a contiguous [n, 12] float32 tensor")
        self._check_bindings()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        tail = (C.byref(self._mlps[0]), C.byref(self._mlps[1]), clip, vf_coef, ent_coef,
                C.c_void_p(self.grad.data_ptr()), C.c_void_p(self.loss.data_ptr()),
                C.c_void_p(self.workspace.data_ptr()), self.workspace.numel(), C.c_void_p(stream), self._prec)
        if runs is None:
            check(lib().fs_ppo_grad_ex(C.c_void_p(rows.data_ptr()), rows.shape[0], *tail))
            return self.loss
        shift = int(run_len).bit_length() - 1
        if run_len < 1 or (1 << shift) != run_len:
            raise ValueError("run_len must be a power of two")
        if runs.dtype != torch.int64 or runs.dim() != 1 or not runs.is_contiguous() or runs.device != rows.device:
            raise ValueError("runs must be a contiguous int64 vector on the rows' device")
        check(lib().fs_ppo_grad_runs(C.c_void_p(rows.data_ptr()), rows.shape[0], C.c_void_p(runs.data_ptr()),
                                     runs.numel(), shift, *tail))
        return self.loss


def gae(rewards, values, dones, gamma, lam):
    """Generalised advantage estimation over [T][N]: values has T + 1 rows (the last one
    bootstraps); dones[t] = 1 cuts the recursion after tick t.  Returns (advantages, returns)."""
    torch = _torch()
    T = rewards.shape[0]
    keep = 1.0 - dones
    delta = rewards + gamma * values[1:] * keep - values[:-1]  # every tick's TD error at once
    coef = (gamma * lam) * keep
    adv = torch.empty_like(rewards)
    adv[T - 1] = delta[T - 1]
    for t in range(T - 2, -1, -1):  # the backward recursion: one fused multiply-add per tick
        torch.addcmul(delta[t], coef[t], adv[t + 1], out=adv[t])
    return adv, adv + values[:-1]


def _selection(sel, device, what):
    """(pointer, count or None) of a P2 selection: a contiguous int32 vector on `device`, or None (every arena)."""
    torch = _torch()
    if sel is None:
        return None, None
    if sel.dtype != torch.int32 or sel.dim() != 1 or not sel.is_contiguous() or sel.device != device or not sel.numel():
        raise ValueError("%s: sel must be a contiguous, non-empty int32 vector on %s (None: every arena)" % (what, device))
    return sel.data_ptr(), sel.numel()


def gae_device(rewards, dones, values, gamma, lam, p2=False, sel=None):
    """gae() in one launch (fs_ppo_gae): rewards [T][N] f64 and dones [T][N] u8 as the trajectory
    holds them, values [T + 1][N] f32; the TD errors in gae()'s op order, the recursion as a fused
    multiply-add (addcmul's), so the two agree to fp32 rounding of that step.

    `p2=True` (fs_ppo_gae_p2): P2's side of a zero-sum self-play trajectory over the arenas `sel` (a
    contiguous int32 device vector [n]; None: all N) -- the same launch on -rewards[:, sel] and
    dones[:, sel], gathered in the kernel; values [T + 1][n], the results [T][n], bit for bit
    gae_device on those arrays gathered first."""
    torch = _torch()
    T, N = rewards.shape
    if sel is not None and not p2:
        raise ValueError("gae_device: sel needs p2=True")
    sel_ptr, n = _selection(sel, values.device, "gae_device")
    n = N if n is None else n
    if (rewards.dtype != torch.float64 or dones.dtype != torch.uint8 or values.dtype != torch.float32
            or tuple(dones.shape) != (T, N) or tuple(values.shape) != (T + 1, n)
            or not all(t.is_contiguous() for t in (rewards, dones, values))):
        raise ValueError("gae_device: contiguous rewards f64 [T][N], dones u8 [T][N], values f32 [T+1][N] "
                         "(p2: [T+1][len(sel)])")
    adv = torch.empty((T, n), dtype=torch.float32, device=values.device)
    ret = torch.empty_like(adv)
    g = torch.tensor([gamma, gamma * lam], dtype=torch.float32)  # the f32 scalars torch's ops use
    stream = torch.cuda.current_stream(values.device).cuda_stream
    head = (C.c_void_p(rewards.data_ptr()), C.c_void_p(dones.data_ptr()), C.c_void_p(values.data_ptr()), T, N)
    tail = (float(g[0]), float(g[1]), C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr()), C.c_void_p(stream))
    if p2:
        check(lib().fs_ppo_gae_p2(*head, C.c_void_p(sel_ptr), n, *tail))
    else:
        check(lib().fs_ppo_gae(*head, *tail))
    return adv, ret


def features_device(tr, out, p2=False, sel=None):
    """obs_features of every [T][N] trajectory row in one launch (fs_ppo_features) into out
    [T][N][8] f32, bit-identical to the torch ops (each division by a host scalar is torch's
    x * f32(1 / b), the reciprocal taken in f64).

    `p2=True` (fs_ppo_features_p2): the rows as P2 sees them, of the arenas `sel` (a contiguous int32
    device vector [n]; None: all N) -- out [T][n][8] = mirror_features(obs_features(...))[:, sel],
    bit for bit; the columns of `tr` are [T][N][2] (or [N][2]: one row)."""
    torch = _torch()
    cols = (tr["guard"], tr["move"], tr["move_frame"], tr["position"])
    if sel is not None and not p2:
        raise ValueError("features_device: sel needs p2=True")
    sel_ptr, n_sel = _selection(sel, out.device, "features_device")
    n = out.numel() // N_FEATURES
    if p2:  # out rows x n_sel samples of rows x N observations
        N = cols[0].shape[-2] if cols[0].dim() >= 2 else 0
        rows = cols[0].numel() // (2 * N) if N else 0
        n_sel = N if n_sel is None else n_sel
        n, n_out = rows * N, rows * n_sel
    else:
        n_out = n
    if (out.dtype != torch.float32 or not out.is_contiguous() or out.shape[-1] != N_FEATURES
            or out.numel() != n_out * N_FEATURES
            or not all(t.is_contiguous() and t.numel() == 2 * n for t in cols)
            or cols[0].dtype != torch.uint8 or cols[1].dtype != torch.uint8
            or cols[2].dtype != torch.float32 or cols[3].dtype != torch.float32):
        raise ValueError("features_device: contiguous u8 guard / move, f32 move_frame / position [..][2], f32 out [..][8] "
                         "(p2: columns [T][N][2], out [T][len(sel)][8])")
    stream = torch.cuda.current_stream(out.device).cuda_stream
    if p2:
        check(lib().fs_ppo_features_p2(*[C.c_void_p(t.data_ptr()) for t in cols], rows, N, C.c_void_p(sel_ptr), n_sel,
                                       C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
    else:
        check(lib().fs_ppo_features(*[C.c_void_p(t.data_ptr()) for t in cols], n, C.c_void_p(out.data_ptr()),
                                    C.c_void_p(stream)))
    return out


def p2_eligible_groups(slots, newest, age, bots, groups=None):
    """Which groups of 128 arenas' P2 samples a both-sides learner may use, as a numpy bool array per group:
    exactly those whose P2 played the learner's own weights at collect time, so nothing off-policy is learnt
    from.  `age`: updates since the opponent (a pool's newest snapshot) was copied from the learner -- above 0,
    no group.  `slots` (uint8 per group, pool_assignment) and `newest`: a pool -- the groups whose slot is
    `newest`; None: a single opponent -- every group.  `bots` (bool per group, bot_groups; None: no league):
    never a bot group.  The group count is slots' or bots' length, else `groups` (default 1).  A pure host
    function."""
    import numpy as np
    if slots is not None:
        slots = np.asarray(slots).reshape(-1)
        ok = slots == int(newest)
    else:
        count = groups if groups is not None else (np.asarray(bots).size if bots is not None else 1)
        ok = np.ones(int(count), dtype=bool)
    if bots is not None:
        bots = np.asarray(bots, dtype=bool).reshape(-1)
        if bots.size != ok.size:
            raise ValueError("p2_eligible_groups: %d groups, but bots holds %d" % (ok.size, bots.size))
        ok = ok & ~bots
    if int(age) != 0:
        ok = np.zeros_like(ok)
    return ok


def p2_selection(eligible, num_envs):
    """The arenas of the eligible groups as a numpy int32 array, ascending (runs of 128 consecutive arenas; the
    last group may be partial and counts with its real size), or None when every arena is selected."""
    import numpy as np
    eligible = np.asarray(eligible, dtype=bool).reshape(-1)
    if eligible.size != pool_groups(num_envs):
        raise ValueError("p2_selection: %d arenas are %d groups, got %d" % (num_envs, pool_groups(num_envs), eligible.size))
    if eligible.all():
        return None
    return np.flatnonzero(np.repeat(eligible, _abi.FS_SELFPLAY_GROUP)[:int(num_envs)]).astype(np.int32)


def pack_rows(x, actions, old, adv, ret, out=None, stats=None):
    """fs_ppo_grad's [M, 12] sample table in one launch (fs_ppo_pack): x [M, 8] f32, actions u8
    [M], old log-probs, advantages and returns f32 [M]; the advantages normalised on the way as
    (adv - mean) / (std + 1e-8) with torch's mean and (unbiased) std -- or with `stats` (a device
    f32 [2]: mean, std), data-parallel PPO's statistics over every rank's advantages."""
    torch = _torch()
    M = x.shape[0]
    if (x.dtype != torch.float32 or tuple(x.shape) != (M, N_FEATURES) or actions.dtype != torch.uint8
            or not all(t.is_contiguous() and t.numel() == M for t in (actions, old, adv, ret))
            or not x.is_contiguous()):
        raise ValueError("pack_rows: contiguous x f32 [M, 8], actions u8 [M], old / adv / ret f32 [M]")
    if stats is None:
        stats = torch.stack([adv.mean(), adv.std()])
    rows = out if out is not None else torch.empty((M, 12), dtype=torch.float32, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    check(lib().fs_ppo_pack(C.c_void_p(x.data_ptr()), C.c_void_p(actions.data_ptr()), C.c_void_p(old.data_ptr()),
                            C.c_void_p(adv.data_ptr()), C.c_void_p(ret.data_ptr()), C.c_void_p(stats.data_ptr()), M,
                            C.c_void_p(rows.data_ptr()), C.c_void_p(stream)))
    return rows


class PPOTrainer:
    """PPO over a FootsiesSim (P2 = whatever the sim was created with).  `horizon` ticks per
    rollout, all arenas in every minibatch round.  `learner_precision` is PPOGrad's: the
    split-bf16 hidden layer by default -- against a float64 autograd reference its gradients are
    within 5e-6 of each tensor's largest entry, as close as torch's own fp32 autograd (up to
    1.1e-5; profiles/r04e_split_error.jsonl) -- or "fp32".

    `frame_skip=True` trains the way the reference does behind FootsiesFrameSkipped: `horizon` counts
    agent decisions, each rollout is one fs_step_skip_policy launch (FusedPolicyRollout.rollout_skipped,
    the handle's P2 the bot or idle), a sample is a decision -- its reward the sum over the ticks it
    ran, its done the decision's `terminated`, discounting per decision -- and `stats` gains
    `ticks_per_decision` (the mean) and `capped` (decisions closed by `max_skip_ticks`).  GAE, the
    sample table and the learners are the same; `train` then returns decisions/s.

    `self_play=True` (a sim created with p2_mode="external"; not with `frame_skip`): P1 learns exactly
    as above while P2 plays a frozen, mirrored copy of the actor inside the same launch
    (FusedSelfPlayRollout, fs_step_n_selfplay; `opponent_seed` is its sampling seed).  The copy is
    re-taken from the learner after every `opponent_refresh`-th update (1: always the latest policy),
    and `stats["opponent_age"]` holds the updates since.  P2's samples are not learnt from unless
    `both_sides=True` (below).  Data-parallel ranks hold identical weights and refresh at the same update.

    `both_sides=True` (with `self_play=True`; not with "decisions", where P2 acts per tick and P1 per decision):
    the game is treated as zero-sum and P2's samples are learnt from as well, wherever P2's weights at collect
    time are the learner's own (p2_eligible_groups): every arena while `opponent_age` is 0 at collect (always so
    with `opponent_refresh=1`), with a pool the groups that drew the newest snapshot while its age is 0, never a
    league's bot group -- nothing off-policy.  P2's observation is the mirrored feature row, its action the
    index it sampled (before swap_left_right), its old log-prob the one it sampled with, its reward P1's
    negated, its done flag P1's `terminated`, its value the same critic's on the mirrored row; a double KO, which
    the reference scores as a P1 win, therefore scores P2 a loss.  The rollout stores P2's samples only when a
    group is eligible; P2's features and GAE come from fs_ppo_features_p2 / fs_ppo_gae_p2 gathered by the
    eligible arenas, and the sample table holds P1's rows and then P2's, the advantages normalised over both.
    Minibatches stay whole runs: of the largest power of two <= 2048 consecutive rows that tiles the table over
    the minibatches (an update without P2 rows keeps the P1-only rule and is the P1-only update, bit for bit).
    `stats` gains `p2_rows` (P2's samples in the last update; 0: none was eligible) and, over P2's samples of
    the first `kl_ticks` ticks, `p2_kl_behaviour_fp32` and `p2_logp_abs_diff` (nan without P2 rows);
    `mean_reward` and the pool and bot entries stay P1's.  Under `group=` only the single-opponent form is
    taken (every rank then has the same row count); `both_sides=False` is the trainer without it, bit for bit.

    `self_play="decisions"` is both at once, the reference's FootsiesFrameSkipped over an env with a
    custom `opponent`: `horizon` counts P1's decisions as under `frame_skip=True` (capped by
    `max_skip_ticks`) while the frozen mirrored copy plays P2 on every tick, the skipped ones included,
    in one fs_step_skip_selfplay launch per rollout (FusedSelfPlayRollout.rollout_skipped).  `stats`
    holds the frame-skip and the self-play entries.  `frame_skip` is implied; `self_play=True` stays
    per tick and still refuses `frame_skip=True`.

    `opponent_pool=K` (K >= 2, with either self-play mode): P2 plays a pool of up to K past snapshots
    instead of one (rollout.OpponentPool; fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool, still one
    launch per rollout).  The pool starts with the initial actor, every `opponent_refresh`-th update pushes
    the learner's weights (over the oldest snapshot once K are held), and every collect() draws a fresh
    assignment of snapshots to groups of 128 arenas: with probability `opponent_latest` the newest, else
    uniform over the pool (OpponentPool.assign of (seed, collect count), keyed by the global group index, so
    G ranks over shards draw what one rank over all arenas would).  `stats` gains `pool_filled` and, of the
    last rollout, `pool_episodes` and `pool_wins` ([K] int64 by slot: rows with `terminated`, and those of
    them with reward > 0 -- decision rows under "decisions"); `opponent_age` is measured against the newest
    snapshot.  Under `group=` these three entries are rank-local.  `opponent_pool=None` is the
    single-opponent trainer, bit for bit.

    `opponent_bot=f` (0 < f < 1, with either self-play mode): a league.  A fraction f of the groups of 128
    arenas -- drawn once by rollout.bot_groups from (seed, the group's global index), so shards draw what one
    rank over all arenas would -- plays the in-game scripted bot for the whole run, inside the same launch
    (fs_step_n_league / fs_step_skip_league); the other groups play the pool, or the single frozen copy,
    which is then held as a one-slot OpponentPool (so the pool entries of `stats` appear with K = 1).
    `stats` gains `bot_episodes` and `bot_wins` (int64 scalars over the bot groups' rows of the last rollout:
    rows with `terminated`, and those of them with reward > 0), the run's win rate against the reference's
    yardstick; `pool_episodes` / `pool_wins` count the remote groups only.  `opponent_bot=None` is the trainer
    without it, bit for bit.

    Data-parallel (`group`: a torch.distributed process group, or "default" for the default one;
    SURVEY.md §8(e)): one trainer per rank, each over its own FootsiesSim (a ShardedSim's handle:
    its arena_base keys the actor's sampling stream, so ranks roll out different arenas), all with
    the same `num_envs`.  The ranks start from rank 0's weights; rollouts, GAE and the sample table
    stay rank-local, the advantages are normalised with the statistics of every rank's advantages
    (parallel.global_mean_std), and each minibatch's gradient -- the mean over this rank's share of
    it -- is averaged over the ranks (parallel.allreduce_mean_, one all_reduce of the flat gradient
    buffer over RCCL) before the Adam step, so every rank applies the same update to the same
    weights: G ranks x N arenas train one policy on G x N arenas' samples per iteration."""

    def __init__(self, sim, actor=None, critic=None, horizon=128, gamma=0.99, lam=0.95, epochs=2, minibatches=4,
                 lr=3e-4, clip=0.2, vf_coef=0.5, ent_coef=0.01, seed=0, old_logp="behaviour", learner="hip",
                 kl_ticks=None, learner_precision="split_bf16", group=None, frame_skip=False, max_skip_ticks=64,
                 self_play=False, opponent_refresh=1, opponent_seed=None, opponent_pool=None, opponent_latest=0.5,
                 opponent_bot=None, both_sides=False):
        torch = _torch()
        decisions = isinstance(self_play, str)
        if decisions and self_play != "decisions":
            raise ValueError("self_play must be False, True (per tick) or 'decisions', got %r" % (self_play,))
        if both_sides:
            if not self_play:
                raise ValueError("both_sides learns from P2's samples too: it needs self_play=True")
            if decisions:
                raise ValueError("both_sides takes self_play=True (per tick), not 'decisions': there P1 acts once per "
                                 "decision while P2 acts on every tick, a different decision process for each side")
            if group is not None and (opponent_pool is not None or opponent_bot is not None):
                raise ValueError("both_sides with opponent_pool or opponent_bot takes no group=: the P2 rows of a rank "
                                 "depend on its own groups' draws, so the ranks' row counts -- and with them the "
                                 "collectives they take per update -- would differ")
        if self_play and sim.p2_mode != "external":
            raise ValueError("self_play needs a sim created with p2_mode='external' (the second actor plays P2), "
                             "got %r" % (sim.p2_mode,))
        if self_play and frame_skip and not decisions:
            raise ValueError("self_play=True is per tick and takes no frame_skip=True: use self_play='decisions' "
                             "(fs_step_skip_selfplay)")
        frame_skip = frame_skip or decisions
        if self_play and int(opponent_refresh) < 1:
            raise ValueError("opponent_refresh must be >= 1, got %r" % (opponent_refresh,))
        if opponent_pool is not None:
            if not self_play:
                raise ValueError("opponent_pool needs self_play=True or 'decisions'")
            if not 2 <= int(opponent_pool) <= _abi.FS_SELFPLAY_POOL_MAX:
                raise ValueError("opponent_pool must be 2 .. %d snapshots (None: one opponent), got %r" % (
                    _abi.FS_SELFPLAY_POOL_MAX, opponent_pool))
            if not 0.0 <= float(opponent_latest) <= 1.0:
                raise ValueError("opponent_latest must be within [0, 1], got %r" % (opponent_latest,))
            if getattr(sim, "arena_base", 0) % _abi.FS_SELFPLAY_GROUP:
                raise ValueError("opponent_pool needs a sim whose arena_base is a multiple of %d, got %d" % (
                    _abi.FS_SELFPLAY_GROUP, sim.arena_base))
        if opponent_bot is not None:
            if not self_play:
                raise ValueError("opponent_bot needs self_play=True or 'decisions'")
            if not 0.0 < float(opponent_bot) < 1.0:
                raise ValueError("opponent_bot must be a fraction of the arena groups within (0, 1) (None: no bot "
                                 "groups), got %r" % (opponent_bot,))
            if getattr(sim, "arena_base", 0) % _abi.FS_SELFPLAY_GROUP:
                raise ValueError("opponent_bot needs a sim whose arena_base is a multiple of %d, got %d" % (
                    _abi.FS_SELFPLAY_GROUP, sim.arena_base))
        if old_logp not in ("behaviour", "fp32"):
            raise ValueError("old_logp must be 'behaviour' or 'fp32'")
        if frame_skip and not 1 <= int(max_skip_ticks) <= _abi.FS_SKIP_POLICY_MAX_TICKS:
            raise ValueError("max_skip_ticks must be 1 .. %d" % _abi.FS_SKIP_POLICY_MAX_TICKS)
        if learner not in ("hip", "torch"):
            raise ValueError("learner must be 'hip' or 'torch'")
        if int(epochs) < 1 or int(minibatches) < 1 or int(horizon) < 1:
            raise ValueError("PPOTrainer needs epochs >= 1, minibatches >= 1 and horizon >= 1")
        self.learner = learner
        self.old_logp = old_logp
        dev = sim.device
        self.sim = sim
        self.actor = actor if actor is not None else make_actor(device=dev, seed=seed)
        self.critic = critic if critic is not None else make_critic(device=dev, seed=seed + 1)
        self.group, self.world = None, 1
        if group is not None:
            import torch.distributed as dist
            self.group = None if group == "default" else group
            self.world = dist.get_world_size(self.group)
        if self.world > 1:
            self._join_ranks(sim.num_envs)
        self.self_play, self.opponent_refresh = bool(self_play), int(opponent_refresh)
        self._updates = self._opponent_taken = 0  # updates done; the count at which the opponent was copied
        self.pool, self.opponent_latest, self._pool_seed = None, float(opponent_latest), int(seed)
        self._collects = 0  # rollouts so far: the pool assignment's iteration
        self.bots = None  # a league: which groups of 128 arenas play the in-game bot, fixed for the run
        if opponent_bot is not None:
            self.bots = bot_groups(seed, getattr(sim, "arena_base", 0) // _abi.FS_SELFPLAY_GROUP,
                                   pool_groups(sim.num_envs), float(opponent_bot))
        if opponent_pool is not None or self.bots is not None:  # the first snapshot: the actor as it is now
            # (a league without opponent_pool: the single frozen copy as a one-slot pool, each push over it)
            self.pool = OpponentPool(sim, int(opponent_pool) if opponent_pool is not None else 1, self.actor)
            self.rollout = FusedSelfPlayRollout(sim, self.actor, seed=seed, opponent_seed=opponent_seed, mirror=True,
                                                pool=self.pool, bots=self.bots)
        elif self.self_play:  # (opponent=None: a copy of the actor as it is now)
            self.rollout = FusedSelfPlayRollout(sim, self.actor, seed=seed, opponent_seed=opponent_seed, mirror=True)
        else:
            self.rollout = FusedPolicyRollout(sim, self.actor, seed=seed)
        self.horizon, self.gamma, self.lam = horizon, gamma, lam
        # the fp32 log-probs behind kl_behaviour_fp32 / logp_abs_diff: every tick when they are
        # PPO's old log-probs, else a sample of the first `kl_ticks` ticks (all arenas)
        self.kl_ticks = horizon if old_logp == "fp32" else min(horizon, kl_ticks or max(1, horizon // 16))
        self.epochs, self.minibatches, self.clip = epochs, minibatches, clip
        self.vf_coef, self.ent_coef = vf_coef, ent_coef
        # one fused kernel per step on the device instead of ~7 foreach launches
        self.opt = torch.optim.Adam(list(self.actor.parameters()) + list(self.critic.parameters()), lr=lr,
                                    fused=dev.type == "cuda")
        self._grad = PPOGrad(self.actor, self.critic, precision=learner_precision) if learner == "hip" else None
        self.traj = sim.alloc_trajectory(horizon)
        n = sim.num_envs
        self.actions = torch.empty((horizon, n), dtype=torch.uint8, device=dev)
        self.logp = torch.empty((horizon, n), dtype=torch.float32, device=dev)
        self.frame_skip, self.max_skip_ticks = bool(frame_skip), int(max_skip_ticks)
        if self.frame_skip:  # per decision: the ticks it ran, and whether max_skip_ticks closed it
            self.ticks = torch.empty((horizon, n), dtype=torch.int32, device=dev)
            self.capped = torch.empty((horizon, n), dtype=torch.uint8, device=dev)
        self.both_sides = bool(both_sides)
        if self.both_sides:  # P2's samples of a rollout, stored where a group is eligible (allocated once)
            self.p2_actions = torch.empty((horizon, n), dtype=torch.uint8, device=dev)
            self.p2_logp = torch.empty((horizon, n), dtype=torch.float32, device=dev)
        # the last rollout's P2 block: None (no eligible group, or both_sides off), else {"sel": the eligible
        # arenas as an int32 device vector or None for all of them, "n": how many}
        self._p2 = None
        self._p2_gap = None  # prepare's fp32 log-prob gap over P2's KL samples
        self.gen = torch.Generator(device=dev)
        self.gen.manual_seed(seed)
        self.stats = {}
        # the observation before the next rollout's first tick: the sim's outputs now, then
        # the last trajectory row (trajectory launches leave the regular outputs untouched)
        self._next_first = None

    def _join_ranks(self, n):
        """Data-parallel start: the same arena count on every rank (each minibatch step is one
        collective per rank, so the ranks must take the same number of them) and rank 0's weights."""
        import torch.distributed as dist
        from .parallel import _on_backend
        torch = _torch()
        counts = [None] * self.world
        dist.all_gather_object(counts, int(n), group=self.group)
        if len(set(counts)) != 1:
            raise ValueError("data-parallel PPO needs the same num_envs on every rank, got %s" % counts)
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        with torch.no_grad():
            for p in list(self.actor.parameters()) + list(self.critic.parameters()):
                b = _on_backend(p.data, self.group)
                dist.broadcast(b, src, group=self.group)
                if b is not p.data:
                    p.data.copy_(b)

    def collect(self):
        """One fused rollout; returns (features [T+1][N][8] f32, actions u8, rewards f64, dones u8)
        as [T][N] device tensors (the trajectory's own buffers)."""
        torch = _torch()
        first = self._next_first if self._next_first is not None else obs_features(self.sim.outputs())
        pool = {}
        slots = None
        if self.pool is not None:  # this rollout's snapshot per arena group
            slots = self.pool.assignment(self._collects, self.opponent_latest, self._pool_seed)
            self.slots = torch.from_numpy(slots).to(self.sim.device)
            pool = {"slots": self.slots}
        self._collects += 1
        self._p2 = None
        if self.both_sides:  # the groups whose P2 plays the learner's own weights in this rollout (host only)
            ok = p2_eligible_groups(slots, self.pool.newest if self.pool is not None else None,
                                    self._updates - self._opponent_taken, self.bots,
                                    groups=pool_groups(self.sim.num_envs))
            if ok.any():
                sel = p2_selection(ok, self.sim.num_envs)
                self._p2 = {"sel": None if sel is None else torch.from_numpy(sel).to(self.sim.device),
                            "n": self.sim.num_envs if sel is None else int(sel.size)}
        if self._p2 is not None:  # (per tick; with a pool or a league the same call takes the slots)
            self.rollout.rollout(self.horizon, self.actions, self.logp, self.p2_actions, self.p2_logp,
                                 trajectory=self.traj, **pool)
        elif self.frame_skip:  # a row per agent decision: its last tick, the rewards of its ticks summed
            # (self_play="decisions": the same call on FusedSelfPlayRollout, P2's samples not stored)
            self.rollout.rollout_skipped(self.horizon, self.actions, self.logp, self.ticks, self.capped,
                                         trajectory=self.traj, max_ticks=self.max_skip_ticks, **pool)
        elif self.self_play and self.pool is not None:
            self.rollout.rollout(self.horizon, self.actions, self.logp, False, False, trajectory=self.traj, **pool)
        elif self.self_play:  # P2's samples are not learnt from: not stored
            self.rollout.rollout(self.horizon, self.actions, self.logp, False, False, trajectory=self.traj)
        else:
            self.rollout.rollout(self.horizon, self.actions, self.logp, trajectory=self.traj)
        cur = torch.cuda.current_stream(self.sim.device)
        if cur != self.sim.stream:  # the trajectory was written on the handle's stream
            cur.wait_stream(self.sim.stream)
        tr = self.traj
        T, N = self.horizon, self.sim.num_envs
        feats = torch.empty((T + 1, N, N_FEATURES), dtype=torch.float32, device=first.device)
        feats[0] = first
        if self._grad is not None:
            features_device(tr, feats[1:])  # obs_features of every tick, one launch
        else:
            f = feats[1:]  # each pair written into its columns
            torch.div(tr["guard"], 3.0, out=f[..., 0:2])
            torch.div(tr["move"], 16.0, out=f[..., 2:4])
            torch.div(tr["move_frame"], 55.0, out=f[..., 4:6])
            torch.div(tr["position"], 4.6, out=f[..., 6:8])
        self._next_first = feats[T]
        return feats, self.actions, tr["reward"], tr["terminated"]

    def prepare(self, feats, actions, rewards, dones):
        """The sample table of one rollout: (rows [T*N][12] -- features, action, old log-prob,
        advantage, return --, gap = behaviour log-prob - fp32 log-prob over the KL samples)."""
        torch = _torch()
        self._p2_gap = None
        if self._p2 is not None:  # both_sides, and the last rollout stored P2's samples of its eligible groups
            return self._prepare_both(feats, actions, rewards, dones)
        T, N = actions.shape
        M = T * N
        nk = self.kl_ticks * N  # samples with an fp32 log-prob (all of them in "fp32" mode)
        with torch.no_grad():
            x = feats[:T].reshape(M, N_FEATURES)
            a = actions.reshape(M)
            behav = self.logp.reshape(M)  # what the kernel sampled with (bf16 actor)
            if self._grad is not None:  # the forward passes, GAE and the sample table
                # old32 -- the fp32 reference the KL diagnostic and old_logp="fp32" are defined
                # against -- always at fp32 FMAs, whatever the learner's precision; the critic values
                # (GAE's baseline) always at the learner's own precision, whatever old_logp is (one
                # call serves both when the learner is fp32 and every sample needs its log-prob)
                if nk == M and self._grad.precision == "fp32":
                    v, old32 = self._grad.evaluate(feats.view(-1, N_FEATURES), a, nk)
                else:
                    v, _ = self._grad.evaluate(feats.view(-1, N_FEATURES))
                    _, old32 = self._grad.evaluate(x[:nk].contiguous(), a, nk, precision="fp32", values=False)
                values = v.view(T + 1, N)
                adv, ret = gae_device(rewards, dones, values, self.gamma, self.lam)
                old = behav if self.old_logp == "behaviour" else old32
                rows = pack_rows(x, a, old, adv.view(M), ret.view(M), stats=self._adv_stats(adv))
            else:
                values = self.critic(feats).squeeze(-1)  # [T+1][N]
                old32 = torch.log_softmax(self.actor(x[:nk]), dim=1).gather(1, a[:nk, None].long())[:, 0]
                adv, ret = gae(rewards.float(), values, dones.float(), self.gamma, self.lam)
                old = behav if self.old_logp == "behaviour" else old32
                adv = adv.reshape(M)
                st = self._adv_stats(adv)
                if st is None:
                    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
                else:
                    adv = (adv - st[0]) / (st[1] + 1e-8)
                rows = torch.cat([x, a[:, None].float(), old[:, None], adv[:, None], ret.reshape(M, 1)], dim=1)  # [M, 12]
            gap = behav[:nk] - old32
        return rows, gap

    def _prepare_both(self, feats, actions, rewards, dones):
        """prepare() of a rollout with eligible P2 samples: one [M1 + M2][12] table, P1's M1 = T x N rows first,
        then P2's M2 = T x n rows of the n selected arenas (tick-major like P1's), the advantages normalised
        over all of them together.  P2's observations are the mirrored rows, its rewards P1's negated, its done
        flags P1's, its values the same critic's on the mirrored rows; `gap` stays P1's, P2's goes to
        ``_p2_gap``."""
        torch = _torch()
        T, N = actions.shape
        sel, n = self._p2["sel"], self._p2["n"]
        idx = None if sel is None else sel.long()
        pick = (lambda t: t) if idx is None else (lambda t: t.index_select(1, idx))
        with torch.no_grad():
            feats2 = torch.empty((T + 1, n, N_FEATURES), dtype=torch.float32, device=feats.device)
            first2 = mirror_features(feats[0])
            feats2[0] = first2 if idx is None else first2.index_select(0, idx)
            if self._grad is not None:
                features_device(self.traj, feats2[1:], p2=True, sel=sel)
            else:
                feats2[1:] = pick(mirror_features(feats[1:]))
            sides = []  # per side: (x, actions, old log-probs, advantages, returns, gap), flat over its rows
            for f, a, behav, w in ((feats, actions.reshape(-1), self.logp.reshape(-1), N),
                                   (feats2, pick(self.p2_actions).reshape(-1), pick(self.p2_logp).reshape(-1), n)):
                p2 = f is feats2
                M, nk = T * w, self.kl_ticks * w
                x = f[:T].reshape(M, N_FEATURES)
                if self._grad is not None:  # (the same calls as prepare's, per side)
                    if nk == M and self._grad.precision == "fp32":
                        v, old32 = self._grad.evaluate(f.view(-1, N_FEATURES), a, nk)
                    else:
                        v, _ = self._grad.evaluate(f.view(-1, N_FEATURES))
                        _, old32 = self._grad.evaluate(x[:nk].contiguous(), a, nk, precision="fp32", values=False)
                    adv, ret = gae_device(rewards, dones, v.view(T + 1, w), self.gamma, self.lam, p2=p2,
                                          sel=sel if p2 else None)
                else:
                    v = self.critic(f).squeeze(-1)
                    old32 = torch.log_softmax(self.actor(x[:nk]), dim=1).gather(1, a[:nk, None].long())[:, 0]
                    r, d = (pick(-rewards), pick(dones)) if p2 else (rewards, dones)
                    adv, ret = gae(r.float(), v, d.float(), self.gamma, self.lam)
                old = behav if self.old_logp == "behaviour" else old32
                sides.append((x, a, old, adv.reshape(M), ret.reshape(M), behav[:nk] - old32))
            adv_all = torch.cat([sides[0][3], sides[1][3]])
            st = self._adv_stats(adv_all)
            if st is None:
                st = torch.stack([adv_all.mean(), adv_all.std()])
            M1 = T * N
            if self._grad is not None:  # each side packed into its part of the table, with the joint statistics
                rows = torch.empty((M1 + T * n, 12), dtype=torch.float32, device=feats.device)
                for (x, a, old, adv, ret, _), out in zip(sides, (rows[:M1], rows[M1:])):
                    pack_rows(x, a, old, adv, ret, out=out, stats=st)
            else:
                rows = torch.cat([torch.cat([x, a[:, None].float(), old[:, None], ((adv - st[0]) / (st[1] + 1e-8))[:, None],
                                             ret[:, None]], dim=1) for x, a, old, adv, ret, _ in sides])
            self._p2_gap = sides[1][5]
        return rows, sides[0][5]

    def _adv_stats(self, adv):
        """The advantage normalisation's (mean, std) over every rank (data-parallel), else None
        (this rank's own, as pack_rows / the torch learner compute them)."""
        if self.world == 1:
            return None
        from .parallel import global_mean_std
        return global_mean_std(adv, self.group)

    def _average_grads(self):
        """Data-parallel: this minibatch's gradient averaged over the ranks before the step."""
        if self.world == 1:
            return
        from .parallel import allreduce_mean_
        if self._grad is not None:
            allreduce_mean_(self._grad.grad, self.group)  # the flat buffer the .grad views share
            return
        torch = _torch()
        ps = [p for p in list(self.actor.parameters()) + list(self.critic.parameters()) if p.grad is not None]
        flat = torch.cat([p.grad.reshape(-1) for p in ps])
        allreduce_mean_(flat, self.group)
        off = 0
        for p in ps:
            p.grad.copy_(flat[off:off + p.numel()].view_as(p.grad))
            off += p.numel()

    def update(self, feats, actions, rewards, dones):
        torch = _torch()
        T, N = actions.shape
        M = T * N
        rows, gap = self.prepare(feats, actions, rewards, dones)
        # Minibatches: a random permutation of runs of _SHUFFLE_CHUNK consecutive samples (one tick,
        # that many consecutive arenas) when they tile the batch, so each minibatch is gathered as
        # whole runs (row copies) instead of 2 M scattered rows; per-sample otherwise.
        C = _SHUFFLE_CHUNK if M % (_SHUFFLE_CHUNK * self.minibatches) == 0 else 1
        if rows.shape[0] != M:  # both_sides with P2 rows: the largest power-of-two run that tiles this table
            # (a table without P2 rows keeps the rule above, so that update is the P1-only trainer's, bit for bit)
            M = rows.shape[0]
            C = _SHUFFLE_CHUNK
            while C > 1 and M % (C * self.minibatches):
                C //= 2
        runs = rows.view(M // C, C, rows.shape[1])
        nb = (M // C + self.minibatches - 1) // self.minibatches
        for _ in range(self.epochs):
            perm = torch.randperm(M // C, device=rows.device, generator=self.gen)
            for i in range(0, M // C, nb):
                if self._grad is not None:  # fused forward + backward straight into .grad, the runs read in place
                    lm = self._grad(rows, self.clip, self.vf_coef, self.ent_coef, runs=perm[i:i + nb], run_len=C)
                    self._average_grads()
                    self.opt.step()
                    continue
                b = runs[perm[i:i + nb]].view(-1, rows.shape[1])
                xb, ab = b[:, :N_FEATURES], b[:, N_FEATURES].long()
                oldb, advb, retb = b[:, N_FEATURES + 1], b[:, N_FEATURES + 2], b[:, N_FEATURES + 3]
                logits = mlp(self.actor, xb)
                lp_all = torch.log_softmax(logits, dim=1)
                lp = lp_all.gather(1, ab[:, None])[:, 0]
                ratio = torch.exp(lp - oldb)
                s1, s2 = ratio * advb, torch.clamp(ratio, 1 - self.clip, 1 + self.clip) * advb
                pg = -torch.min(s1, s2).mean()
                vf = (mlp(self.critic, xb).squeeze(-1) - retb).pow(2).mean()
                ent = -(lp_all.exp() * lp_all).sum(1).mean()
                loss = pg + self.vf_coef * vf - self.ent_coef * ent
                self.opt.zero_grad(set_to_none=True)
                loss.backward()
                self._average_grads()
                self.opt.step()
        self.rollout.refresh(self.actor)
        self._updates += 1
        pool_stats = self._pool_stats(rewards, dones) if self.pool is not None else {}  # (before the push)
        bot_stats = self._bot_stats(rewards, dones) if self.bots is not None else {}
        if self.self_play and self._updates % self.opponent_refresh == 0:  # (every rank at the same update)
            if self.pool is not None:
                self.pool.push(self.actor)
            else:
                self.rollout.refresh_opponent(self.actor)
            self._opponent_taken = self._updates
        if self._grad is not None:
            pg, vf, ent = lm[0].clone(), lm[1].clone(), lm[2].clone()
            loss = pg + self.vf_coef * vf - self.ent_coef * ent
        if self.world > 1:  # the last minibatch's losses, averaged like its gradient
            from .parallel import allreduce_mean_
            torch = _torch()
            red = allreduce_mean_(torch.stack([loss.detach(), pg.detach(), vf.detach(), ent.detach()]), self.group)
            loss, pg, vf, ent = red[0], red[1], red[2], red[3]
        self.stats = {"loss": loss.detach(), "policy_loss": pg.detach(), "value_loss": vf.detach(),
                      "entropy": ent.detach(), "mean_reward": rewards.mean(), "kl_behaviour_fp32": gap.mean(),
                      "logp_abs_diff": gap.abs().mean()}
        if self.frame_skip:
            self.stats["ticks_per_decision"] = self.ticks.float().mean()
            self.stats["capped"] = self.capped.sum()
        if self.self_play:  # updates since the opponent's weights were copied from the learner
            self.stats["opponent_age"] = torch.tensor(self._updates - self._opponent_taken)
        if self.both_sides:  # P2's samples in this update (0: no group was eligible; its two diagnostics are then nan)
            p2_gap = self._p2_gap if self._p2_gap is not None else torch.full((1,), float("nan"), device=rows.device)
            self.stats.update(p2_rows=torch.tensor(rows.shape[0] - T * N), p2_kl_behaviour_fp32=p2_gap.mean(),
                              p2_logp_abs_diff=p2_gap.abs().mean())
        if self.pool is not None:
            self.stats.update(pool_stats, pool_filled=torch.tensor(self.pool.filled))
        if self.bots is not None:
            self.stats.update(bot_stats)

    def _pool_stats(self, rewards, dones):
        """Per slot of the pool, over the last rollout's rows (this rank's): episodes that ended and those of
        them P1 won (the reference's win counter: `terminated` with reward > 0), as [K] int64 tensors."""
        torch = _torch()
        arena_slot = self.slots.long().repeat_interleave(_abi.FS_SELFPLAY_GROUP)[:self.sim.num_envs]
        arena_slot = arena_slot.clamp_(max=self.pool.capacity - 1)
        done = dones != 0
        if self.bots is not None:  # (a league: the bot groups' rows belong to no slot, whatever byte they carry)
            done = done & ~self._bot_arenas(dones.device)
        zero = torch.zeros(self.pool.capacity, dtype=torch.int64, device=dones.device)
        return {"pool_episodes": zero.index_add(0, arena_slot, done.sum(0)),
                "pool_wins": zero.index_add(0, arena_slot, (done & (rewards > 0)).sum(0))}

    def _bot_arenas(self, device):
        """[N] bool: the arenas of the league's bot groups."""
        torch = _torch()
        return torch.from_numpy(self.bots).to(device).repeat_interleave(_abi.FS_SELFPLAY_GROUP)[:self.sim.num_envs]

    def _bot_stats(self, rewards, dones):
        """Over the bot groups' rows of the last rollout (this rank's): episodes that ended and those of them P1
        won, as int64 scalars -- the win rate against the scripted bot the reference reports."""
        done = (dones != 0) & self._bot_arenas(dones.device)
        return {"bot_episodes": done.sum(), "bot_wins": (done & (rewards > 0)).sum()}

    def iterate(self):
        self.update(*self.collect())

    def train(self, iterations, sync=True):
        """Run `iterations` PPO iterations; returns env-steps/s of the whole loop (rollout +
        learning), timed around device synchronisation."""
        torch = _torch()
        torch.cuda.synchronize(self.sim.device)
        t0 = time.perf_counter()
        for _ in range(iterations):
            self.iterate()
        if sync:
            torch.cuda.synchronize(self.sim.device)
        return iterations * self.horizon * self.sim.num_envs / (time.perf_counter() - t0)


__all__ = ["PPOTrainer", "PPOGrad", "make_critic", "gae", "gae_device", "pack_rows", "features_device",
           "p2_eligible_groups", "p2_selection", "N_ACTIONS"]
