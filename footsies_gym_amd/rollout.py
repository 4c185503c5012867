"""On-device rollouts with a policy in the loop.

Every step: the simulator's outputs (device tensors, written in place by libfootsies.so)
-> features -> a 2x64 MLP actor -> a sampled action per arena (Gumbel-max over Exp(1) noise,
with its log-probability for PPO) -> fs_step with device actions.  Nothing leaves the GPU and
nothing synchronises, so a block of steps is captured once into a HIP graph and
replayed: the loop then costs graph launches, not the ~20 kernel launches per step.

Graph replays do not advance the handle's host-side step counter (fs_steps_taken), which
only the hashed-action stream and frame_delay > 0 read; use eager steps for those.

:class:`FusedPolicyRollout` goes one step further: the actor runs inside the simulator's
fused tick loop (fs_step_n_policy, csrc/fs_policy.h) as bf16 MFMAs, so a block of n
policy-driven ticks is one kernel launch with the arena state in registers throughout;
``rollout_skipped`` runs n agent decisions per arena the same way (fs_step_skip_policy), the actor
asked once per decision and each arena skipping its own frames as under FootsiesFrameSkipped.

:class:`FusedSelfPlayRollout` adds a second in-kernel actor for P2 (fs_step_n_selfplay): self-play,
or any learned opponent of the same shape, with both fighters reacting every tick inside one launch;
its ``rollout_skipped`` (fs_step_skip_selfplay) runs agent decisions instead, P1's actor asked once per
decision and the opponent on every tick, the ones P1 skips included.
"""
import ctypes as C

from . import _abi
from ._lib import check, lib

N_FEATURES = 8
N_ACTIONS = 8  # (left, right, attack) combinations, FootsiesActionCombinationsDiscretized


def _torch():
    import torch
    return torch


def obs_features(out):
    """[N, 8] float32: guard / 3, move / 16, move_frame / 55, position / 4.6 for P1 and P2
    (the reference's normalisation constants, wrappers/normalization.py)."""
    torch = _torch()
    return torch.cat([out["guard"].float() / 3.0, out["move"].float() / 16.0, out["move_frame"] / 55.0,
                      out["position"] / 4.6], dim=1)


def make_actor(hidden=64, device=None, seed=0):
    """The C5 actor: Linear(8, 64) - tanh - Linear(64, 64) - tanh - Linear(64, 8), random init."""
    torch = _torch()
    g = torch.Generator().manual_seed(seed)
    nn = torch.nn
    net = nn.Sequential(nn.Linear(N_FEATURES, hidden), nn.Tanh(), nn.Linear(hidden, hidden), nn.Tanh(),
                        nn.Linear(hidden, N_ACTIONS))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    return net.to(device)


class PolicyRollout:
    """Steps `sim` (a FootsiesSim) with actions sampled from `actor`; P2 is whatever the
    handle was created with (bot, noop, or `p2_actions` for external)."""

    def __init__(self, sim, actor, p2_actions=None):
        torch = _torch()
        self.sim, self.actor = sim, actor
        n = sim.num_envs
        dev = sim.device
        self.action = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.logp = torch.zeros(n, dtype=torch.float32, device=dev)
        # obs_features' divisors per column: one cat + one division gives its values bit for bit
        self._div = torch.tensor([3.0, 3.0, 16.0, 16.0, 55.0, 55.0, 4.6, 4.6], dtype=torch.float32, device=dev)
        self.p2 = p2_actions if p2_actions is not None else torch.zeros(n, dtype=torch.uint8, device=dev)
        self.graph = None
        self.graph_steps = 0
        self.action_log = None  # [graph steps][N] actions of the last replay when capture(log=True)

    def _step(self, log_row=None):
        torch = _torch()
        out = self.sim.outputs()
        with torch.no_grad():  # (17 kernels per step with fs_step: each one is a graph node)
            x = torch.cat([out["guard"].float(), out["move"].float(), out["move_frame"], out["position"]], dim=1)
            logits = self.actor(x.div_(self._div))  # == obs_features(out)
            # Gumbel-max with -log(-log U) = -log E, E ~ Exp(1)
            a = torch.argmax(logits - torch.empty_like(logits).exponential_().log_(), dim=1)
            torch.gather(torch.log_softmax(logits, dim=1), 1, a[:, None], out=self.logp.view(-1, 1))
            self.action.copy_(a)
            if log_row is not None:
                log_row.copy_(self.action)
        check(lib().fs_step(self.sim.handle, C.c_void_p(self.action.data_ptr()), C.c_void_p(self.p2.data_ptr()),
                            _abi.FS_ACT_DEVICE), self.sim.handle)

    def step_eager(self, n=1):
        for _ in range(n):
            self._step()

    def capture(self, steps, warmup=2, log=False):
        """Capture `steps` policy+simulator steps into one HIP graph on a private stream, after
        `warmup` eager steps there (library / BLAS handles and the allocator settle outside the
        capture).  Returns the warm-up steps' actions ([warmup][N], host) so they can be replayed."""
        torch = _torch()
        stream = torch.cuda.Stream(device=self.sim.device)
        self.sim.use_torch_stream(stream)  # the library issues its kernels on the capture stream
        warm = []
        with torch.cuda.stream(stream):
            for _ in range(warmup):
                self._step()
                warm.append(self.action.cpu())
        stream.synchronize()
        if log:
            self.action_log = torch.zeros((steps, self.sim.num_envs), dtype=torch.uint8, device=self.sim.device)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            for i in range(steps):
                self._step(self.action_log[i] if log else None)
        self.graph, self.graph_steps, self.stream = g, steps, stream
        return warm

    def replay(self, times=1):
        for _ in range(times):
            self.graph.replay()


def _weights(actor):
    """weight, bias of each Linear of `actor`, in order"""
    torch = _torch()
    return [t for m in actor if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)]


def _actor_params(sim, actor):
    """The six fp32 tensors of an in-kernel actor on sim's device (the module's own where it already
    holds them so)."""
    torch = _torch()
    w = _weights(actor)
    shapes = [tuple(t.shape) for t in w[::2]]
    if shapes != [(64, N_FEATURES), (64, 64), (N_ACTIONS, 64)]:
        raise ValueError("the fused actor is 8 -> 64 -> 64 -> 8; got %s" % (shapes,))
    with torch.no_grad():
        return [t.detach().to(device=sim.device, dtype=torch.float32).contiguous() for t in w]


def _copy_weights(params, actor):
    torch = _torch()
    with torch.no_grad():
        for dst, src in zip(params, _weights(actor)):
            dst.copy_(src)


def _buffer(given, shape, dtype, device):
    """A sample array argument: allocated when None, kept when given, False = off."""
    return _torch().empty(shape, dtype=dtype, device=device) if given is None else given


def _ptr(t):
    return None if t is False else t.data_ptr()


def _policy(params, seed, actions, logp):
    """fs_policy of an actor's six tensors, its seed and its sample arrays (False = off)."""
    w1, b1, w2, b2, w3, b3 = (t.data_ptr() for t in params)
    return _abi.fs_policy(w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3, seed=seed, actions_out=_ptr(actions),
                          logp_out=_ptr(logp))


def _skip_counts(n, max_ticks):
    n, max_ticks = int(n), int(max_ticks)
    if n < 1:
        raise ValueError("rollout_skipped: n must be >= 1, got %d" % n)
    if not 1 <= max_ticks <= _abi.FS_SKIP_POLICY_MAX_TICKS:
        raise ValueError("rollout_skipped: max_ticks must be 1 .. %d, got %d" % (_abi.FS_SKIP_POLICY_MAX_TICKS, max_ticks))
    return n, max_ticks


def _byref(struct):
    return None if struct is None else C.byref(struct)


class FusedPolicyRollout:
    """C5 in one launch per block of ticks: `actor` (the make_actor shape, 8-64-64-8 with tanh)
    is evaluated in bf16 inside the simulator kernel, P1's action drawn from its softmax by
    inverse CDF with a counter-based uniform of (seed, env, step).  P2 is whatever the handle
    was created with (bot, noop, or `p2_actions` [n][N] per call for external)."""

    def __init__(self, sim, actor, seed=0):
        self.params = _actor_params(sim, actor)
        self.sim, self.seed = sim, int(seed) & (2**64 - 1)
        self.last_capped = None  # rollout_skipped: the last call's capped flags

    def refresh(self, actor):
        """Copy new actor weights in (after an optimiser step); the buffers stay put."""
        _copy_weights(self.params, actor)

    def _decision_buffers(self, n, actions, logp, ticks, capped):
        """rollout_skipped's [n][N] arrays by decision and the fs_skip_traj of the last two"""
        torch = _torch()
        shape, dev = (n, self.sim.num_envs), self.sim.device
        actions, logp = _buffer(actions, shape, torch.uint8, dev), _buffer(logp, shape, torch.float32, dev)
        ticks, capped = _buffer(ticks, shape, torch.int32, dev), _buffer(capped, shape, torch.uint8, dev)
        return actions, logp, ticks, capped, _abi.fs_skip_traj(ticks=_ptr(ticks), capped=_ptr(capped))

    def rollout(self, n, actions=None, logp=None, p2_actions=None, trajectory=None):
        """n policy-driven ticks in one launch.  `actions` (uint8) / `logp` (float32) [n][N]
        device tensors receive P1's samples (allocated when None; pass False to skip one).
        Returns (actions, logp)."""
        torch = _torch()
        shape, dev = (n, self.sim.num_envs), self.sim.device
        actions, logp = _buffer(actions, shape, torch.uint8, dev), _buffer(logp, shape, torch.float32, dev)
        pol = _policy(self.params, self.seed, actions, logp)
        check(lib().fs_step_n_policy(self.sim.handle, int(n), C.byref(pol),
                                     None if p2_actions is None else C.c_void_p(p2_actions.data_ptr()),
                                     _byref(_abi.trajectory_outputs(trajectory))), self.sim.handle)
        return actions, logp

    def rollout_skipped(self, n, actions=None, logp=None, ticks=None, capped=None, trajectory=None,
                        max_ticks=_abi.FS_SKIP_DEFAULT_MAX_TICKS):
        """n agent decisions per arena in one launch (fs_step_skip_policy): the actor is asked once
        per decision, and each arena then skips the frames in which P1 cannot act, as under the
        reference's FootsiesFrameSkipped, its rewards summed.  Every array is [n][N] by decision:
        `actions` (uint8) / `logp` (float32) P1's samples, `ticks` (int32) the ticks each decision
        ran, `capped` (uint8) 1 where `max_ticks` closed a decision that was still skippable; each is
        allocated when None, pass False to skip one.  `trajectory` rows hold each decision's last
        tick with the summed reward.  The handle's P2 must be the bot or idle.  Returns (actions,
        logp, ticks); the `capped` array of the call stays in ``last_capped``."""
        n, max_ticks = _skip_counts(n, max_ticks)
        actions, logp, ticks, capped, skip = self._decision_buffers(n, actions, logp, ticks, capped)
        pol = _policy(self.params, self.seed, actions, logp)
        check(lib().fs_step_skip_policy(self.sim.handle, n, C.byref(pol), max_ticks,
                                        _byref(_abi.trajectory_outputs(trajectory)), C.byref(skip)), self.sim.handle)
        self.last_capped = capped
        return actions, logp, ticks


def mirror_features(x):
    """The [..., 8] feature rows of obs_features as P2 sees the game from its own side
    (FS_SELFPLAY_MIRROR): each pair swapped and both positions negated,
    g2, g1, m2, m1, mf2, mf1, -x2, -x1.  numpy array or torch tensor; its own inverse."""
    y = x[..., [1, 0, 3, 2, 5, 4, 7, 6]]
    y[..., 6:] = -y[..., 6:]  # (the fancy index above made a copy)
    return y


def swap_left_right(a):
    """Action indices (Left = 1, Right = 2, Attack = 4) with Left and Right exchanged: the game
    input of a mirrored P2 actor's sampled index.  numpy array, torch tensor or int; its own inverse."""
    return (a & 4) | ((a & 1) << 1) | ((a >> 1) & 1)


class FusedSelfPlayRollout(FusedPolicyRollout):
    """Self-play in one launch per block of ticks (fs_step_n_selfplay): `actor` plays P1 as in
    FusedPolicyRollout and a second in-kernel actor, `opponent`, plays P2 of a handle created with
    p2_mode="external", reacting to the game every tick.  `opponent=None` takes a copy of
    `actor`'s weights (refresh_opponent re-takes it).  With `mirror` the opponent sees the game from
    its own side (mirror_features) and its sampled index reaches the game with Left and Right
    exchanged (swap_left_right), so one set of weights plays either side; without it the opponent
    receives P1's observation and its index is P2's input as is, which is what the reference hands
    a custom `opponent` policy.  `opponent_seed=None` derives a seed different from `seed`: with
    equal weights, equal seeds and `mirror` both fighters would act identically for as long as the
    game stays symmetric."""

    def __init__(self, sim, actor, opponent=None, seed=0, opponent_seed=None, mirror=True):
        super().__init__(sim, actor, seed=seed)
        # (cloned: the tensors may be the module's own when it already sits on the device in fp32,
        # and the opponent has to stay what it was while the learner moves on)
        self.params2 = [p.clone() for p in _actor_params(sim, actor if opponent is None else opponent)]
        if opponent_seed is None:
            opponent_seed = self.seed ^ 0x9E3779B97F4A7C15  # (never equal to seed)
        self.opponent_seed = int(opponent_seed) & (2**64 - 1)
        self.mirror = bool(mirror)

    def refresh_opponent(self, actor):
        """Copy new weights into the opponent's buffers, which stay put."""
        _copy_weights(self.params2, actor)

    def _flags(self):
        return _abi.FS_SELFPLAY_MIRROR if self.mirror else 0

    def rollout(self, n, actions=None, logp=None, p2_actions=None, p2_logp=None, trajectory=None):
        """n ticks in one launch, both fighters sampled in-kernel.  `actions` / `logp` receive P1's
        samples, `p2_actions` / `p2_logp` P2's (its sampled index, before swap_left_right; [n][N]
        uint8 / float32 device tensors, allocated when None; pass False to skip one).  Rewards and
        `trajectory` are P1's, as in FusedPolicyRollout.  Returns (actions, logp, p2_actions, p2_logp)."""
        torch = _torch()
        n = int(n)
        shape, dev = (n, self.sim.num_envs), self.sim.device
        out = tuple(_buffer(given, shape, dtype, dev) for given, dtype in (
            (actions, torch.uint8), (logp, torch.float32), (p2_actions, torch.uint8), (p2_logp, torch.float32)))
        p1 = _policy(self.params, self.seed, out[0], out[1])
        p2 = _policy(self.params2, self.opponent_seed, out[2], out[3])
        check(lib().fs_step_n_selfplay(self.sim.handle, n, C.byref(p1), C.byref(p2), self._flags(),
                                       _byref(_abi.trajectory_outputs(trajectory))), self.sim.handle)
        return out

    def rollout_skipped(self, n, actions=None, logp=None, ticks=None, capped=None, p2_actions=False, p2_logp=False,
                        trajectory=None, max_ticks=_abi.FS_SKIP_DEFAULT_MAX_TICKS):
        """n agent decisions per arena in one launch (fs_step_skip_selfplay): P1's actor is asked once
        per decision and the arena skips the frames in which P1 cannot act, as in
        FusedPolicyRollout.rollout_skipped, while the opponent acts on every tick, the skipped ones
        included -- the reference's FootsiesFrameSkipped over an env with a custom `opponent`.
        `actions` / `logp` / `ticks` / `capped` are [n][N] by decision (allocated when None, pass False
        to skip one).  `p2_actions` (uint8) / `p2_logp` (float32) are [n][max_ticks][N] by decision and
        tick within it -- the opponent's sampled index before swap_left_right -- and off by default:
        pass None to have one allocated (entries of ticks that did not run are left as they were) or a
        tensor of that shape.  Returns (actions, logp, ticks); `last_capped` holds the call's capped
        flags and `last_p2` the (p2_actions, p2_logp) pair (False where off)."""
        n, max_ticks = _skip_counts(n, max_ticks)
        actions, logp, ticks, capped, skip = self._decision_buffers(n, actions, logp, ticks, capped)
        torch = _torch()
        shape, dev = (n, max_ticks, self.sim.num_envs), self.sim.device
        p2_actions, p2_logp = _buffer(p2_actions, shape, torch.uint8, dev), _buffer(p2_logp, shape, torch.float32, dev)
        p1 = _policy(self.params, self.seed, actions, logp)
        p2 = _policy(self.params2, self.opponent_seed, p2_actions, p2_logp)
        check(lib().fs_step_skip_selfplay(self.sim.handle, n, C.byref(p1), C.byref(p2), self._flags(), max_ticks,
                                          _byref(_abi.trajectory_outputs(trajectory)), C.byref(skip)), self.sim.handle)
        self.last_capped = capped
        self.last_p2 = (p2_actions, p2_logp)
        return actions, logp, ticks
