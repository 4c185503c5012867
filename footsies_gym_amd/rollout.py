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

:class:`OpponentPool` holds several opponent snapshots in one device buffer, and
``FusedSelfPlayRollout(sim, actor, pool=pool)`` plays them all in the same one launch
(fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool): each group of 128 consecutive arenas meets the
snapshot its byte of ``slots`` names.  With ``bots=`` (a bool per group, :func:`bot_groups`) those groups play
the in-game scripted bot instead, still in the same launch (fs_step_n_league / fs_step_skip_league).
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
    w = _weights(_checked_actor(actor))
    with torch.no_grad():
        return [t.detach().to(device=sim.device, dtype=torch.float32).contiguous() for t in w]


def _checked_actor(actor):
    """`actor`, or ValueError unless it has the in-kernel actor's shape."""
    shapes = [tuple(t.shape) for t in _weights(actor)[::2]]
    if shapes != [(64, N_FEATURES), (64, 64), (N_ACTIONS, 64)]:
        raise ValueError("the fused actor is 8 -> 64 -> 64 -> 8; got %s" % (shapes,))
    return actor


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

    def __new__(cls, sim=None, actor=None, *args, pool=None, **kwargs):
        # FusedSelfPlayRollout(sim, actor, pool=...) is a FusedPoolSelfPlayRollout, whose rollout calls take
        # `slots`; without a pool this class is untouched, its methods' signatures included
        if pool is not None and cls is FusedSelfPlayRollout:
            cls = FusedPoolSelfPlayRollout
        return super().__new__(cls)

    def __init__(self, sim, actor, opponent=None, seed=0, opponent_seed=None, mirror=True, pool=None, bots=None):
        if bots is not None:  # (checked before the device is touched)
            import numpy as np
            if pool is None:
                raise ValueError("FusedSelfPlayRollout: bots= needs pool= (the league calls take a pool)")
            bots = np.asarray(bots, dtype=bool).reshape(-1)
            if bots.size != pool_groups(sim.num_envs):
                raise ValueError("bots must hold one bool per group: %d groups of %d arenas, got %d" % (
                    pool_groups(sim.num_envs), _abi.FS_SELFPLAY_GROUP, bots.size))
        super().__init__(sim, actor, seed=seed)
        self.pool = pool
        self.bots = bots
        if pool is None:
            # (cloned: the tensors may be the module's own when it already sits on the device in fp32,
            # and the opponent has to stay what it was while the learner moves on)
            self.params2 = [p.clone() for p in _actor_params(sim, actor if opponent is None else opponent)]
        elif opponent is not None:
            raise ValueError("FusedSelfPlayRollout takes `opponent` or `pool`, not both")
        elif pool.sim is not sim:
            raise ValueError("the pool belongs to another sim")
        if opponent_seed is None:
            opponent_seed = self.seed ^ 0x9E3779B97F4A7C15  # (never equal to seed)
        self.opponent_seed = int(opponent_seed) & (2**64 - 1)
        self.mirror = bool(mirror)
        if bots is not None:
            # a league: these groups' arenas play the in-game bot from here on (fs_step_n_league /
            # fs_step_skip_league; the handle's P2 bit says who plays a group)
            import numpy as np
            sim.set_p2_mode("bot", np.repeat(bots, _abi.FS_SELFPLAY_GROUP)[:sim.num_envs])

    def refresh_opponent(self, actor):
        """Copy new weights into the opponent's buffers, which stay put."""
        if self.pool is not None:
            raise ValueError("this rollout plays a pool: push(actor) to it instead")
        _copy_weights(self.params2, actor)

    def _flags(self):
        return _abi.FS_SELFPLAY_MIRROR if self.mirror else 0

    def _opponent(self, call, slots, p2_actions, p2_logp):
        """(the library's `call`, its P2 argument): fs_policy of the one opponent, or with `slots` the pool
        form of the call and its fs_policy_pool"""
        if self.pool is None:
            return getattr(lib(), call), _policy(self.params2, self.opponent_seed, p2_actions, p2_logp)
        name = call + "_pool" if self.bots is None else call.replace("selfplay", "league")
        return getattr(lib(), name), self.pool.argument(slots, self.opponent_seed, p2_actions, p2_logp)

    def rollout(self, n, actions=None, logp=None, p2_actions=None, p2_logp=None, trajectory=None):
        """n ticks in one launch, both fighters sampled in-kernel.  `actions` / `logp` receive P1's
        samples, `p2_actions` / `p2_logp` P2's (its sampled index, before swap_left_right; [n][N]
        uint8 / float32 device tensors, allocated when None; pass False to skip one).  Rewards and
        `trajectory` are P1's, as in FusedPolicyRollout.  Returns (actions, logp, p2_actions, p2_logp)."""
        return self._rollout(None, n, actions, logp, p2_actions, p2_logp, trajectory)

    def _rollout(self, slots, n, actions, logp, p2_actions, p2_logp, trajectory):
        torch = _torch()
        n = int(n)
        shape, dev = (n, self.sim.num_envs), self.sim.device
        out = tuple(_buffer(given, shape, dtype, dev) for given, dtype in (
            (actions, torch.uint8), (logp, torch.float32), (p2_actions, torch.uint8), (p2_logp, torch.float32)))
        p1 = _policy(self.params, self.seed, out[0], out[1])
        call, p2 = self._opponent("fs_step_n_selfplay", slots, out[2], out[3])
        check(call(self.sim.handle, n, C.byref(p1), C.byref(p2), self._flags(),
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
        return self._rollout_skipped(None, n, actions, logp, ticks, capped, p2_actions, p2_logp, trajectory, max_ticks)

    def _rollout_skipped(self, slots, n, actions, logp, ticks, capped, p2_actions, p2_logp, trajectory, max_ticks):
        n, max_ticks = _skip_counts(n, max_ticks)
        actions, logp, ticks, capped, skip = self._decision_buffers(n, actions, logp, ticks, capped)
        torch = _torch()
        shape, dev = (n, max_ticks, self.sim.num_envs), self.sim.device
        p2_actions, p2_logp = _buffer(p2_actions, shape, torch.uint8, dev), _buffer(p2_logp, shape, torch.float32, dev)
        p1 = _policy(self.params, self.seed, actions, logp)
        call, p2 = self._opponent("fs_step_skip_selfplay", slots, p2_actions, p2_logp)
        check(call(self.sim.handle, n, C.byref(p1), C.byref(p2), self._flags(), max_ticks,
                   _byref(_abi.trajectory_outputs(trajectory)), C.byref(skip)), self.sim.handle)
        self.last_capped = capped
        self.last_p2 = (p2_actions, p2_logp)
        return actions, logp, ticks


class FusedPoolSelfPlayRollout(FusedSelfPlayRollout):
    """FusedSelfPlayRollout against an OpponentPool (what ``FusedSelfPlayRollout(sim, actor, pool=pool)``
    builds): the same two launches, fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool, with P2's weights
    chosen per group of 128 consecutive arenas.  `slots` is the uint8 device tensor of each group's slot
    (OpponentPool.assign, or any [ceil(N / 128)] tensor; a value past the pool's capacity plays the last
    slot).  Every arena's results are bit for bit those of the single-opponent call with its group's
    weights.  Everything else is FusedSelfPlayRollout's.

    With `bots` (a bool per group, e.g. bot_groups) the run is a league: those groups' arenas are switched to
    the in-game bot once (sim.set_p2_mode) and both rollouts go through fs_step_n_league /
    fs_step_skip_league -- P1's actor against the scripted BattleAI there, the pool elsewhere, in the same
    launch.  A bot group's slot is ignored and its entries of p2_actions / p2_logp are left as they were."""

    def rollout(self, n, actions=None, logp=None, p2_actions=None, p2_logp=None, trajectory=None, slots=None):
        return self._rollout(slots, n, actions, logp, p2_actions, p2_logp, trajectory)

    def rollout_skipped(self, n, actions=None, logp=None, ticks=None, capped=None, p2_actions=False, p2_logp=False,
                        trajectory=None, max_ticks=_abi.FS_SKIP_DEFAULT_MAX_TICKS, slots=None):
        return self._rollout_skipped(slots, n, actions, logp, ticks, capped, p2_actions, p2_logp, trajectory, max_ticks)


def pool_groups(num_envs):
    """Groups of FS_SELFPLAY_GROUP arenas in a handle of `num_envs` (the last may be partial)."""
    return (int(num_envs) + _abi.FS_SELFPLAY_GROUP - 1) // _abi.FS_SELFPLAY_GROUP


def bot_groups(seed, first_group, groups, fraction):
    """Which of `groups` consecutive arena groups from global group `first_group` on play the in-game bot, as a
    numpy bool array, fixed for a run: group G is a bot group when mix64(seed ^ G * 0x9E3779B97F4A7C15 ^
    0xB07 * 0xD1B54A32D192ED03) >> 40 < fraction * 2^24.  A pure function of (seed, G), counter-based like
    pool_assignment, so a shard draws what the unsharded run draws for its groups."""
    import numpy as np
    if not 0.0 <= float(fraction) <= 1.0:
        raise ValueError("fraction must be within [0, 1], got %r" % (fraction,))
    m = 2**64 - 1
    g = np.arange(int(first_group), int(first_group) + int(groups), dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = np.uint64(int(seed) & m) ^ (g * np.uint64(0x9E3779B97F4A7C15))
        v = _mix64(key ^ np.uint64((0xB07 * 0xD1B54A32D192ED03) & m)) >> np.uint64(40)
    return v < np.uint64(int(round(float(fraction) * 2**24)))


def _mix64(x):
    """policy_uniform's splitmix64 finaliser on a numpy uint64 array (csrc/fs_policy.h)."""
    import numpy as np
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def pool_assignment(seed, iteration, first_group, groups, filled, newest, latest=0.5):
    """The slot of each of `groups` consecutive arena groups from global group `first_group` on, as a numpy
    uint8 array: a pure function of its arguments, counter-based like the kernels' policy_uniform.
    Group G draws two 24-bit integers v_k = mix64(seed ^ G * 0x9E3779B97F4A7C15 ^ (iteration + (k << 40)) *
    0xD1B54A32D192ED03) >> 40, k = 0, 1 (policy_uniform's bits on counter iteration + (k << 40)): it plays
    `newest` when v_0 < latest * 2^24, else slot (v_1 * filled) >> 24, uniform over the filled slots
    0 .. filled - 1."""
    import numpy as np
    if not 0.0 <= float(latest) <= 1.0:
        raise ValueError("latest must be within [0, 1], got %r" % (latest,))
    if not (1 <= int(filled) <= _abi.FS_SELFPLAY_POOL_MAX and 0 <= int(newest) < int(filled)):
        raise ValueError("filled must be 1 .. %d and newest below it, got %r, %r" % (
            _abi.FS_SELFPLAY_POOL_MAX, filled, newest))
    m = 2**64 - 1
    g = np.arange(int(first_group), int(first_group) + int(groups), dtype=np.uint64)
    with np.errstate(over="ignore"):
        key = np.uint64(int(seed) & m) ^ (g * np.uint64(0x9E3779B97F4A7C15))
        v = [_mix64(key ^ np.uint64(((int(iteration) + (k << 40)) * 0xD1B54A32D192ED03) & m)) >> np.uint64(40)
             for k in (0, 1)]
    drawn = (v[1] * np.uint64(int(filled))) >> np.uint64(24)
    return np.where(v[0] < np.uint64(int(round(float(latest) * 2**24))), np.uint64(int(newest)), drawn).astype(np.uint8)


class OpponentPool:
    """Up to `capacity` (1 .. 256) opponent snapshots for FusedSelfPlayRollout(sim, actor, pool=...), in one
    [capacity][5256] fp32 device buffer that stays put (``weights``; a slot is w1 | b1 | w2 | b2 | w3 | b3 in
    torch layouts, FS_PPO_ACTOR_PARAMS floats).  `actor`, when given, is pushed as the first snapshot."""

    def __init__(self, sim, capacity, actor=None):
        torch = _torch()
        capacity = int(capacity)
        if not 1 <= capacity <= _abi.FS_SELFPLAY_POOL_MAX:
            raise ValueError("OpponentPool: capacity must be 1 .. %d, got %d" % (_abi.FS_SELFPLAY_POOL_MAX, capacity))
        self.sim, self.capacity = sim, capacity
        self.weights = torch.zeros((capacity, _abi.FS_PPO_ACTOR_PARAMS), dtype=torch.float32, device=sim.device)
        self.pushes = 0  # snapshots taken so far: slot pushes % capacity is the next one's
        if actor is not None:
            self.push(actor)

    @property
    def filled(self):
        """Slots that hold a snapshot: 0 .. filled - 1."""
        return min(self.pushes, self.capacity)

    @property
    def newest(self):
        """The slot last pushed (None before the first push)."""
        return (self.pushes - 1) % self.capacity if self.pushes else None

    def params(self, slot):
        """The six tensors of `slot` in fs_policy order, as views of the buffer."""
        row, out, at = self.weights[int(slot)], [], 0
        for shape in ((64, N_FEATURES), (64,), (64, 64), (64,), (N_ACTIONS, 64), (N_ACTIONS,)):
            size = shape[0] * (shape[1] if len(shape) > 1 else 1)
            out.append(row[at:at + size].view(shape))
            at += size
        return out

    def push(self, actor):
        """Copy `actor`'s weights into the next free slot, or over the oldest snapshot once the pool is full.
        Returns the slot."""
        slot = self.pushes % self.capacity
        _copy_weights(self.params(slot), _checked_actor(actor))
        self.pushes += 1
        return slot

    def assign(self, iteration, latest=0.5, seed=0):
        """The uint8 device tensor [ceil(N / 128)] of each arena group's slot for rollout(slots=...): with
        probability `latest` the newest snapshot, else a uniform draw over the filled slots.  A pure function
        (pool_assignment, computed on the host) of (seed, iteration, the group's global index (arena_base +
        128 g) / 128, filled, newest): a sharded run's assignments are the unsharded run's, cut at the shard
        boundaries.  ValueError when the sim's arena_base is no multiple of 128 (groups would straddle shards)."""
        return _torch().from_numpy(self.assignment(iteration, latest, seed)).to(self.sim.device)

    def assignment(self, iteration, latest=0.5, seed=0):
        """assign()'s slots as the numpy uint8 array they are drawn as on the host."""
        base = int(self.sim.arena_base)
        if base % _abi.FS_SELFPLAY_GROUP:
            raise ValueError("OpponentPool.assign: arena_base %d is not a multiple of %d" % (base, _abi.FS_SELFPLAY_GROUP))
        if not self.pushes:
            raise ValueError("OpponentPool.assign: the pool is empty")
        return pool_assignment(seed, iteration, base // _abi.FS_SELFPLAY_GROUP, pool_groups(self.sim.num_envs),
                               self.filled, self.newest, latest)

    def argument(self, slots, seed, actions, logp):
        """fs_policy_pool of this pool under `slots`, with P2's seed and sample arrays (False = off)."""
        torch = _torch()
        if slots is None:
            raise ValueError("a rollout against a pool needs slots= (OpponentPool.assign)")
        if slots.dtype != torch.uint8 or slots.device != self.weights.device or not slots.is_contiguous() or \
                slots.numel() != pool_groups(self.sim.num_envs):
            raise ValueError("slots must be a contiguous uint8 tensor of %d groups on %s" % (
                pool_groups(self.sim.num_envs), self.weights.device))
        self._slots = slots  # (kept until the next call: the launch is asynchronous)
        return _abi.fs_policy_pool(weights=self.weights.data_ptr(), n_slots=self.capacity, slot=slots.data_ptr(),
                                   seed=seed, actions_out=_ptr(actions), logp_out=_ptr(logp))
