"""The sampler of the in-kernel actor (policy_act_side, footsies_gym_amd/csrc/fs_policy.h) restated with no
tolerance, for tests/test_sampler_ref.py (host) and tests/test_gpu_sampler_exact.py (GPU).

With W3 = 0 the kernel's logits are exactly the bf16 hi + lo pair of b3, whatever the game state and the hidden
layers are: the layer-3 weight fragments hold -2 * 0, and a zero times a finite r adds nothing to the bias MFMA.
A draw is then a function of (seed, arena, counter) alone.

- `constant_logit_actor`: such an actor, its hidden layers random (they must not matter).
- `exact_draw`: logits 0 on a `live` set and -200 elsewhere.  Every softmax weight is exactly 1 or 0 (2^(-200
  log2 e) is far below the smallest float), every partial sum a small integer, so target = f32(u) * f32(K) is the
  kernel's one rounding and the action is live[floor(target)]; the log-probability is -ln K.
- `kernel_draw`: the kernel's fp32 selection arithmetic on arbitrary logits, under the association it had
  before the zero-weight rule ("parent") and with the rule ("fixed").
- `zero_weight_cases`: logits and pinned (seed, arena, counter) triples for which "parent" returns action 7,
  whose weight is exactly zero.
"""
import numpy as np

from tests import policy_ref

F = np.float32
DEAD = -200.0  # exactly a bf16; e^-200 is 0 in float32
TOP, SECOND = 0xFFFFFF, 0xFFFFFE  # the 24 bits of the uniforms 1 - 2^-24 and 1 - 2^-23

# the live sets of the exact GPU tests: the singletons, each half, everything, pairs across and at the ends of
# the halves, mixed sets, everything but the first / the last action, and the same register of both halves
LIVE_SETS = tuple([(a,) for a in range(8)] + [
    (0, 1, 2, 3), (4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6, 7), (3, 4), (0, 7), (1, 2, 5), (0, 2, 4, 5, 6),
    (1, 3, 4, 5, 6, 7), (1, 2, 3, 4, 5, 6, 7), (0, 1, 2, 3, 4, 5, 6), (2, 6)])


def live_logits(live):
    """b3 of the live set: 0 there, DEAD elsewhere."""
    b3 = np.full(8, DEAD, dtype=F)
    b3[list(live)] = 0.0
    return b3


def constant_logit_actor(b3, hidden_seed, scale=1, device=None):
    """make_actor(hidden_seed) with every parameter multiplied by `scale` (tests/ppo_ref.scaled_nets), then w3
    zeroed and the last bias set to `b3`: the logits are b3 for every observation."""
    import torch
    from footsies_gym_amd.rollout import make_actor
    actor = make_actor(seed=hidden_seed)
    last = [m for m in actor if isinstance(m, torch.nn.Linear)][-1]
    with torch.no_grad():
        for p in actor.parameters():
            p.mul_(scale)
        last.weight.zero_()
        last.bias.copy_(torch.as_tensor(np.asarray(b3, dtype=F)))
    return actor.to(device)


def exact_draw(live, seed, arena, counter):
    """The kernel's draw for live_logits(live): (action uint8, -ln K as float64, target float32), over the
    broadcast of `arena` and `counter` (global arena indices; uint64 counters)."""
    live = np.asarray(sorted(live), dtype=np.uint8)
    u = policy_ref.policy_uniform(seed, arena, np.asarray(counter, dtype=np.uint64))
    target = u * F(len(live))  # float32 * float32, rounded once
    assert target.dtype == F
    idx = np.floor(target).astype(np.int64)
    assert (idx < len(live)).all()  # (u < 1 keeps the rounded product below K: tests/test_sampler_ref.py)
    return live[idx], -np.log(np.float64(len(live))), target


def fast_exp(x):
    """fs_policy.h fast_exp in float32: 2^(x * log2 e), correctly rounded here (v_exp_f32 is within 1 ulp),
    results below the normal range flushed to 0."""
    with np.errstate(under="ignore"):
        e = np.exp2((np.asarray(x, dtype=F) * F(1.4426950408889634)).astype(np.float64)).astype(F)
    e[e < F(2.0 ** -126)] = 0
    return e


def kernel_draw(lg, u, rule):
    """policy_act_side's selection in float32 on logits `lg` [M, 8] (float32) and uniforms `u` [M] (float32).
    rule "parent": the fall-through of each half is its fourth action.  rule "fixed": it is the half's last
    action whose weight is non-zero.  Returns (action, e [M, 8], target, total)."""
    lg, u = np.asarray(lg, dtype=F), np.asarray(u, dtype=F)
    e = fast_exp(lg - lg.max(axis=1, keepdims=True))
    s_lo = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
    s_hi = ((e[:, 4] + e[:, 5]) + e[:, 6]) + e[:, 7]
    total = s_lo + s_hi
    target = u * total
    act = []
    for h, base in ((0, np.zeros_like(s_lo)), (1, s_lo)):
        w = e[:, 4 * h:4 * h + 4]
        c0 = base + w[:, 0]
        c1 = c0 + w[:, 1]
        c2 = c1 + w[:, 2]
        if rule == "parent":
            last = np.full(len(u), 3)
        elif rule == "fixed":
            last = np.where(w[:, 3] > 0, 3, np.where(w[:, 2] > 0, 2, np.where(w[:, 1] > 0, 1, 0)))
        else:
            raise ValueError(rule)
        act.append(np.where(target < c0, 0, np.where(target < c1, 1, np.where(target < c2, 2, last))))
    for x in (s_lo, total, target):
        assert x.dtype == F
    return np.where(target < s_lo, act[0], 4 + act[1]).astype(np.uint8), e, target, total


# Pinned draws: (seed, arena_base, arena within the handle, counter, the uniform's 24 bits), found by a search
# over seeds with policy_ref.policy_uniform (about 2^24 seeds per hit).  Counters of the per-tick kernels are the
# tick; of P2 in the per-decision self-play kernel, decision + (tick within it << 40).
TICK_PINS = (
    (3747935, 0, 0, 0, TOP), (1806949, 0, 37, 0, SECOND), (15855147, 45, 33, 5, TOP), (416923, 45, 64, 31, SECOND),
    (5374434, 0, 1, 0, TOP), (6245250, 0, 63, 0, SECOND), (17991487, 45, 5, 3, TOP), (6715914, 45, 69, 5, SECOND))
# (Decision 1, not 0: a fresh arena's first decision is one tick long whatever P1 does -- the first frame of a
# move shows move_frame 0, which is not skippable -- while an attack held into decision 1 runs on for ticks.)
SKIP_PINS = (
    (4309194, 0, 2, 1 + (1 << 40), TOP), (2693467, 45, 40, 1 + (2 << 40), SECOND),
    (25383508, 45, 2, 1 + (1 << 40), SECOND), (3075356, 0, 40, 1 + (2 << 40), TOP))
# Draws on a boundary: for all eight actions live, u = k / 8 makes target = k exactly, the threshold between
# actions k - 1 and k, where "the first action whose cumulative weight exceeds the target" is k.  Random draws
# land there once in 2^24; these are pinned: BOUNDARY_PINS[k] = (seed, arena_base, arena within the handle,
# counter), with the arena 7 k + 3 and the counter k.
BOUNDARY_PINS = tuple((seed, 45, 7 * k + 3, k) for k, seed in enumerate(
    (13534129, 18373408, 7387884, 7015673, 24391144, 1770404, 2481367, 4163399)))
BOUNDARY_N = 70  # arenas of a boundary launch
ZERO_WEIGHT_N = 75  # arenas of a zero-weight launch: every pinned arena, 150 lanes, a part-filled third wave


def zero_weight_cases():
    """Logits for which the upper half's running thresholds end below the softmax total although the last
    action's weight is exactly 0.  One action k of the lower half has weight 1; family 0: actions 4, 5, 6 have
    e^-17.19 = 3.4e-8 each -- below half an ulp of 1, together above it -- and 7 is dead; family 1: 4 and 5 have
    e^-16.98 = 4.2e-8 (each within (2^-25, 2^-24)), 6 and 7 are dead.  Either way every threshold rounds to 1.0
    and total = 1 + 2^-23, so a uniform of 1 - 2^-24 or 1 - 2^-23 gives target = 1.0 >= c2.  Each case: its name,
    b3, the actions of non-zero weight, and one pinned draw for the per-tick kernels and one for P2's
    decision-tick counter."""
    out = []
    for fam, (g, upper) in enumerate(((17.19, (4, 5, 6)), (16.98, (4, 5)))):
        for k in range(4):
            b3 = np.full(8, DEAD, dtype=F)
            b3[k] = 0.0
            b3[list(upper)] = -g
            out.append(dict(name="g%.2f-live%d" % (g, k), b3=b3, allowed=(k,) + upper, tick=TICK_PINS[4 * fam + k],
                            skip=SKIP_PINS[(k + fam) % 4]))
    return out


def kernel_logits(b3):
    """What the kernel holds for b3 when W3 = 0: the bf16 hi + lo pair, summed in float32 (exact: the pair's
    bits do not overlap)."""
    b3 = np.asarray(b3, dtype=F)
    hi = policy_ref.bf16(b3)
    return hi + policy_ref.bf16(b3 - hi)
