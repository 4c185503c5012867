#!/usr/bin/env python3
"""Policy rollouts at decision granularity: the fused launch against the per-decision loop (measurement only).

  python tools/skip_policy_time.py [--rounds R] [--envs N] [--launches L] [--decisions D] [--baseline B] [--warmup W]

One GPU, N arenas (default 65 536) against the in-game bot, a rollout.make_actor actor, two legs on
two handles created alike, alternating in one process so drift of the box hits both:

  fused      FusedPolicyRollout.rollout_skipped: D (64) agent decisions per launch with a trajectory,
             L launches per round (fs_step_skip_policy, the actor in the kernel)
  baseline   the per-decision loop: the torch actor's forward on sim.outputs() and its sampling
             (PolicyRollout._step's feature / sample code), then one sim.step_skip launch with the
             device actions; B decisions per round.  The pending count is not read back (no host
             synchronisation per decision), and each decision's tick counts are added up on the
             device (one [N] add per decision, inside the timed window: under 1 % of a decision;
             the fused leg sums its [D][N] tick array once per launch the same way).

Each round times both legs with a host clock around work that ends in a device synchronise, after
W warm-up launches / decisions of each.  Reported: decisions/s and env ticks/s (arena decisions and
arena ticks per second) per round, then the median and the spread (min .. max) per leg, and whether
every fused round beat every baseline round.  From the fused leg's last `ticks` array on the host:
the mean ticks per decision, and the mean over waves (32 consecutive arenas) of the per-decision
maximum -- a wave's lanes stay in the tick loop until its slowest arena leaves, so mean / mean-of-max
is the share of the loop's tick issue that does an arena's work.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=40, help="fused launches per round")
    ap.add_argument("--decisions", type=int, default=64, help="decisions per fused launch")
    ap.add_argument("--baseline", type=int, default=640, help="baseline decisions per round")
    ap.add_argument("--warmup", type=int, default=3, help="fused launches (x 8: baseline decisions) before the rounds")
    a = ap.parse_args()
    import numpy as np
    import torch
    from footsies_gym_amd.rollout import FusedPolicyRollout, PolicyRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("skip_policy_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, D = a.envs, a.decisions
    actor = make_actor(device=dev, seed=4)
    fsim, bsim = (FootsiesSim(N, p2_mode="bot", seed=3) for _ in range(2))
    fused = FusedPolicyRollout(fsim, actor, seed=7)
    traj = fsim.alloc_trajectory(D)
    acts = torch.empty((D, N), dtype=torch.uint8, device=dev)
    logp = torch.empty((D, N), dtype=torch.float32, device=dev)
    ticks = torch.empty((D, N), dtype=torch.int32, device=dev)
    capped = torch.empty((D, N), dtype=torch.uint8, device=dev)
    base = PolicyRollout(bsim, actor)
    bticks = torch.zeros(N, dtype=torch.int64, device=dev)

    fticks = torch.zeros((), dtype=torch.int64, device=dev)

    def fused_launch():
        fused.rollout_skipped(D, acts, logp, ticks, capped, trajectory=traj)
        fticks.add_(ticks.sum(dtype=torch.int64))

    def baseline_decision():
        out = bsim.outputs()
        with torch.no_grad():  # (PolicyRollout._step up to its fs_step call)
            x = torch.cat([out["guard"].float(), out["move"].float(), out["move_frame"], out["position"]], dim=1)
            logits = base.actor(x.div_(base._div))
            act = torch.argmax(logits - torch.empty_like(logits).exponential_().log_(), dim=1)
            torch.gather(torch.log_softmax(logits, dim=1), 1, act[:, None], out=base.logp.view(-1, 1))
            base.action.copy_(act)
        bsim.step_skip(base.action)
        bticks.add_(bsim.skip_ticks)

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    timed(fused_launch, a.warmup)
    timed(baseline_decision, 8 * a.warmup)
    print("# %d arenas vs the bot, fused: %d launches x %d decisions per round, baseline: %d decisions per round" % (
        N, a.launches, D, a.baseline), flush=True)
    res = {"fused": [], "baseline": []}
    for r in range(a.rounds):
        fticks.zero_()
        dt = timed(fused_launch, a.launches)
        ft, n_dec = int(fticks), a.launches * D * N
        res["fused"].append((n_dec / dt, ft / dt))
        print("round %d fused     %8.3f ms/launch %8.4f ms/decision  %.3e decisions/s  %.3e ticks/s  %.2f ticks/decision" % (
            r, 1e3 * dt / a.launches, 1e3 * dt / (a.launches * D), n_dec / dt, ft / dt, ft / float(n_dec)), flush=True)
        bticks.zero_()
        dt = timed(baseline_decision, a.baseline)
        bt = int(bticks.sum())
        res["baseline"].append((a.baseline * N / dt, bt / dt))
        print("round %d baseline  %8s %11s %8.4f ms/decision  %.3e decisions/s  %.3e ticks/s  %.2f ticks/decision" % (
            r, "", "", 1e3 * dt / a.baseline, a.baseline * N / dt, bt / dt, bt / float(a.baseline * N)), flush=True)
    for leg, v in res.items():
        d, t = sorted(x[0] for x in v), sorted(x[1] for x in v)
        print("%-9s decisions/s median %.3e (min %.3e .. max %.3e)  ticks/s median %.3e (min %.3e .. max %.3e)" % (
            leg, d[len(d) // 2], d[0], d[-1], t[len(t) // 2], t[0], t[-1]), flush=True)
    fd, bd = [x[0] for x in res["fused"]], [x[0] for x in res["baseline"]]
    print("fused / baseline (median decisions/s): %.2f; baseline's own spread max / min: %.3f; every fused round ahead "
          "of every baseline round: %s" % (sorted(fd)[len(fd) // 2] / sorted(bd)[len(bd) // 2], max(bd) / min(bd),
                                           min(fd) > max(bd)), flush=True)
    tk = ticks.cpu().numpy().astype(np.int64)
    waves = tk[:, :N // 32 * 32].reshape(D, -1, 32)
    mean, wmax = float(tk.mean()), float(waves.max(axis=2).mean())
    print("ticks per decision (last fused launch): mean %.3f, max %d, capped %d; per-wave maximum, mean over waves and "
          "decisions: %.3f; mean / mean-of-max = %.3f of the divergent loop's tick issue is an arena's own work" % (
              mean, int(tk.max()), int(capped.sum()), wmax, mean / wmax), flush=True)
    fsim.close()
    bsim.close()


if __name__ == "__main__":
    main()
