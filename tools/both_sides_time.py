#!/usr/bin/env python3
"""PPO self-play learning from both sides: what P2's samples cost and what they add (measurement only).

  python tools/both_sides_time.py [--rounds R] [--envs N] [--horizon T] [--iters I] [--warmup W] [--reps K]
                                  [--root TREE] [--tag NAME]

One GPU, N arenas (default 65 536) with a remote P2, horizon T (default 128), PPOTrainer(self_play=True) with its
defaults otherwise (opponent_refresh=1: every rollout's P2 plays the learner's weights, so with both_sides every
arena's P2 samples are learnt from).  Two trainers, `off` (both_sides=False) and `on` (both_sides=True), each over
a handle of its own, alternate in one process so drift of the box hits both; each round times I iterations of each
(default 30), every iteration with a host clock between two device synchronises, after W warm-up iterations of
each.  Reported per leg: the mean ms per iteration of each round, then the median and the spread (min .. max)
over the rounds, the samples learnt per second (P1's rows plus P2's, `p2_rows` of the trainer's stats), and
on / off.

Then the two P2 kernels beside their one-side neighbours on the same shapes ([T][N] trajectory columns, every
arena selected, first through the identity and then through an explicit index vector), as device-event times over
K launches each: fs_ppo_features against fs_ppo_features_p2, fs_ppo_gae against fs_ppo_gae_p2.

--root TREE imports footsies_gym_amd from another checkout (built there), e.g. the parent commit's: a tree whose
PPOTrainer has no `both_sides` runs the `off` leg alone and skips the kernels it lacks, so the same tool times
both trees and a driver can alternate them.  --tag names the tree in every line.  Fails when there is no GPU.
"""
import argparse
import inspect
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--iters", type=int, default=30, help="PPO iterations per leg and round")
    ap.add_argument("--warmup", type=int, default=2, help="iterations of each leg before the rounds")
    ap.add_argument("--reps", type=int, default=20, help="launches per kernel timing")
    ap.add_argument("--root", default=ROOT, help="the checkout to import footsies_gym_amd from")
    ap.add_argument("--tag", default="tree")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    import torch
    from footsies_gym_amd import ppo
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("both_sides_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, T = a.envs, a.horizon
    has = "both_sides" in inspect.signature(ppo.PPOTrainer.__init__).parameters
    legs = [("off", {})] + ([("on", {"both_sides": True})] if has else [])
    sims, trainers = [], {}
    for name, kw in legs:
        sims.append(FootsiesSim(N, p2_mode="external", seed=3))
        trainers[name] = ppo.PPOTrainer(sims[-1], horizon=T, seed=1, self_play=True, **kw)

    def timed(tr, iters):
        total = 0.0
        for _ in range(iters):  # each iteration between two device synchronises: nothing of the next one overlaps it
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.iterate()
            torch.cuda.synchronize()
            total += time.perf_counter() - t0
        return total / iters

    print("# %s: %d arenas, a remote P2 (mirrored self-play, opponent_refresh=1), horizon %d, %d iterations per leg "
          "and round; both_sides %s" % (a.tag, N, T, a.iters, "available" if has else "not in this tree"), flush=True)
    for name, _ in legs:
        timed(trainers[name], a.warmup)
    res = {name: [] for name, _ in legs}
    rows = {}
    for r in range(a.rounds):
        for name, _ in legs:
            dt = timed(trainers[name], a.iters)
            res[name].append(dt)
            rows[name] = T * N + int(trainers[name].stats.get("p2_rows", 0))
            print("%s round %d %-3s %9.3f ms/iteration  %d samples learnt  %.3e samples/s" % (
                a.tag, r, name, 1e3 * dt, rows[name], rows[name] / dt), flush=True)
    med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
    for name, v in res.items():
        print("%s %-3s ms/iteration median %.3f (min %.3f .. max %.3f)  %.3e samples learnt/s  / off %.3f" % (
            a.tag, name, 1e3 * med[name], 1e3 * min(v), 1e3 * max(v), rows[name] / med[name], med[name] / med["off"]),
            flush=True)
    if has:
        print("%s on / off: %.3f x the time for %.3f x the samples: %.3f x the samples learnt per second" % (
            a.tag, med["on"] / med["off"], rows["on"] / rows["off"],
            (rows["on"] / med["on"]) / (rows["off"] / med["off"])), flush=True)

    # ---- the kernels, on the last rollout's trajectory of the `off` leg
    tr = trainers["off"]
    traj, rew, done = tr.traj, tr.traj["reward"], tr.traj["terminated"]
    val = torch.randn((T + 1, N), device=dev)
    out = torch.empty((T, N, 8), dtype=torch.float32, device=dev)
    ident = torch.arange(N, dtype=torch.int32, device=dev)

    def event_ms(fn):
        fn()
        times = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        times.sort()
        return times[len(times) // 2], times[0], times[-1]

    kernels = [("fs_ppo_features", lambda: ppo.features_device(traj, out)),
               ("fs_ppo_gae", lambda: ppo.gae_device(rew, done, val, 0.99, 0.95))]
    if has:
        kernels += [("fs_ppo_features_p2 sel=NULL", lambda: ppo.features_device(traj, out, p2=True)),
                    ("fs_ppo_features_p2 sel=0..N-1", lambda: ppo.features_device(traj, out, p2=True, sel=ident)),
                    ("fs_ppo_gae_p2 sel=NULL", lambda: ppo.gae_device(rew, done, val, 0.99, 0.95, p2=True)),
                    ("fs_ppo_gae_p2 sel=0..N-1", lambda: ppo.gae_device(rew, done, val, 0.99, 0.95, p2=True, sel=ident))]
    print("## %s kernels at [%d][%d]: device-event ms over %d launches (gae_device's include its two output "
          "allocations, the same in every row)" % (a.tag, T, N, a.reps), flush=True)
    for name, fn in kernels:
        m, lo, hi = event_ms(fn)
        print("%s %-30s median %.4f ms (min %.4f .. max %.4f)" % (a.tag, name, m, lo, hi), flush=True)
    for s in sims:
        s.close()


if __name__ == "__main__":
    main()
