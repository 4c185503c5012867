#!/usr/bin/env python3
"""Self-play against a pool of opponents: the pool launch against the single-opponent launch and against
what a pool cost before it (measurement only).

  python tools/selfplay_pool_time.py [--rounds R] [--envs N] [--ticks T] [--launches L] [--dlaunches D] [--warmup W]

One GPU, N arenas (default 65 536) with a remote P2, rollout.make_actor actors, six legs alternating in one
process so drift of the box hits all of them, first per tick (rollout: T = 64 ticks per launch with a
trajectory and all four sample arrays), then per decision (rollout_skipped: T decisions per launch with a
trajectory, P2's samples off):

  single    FusedSelfPlayRollout against one opponent (fs_step_n_selfplay / fs_step_skip_selfplay), handle A
  pool1     the pool launch with a pool of one holding that opponent, on handle A and single's buffers too:
            the two legs take turns over one game (the pool launch continues it bit for bit), so pool1 /
            single is the kernel's own difference: the slot byte and the staging address
  single_b  the controls: what single and pool1 do, both with the single-opponent launch, on a second
  single_b2 handle B created alike with buffers of its own.  B's game is A's bit for bit at every step, so
            single_b / single and single_b2 / pool1 are what a handle and its buffers make
  pool8     the pool launch with eight snapshots under a random assignment (OpponentPool.assign, latest = 0),
            on a handle of its own: other opponents, so another game (per decision: other tick counts)
  split8    a pool without the pool launch: eight handles of N / 8 arenas, one opponent each, eight
            launches per step (each handle at or below one wave per SIMD for N = 65 536)

Each round times every leg with a host clock around work that ends in a device synchronise, after W warm-up
steps of each.  Reported per form: ms per step (a step is one launch, eight for split8) per round, then the
median and the spread (min .. max) per leg, each leg's median over single's, and whether it lies inside the
spread of single's rounds.
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
    ap.add_argument("--ticks", type=int, default=64, help="ticks (decisions) per launch")
    ap.add_argument("--launches", type=int, default=200, help="per-tick steps per round")
    ap.add_argument("--dlaunches", type=int, default=20, help="per-decision steps per round")
    ap.add_argument("--warmup", type=int, default=2, help="steps of each leg before the rounds")
    a = ap.parse_args()
    import torch
    from footsies_gym_amd.rollout import FusedSelfPlayRollout, OpponentPool, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("selfplay_pool_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, T, K = a.envs, a.ticks, 8
    if N % (K * 128):
        sys.exit("selfplay_pool_time: --envs must be a multiple of %d" % (K * 128))
    actor = make_actor(device=dev, seed=4)
    snapshots = [make_actor(device=dev, seed=5 + i) for i in range(K)]

    def buffers(sim):
        n = sim.num_envs
        return dict(traj=sim.alloc_trajectory(T), a1=torch.empty((T, n), dtype=torch.uint8, device=dev),
                    lp1=torch.empty((T, n), dtype=torch.float32, device=dev),
                    a2=torch.empty((T, n), dtype=torch.uint8, device=dev),
                    lp2=torch.empty((T, n), dtype=torch.float32, device=dev),
                    ticks=torch.empty((T, n), dtype=torch.int32, device=dev),
                    capped=torch.empty((T, n), dtype=torch.uint8, device=dev))

    def step_fns(ro, b, **slots):
        def tick():
            ro.rollout(T, b["a1"], b["lp1"], b["a2"], b["lp2"], trajectory=b["traj"], **slots)

        def decision():
            ro.rollout_skipped(T, b["a1"], b["lp1"], b["ticks"], b["capped"], trajectory=b["traj"], **slots)
        return tick, decision

    sims = [FootsiesSim(N, p2_mode="external", seed=3) for _ in range(3)]
    shared = buffers(sims[0])
    single = step_fns(FusedSelfPlayRollout(sims[0], actor, opponent=snapshots[0], seed=7, opponent_seed=8), shared)
    other, eighth = buffers(sims[1]), buffers(sims[2])
    single_b = step_fns(FusedSelfPlayRollout(sims[1], actor, opponent=snapshots[0], seed=7, opponent_seed=8), other)
    pool1 = OpponentPool(sims[0], 1, snapshots[0])
    one = step_fns(FusedSelfPlayRollout(sims[0], actor, seed=7, opponent_seed=8, pool=pool1), shared, slots=pool1.assign(0))
    pool8 = OpponentPool(sims[2], K)
    for s in snapshots:
        pool8.push(s)
    slots8 = pool8.assign(0, latest=0.0, seed=1)
    eight = step_fns(FusedSelfPlayRollout(sims[2], actor, seed=7, opponent_seed=8, pool=pool8), eighth, slots=slots8)
    parts = [FootsiesSim(N // K, p2_mode="external", seed=3, arena_base=i * (N // K)) for i in range(K)]
    split = [step_fns(FusedSelfPlayRollout(p, actor, opponent=snapshots[i], seed=7, opponent_seed=8), buffers(p))
             for i, p in enumerate(parts)]

    def split_step(form):
        def step():
            for fns in split:
                fns[form]()
        return step

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print("# %d arenas, a remote P2, P2 mirrored; pool8's slots over %d groups: %s" % (
        N, slots8.numel(), torch.bincount(slots8.long(), minlength=K).tolist()), flush=True)
    for form, what, reps in ((0, "tick", a.launches), (1, "decision", a.dlaunches)):
        legs = (("single", single[form]), ("single_b", single_b[form]), ("pool1", one[form]), ("single_b2", single_b[form]),
                ("pool8", eight[form]), ("split8", split_step(form)))
        for _, fn in legs:
            timed(fn, a.warmup)
        print("## per %s: %d steps of %d %ss per round" % (what, reps, T, what), flush=True)
        res = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in legs:
                dt = timed(fn, reps)
                res[name].append(dt / reps)
                print("round %d %-9s %9.3f ms/step  %.3e arena-%ss/s" % (r, name, 1e3 * dt / reps, reps * T * N / dt, what),
                      flush=True)
        lo, hi = min(res["single"]), max(res["single"])
        med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
        for name, v in res.items():
            print("%-9s ms/step median %.3f (min %.3f .. max %.3f)  / single %.3f  median inside single's spread: %s" % (
                name, 1e3 * med[name], 1e3 * min(v), 1e3 * max(v), med[name] / med["single"], lo <= med[name] <= hi),
                flush=True)
        if form == 1:  # what the games cost: the launch lasts as long as its slowest arena's sum of ticks
            for name, b in (("single", shared), ("single_b", other), ("pool8", eighth)):
                t = b["ticks"].long()
                print("%-9s last launch: %.3f ticks per decision, the slowest arena's %d decisions ran %d ticks" % (
                    name, float(t.float().mean()), T, int(t.sum(0).max())), flush=True)
    for s in sims + parts:
        s.close()


if __name__ == "__main__":
    main()
