#!/usr/bin/env python3
"""Self-play leagues: the league launch against the pool launch it extends, and what a bot group costs beside a
remote one (measurement only).

  python tools/league_time.py [--rounds R] [--envs N] [--ticks T] [--launches L] [--dlaunches D] [--warmup W]

One GPU, N arenas (default 65 536) with a remote P2, rollout.make_actor actors, a pool of eight snapshots under
one random assignment, the legs alternating in one process so drift of the box hits all of them, first per tick
(rollout: T = 64 ticks per launch with a trajectory and all four sample arrays), then per decision
(rollout_skipped: T decisions per launch with a trajectory, P2's samples off):

  pool       FusedSelfPlayRollout(pool=...) (fs_step_n_selfplay_pool / fs_step_skip_selfplay_pool), handle A
  league0    the league launch (fs_step_n_league / fs_step_skip_league) with no group on the bot, on handle A and
             pool's buffers too: the two legs take turns over one game (the league launch continues it bit for
             bit), so league0 / pool is the kernel's own difference: the header read and the block's branch
  pool_b     the controls: what pool and league0 do, both with the pool launch, on a second handle B created
  pool_b2    alike with buffers of its own.  B's game is A's bit for bit at every step, so pool_b / pool and
             pool_b2 / league0 are what a handle and its buffers make
  league25   the league launch with a quarter of the groups on the bot (rollout.bot_groups, the draw the trainer
             makes: random groups, not every fourth, which would put the bot blocks on two of the eight XCDs), on a
             handle of its own: another game
  league100  the league launch with every group on the bot, on a handle of its own
  policy_bot per tick only: fs_step_n_policy (FusedPolicyRollout under P2 rows it ignores) on a handle with every
             arena switched, i.e. league100's game in the kernel the bot body was taken from

Each round times every leg with a host clock around work that ends in a device synchronise, after W warm-up steps
of each.  Reported per form: ms per step (a step is one launch) per round, then the median and the spread
(min .. max) per leg, each leg's median over pool's, and whether it lies inside the spread of pool's rounds.
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
    import numpy as np
    import torch
    from footsies_gym_amd.rollout import (FusedPolicyRollout, FusedSelfPlayRollout, OpponentPool, bot_groups,
                                          make_actor, pool_assignment, pool_groups)
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("league_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, T, K = a.envs, a.ticks, 8
    G = pool_groups(N)
    actor = make_actor(device=dev, seed=4)
    snapshots = [make_actor(device=dev, seed=5 + i) for i in range(K)]
    slots = torch.from_numpy(pool_assignment(1, 0, 0, G, K, K - 1, 0.0)).to(dev)

    def buffers(sim):
        n = sim.num_envs
        return dict(traj=sim.alloc_trajectory(T), a1=torch.empty((T, n), dtype=torch.uint8, device=dev),
                    lp1=torch.empty((T, n), dtype=torch.float32, device=dev),
                    a2=torch.empty((T, n), dtype=torch.uint8, device=dev),
                    lp2=torch.empty((T, n), dtype=torch.float32, device=dev),
                    ticks=torch.empty((T, n), dtype=torch.int32, device=dev),
                    capped=torch.empty((T, n), dtype=torch.uint8, device=dev))

    def pool_of(sim):
        pool = OpponentPool(sim, K)
        for s in snapshots:
            pool.push(s)
        return pool

    def step_fns(sim, b, bots=None):
        ro = FusedSelfPlayRollout(sim, actor, seed=7, opponent_seed=8, pool=pool_of(sim), bots=bots)

        def tick():
            ro.rollout(T, b["a1"], b["lp1"], b["a2"], b["lp2"], trajectory=b["traj"], slots=slots)

        def decision():
            ro.rollout_skipped(T, b["a1"], b["lp1"], b["ticks"], b["capped"], trajectory=b["traj"], slots=slots)
        return tick, decision

    sims = [FootsiesSim(N, p2_mode="external", seed=3) for _ in range(5)]
    shared, other, quarter_b, all_b, policy_b = (buffers(s) for s in sims)
    pool = step_fns(sims[0], shared)
    league0 = step_fns(sims[0], shared, np.zeros(G, bool))
    pool_b = step_fns(sims[1], other)
    quarter = bot_groups(1, 0, G, 0.25)
    league25 = step_fns(sims[2], quarter_b, quarter)
    league100 = step_fns(sims[3], all_b, np.ones(G, bool))
    sims[4].set_p2_mode("bot")
    ro_policy = FusedPolicyRollout(sims[4], actor, seed=7)
    p2_rows = torch.zeros((T, N), dtype=torch.uint8, device=dev)

    def policy_bot():
        ro_policy.rollout(T, policy_b["a1"], policy_b["lp1"], p2_actions=p2_rows, trajectory=policy_b["traj"])

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    print("# %d arenas in %d groups, a remote P2, P2 mirrored, a pool of %d; league25: %d groups on the bot" % (
        N, G, K, int(quarter.sum())), flush=True)
    for form, what, reps in ((0, "tick", a.launches), (1, "decision", a.dlaunches)):
        legs = [("pool", pool[form]), ("pool_b", pool_b[form]), ("league0", league0[form]), ("pool_b2", pool_b[form]),
                ("league25", league25[form]), ("league100", league100[form])]
        if form == 0:
            legs.append(("policy_bot", policy_bot))
        for _, fn in legs:
            timed(fn, a.warmup)
        print("## per %s: %d steps of %d %ss per round" % (what, reps, T, what), flush=True)
        res = {name: [] for name, _ in legs}
        for r in range(a.rounds):
            for name, fn in legs:
                dt = timed(fn, reps)
                res[name].append(dt / reps)
                print("round %d %-10s %9.3f ms/step  %.3e arena-%ss/s" % (r, name, 1e3 * dt / reps, reps * T * N / dt, what),
                      flush=True)
        lo, hi = min(res["pool"]), max(res["pool"])
        med = {name: sorted(v)[len(v) // 2] for name, v in res.items()}
        for name, v in res.items():
            print("%-10s ms/step median %.3f (min %.3f .. max %.3f)  / pool %.3f  median inside pool's spread: %s" % (
                name, 1e3 * med[name], 1e3 * min(v), 1e3 * max(v), med[name] / med["pool"], lo <= med[name] <= hi),
                flush=True)
        if form == 1:  # what the games cost: a block lasts as long as its slowest arena's sum of ticks
            for name, b, bots in (("pool", shared, None), ("league25", quarter_b, quarter), ("league100", all_b, None)):
                t = b["ticks"].long()
                print("%-10s last launch: %.3f ticks per decision, the slowest arena's %d decisions ran %d ticks" % (
                    name, float(t.float().mean()), T, int(t.sum(0).max())), flush=True)
                if bots is not None:
                    m = torch.from_numpy(np.repeat(bots, 128)[:N]).to(dev)
                    print("%-10s   bot groups %.3f ticks per decision (slowest arena %d), remote groups %.3f (%d)" % (
                        name, float(t[:, m].float().mean()), int(t[:, m].sum(0).max()),
                        float(t[:, ~m].float().mean()), int(t[:, ~m].sum(0).max())), flush=True)
    for s in sims:
        s.close()


if __name__ == "__main__":
    main()
