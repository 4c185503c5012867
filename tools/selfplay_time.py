#!/usr/bin/env python3
"""Self-play rollouts: the fused launch against one in-kernel actor and against the per-tick loop (measurement only).

  python tools/selfplay_time.py [--rounds R] [--envs N] [--launches L] [--ticks T] [--baseline B] [--warmup W]

One GPU, N arenas (default 65 536) with a remote P2, rollout.make_actor actors, three legs on three
handles created alike, alternating in one process so drift of the box hits all of them:

  selfplay   FusedSelfPlayRollout.rollout: T (64) ticks per launch with a trajectory and all four
             sample arrays, both fighters sampled in the kernel, P2 mirrored (fs_step_n_selfplay);
             L launches per round
  one_actor  FusedPolicyRollout.rollout on the same kind of handle with P2's inputs read from hashed
             action rows [T][N] made before the rounds (fs_step_n_policy): the same launch without
             the second actor, so selfplay - one_actor is what the second actor costs
  loop       what the fused launch replaces: per tick, two torch actor forwards with sampling
             (PolicyRollout._step's feature / sample code; P2's on mirror_features, its index through
             swap_left_right) and one fs_step with the device actions, eager, no host
             synchronisation per tick; B ticks per round

Each round times every leg with a host clock around work that ends in a device synchronise, after W
warm-up launches (x 8: loop ticks) of each.  Reported: ms per launch, us per tick and env-steps/s
(arena ticks per second) per round, then the median and the spread (min .. max) per leg, the ratio
selfplay / one_actor per tick, and whether every fused round beat every round of the loop.
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
    ap.add_argument("--launches", type=int, default=40, help="fused launches per round (both fused legs)")
    ap.add_argument("--ticks", type=int, default=64, help="ticks per fused launch")
    ap.add_argument("--baseline", type=int, default=640, help="loop ticks per round")
    ap.add_argument("--warmup", type=int, default=3, help="fused launches (x 8: loop ticks) before the rounds")
    a = ap.parse_args()
    import torch
    from footsies_gym_amd.rollout import (FusedPolicyRollout, FusedSelfPlayRollout, PolicyRollout, make_actor,
                                          mirror_features, swap_left_right)
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("selfplay_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, T = a.envs, a.ticks
    actor, opponent = make_actor(device=dev, seed=4), make_actor(device=dev, seed=5)
    ssim, osim, lsim = (FootsiesSim(N, p2_mode="external", seed=3) for _ in range(3))
    selfplay = FusedSelfPlayRollout(ssim, actor, opponent=opponent, seed=7, opponent_seed=8, mirror=True)
    one = FusedPolicyRollout(osim, actor, seed=7)
    straj, otraj = ssim.alloc_trajectory(T), osim.alloc_trajectory(T)
    acts, acts2, oacts = (torch.empty((T, N), dtype=torch.uint8, device=dev) for _ in range(3))
    logp, logp2, ologp = (torch.empty((T, N), dtype=torch.float32, device=dev) for _ in range(3))
    p2_rows = osim.hash_actions(T, seed=11)[1]
    loop = PolicyRollout(lsim, actor)  # (its action / logp buffers and feature divisors; P2's beside them)
    act2 = torch.zeros(N, dtype=torch.uint8, device=dev)
    logp2_row = torch.zeros(N, dtype=torch.float32, device=dev)

    def selfplay_launch():
        selfplay.rollout(T, acts, logp, acts2, logp2, trajectory=straj)

    def one_actor_launch():
        one.rollout(T, oacts, ologp, p2_actions=p2_rows, trajectory=otraj)

    def sample(net, x, action, lp):
        logits = net(x)
        act = torch.argmax(logits - torch.empty_like(logits).exponential_().log_(), dim=1)
        torch.gather(torch.log_softmax(logits, dim=1), 1, act[:, None], out=lp.view(-1, 1))
        action.copy_(act)

    def loop_tick():
        out = lsim.outputs()
        with torch.no_grad():  # (PolicyRollout._step up to its fs_step call, once per fighter)
            x = torch.cat([out["guard"].float(), out["move"].float(), out["move_frame"], out["position"]], dim=1)
            x.div_(loop._div)
            sample(actor, x, loop.action, loop.logp)
            sample(opponent, mirror_features(x), act2, logp2_row)
            lsim.step(loop.action, swap_left_right(act2))

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    legs = (("selfplay", selfplay_launch, a.launches, T), ("one_actor", one_actor_launch, a.launches, T),
            ("loop", loop_tick, a.baseline, 1))
    for name, fn, reps, per in legs:
        timed(fn, a.warmup * (8 if per == 1 else 1))
    print("# %d arenas, a remote P2; fused legs: %d launches x %d ticks per round, loop: %d ticks per round" % (
        N, a.launches, T, a.baseline), flush=True)
    res = {name: [] for name, _, _, _ in legs}
    for r in range(a.rounds):
        for name, fn, reps, per in legs:
            dt = timed(fn, reps)
            ticks = reps * per
            res[name].append(dt / ticks)
            print("round %d %-9s %9s  %8.3f us/tick  %.3e env-steps/s" % (
                r, name, "%.3f ms/launch" % (1e3 * dt / reps) if per > 1 else "", 1e6 * dt / ticks, ticks * N / dt), flush=True)
    med = {}
    for name, v in res.items():
        s = sorted(v)
        med[name] = s[len(s) // 2]
        print("%-9s us/tick median %.3f (min %.3f .. max %.3f)  env-steps/s median %.3e (min %.3e .. max %.3e)" % (
            name, 1e6 * med[name], 1e6 * s[0], 1e6 * s[-1], N / med[name], N / s[-1], N / s[0]), flush=True)
    worst_fused = max(res["selfplay"] + res["one_actor"])
    print("selfplay / one_actor (median us/tick): %.2f; loop / selfplay: %.1f; the loop's own spread max / min: %.3f; "
          "every fused round ahead of every loop round: %s" % (
              med["selfplay"] / med["one_actor"], med["loop"] / med["selfplay"], max(res["loop"]) / min(res["loop"]),
              worst_fused < min(res["loop"])), flush=True)
    for s in (ssim, osim, lsim):
        s.close()


if __name__ == "__main__":
    main()
