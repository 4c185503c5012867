#!/usr/bin/env python3
"""Self-play per agent decision: the fused launch beside its two parents (measurement only).

  python tools/selfplay_skip_time.py [--rounds R] [--envs N] [--launches L] [--decisions D] [--warmup W]

One GPU, N arenas (default 65 536), one rollout.make_actor actor, three legs on three handles,
alternating in one process so drift of the box hits all of them:

  skip_selfplay  FusedSelfPlayRollout.rollout_skipped: D (64) decisions per launch with a trajectory,
                 P1's samples, ticks and capped; the opponent is the mirrored copy of the actor and
                 acts on every tick (fs_step_skip_selfplay); a remote-P2 handle
  selfplay       FusedSelfPlayRollout.rollout on a handle created alike: D ticks per launch, the
                 same two actors per tick (fs_step_n_selfplay)
  skip_bot       FusedPolicyRollout.rollout_skipped against the in-game bot: D decisions per launch
                 (fs_step_skip_policy)

Each round times L launches of every leg with a host clock around work that ends in a device
synchronise, after W warm-up launches of each.  The two skip legs keep every launch's tick counts
(read after the clock stops), so a round's env ticks are counted, not estimated.  Reported per round
and as median (min .. max): decisions/s and env ticks/s (arena ticks per second) of skip_selfplay, env
ticks/s of selfplay, decisions/s of skip_bot; then the mean ticks per decision of both skip legs and
the share of skip_selfplay's wave ticks that are an arena's own work: a wave of 32 arenas runs until
its slowest arena has finished its D decisions, so the share is the sum of all arenas' ticks over
32 x the sum of the waves' maxima of per-arena tick sums.  Beside it, the same share with every
wave charged the launch's slowest arena (all waves of 65 536 arenas are resident at once, so a
launch lasts as long as its slowest wave and nothing fills the SIMDs the others leave).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WAVE = 32  # arenas per wave (two lanes each)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--launches", type=int, default=8, help="launches per leg and round")
    ap.add_argument("--decisions", type=int, default=64, help="decisions (selfplay: ticks) per launch")
    ap.add_argument("--warmup", type=int, default=2, help="launches of each leg before the rounds")
    a = ap.parse_args()
    import torch
    from footsies_gym_amd.rollout import FusedPolicyRollout, FusedSelfPlayRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    if not torch.cuda.is_available():
        sys.exit("selfplay_skip_time: no GPU (a timing needs one)")
    dev = torch.device("cuda", 0)
    N, D, L = a.envs, a.decisions, a.launches
    actor = make_actor(device=dev, seed=4)
    ksim, ssim = (FootsiesSim(N, p2_mode="external", seed=3) for _ in range(2))
    bsim = FootsiesSim(N, p2_mode="bot", seed=3)
    skip_sp = FusedSelfPlayRollout(ksim, actor, seed=7, opponent_seed=8, mirror=True)  # (opponent: the copy)
    sp = FusedSelfPlayRollout(ssim, actor, seed=7, opponent_seed=8, mirror=True)
    skip_bot = FusedPolicyRollout(bsim, actor, seed=7)
    trajs = [s.alloc_trajectory(D) for s in (ksim, ssim, bsim)]
    acts = [torch.empty((D, N), dtype=torch.uint8, device=dev) for _ in range(3)]
    logp = [torch.empty((D, N), dtype=torch.float32, device=dev) for _ in range(3)]
    capped = [torch.empty((D, N), dtype=torch.uint8, device=dev) for _ in range(2)]
    ticks = {name: torch.zeros((L, D, N), dtype=torch.int32, device=dev) for name in ("skip_selfplay", "skip_bot")}

    def skip_selfplay_launch(i):
        skip_sp.rollout_skipped(D, acts[0], logp[0], ticks["skip_selfplay"][i], capped[0], trajectory=trajs[0])

    def selfplay_launch(i):
        sp.rollout(D, acts[1], logp[1], False, False, trajectory=trajs[1])

    def skip_bot_launch(i):
        skip_bot.rollout_skipped(D, acts[2], logp[2], ticks["skip_bot"][i], capped[1], trajectory=trajs[2])

    def timed(fn, reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(reps):
            fn(i)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    legs = (("skip_selfplay", skip_selfplay_launch), ("selfplay", selfplay_launch), ("skip_bot", skip_bot_launch))
    for name, fn in legs:
        timed(fn, a.warmup)
    print("# %d arenas; %d launches x %d decisions (selfplay: ticks) per leg and round; the opponent is the mirrored "
          "copy of the actor" % (N, L, D), flush=True)
    rate = {k: [] for k in ("skip_selfplay decisions/s", "skip_selfplay env ticks/s", "selfplay env ticks/s",
                            "skip_bot decisions/s", "skip_bot env ticks/s")}
    tpd = {"skip_selfplay": [], "skip_bot": []}
    share, share_launch = [], []
    full = N // WAVE * WAVE
    for r in range(a.rounds):
        for name, fn in legs:
            dt = timed(fn, L)
            line = "round %d %-13s %8.3f ms/launch" % (r, name, 1e3 * dt / L)
            if name == "selfplay":
                rate["selfplay env ticks/s"].append(L * D * N / dt)
                line += "  %.3e env ticks/s" % rate["selfplay env ticks/s"][-1]
            else:
                t = ticks[name]
                total = int(t.sum(dtype=torch.int64))
                rate[name + " decisions/s"].append(L * D * N / dt)
                rate[name + " env ticks/s"].append(total / dt)
                tpd[name].append(total / (L * D * N))
                line += "  %.3e decisions/s  %.3e env ticks/s  %.3f ticks/decision" % (
                    rate[name + " decisions/s"][-1], rate[name + " env ticks/s"][-1], tpd[name][-1])
                if name == "skip_selfplay" and full:
                    per_arena = t[:, :, :full].sum(dim=1, dtype=torch.int64).view(L, -1, WAVE)  # [L][waves][32]
                    wave_ticks = int(per_arena.max(dim=2).values.sum())
                    share.append(int(per_arena.sum()) / (WAVE * wave_ticks))
                    share_launch.append(int(per_arena.sum()) / (full * int(per_arena.amax(dim=(1, 2)).sum())))
                    line += "  own-work share of wave ticks %.3f (of the slowest wave's: %.3f)" % (share[-1], share_launch[-1])
            print(line, flush=True)

    def med(v):
        s = sorted(v)
        return s[len(s) // 2], s[0], s[-1]
    for k, v in rate.items():
        print("%-26s median %.3e (min %.3e .. max %.3e)" % ((k,) + med(v)), flush=True)
    for k, v in tpd.items():
        print("%-13s mean ticks per decision: median %.3f (min %.3f .. max %.3f)" % ((k,) + med(v)), flush=True)
    if share:
        print("skip_selfplay share of wave ticks that are an arena's own work: median %.3f (min %.3f .. max %.3f)" % med(share),
              flush=True)
        print("  ... with every wave charged its launch's slowest arena: median %.3f (min %.3f .. max %.3f)" % med(share_launch),
              flush=True)
        m = med(rate["skip_selfplay env ticks/s"])[0] / med(rate["selfplay env ticks/s"])[0]
        print("skip_selfplay / selfplay env ticks/s (medians): %.3f (expected, unmeasured before: about the share above)" % m,
              flush=True)
    for s in (ksim, ssim, bsim):
        s.close()


if __name__ == "__main__":
    main()
