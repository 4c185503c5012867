"""The hit gate of the specialised row loops (fs_kernels.hip wave_has_hit) against the CPU oracle,
bit for bit over every output row and the final canonical state.

A wave of those loops resolves hits, the KO test and the reward only on ticks on which one of its
lanes is hit.  80 arenas are two full two-lane waves and a half-full one; launches of 1, 2, 3 and 41
ticks run from loaded states in which each named event happens on a chosen tick.  The states are
mined from the oracle: a pool of arenas played from reset, then followed for 41 ticks on random
rows, and each case picks the arenas (state and action columns; arenas do not interact) that show
its event where it wants it.  Every case asserts from the oracle's trace alone, before any GPU
result is looked at, that some 32-arena wave-tick has a hit (a hitstun rising, a guard falling or
a round ending) and some has none; the no-hit case asserts that none has.

The cases: no hit anywhere (fighters out of reach, nobody walking forward); proximity without a hit
(the latch sets on the no-hit path, GUARD_PROXIMITY follows); one hit in a wave, alone on its tick,
on the launch's first tick and on the last of the 1-, 2-, 3- and 41-tick launches (both halves of
the unrolled pair); a trade; the overlap that stays after an attack has hit ("multi_hit": every
attack of the frame data has number_of_hit 1, so no second hit exists -- what the data does hold is
the attack going on with its hit count used up, its boxes still overlapping and resolving to no
hit, which takes the no-hit path); a guarded hit (reward -+0.3, no KO); a guard break (the guarded
hits, loaded with no guard left); KOs with their same-step burst, on the first ticks and the last;
hit and no-hit arenas side by side in one wave; and a fighter loaded at vital 0 with no hit, whose
wave must report the round over on its first tick (it is outside the fast set and runs the generic
loop).

At 80 arenas the multi-tick launches run the request-prefetch kernels (kLmFast); a child process
repeats every case with FOOTSIES_PRIO=1, so the same launches run k_step_n / k_step_n_packed in
kLmFastPrio, the benchmark's loop.  With an idle P2 nothing ever hits or pushes back P1, P2 never
holds back and never attacks: the cases that need that (trade, proximity guard, guarded hit, guard
break) exist with a remote P2 only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import compare_outputs, compare_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables as G  # noqa: E402

CHILD = "FOOTSIES_HIT_GATE_CHILD"  # set in the child process that forces the priority slices on
P2 = {"external": _abi.FS_P2_EXTERNAL, "noop": _abi.FS_P2_NOOP}
N, WAVE, TICKS = 80, 32, 41
LAUNCHES = (1, 2, 3, 41)
POOL, WARM = 8192, 700
STAND, GUARD_BREAK, GUARD_PROXIMITY = 0, 310, 350
ATTACKS, STRUCK = (100, 105, 110, 115), (200, 301, 305, 306)  # actionIDs (data/f00.json)
CASES = ("no_hit", "proximity", "one_hit", "trade", "multi_hit", "guarded", "guard_break", "ko", "mixed", "vital0")
NEEDS_P2 = ("proximity", "trade", "guarded", "guard_break")

_CACHE = {}
FRAME_DATA = G.load()  # data/f00.json


def rows(n, seed, p2):
    rng = np.random.default_rng(seed)
    h1 = rng.integers(0, 8, (TICKS, n)).astype(np.uint8)
    h2 = rng.integers(0, 8, (TICKS, n)).astype(np.uint8)  # (an idle P2 ignores its rows; the sim gets none)
    return h1, h2


def trace(oracle_lib, st, h1, h2, p2):
    """The oracle over the rows from the loaded states: per tick the outputs and the state after it."""
    ora = oracle_lib.Oracle(len(st), p2_mode=P2[p2], base_seed=3)
    assert ora.set_state(st) == 0
    outs, states = [], []
    for t in range(len(h1)):
        outs.append(ora.step(h1[t], h2[t] if p2 == "external" else None))
        states.append(ora.state())
    ora.close()
    return outs, states


def real_box_overlap(d, fa, fd_, k):
    """Does a non-proximity hitbox of fighter `fa` (player k) overlap a hurtbox of fighter `fd_`, by
    BoxBase.Overlaps (F:8-26, inclusive, x the centre) over the boxes of their (action, frame) in the
    frame data `d` at their positions (TransformToFightRect, F:706-719), in binary32?"""
    F = np.float32
    acts = {a["id"]: a for a in d["actions"]}

    def boxes(kind, f, sign, base=None):
        out = []
        for h in acts[int(f["action_id"])][kind]:
            if h["win"][0] <= int(f["action_frame"]) <= h["win"][1] and not h.get("proximity", False):
                r = base if h.get("use_base") else h["rect"]
                x = F(f["position_x"]) + F(r[0]) * F(sign)
                hw = F(r[2]) / F(2)
                out.append((x - hw, x + hw, F(r[1]), F(r[1]) + F(r[3])))
        return out
    sa = 1 if k == 0 else -1
    return any(u[1] >= h[0] and u[0] <= h[1] and u[3] >= h[2] and u[2] <= h[3]
               for h in boxes("hitboxes", fa, sa)
               for u in boxes("hurtboxes", fd_, -sa, d["fighter"]["base_hurtbox"]))


def events(st0, outs, states):
    """Per (tick, arena) what the oracle's trace shows: `hit` (a hitstun rose, a guard fell or the
    round ended -- the gate's wave test must have fired), and the kinds the cases name."""
    ev = {k: np.zeros((len(outs), len(st0)), bool) for k in
          ("hit", "trade", "guarded", "guard_break", "ko", "after_hit", "prox")}
    prev = st0
    for t, (o, s) in enumerate(zip(outs, states)):
        pf, f = prev["f"], s["f"]
        term = np.asarray(o["terminated"]).astype(bool)
        stun_up = f["hitstun"] > pf["hitstun"]
        guard_down = f["guard"] < pf["guard"]
        ev["ko"][t] = term
        ev["hit"][t] = term | stun_up.any(1) | guard_down.any(1)
        # (a landed hit stops both fighters: who was hit is who entered a damage or guard action)
        was_hit = np.isin(f["action_id"], STRUCK) & (f["action_frame"] == 0) & stun_up
        ev["trade"][t] = ~term & was_hit.all(1)
        ev["guarded"][t] = ~term & (was_hit & guard_down & np.isin(f["action_id"], STRUCK[1:])).any(1) & \
            (np.abs(np.abs(np.asarray(o["reward"])) - 0.3) < 1e-9)
        ev["guard_break"][t] = ~term & ((f["reserve_action_id"] == GUARD_BREAK) &
                                        (pf["reserve_action_id"] != GUARD_BREAK)).any(1)
        # the attack that hit on the tick before goes on, its hit count at number_of_hit (1 for every
        # attack of the frame data), and a real hitbox of it still overlaps a hurtbox of the opponent
        # (the state after the tick holds the frames and positions its boxes were built from): an
        # overlap that resolves to no hit
        if t > 0:
            attacker = np.isin(f["action_id"], ATTACKS) & (f["action_id"] == pf["action_id"]) & (f["hit_count"] == 1)
            cand = ev["hit"][t - 1] & ~ev["ko"][t - 1] & ~ev["hit"][t]
            for a in np.flatnonzero(cand & attacker.any(1)):
                ev["after_hit"][t, a] = any(attacker[a, k] and real_box_overlap(FRAME_DATA, f[a, k], f[a, 1 - k], k)
                                            for k in range(2))
        ev["prox"][t] = ~ev["hit"][t] & ((f["is_reserve_proximity_guard"] == 1) &
                                         (pf["is_reserve_proximity_guard"] == 0)).any(1)
        prev = s
    return ev


def pool(oracle_lib, p2):
    """POOL arenas played from reset for WARM ticks of hashed actions, then their trace over random
    rows: (states, rows, events)."""
    key = ("pool", p2)
    if key not in _CACHE:
        ora = oracle_lib.Oracle(POOL, p2_mode=P2[p2], base_seed=7)
        ora.reset()
        ora.step_n_hashed(WARM, 0x5EED)
        st = ora.state()
        ora.close()
        h1, h2 = rows(POOL, 0xB1, p2)
        outs, states = trace(oracle_lib, st, h1, h2, p2)
        _CACHE[key] = (st, h1, h2, events(st, outs, states))
    return _CACHE[key]


def far_apart(st, idx):
    """Arenas `idx` as two standing fighters at x = -4 / +4, out of every box's reach."""
    for k, x in ((0, -4.0), (1, 4.0)):
        f = st["f"][idx, k]
        f["position_x"], f["action_id"], f["action_frame"], f["hit_count"], f["hitstun"] = x, STAND, 0, 0, 0
        f["buffer_action_id"], f["reserve_action_id"], f["is_reserve_proximity_guard"] = -1, -1, 0
        f["input_dir_history"], f["attack_hold"] = 0, 0
        st["f"][idx, k] = f


def build_case(oracle_lib, case, p2):
    """(states, h1, h2) of the 80 arenas of `case`."""
    st, h1, h2, ev = pool(oracle_lib, p2)
    quiet = np.flatnonzero(~ev["hit"][[0, 1, 2, TICKS - 1]].any(0))  # no hit on the ticks the cases place one

    def having(kind, t=None, n=1):
        rows_ = ev[kind] if t is None else ev[kind][t:t + 1]
        idx = np.flatnonzero(rows_.any(0))
        assert len(idx) >= n, (case, p2, kind, t, len(idx))
        return idx[:n]

    pick = quiet[:N].copy()
    if case == "no_hit" or case == "vital0":
        pass
    elif case == "proximity":
        pick[[0, 1, 40, 70]] = having("prox", n=4)
    elif case == "one_hit":  # first tick (and the 1-tick launch's last), the 2- and 3-tick launches' last, the 41st
        pick[5], pick[37], pick[66], pick[20] = having("hit", 0)[0], having("hit", 1)[0], having("hit", 2)[0], \
            having("hit", TICKS - 1)[0]
    elif case == "mixed":
        pick[0:32:4] = having("hit", 1, 8)
        pick[64:80:4] = having("hit", 2, 4)
    elif case == "ko":
        got = [having("ko", t)[0] for t in (0, 1, 2, TICKS - 1) if ev["ko"][t].any()]
        assert len(got) >= 2, (case, p2, got)
        pick[[3, 35, 67, 12][:len(got)]] = got
        pick[50:54] = having("ko", n=4)
    elif case != "guard_break":
        kind = {"multi_hit": "after_hit"}.get(case, case)
        pick[[1, 33, 65]] = having(kind, n=3)
    if case == "guard_break":
        pick[[1, 33, 65]] = having("guarded", n=3)
    cst, c1, c2 = st[pick].copy(), h1[:, pick].copy(), h2[:, pick].copy()
    if case == "guard_break":  # the guarded hits of those arenas, with no guard left to take them
        cst["f"]["guard"][[1, 33, 65]] = 0
    if case == "no_hit":  # nobody in reach, nobody walking or dashing forward (P1 backward = Left, P2 = Right)
        far_apart(cst, np.arange(N))
        rng = np.random.default_rng(0xB2)
        c1 = rng.choice(np.array([0, 1, 4, 5], np.uint8), (TICKS, N))
        c2 = rng.choice(np.array([0, 2, 4, 6], np.uint8), (TICKS, N))
    if case == "vital0":  # P1 of arena 9 at vital 0, standing, nothing in reach: the round is over on tick 0
        far_apart(cst, np.array([9]))
        cst["f"]["vital"][9, 0] = 0
        c1[:3, 9] = 0
        c2[:3, 9] = 0
    return cst, c1, c2


def reference(oracle_lib, case, p2):
    """The case's states, rows and oracle trace, with the condition on the trace asserted."""
    key = ("case", case, p2)
    if key not in _CACHE:
        st, h1, h2 = build_case(oracle_lib, case, p2)
        outs, states = trace(oracle_lib, st, h1, h2, p2)
        ev = events(st, outs, states)
        waves = [slice(w, min(w + WAVE, N)) for w in range(0, N, WAVE)]
        wave_hit = np.stack([ev["hit"][:, w].any(1) for w in waves], 1)  # [tick][wave]
        if case == "no_hit":
            assert not wave_hit.any() and not ev["prox"].any()
        else:
            assert wave_hit.any() and not wave_hit.all(), (case, p2, wave_hit.sum())
        if case == "one_hit":
            for t, a in ((0, 5), (1, 37), (2, 66), (TICKS - 1, 20)):
                w = slice(a // WAVE * WAVE, min(a // WAVE * WAVE + WAVE, N))
                assert ev["hit"][t, a] and ev["hit"][t, w].sum() == 1, (t, a)
        elif case == "mixed":
            assert ev["hit"][1, 0:32:4].all() and ev["hit"][1, :32].sum() == 8
        elif case == "vital0":
            assert outs[0]["terminated"][9] and not ev["hit"][0, :9].any() and not ev["hit"][0, 10:32].any()
        elif case == "proximity":
            assert ev["prox"].any() and any((s["f"]["action_id"] == GUARD_PROXIMITY).any() for s in states)
        elif case == "ko":
            assert ev["ko"].any()
        elif case != "no_hit":
            assert ev[{"multi_hit": "after_hit"}.get(case, case)].any(), case
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


def launch_vs_oracle(ref, p2, ticks, packed):
    """One fused launch of `ticks` ticks from the loaded states: every row and the final state."""
    import torch
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim, unpack_trajectory
    st, h1, h2, outs, states = ref
    sim = FootsiesSim(len(st), p2_mode=p2, seed=3)
    sim.set_state(st)
    if packed or ticks > 1:  # (a per-field launch of one tick is k_step)
        name = "k_step_n_packed" if packed else "k_step_n"
        if ticks > 1 and not os.environ.get(CHILD):  # one wave per SIMD: the request-prefetch kernels, kLmFast
            name += "_pf"
        want = "fsk::%s<0, %d>" % (name, P2[p2])
        assert lib().fs_step_kernel(sim.handle, ticks, _abi.FS_KERNEL_PACKED if packed else 0).decode() == want
    p1 = torch.from_numpy(h1[:ticks].copy()).to(sim.device)
    p2a = torch.from_numpy(h2[:ticks].copy()).to(sim.device) if p2 == "external" else None
    if packed:
        traj = sim.alloc_packed_trajectory(ticks)
        sim.step_n_packed(ticks, p1, p2a, trajectory=traj)
        torch.cuda.synchronize()
        got = unpack_trajectory({k: (None if v is None else v.cpu().numpy()) for k, v in traj.items()})
    else:
        traj = sim.alloc_trajectory(ticks)
        sim.step_n(ticks, p1, p2a, trajectory=traj)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in traj.items()}
    for t in range(ticks):
        compare_outputs(outs[t], {k: np.ascontiguousarray(v[t]) for k, v in got.items()}, step=t)
    compare_states(states[ticks - 1], sim.get_state(), step=ticks)
    sim.close()


def case_params():
    return [(c, p2) for p2 in ("external", "noop") for c in CASES if p2 == "external" or c not in NEEDS_P2]


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("case,p2", case_params())
def test_hit_gate(oracle_lib, case, p2, packed):
    ref = reference(oracle_lib, case, p2)  # (asserts the condition on the oracle's trace first)
    for ticks in LAUNCHES:
        launch_vs_oracle(ref, p2, ticks, packed)


def test_every_case_with_priority_slices_forced_on():
    """The cases above in a child process with FOOTSIES_PRIO=1 (and the two-lane kernel forced):
    k_step_n and k_step_n_packed, not the _pf kernels, run every launch (launch_vs_oracle asserts
    the name), their specialised waves in kLmFastPrio."""
    path = os.path.join(ROOT, "tests", "test_gpu_hit_gate.py")
    env = dict(os.environ, FOOTSIES_PRIO="1", FOOTSIES_FUSED_LANES="2", **{CHILD: "1"})
    env.pop("FOOTSIES_PREFETCH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        path + "::test_hit_gate"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % (2 * len(case_params())) in r.stdout, r.stdout[-2000:]
