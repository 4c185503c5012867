"""The fast row loops' per-wave choice on the invariant set I (fs_kernels.hip kLmFast, in_fast_set:
hasWon clear, no DEAD / WIN as action, buffer or reserve, action frame below kTickFrames, vital at
most 1) against the CPU oracle, bit for bit over every output and the canonical state.

96 arenas are three waves of the two-lane kernel.  Wave 0 holds reset states only and takes the
fast loop.  Wave 1 holds states inside I and exactly one poisoned arena (the parameter), which
sends the whole wave to the generic loop: the clean lanes beside it must match as well.  Wave 2
holds states on the edge of I, which takes the fast loop: frame 63 of every action, and fighters
on their last vital that a special kills on a launch's first tick and on its last (the record of
that tick follows the same-step burst; the final_* record shows DEAD remapped to STAND).

300 ticks in launches of 1, 2, 3, 5 and 50 ticks, both trajectory layouts, both float models.  At
this size the multi-tick launches run the request-prefetch kernels (kLmFast); child processes
repeat everything with FOOTSIES_PRIO=1 FOOTSIES_FUSED_LANES=2 (k_step_n / k_step_n_packed in
kLmFastPrio, the loop of the benchmark's launch) and with FOOTSIES_PREFETCH=1."""
import os
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import ACTION_FRAMES, compare_outputs, compare_states, random_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "FOOTSIES_FAST_LOOP_CHILD"  # "prio" / "pf" in the child processes
N, TICKS = 96, 300
LAUNCHES = (1, 2, 3, 5, 50)
FM = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
DEAD, WIN, N_SPECIAL = 500, 510, 110
POISON_ARENA = 40
POISONS = ["has_won", "dead_f0", "dead_f63", "dead_f64", "dead_f499", "win_f32", "attack_f70", "vital3_special"]
# the launches of one pass over LAUNCHES: first ticks 0, 1, 3, 6, 11 and last ticks 0, 2, 5, 10, 60
KO_FIRST, KO_LAST = (3, 6, 11), (2, 5, 10)

_CACHE = {}


def schedule():
    """(first tick, tick count) of every launch: LAUNCHES in turn until TICKS are stepped."""
    out, t, i = [], 0, 0
    while t < TICKS:
        n = min(LAUNCHES[i % len(LAUNCHES)], TICKS - t)
        out.append((t, n))
        t += n
        i += 1
    return out


def inside_states(n, seed):
    """Arbitrary loadable states inside I."""
    st = random_states(n, np.random.default_rng(seed))
    st["reset_pending"] = 0
    f = st["f"]
    f["has_won"] = 0
    f["vital"] = 1
    out = (f["action_id"] == DEAD) | (f["action_id"] == WIN)
    f["action_id"][out] = 0
    f["action_frame"][out] = 0
    for field in ("buffer_action_id", "reserve_action_id"):
        f[field][(f[field] == DEAD) | (f[field] == WIN)] = -1
    assert (f["action_frame"] < 64).all()
    return st


def rows(n, ticks, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 8, (ticks, n)).astype(np.uint8), rng.integers(0, 8, (ticks, n)).astype(np.uint8)


def searched(oracle_lib):
    """From 16 384 arenas inside I on random rows (strict model): arenas whose round a special ends
    at each tick of KO_FIRST / KO_LAST, and -- with P1 loaded at vital 3 -- one in which P1 takes a
    special's hit within the first ticks and lies DEAD with no KO."""
    if "searched" not in _CACHE:
        m, ticks = 16384, max(KO_FIRST + KO_LAST) + 1
        h1, h2 = rows(m, ticks, 0xB1)
        st = inside_states(m, 21)
        ora = oracle_lib.Oracle(m, base_seed=3)
        assert ora.set_state(st) == 0
        term = np.stack([np.asarray(ora.step(h1[t], h2[t])["terminated"]).astype(bool) for t in range(ticks)])
        ora.close()
        first = term.argmax(0)  # the first KO of each arena (0 where none: term[0] tells)
        picks = []
        for t in KO_FIRST + KO_LAST:
            hit = np.flatnonzero(term[t] & (first == t))[:2]
            assert len(hit) == 2, ("no arena with its first KO at tick", t)
            picks += list(hit)
        st3 = st.copy()
        st3["f"]["vital"][:, 0] = 3
        ora = oracle_lib.Oracle(m, base_seed=3)
        assert ora.set_state(st3) == 0
        found, over = None, np.zeros(m, bool)
        for t in range(8):
            over |= np.asarray(ora.step(h1[t], h2[t])["terminated"]).astype(bool)
            s = ora.state()
            down = (s["f"]["action_id"][:, 0] == DEAD) & (s["f"]["vital"][:, 0] == 2) & ~over
            if down.any():
                found = int(np.flatnonzero(down)[0])
                break
        ora.close()
        assert found is not None
        _CACHE["searched"] = (st[picks].copy(), h1[:, picks].copy(), h2[:, picks].copy(),
                              st3[found].copy(), h1[:, found].copy(), h2[:, found].copy())
    return _CACHE["searched"]


def build_case(oracle_lib, poison):
    """The 96 loaded states and 300 action rows of one poisoning."""
    ko_st, ko_h1, ko_h2, v3_st, v3_h1, v3_h2 = searched(oracle_lib)
    st = inside_states(N, 22)
    h1, h2 = rows(N, TICKS, 0xB2)
    # wave 0: reset states
    ora = oracle_lib.Oracle(N, base_seed=3)
    ora.reset()
    st[:32] = ora.state()[:32]
    ora.close()
    # wave 2: frame 63 of every action inside I (P1 and P2 in turn), then the lethal hits
    ids = [a for a in sorted(ACTION_FRAMES) if a not in (DEAD, WIN)]
    for j, a in enumerate(ids):
        st["f"]["action_id"][64 + j, j & 1] = a
        st["f"]["action_frame"][64 + j, j & 1] = 63
    k = len(ko_st)
    lo = 64 + len(ids)
    assert lo + k <= N
    st[lo:lo + k] = ko_st
    h1[: len(ko_h1), lo:lo + k] = ko_h1
    h2[: len(ko_h2), lo:lo + k] = ko_h2
    # wave 1: one poisoned arena
    f = st["f"][POISON_ARENA]
    if poison == "has_won":
        f["has_won"][0] = 1
    elif poison.startswith("dead_f"):
        f["action_id"][1], f["action_frame"][1] = DEAD, int(poison[6:])
    elif poison == "win_f32":
        f["action_id"][0], f["action_frame"][0] = WIN, 32
    elif poison == "attack_f70":
        f["action_id"][0], f["action_frame"][0] = N_SPECIAL, 70
    elif poison == "vital3_special":
        st[POISON_ARENA] = v3_st
        h1[: len(v3_h1), POISON_ARENA] = v3_h1
        h2[: len(v3_h2), POISON_ARENA] = v3_h2
    else:
        raise AssertionError(poison)
    f = st["f"]
    outside = ((f["has_won"] != 0) | (f["vital"] > 1) | (f["action_frame"] >= 64) |
               np.isin(f["action_id"], (DEAD, WIN)) | np.isin(f["buffer_action_id"], (DEAD, WIN)) |
               np.isin(f["reserve_action_id"], (DEAD, WIN))).any(1)
    assert list(np.flatnonzero(outside)) == [POISON_ARENA]
    return st, h1, h2


def reference(oracle_lib, poison, fm):
    """The oracle over the case: every tick's outputs, the state at every launch boundary."""
    key = (poison, fm)
    if key not in _CACHE:
        st, h1, h2 = build_case(oracle_lib, poison)
        ends = {t + n - 1 for t, n in schedule()}
        ora = oracle_lib.Oracle(N, float_mode=FM[fm], base_seed=3)
        assert ora.set_state(st) == 0
        outs, states = [], {}
        for t in range(TICKS):
            outs.append(ora.step(h1[t], h2[t]))
            if t in ends:
                states[t] = ora.state()
        ora.close()
        if fm == "strict":  # (the search ran in this model)
            lo = 64 + len(ACTION_FRAMES) - 2
            for j, t in enumerate(KO_FIRST + KO_LAST):
                for a in (lo + 2 * j, lo + 2 * j + 1):
                    assert outs[t]["terminated"][a], (t, a)
                    assert 0 in outs[t]["final_move"][a]  # (the fallen fighter: DEAD reported as STAND)
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


@pytest.mark.parametrize("fm", ["strict", "double"])
@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("poison", POISONS)
def test_waves_inside_and_outside_the_set(oracle_lib, poison, packed, fm):
    import torch
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim, unpack_trajectory
    st, h1, h2, outs, states = reference(oracle_lib, poison, fm)
    sim = FootsiesSim(N, p2_mode="external", float_mode=fm, seed=3)
    sim.set_state(st)
    p1, p2 = torch.from_numpy(h1).to(sim.device), torch.from_numpy(h2).to(sim.device)
    child = os.environ.get(CHILD)
    for t0, n in schedule():
        if child and (packed or n > 1):  # (a per-field launch of one tick is k_step)
            want = "fsk::%s%s<%d, 0>" % ("k_step_n_packed" if packed else "k_step_n",
                                         "_pf" if child == "pf" and n > 1 else "", FM[fm])
            assert lib().fs_step_kernel(sim.handle, n, _abi.FS_KERNEL_PACKED if packed else 0).decode() == want
        if packed:
            traj = sim.alloc_packed_trajectory(n)
            sim.step_n_packed(n, p1[t0:t0 + n], p2[t0:t0 + n], trajectory=traj)
            torch.cuda.synchronize()
            got = unpack_trajectory({k: (None if v is None else v.cpu().numpy()) for k, v in traj.items()})
        else:
            traj = sim.alloc_trajectory(n)
            sim.step_n(n, p1[t0:t0 + n], p2[t0:t0 + n], trajectory=traj)
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in traj.items()}
        for t in range(n):
            compare_outputs(outs[t0 + t], {k: np.ascontiguousarray(v[t]) for k, v in got.items()}, step=t0 + t)
        compare_states(states[t0 + n - 1], sim.get_state(), step=t0 + n)
    sim.close()


@pytest.mark.parametrize("mode,env", [("prio", {"FOOTSIES_PRIO": "1", "FOOTSIES_FUSED_LANES": "2"}),
                                      ("pf", {"FOOTSIES_PREFETCH": "1"})], ids=["prio_slices", "prefetch"])
def test_every_case_in_the_other_fast_loops(mode, env):
    """Every case above in a child process: with the priority slices forced on (k_step_n /
    k_step_n_packed, kLmFastPrio) and with the request prefetch forced on (the _pf kernels, kLmFast);
    the parent asserts nothing about the kernel, the children assert its name per launch."""
    if os.environ.get(CHILD):
        pytest.skip("already the child")
    path = os.path.join(ROOT, "tests", "test_gpu_fast_loop_invariants.py")
    e = dict(os.environ, **env, **{CHILD: mode})
    for k in ("FOOTSIES_PRIO", "FOOTSIES_FUSED_LANES", "FOOTSIES_PREFETCH"):
        if k not in env:
            e.pop(k, None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        path + "::test_waves_inside_and_outside_the_set"], cwd=ROOT, env=e, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "%d passed" % (4 * len(POISONS)) in r.stdout, r.stdout[-2000:]
