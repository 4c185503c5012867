"""The specialised row loops' table dash parser (fs_kernels.hip take_input, fs_tables.h ParserTable)
against the CPU oracle, bit for bit over every output and the canonical state, input history included.

The loops carry the parser's automaton state instead of parsing the history, and the history itself
in another form, so what can go wrong is the state at loop entry (derived from a loaded history), the
conversion back at loop exit, the state after a KO's ClearInput and reset burst, and any table entry.
Scripted rows, per arena and player: a direction held for 1, 2, 7, 8 or 9 frames, 0 .. 9 neutral
frames, then the same direction (a double tap with its first direction at each of input[1..8], and
past the window), the opposite one or both together, then 0 .. 9 neutral frames before the pattern
repeats; a third of the arenas press attack now and then, so rounds end in the middle of a tap
sequence (ClearInput, the burst's stale input).  States are loaded with random 32-bit histories and
attack holds 0 .. 63.  33 arenas are a full wave and a wave of one arena; 96 put a wave outside the
invariant set (the generic loop, which keeps update_input) beside two ring waves.  Launches of
1 .. 2 D + 1 ticks, one of 300, two chained; both layouts, both float models, P2 remote and idle.
In this process the launches take the library's own choice (the request-prefetch kernels at these
sizes); child processes repeat everything with FOOTSIES_PREFETCH=1 (the _pf kernels, forced) and with
FOOTSIES_PRIO=1 FOOTSIES_FUSED_LANES=2 (k_step_n / k_step_n_packed in kLmFastPrio, the benchmark's loop:
the switches are read once per process)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import compare_outputs, compare_states, fused_kernel, random_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "FOOTSIES_INPUT_PARSER_CHILD"  # set in the child processes
LONG, CHAIN = 300, (7, 5)
FM = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
P2 = {"external": _abi.FS_P2_EXTERNAL, "noop": _abi.FS_P2_NOOP}
P2_KERNEL = {"external": 0, "noop": 2}  # the kernels' second template argument
DEAD, WIN = 500, 510
DASH_MOVES = (_abi.MOVE_ID_TO_INDEX[10], _abi.MOVE_ID_TO_INDEX[11])
OUTSIDE_ARENA = 70  # (of 96: in the third wave)
LEFT, RIGHT, ATTACK = 1, 2, 4

_CACHE = {}


def ring_depth():
    src = open(os.path.join(ROOT, "footsies_gym_amd", "csrc", "fs_kernels.hip")).read()
    d = int(re.search(r"^#define FS_ROW_DEPTH2 (\d+)", src, re.M).group(1))
    assert 2 <= d <= 4
    return d


def loaded_states(n, p2):
    """Loadable states inside the fast loops' invariant set, with random 32-bit input histories and
    attack holds 0 .. 63 (random_states); of 96, one arena outside the set (vital 2)."""
    st = random_states(n, np.random.default_rng(47), p2=p2)
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
    assert len(set(f["attack_hold"].ravel().tolist())) > 30 and (f["input_dir_history"] > 0xFFFF).any()
    if n > OUTSIDE_ARENA:
        f["vital"][OUTSIDE_ARENA, 0] = 2
    return st


def scripted_rows(n, player):
    """[LONG, n] inputs: the tap patterns of the module docstring, one parameter set per arena."""
    rng = np.random.default_rng(0x7A9 + player)
    rows = np.zeros((LONG, n), np.uint8)
    for a in range(n):
        i = a + 7 * player
        d = (LEFT, RIGHT)[i % 2]
        hold = (1, 2, 7, 8, 9)[(i // 2) % 5]
        gap = (i // 10) % 10
        second = (d, d ^ 3, 3)[(i // 3) % 3] if a % 4 else d  # (every fourth arena: plain double taps)
        tail = (i // 5) % 10
        pattern = [d] * hold + [0] * gap + [second] * (1 + i % 2) + [0] * tail
        lead = i % 11  # (offsets the pattern against the launch boundaries)
        stream = ([0] * lead + pattern * (LONG // len(pattern) + 1))[:LONG]
        col = np.array(stream, np.uint8)
        if a % 3 == 0:  # attack presses and holds on top: hits, guard breaks, KOs inside the sequences
            col |= (ATTACK * (rng.random(LONG) < 0.2)).astype(np.uint8)
        rows[:, a] = col
    return rows


def reference(oracle_lib, n, p2, fm):
    """The oracle over LONG ticks from the loaded state: every tick's outputs, the state after each of
    the ticks a launch below ends on."""
    key = (n, p2, fm)
    if key not in _CACHE:
        st = loaded_states(n, p2)
        h1, h2 = scripted_rows(n, 0), scripted_rows(n, 1)
        ends = set(range(2 * ring_depth() + 1)) | {CHAIN[0] - 1, sum(CHAIN) - 1, LONG - 1}
        ora = oracle_lib.Oracle(n, p2_mode=P2[p2], float_mode=FM[fm], base_seed=3)
        assert ora.set_state(st) == 0
        outs, states = [], {}
        for t in range(LONG):
            outs.append(ora.step(h1[t], h2[t] if p2 == "external" else None))
            if t in ends:
                states[t] = ora.state()
        ora.close()
        # the scripts do what they are for: dashes of both kinds by both players, and rounds that end
        moves = np.stack([np.asarray(o["move"]) for o in outs])  # [LONG, n, 2]
        for k in range(2 if p2 == "external" else 1):
            for m in DASH_MOVES:
                assert (moves[:, :, k] == m).any(), ("no dash", k, m)
        assert sum(int(np.asarray(o["terminated"]).sum()) for o in outs) >= 3
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


@pytest.mark.parametrize("fm", ["strict", "double"])
@pytest.mark.parametrize("p2", ["external", "noop"])
@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("n", [33, 96])
def test_scripted_taps_match_the_oracle(oracle_lib, n, packed, p2, fm):
    import torch
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim, unpack_trajectory
    st, h1, h2, outs, states = reference(oracle_lib, n, p2, fm)
    sim = FootsiesSim(n, p2_mode=p2, float_mode=fm, seed=3)
    p1 = torch.from_numpy(h1).to(sim.device)
    q2 = torch.from_numpy(h2).to(sim.device) if p2 == "external" else None
    child = os.environ.get(CHILD)

    def launch(t0, ticks):
        if packed or ticks > 1:  # (a per-field launch of one tick is k_step)
            want = "fsk::%s<%d, %d>" % ("k_step_n_packed" if packed else "k_step_n", FM[fm], P2_KERNEL[p2])
            if child == "pf":
                assert os.environ.get("FOOTSIES_PREFETCH") == "1"
            if child != "prio" and ticks > 1:
                want = fused_kernel(want, n)
            assert lib().fs_step_kernel(sim.handle, ticks, _abi.FS_KERNEL_PACKED if packed else 0).decode() == want
        rows2 = None if q2 is None else q2[t0:t0 + ticks]
        if packed:
            traj = sim.alloc_packed_trajectory(ticks)
            sim.step_n_packed(ticks, p1[t0:t0 + ticks], rows2, trajectory=traj)
            torch.cuda.synchronize()
            got = unpack_trajectory({k: (None if v is None else v.cpu().numpy()) for k, v in traj.items()})
        else:
            traj = sim.alloc_trajectory(ticks)
            sim.step_n(ticks, p1[t0:t0 + ticks], rows2, trajectory=traj)
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in traj.items()}
        for t in range(ticks):
            compare_outputs(outs[t0 + t], {k: np.ascontiguousarray(v[t]) for k, v in got.items()}, step=t0 + t)
        compare_states(states[t0 + ticks - 1], sim.get_state(), step=t0 + ticks)  # (input_dir_history among the fields)

    for ticks in list(range(1, 2 * ring_depth() + 2)) + [LONG]:
        sim.set_state(st)
        launch(0, ticks)
    sim.set_state(st)
    launch(0, CHAIN[0])
    launch(CHAIN[0], CHAIN[1])
    sim.close()


@pytest.mark.parametrize("mode", ["pf", "prio"])
def test_every_case_in_a_process_of_its_own(mode):
    """Every case above in a child process with the kernel choice forced (the switches are read once
    per process): `pf` the request-prefetch kernels, `prio` k_step_n / k_step_n_packed with the
    priority slices (kLmFastPrio).  The child asserts the kernel per launch."""
    if os.environ.get(CHILD):
        pytest.skip("already the child")
    e = dict(os.environ, **{CHILD: mode})
    for v in ("FOOTSIES_PREFETCH", "FOOTSIES_PRIO", "FOOTSIES_FUSED_LANES"):
        e.pop(v, None)
    e.update({"FOOTSIES_PREFETCH": "1"} if mode == "pf" else {"FOOTSIES_PRIO": "1", "FOOTSIES_FUSED_LANES": "2"})
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_input_parser.py") + "::test_scripted_taps_match_the_oracle"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "16 passed" in r.stdout, r.stdout[-2000:]
