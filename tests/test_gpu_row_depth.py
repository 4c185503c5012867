"""The specialised row loops' D-slot row ring (fs_kernels.hip row_ring, FS_ROW_DEPTH2) against the
CPU oracle, bit for bit over every output and the canonical state.

33 arenas are a full wave and a wave of one arena (its idle lanes hold slots too); 96 are three
waves, the third with one arena loaded at vital 2: outside the fast loops' invariant set, so that
wave runs the generic two-slot loop beside two ring waves of one block.  From one loaded state:
launches of 1 .. 2 D + 1 ticks (every remainder of the unrolled loop, launches shorter than the
ring, re-reads clamped to the last row), one launch of 300 ticks (hits, KOs and same-step bursts
with rows in flight), and two chained launches of 7 and 5 ticks from row offsets inside one table.
Both trajectory layouts, both float models, P2 remote and idle.  At these sizes a multi-tick launch
runs the request-prefetch kernels (kLmFast); a child process repeats everything with FOOTSIES_PRIO=1
FOOTSIES_FUSED_LANES=2 (k_step_n / k_step_n_packed in kLmFastPrio, the benchmark's loop)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import compare_outputs, compare_states, random_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "FOOTSIES_ROW_DEPTH_CHILD"  # set in the child process
LONG, CHAIN = 300, (7, 5)
FM = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
P2 = {"external": _abi.FS_P2_EXTERNAL, "noop": _abi.FS_P2_NOOP}
P2_KERNEL = {"external": 0, "noop": 2}  # the kernels' second template argument
DEAD, WIN = 500, 510
OUTSIDE_ARENA = 70  # (of 96: in the third wave)

_CACHE = {}


def ring_depth():
    src = open(os.path.join(ROOT, "footsies_gym_amd", "csrc", "fs_kernels.hip")).read()
    d = int(re.search(r"^#define FS_ROW_DEPTH2 (\d+)", src, re.M).group(1))
    assert 2 <= d <= 4
    return d


def loaded_states(n, p2):
    """Arbitrary loadable states inside the invariant set; of 96, one arena outside it (vital 2)."""
    st = random_states(n, np.random.default_rng(31), p2=p2)
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
    if n > OUTSIDE_ARENA:
        f["vital"][OUTSIDE_ARENA, 0] = 2
    return st


def reference(oracle_lib, n, p2, fm):
    """The oracle over LONG ticks from the loaded state: every tick's outputs, the state after each of
    the ticks a launch below ends on."""
    key = (n, p2, fm)
    if key not in _CACHE:
        st = loaded_states(n, p2)
        rng = np.random.default_rng(0xD4)
        h1, h2 = (rng.integers(0, 8, (LONG, n)).astype(np.uint8) for _ in range(2))
        ends = set(range(2 * ring_depth() + 1)) | {CHAIN[0] - 1, sum(CHAIN) - 1, LONG - 1}
        ora = oracle_lib.Oracle(n, p2_mode=P2[p2], float_mode=FM[fm], base_seed=3)
        assert ora.set_state(st) == 0
        outs, states = [], {}
        for t in range(LONG):
            outs.append(ora.step(h1[t], h2[t] if p2 == "external" else None))
            if t in ends:
                states[t] = ora.state()
        ora.close()
        # the long launch meets what the ring must survive: rounds that end (the same-step burst)
        assert sum(int(np.asarray(o["terminated"]).sum()) for o in outs) >= 3
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


@pytest.mark.parametrize("fm", ["strict", "double"])
@pytest.mark.parametrize("p2", ["external", "noop"])
@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("n", [33, 96])
def test_every_launch_length_matches_the_oracle(oracle_lib, n, packed, p2, fm):
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
            want = "fsk::%s%s<%d, %d>" % ("k_step_n_packed" if packed else "k_step_n",
                                          "" if child or ticks == 1 else "_pf", FM[fm], P2_KERNEL[p2])
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
        compare_states(states[t0 + ticks - 1], sim.get_state(), step=t0 + ticks)

    for ticks in list(range(1, 2 * ring_depth() + 2)) + [LONG]:
        sim.set_state(st)
        launch(0, ticks)
    sim.set_state(st)
    launch(0, CHAIN[0])
    launch(CHAIN[0], CHAIN[1])
    sim.close()


def test_every_case_with_the_priority_slices():
    """Every case above in a child process with the slices forced on: k_step_n / k_step_n_packed in
    kLmFastPrio (the switches are read once per process); the child asserts the kernel per launch."""
    if os.environ.get(CHILD):
        pytest.skip("already the child")
    e = dict(os.environ, FOOTSIES_PRIO="1", FOOTSIES_FUSED_LANES="2", **{CHILD: "prio"})
    e.pop("FOOTSIES_PREFETCH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_row_depth.py") + "::test_every_launch_length_matches_the_oracle"],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "16 passed" in r.stdout, r.stdout[-2000:]
