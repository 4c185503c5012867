"""The fused row loops' launch modes (fs_kernels.hip kLmFast / kLmFastPrio, step_body's per-wave
choice) against the CPU oracle, bit for bit over every output and the canonical state.

A wave of a standard fused row launch (remote or idle P2) runs a loop compiled for same-step
auto-reset, dense reward and no lane with a reset pending; every other wave runs the generic loop.
96 arenas are three two-lane waves, the last half full.  Launches of 1, 2, 3, 4, 5 and 37 ticks
(odd and even tails) run from loaded states: same-step with the dense and the sparse reward,
next-step mode (generic loop), a same-step handle whose middle wave alone holds pending arenas
exported from a next-step handle (a generic wave between two specialised ones), KOs with their
same-step reset in the last and the last but one tick of a launch.  At 96 arenas the multi-tick
launches run the request-prefetch kernels (kLmFast); a child process repeats all of these cases
with FOOTSIES_PRIO=1, which turns the prefetch off and the priority slices on, so the same launches
run k_step_n / k_step_n_packed in kLmFastPrio, the loop of the benchmark's launch.  One case runs
that loop unforced, at the smallest grid that has two waves per SIMD."""
import os
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import compare_outputs, compare_states, fused_kernel, random_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "FOOTSIES_LAUNCH_MODES_CHILD"  # set in the child process that forces the priority slices on

P2 = {"external": _abi.FS_P2_EXTERNAL, "bot": _abi.FS_P2_BOT}
AR = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}
N = 96
LAUNCHES = (1, 2, 3, 4, 5, 37)

_CACHE = {}


def rows_for(n, ticks, seed, p2):
    rng = np.random.default_rng(seed)
    h1 = rng.integers(0, 8, (ticks, n)).astype(np.uint8)
    h2 = rng.integers(0, 8, (ticks, n)).astype(np.uint8) if p2 == "external" else None
    return h1, h2


def oracle_run(oracle_lib, key, st, h1, h2, p2, ar, dense=True):
    """The oracle stepped over the rows h1 / h2 from the loaded states: each tick's outputs and the
    state after it, computed once per key."""
    if key not in _CACHE:
        ora = oracle_lib.Oracle(len(st), p2_mode=P2[p2], autoreset_mode=AR[ar], dense_reward=dense, base_seed=3)
        assert ora.set_state(st) == 0
        outs, states = [], []
        for t in range(len(h1)):
            outs.append(ora.step(h1[t], None if h2 is None else h2[t]))
            states.append(ora.state())
        ora.close()
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


def launch_vs_oracle(ref, p2, ar, ticks, packed, dense=True, kernel=None):
    """One fused launch of `ticks` ticks from the loaded states: every row and the final state."""
    import torch
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim, unpack_trajectory
    st, h1, h2, outs, states = ref
    sim = FootsiesSim(len(st), p2_mode=p2, autoreset_mode=ar, dense_reward=dense, seed=3)
    sim.set_state(st)
    if os.environ.get(CHILD) and (packed or ticks > 1):  # (a per-field launch of one tick is k_step)
        # slices forced on: no request prefetch, so the two-lane kernels themselves
        kernel = "fsk::%s<0, %d>" % ("k_step_n_packed" if packed else "k_step_n", P2[p2])
    if kernel is not None:
        assert lib().fs_step_kernel(sim.handle, ticks, _abi.FS_KERNEL_PACKED if packed else 0).decode() == kernel
    p1 = torch.from_numpy(h1[:ticks].copy()).to(sim.device)
    p2a = None if h2 is None else torch.from_numpy(h2[:ticks].copy()).to(sim.device)
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
        compare_outputs(outs[t], {k: np.ascontiguousarray(v[t]) for k, v in got.items()}, step=t,
                        same_step=ar == "same_step")
    compare_states(states[ticks - 1], sim.get_state(), step=ticks)
    sim.close()


def loaded_states(p2):
    st = random_states(N, np.random.default_rng(11), p2=p2)
    st["reset_pending"] = 0
    return st


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("p2", ["external", "bot"])
@pytest.mark.parametrize("ar,dense", [("same_step", True), ("same_step", False), ("next_step", True)],
                         ids=["same_step_dense", "same_step_sparse", "next_step"])
def test_launch_modes(oracle_lib, ar, dense, p2, packed):
    """The specialised loop (same-step, dense), and the generic one for the sparse reward and for
    next-step mode, whose KO arenas (random_states loads some fighters dead) then run the pending
    path."""
    h1, h2 = rows_for(N, max(LAUNCHES), 0xA1, p2)
    ref = oracle_run(oracle_lib, ("modes", p2, ar, dense), loaded_states(p2), h1, h2, p2, ar, dense)
    for ticks in LAUNCHES:
        launch_vs_oracle(ref, p2, ar, ticks, packed, dense)


def pending_states(oracle_lib, p2):
    """States exported from a next-step handle right after a KO in every arena of the middle wave
    (arenas 32..63), and nowhere else: a same-step handle that loads them runs that wave in the
    generic loop between two waves in the specialised one."""
    from footsies_gym_amd.simulator import FootsiesSim
    st = random_states(N, np.random.default_rng(12), p2=p2)
    st["reset_pending"] = 0
    st["f"]["vital"] = 1
    st["f"]["vital"][32:64, 0] = 0
    st["f"]["vital"][40:48, 1] = 0  # (and both at once)
    h1, h2 = rows_for(N, 1, 0xA2, p2)

    def after_one_tick():
        ora = oracle_lib.Oracle(N, p2_mode=P2[p2], autoreset_mode=AR["next_step"], base_seed=3)
        assert ora.set_state(st) == 0
        ora.step(h1[0], None if h2 is None else h2[0])
        s = ora.state()
        ora.close()
        return s
    # an arena of the other waves whose round a hit ends on that tick becomes a copy of one that plays on
    pend = after_one_tick()["reset_pending"].astype(bool)
    pend[32:64] = False
    keep = np.flatnonzero(~pend[:32])[0]
    st[pend] = st[keep]
    h1[0, pend] = h1[0, keep]
    if h2 is not None:
        h2[0, pend] = h2[0, keep]
    sim = FootsiesSim(N, p2_mode=p2, autoreset_mode="next_step", seed=3)
    sim.set_state(st)
    sim.step(h1[0], None if h2 is None else h2[0])
    out = sim.get_state()
    sim.close()
    compare_states(after_one_tick(), out)
    assert np.array_equal(np.flatnonzero(out["reset_pending"]), np.arange(32, 64))
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("p2", ["external", "bot"])
def test_same_step_handle_with_pending_lanes(oracle_lib, p2, packed):
    """The pending arenas run their reset burst on the first tick and play on from it, as the
    oracle does when it loads the same states under same-step auto-reset."""
    key = ("pending", p2)
    if key not in _CACHE:
        h1, h2 = rows_for(N, max(LAUNCHES), 0xA3, p2)
        oracle_run(oracle_lib, key, pending_states(oracle_lib, p2), h1, h2, p2, "same_step")
    ref = _CACHE[key]
    assert not ref[3][0]["terminated"][32:64].any() and ref[4][0]["reset_pending"].sum() == 0
    for ticks in LAUNCHES:
        launch_vs_oracle(ref, p2, "same_step", ticks, packed)


def ko_tick_states(oracle_lib):
    """96 arenas, all fighters alive, in which a round ends at tick 2, 3 or 4: drawn from 16 384
    random arenas the oracle plays for five ticks on random rows."""
    key = "ko_ticks"
    if key not in _CACHE:
        m, ticks = 16384, 5
        st = random_states(m, np.random.default_rng(13))
        st["reset_pending"] = 0
        st["f"]["vital"] = 1
        h1, h2 = rows_for(m, ticks, 0xA4, "external")
        ora = oracle_lib.Oracle(m, p2_mode=P2["external"], base_seed=3)
        assert ora.set_state(st) == 0
        term = np.stack([np.asarray(ora.step(h1[t], h2[t])["terminated"]).astype(bool) for t in range(ticks)])
        ora.close()
        pick = np.flatnonzero(term[2:].any(0))[:N]
        assert term[2, pick].any() and term[3, pick].any() and term[4, pick].any(), term[:, pick].sum(1)
        pick = np.concatenate([pick, np.setdiff1d(np.arange(m), pick)[: N - len(pick)]])
        _CACHE[key] = (st[pick].copy(), h1[:, pick].copy(), h2[:, pick].copy())
    return _CACHE[key]


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
def test_ko_in_the_last_ticks_of_a_launch(oracle_lib, packed):
    """KO and same-step reset in the last tick of a launch and in the last but one (launches of 3,
    4 and 5 ticks over arenas whose rounds end at ticks 2, 3 and 4)."""
    st, h1, h2 = ko_tick_states(oracle_lib)
    ref = oracle_run(oracle_lib, ("ko_run",), st, h1, h2, "external", "same_step")
    assert all(ref[3][t]["terminated"].any() for t in (2, 3, 4))
    for ticks in (3, 4, 5):
        launch_vs_oracle(ref, "external", "same_step", ticks, packed)


def test_every_case_with_priority_slices_forced_on():
    """The cases above in a child process with FOOTSIES_PRIO=1 (and the two-lane kernel forced):
    k_step_n and k_step_n_packed, not the _pf kernels, run every launch (launch_vs_oracle asserts
    the name), their specialised waves in kLmFastPrio."""
    if os.environ.get(CHILD):
        pytest.skip("already the child")
    path = os.path.join(ROOT, "tests", "test_gpu_launch_modes.py")
    tests = ["test_launch_modes", "test_same_step_handle_with_pending_lanes", "test_ko_in_the_last_ticks_of_a_launch"]
    env = dict(os.environ, FOOTSIES_PRIO="1", FOOTSIES_FUSED_LANES="2", **{CHILD: "1"})
    env.pop("FOOTSIES_PREFETCH", None)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] +
                       [path + "::" + t for t in tests], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "18 passed" in r.stdout, r.stdout[-2000:]


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
def test_priority_slices_on(oracle_lib, packed):
    """The specialised loop with priority slices: the smallest ragged grid with more waves than the
    device has SIMDs (two-lane kernel, no request prefetch), 4 ticks."""
    import torch
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 32 * simds + 33
    st = random_states(n, np.random.default_rng(14))
    st["reset_pending"] = 0
    h1, h2 = rows_for(n, 4, 0xA5, "external")
    ref = oracle_run(oracle_lib, ("prio", n), st, h1, h2, "external", "same_step")
    name = "fsk::k_step_n_packed<0, 0>" if packed else "fsk::k_step_n<0, 0>"
    launch_vs_oracle(ref, "external", "same_step", 4, packed, kernel=fused_kernel(name, n, mi355x_simds=simds))
