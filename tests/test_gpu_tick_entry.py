"""The fused kernels' tick entry (fs_tables.h Tables::tick, fs_kernels.hip tick_entry /
tick_entry_slow) against the CPU oracle, from loaded states no rollout reaches quickly.

The fused kernels take the next tick's frame, frame record and request class from one table
word per (action, hitstun > 0, frame), re-read after every collision and after every reset burst,
and from ActionInfo arithmetic for frames past the table.  Here every (action, frame, hitstun)
is loaded with fs_set_state and stepped in short launches through every fused row loop; a KO
with hitstun surviving the reset burst; and a part-filled wave."""
import os
import subprocess
import sys

import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.parity_utils import ACTION_FRAMES, compare_outputs, compare_states, random_states

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P2 = {"external": _abi.FS_P2_EXTERNAL, "bot": _abi.FS_P2_BOT}
AR = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}
DEAD, WIN = 500, 510
N_ENUM = 2048
LAUNCHES = (1, 2, 3, 5)  # the odd tail of the row loop; a _pf launch's first tick has no prepared request


def enumerated_states(p2):
    """2 048 arenas whose fighters cover every action x every frame 0..frameCount (DEAD 0..500, WIN
    to its last frame) x hitstun {0, 1, 2}; everything else (positions, buffer / reserve, hasWon,
    histories, bot queues) as random_states draws it.  The enumerated fighters are alive, so no
    arena ends before its fighters' entries are used; the arenas behind them stay random."""
    rng = np.random.default_rng(4242)
    st = random_states(N_ENUM, rng, p2=p2)
    combos = [(a, f, h) for a, fc in sorted(ACTION_FRAMES.items())
              for f in range(fc + (0 if a == WIN else 1)) for h in (0, 1, 2)]
    assert len(combos) <= 2 * N_ENUM
    order = rng.permutation(len(combos))
    for slot, c in enumerate(order):
        a, f, h = combos[c]
        fs = st["f"][slot >> 1, slot & 1]
        fs["action_id"], fs["action_frame"], fs["hitstun"], fs["vital"] = a, f, h, 1
    n_arenas = (len(combos) + 1) // 2
    st["f"]["vital"][:n_arenas] = 1
    got = {(int(a), int(f), int(h)) for a, f, h in zip(st["f"]["action_id"][:n_arenas].ravel(),
                                                       st["f"]["action_frame"][:n_arenas].ravel(),
                                                       st["f"]["hitstun"][:n_arenas].ravel())}
    assert got >= set(combos)
    fe = st["f"][:n_arenas]
    dead = fe["action_id"] == DEAD
    for fr in (61, 62, 63, 64, 498, 499, 500):  # the table's last frames and DEAD's end, alive
        assert (dead & (fe["action_frame"] == fr) & (fe["vital"] == 1)).any(), fr
    assert fe["has_won"].any() and (fe["buffer_action_id"] >= 0).any() and (fe["reserve_action_id"] >= 0).any()
    return st


_CACHE = {}


def oracle_run(oracle_lib, key, make_states, p2, ar, ticks, seed):
    """The oracle stepped `ticks` ticks from make_states() on the hashed rows of `seed`: the rows,
    each tick's outputs and the state after each tick, computed once per key."""
    if key not in _CACHE:
        from footsies_gym_amd.simulator import FootsiesSim
        st = make_states()
        n = len(st)
        sim = FootsiesSim(n, p2_mode=p2, seed=3)
        p1, p2a = sim.hash_actions(ticks, seed=seed, p2=p2 == "external")
        h1, h2 = p1.cpu().numpy(), (None if p2a is None else p2a.cpu().numpy())
        sim.close()
        ora = oracle_lib.Oracle(n, p2_mode=P2[p2], autoreset_mode=AR[ar], base_seed=3)
        assert ora.set_state(st) == 0
        outs, states = [], []
        for t in range(ticks):
            outs.append(ora.step(h1[t], None if h2 is None else h2[t]))
            states.append(ora.state())
        ora.close()
        _CACHE[key] = (st, h1, h2, outs, states)
    return _CACHE[key]


def launch_vs_oracle(ref, p2, ar, ticks, packed, seed):
    """One fused launch of `ticks` ticks from the loaded states: every row and the final state."""
    import torch
    from footsies_gym_amd.simulator import FootsiesSim, unpack_trajectory
    st, h1, h2, outs, states = ref
    sim = FootsiesSim(len(st), p2_mode=p2, autoreset_mode=ar, seed=3)
    sim.set_state(st)
    p1, p2a = sim.hash_actions(ticks, seed=seed, p2=p2 == "external")
    assert np.array_equal(p1.cpu().numpy(), h1[:ticks])
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


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("p2", ["external", "bot"])
def test_enumerated_states(oracle_lib, p2, packed):
    """Every action x frame x hitstun {0, 1, 2}, stepped in launches of 1, 2, 3 and 5 ticks."""
    ref = oracle_run(oracle_lib, ("enum", p2), lambda: enumerated_states(p2), p2, "same_step", max(LAUNCHES), 0xE1)
    for ticks in LAUNCHES:
        launch_vs_oracle(ref, p2, "same_step", ticks, packed, 0xE1)


@pytest.mark.parametrize("env", [{"FOOTSIES_PREFETCH": "1", "FOOTSIES_FUSED_LANES": "2"},
                                 {"FOOTSIES_PREFETCH": "0", "FOOTSIES_FUSED_LANES": "2"},
                                 {"FOOTSIES_FUSED_LANES": "1"}], ids=["prefetch", "no_prefetch", "one_lane"])
def test_enumerated_states_through_the_other_loops(env):
    """The same enumeration in child processes with the request-prefetch loop forced on, forced off
    (the loop of the launches with two or more waves per SIMD) and the one-lane kernel forced."""
    if os.environ.get("FOOTSIES_TICK_ENTRY_CHILD"):
        pytest.skip("already the child")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                        os.path.join(ROOT, "tests", "test_gpu_tick_entry.py") + "::test_enumerated_states"],
                       cwd=ROOT, env=dict(os.environ, FOOTSIES_TICK_ENTRY_CHILD="1", **env), capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, str(env) + r.stdout[-4000:] + r.stderr[-2000:]
    assert "4 passed" in r.stdout, r.stdout[-2000:]


def ko_states():
    """256 arenas in which one fighter is dead at the first KO test while both are in hitstun
    (0..6 left, so that it runs out before, during and after the reset burst)."""
    rng = np.random.default_rng(77)
    n = 256
    st = random_states(n, rng)
    st["f"]["hitstun"] = rng.integers(0, 7, (n, 2))
    st["f"]["hitstun"][: n // 2] = np.maximum(st["f"]["hitstun"][: n // 2], 1)
    st["f"]["vital"] = 1
    loser = rng.integers(0, 2, n)
    st["f"]["vital"][np.arange(n), loser] = 0
    st["f"]["vital"][::16] = 0  # both at once
    st["reset_pending"] = 0
    return st


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("ar", ["same_step", "next_step"])
def test_ko_with_surviving_hitstun(oracle_lib, ar, packed):
    """Both fighters in hitstun when one dies: the burst ends on STAND at frame 0 (stunned) or 1
    with the hitstun SetupBattleStart keeps, same-step and next-step auto-reset, then 30 ticks."""
    ref = oracle_run(oracle_lib, ("ko", ar), ko_states, "external", ar, 31, 0xE2)
    launch_vs_oracle(ref, "external", ar, 31, packed, 0xE2)


@pytest.mark.parametrize("packed", [False, True], ids=["per_field", "packed"])
@pytest.mark.parametrize("p2", ["external", "bot"])
def test_part_filled_wave(oracle_lib, p2, packed):
    """100 arenas (a part-filled wave: the wave-uniform test for frames past the table runs over
    the active lanes only), 64 ticks from random loaded states."""
    ref = oracle_run(oracle_lib, ("part", p2), lambda: random_states(100, np.random.default_rng(5), p2=p2), p2,
                     "same_step", 64, 0xE3)
    launch_vs_oracle(ref, p2, "same_step", 64, packed, 0xE3)
