"""The league's host side without a GPU: the two calls and their fs_step_kernel flags in the C-ABI (gcc on the
header against the ctypes mirror, the exported symbols), rollout.bot_groups -- a pure function of (seed, global
group index) -- and the argument checks of FusedSelfPlayRollout(bots=...) and PPOTrainer(opponent_bot=...), which
raise before any device call.  The kernels are checked in test_gpu_league.py."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest

from footsies_gym_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "footsies.h")
CTYPE = {"fs_handle": C.c_void_p, "int": C.c_int, "const fs_policy*": C.POINTER(_abi.fs_policy),
         "const fs_policy_pool*": C.POINTER(_abi.fs_policy_pool), "const fs_outputs*": C.POINTER(_abi.fs_outputs),
         "const fs_skip_traj*": C.POINTER(_abi.fs_skip_traj)}


def test_header_compiles_as_c99_with_the_new_declarations(tmp_path):
    lines = ['#include <stdio.h>', '#include "footsies.h"',
             "typedef int (*league_n_fn)(fs_handle, int, const fs_policy*, const fs_policy_pool*, int, const fs_outputs*);",
             "typedef int (*league_skip_fn)(fs_handle, int, const fs_policy*, const fs_policy_pool*, int, int,",
             "                              const fs_outputs*, const fs_skip_traj*);",
             "int main(void){",
             "league_n_fn f = 0; league_skip_fn g = 0;",
             "if (0) { f = fs_step_n_league; g = fs_step_skip_league; } (void)f; (void)g;",
             'printf("kernel_n %d\\n", FS_KERNEL_LEAGUE); printf("kernel_skip %d\\n", FS_KERNEL_SKIP_LEAGUE);',
             'printf("group %d\\n", FS_SELFPLAY_GROUP); printf("abi %d\\n", FS_ABI_VERSION);',
             "return 0;}"]
    src = tmp_path / "league.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "league"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["kernel_n"] == _abi.FS_KERNEL_LEAGUE == 512 and c["kernel_skip"] == _abi.FS_KERNEL_SKIP_LEAGUE == 1024
    older = (_abi.FS_KERNEL_HASHED | _abi.FS_KERNEL_POLICY | _abi.FS_KERNEL_PACKED | _abi.FS_KERNEL_SKIP_POLICY |
             _abi.FS_KERNEL_SELFPLAY | _abi.FS_KERNEL_SKIP_SELFPLAY | _abi.FS_KERNEL_SELFPLAY_POOL |
             _abi.FS_KERNEL_SKIP_SELFPLAY_POOL | 8)
    assert c["kernel_n"] & older == 0 and c["kernel_skip"] & older == 0 and c["kernel_n"] & c["kernel_skip"] == 0
    assert c["group"] == _abi.FS_SELFPLAY_GROUP == 128
    assert c["abi"] == _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed


@pytest.mark.parametrize("name,n_args", [("fs_step_n_league", 6), ("fs_step_skip_league", 8)])
def test_the_calls_are_exported_with_the_declared_arguments(name, n_args):
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert hasattr(lib, name)
    m = re.search(r"^int %s\(([^;]*)\);" % name, open(HEADER).read(), re.M | re.S)
    assert m, "include/footsies.h does not declare %s" % name
    declared = [CTYPE[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS[name]
    assert restype is C.c_int and argtypes == declared and len(declared) == n_args
    # the pool call it extends has the same list
    twin = name.replace("league", "selfplay_pool")
    assert _abi.LIB_FUNCTIONS[twin] == (restype, argtypes)
    # without a handle the call is refused before anything else is looked at
    f = getattr(lib, name)
    f.restype, f.argtypes = restype, argtypes
    pol, pool = _abi.fs_policy(), _abi.fs_policy_pool()
    tail = (None,) if n_args == 6 else (8, None, None)
    assert f(None, 4, C.byref(pol), C.byref(pool), _abi.FS_SELFPLAY_MIRROR, *tail) == _abi.FS_E_INVALID
    k = lib.fs_step_kernel
    k.restype, k.argtypes = _abi.LIB_FUNCTIONS["fs_step_kernel"]
    assert k(None, 8, _abi.FS_KERNEL_LEAGUE) is None and k(None, 8, _abi.FS_KERNEL_SKIP_LEAGUE) is None
    assert lib.fs_abi_version() == 8


def test_bot_groups_is_a_pure_counter_based_function():
    from footsies_gym_amd.rollout import bot_groups
    a = bot_groups(9, 0, 4096, 0.25)
    assert a.dtype == np.bool_ and a.shape == (4096,)
    assert np.array_equal(a, bot_groups(9, 0, 4096, 0.25))          # deterministic: fixed for a run
    assert not np.array_equal(a, bot_groups(10, 0, 4096, 0.25))     # keyed by the seed
    # the share within four binomial standard deviations of the fraction
    for frac in (0.25, 0.5, 0.9):
        share = int(bot_groups(9, 0, 4096, frac).sum())
        assert abs(share - 4096 * frac) < 4 * np.sqrt(4096 * frac * (1 - frac)), (frac, share)
    assert not bot_groups(9, 0, 4096, 0.0).any() and bot_groups(9, 0, 4096, 1.0).all()
    # a larger fraction only adds groups (one draw per group, compared with the fraction)
    assert (bot_groups(9, 0, 4096, 0.5) >= a).all()
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="fraction"):
            bot_groups(9, 0, 8, bad)


def test_shards_draw_what_the_unsharded_run_draws():
    from footsies_gym_amd.rollout import bot_groups
    whole = bot_groups(1, 0, 512, 0.5)
    parts = [bot_groups(1, first, 256, 0.5) for first in (0, 256)]
    assert np.array_equal(np.concatenate(parts), whole) and not np.array_equal(parts[0], parts[1])
    assert np.array_equal(bot_groups(1, 100, 7, 0.5), whole[100:107])


def test_the_rollout_checks_bots_before_the_device():
    from footsies_gym_amd.rollout import FusedSelfPlayRollout
    # (no device, no handle, no actor: a check that got past would fail on them)
    sim = types.SimpleNamespace(num_envs=289, p2_mode="external")
    pool = types.SimpleNamespace(sim=sim)
    for bad in ([True, False], [True] * 4, []):
        with pytest.raises(ValueError, match="one bool per group: 3 groups"):
            FusedSelfPlayRollout(sim, None, pool=pool, bots=bad)
    with pytest.raises(ValueError, match="pool="):
        FusedSelfPlayRollout(sim, None, bots=[True, False, True])


def test_ppo_trainer_checks_opponent_bot_before_the_device():
    from footsies_gym_amd.ppo import PPOTrainer
    ext = types.SimpleNamespace(p2_mode="external")
    for mode in (True, "decisions"):
        for f in (0, 0.0, 1, 1.0, -0.2, 1.5, float("nan")):
            with pytest.raises(ValueError, match="opponent_bot"):
                PPOTrainer(ext, self_play=mode, opponent_bot=f)
            with pytest.raises(ValueError, match="opponent_bot"):
                PPOTrainer(ext, self_play=mode, opponent_pool=3, opponent_bot=f)
    with pytest.raises(ValueError, match="self_play"):
        PPOTrainer(ext, opponent_bot=0.5)
    with pytest.raises(ValueError, match="self_play"):
        PPOTrainer(types.SimpleNamespace(p2_mode="bot"), opponent_bot=0.5)
    with pytest.raises(ValueError, match="arena_base"):
        PPOTrainer(types.SimpleNamespace(p2_mode="external", arena_base=64), self_play=True, opponent_bot=0.5)
