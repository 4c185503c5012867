"""fs_step_skip_selfplay's host side without a GPU: the constant and the call in the C-ABI (gcc on the
header against the ctypes mirror, the exported symbol) and PPOTrainer's argument checks for
self_play="decisions".  The kernel is checked in test_gpu_selfplay_skip.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

from footsies_gym_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "footsies.h")


def test_header_compiles_as_c_with_the_new_constant(tmp_path):
    # (the prototype is only type-checked against a pointer of the declared shape: nothing links the library)
    lines = ['#include <stdio.h>', '#include "footsies.h"',
             "typedef int (*skip_selfplay_fn)(fs_handle, int, const fs_policy*, const fs_policy*, int, int,",
             "                                const fs_outputs*, const fs_skip_traj*);",
             "int main(void){", "skip_selfplay_fn f = 0; if (0) f = fs_step_skip_selfplay; (void)f;",
             'printf("kernel %d\\n", FS_KERNEL_SKIP_SELFPLAY); printf("max_ticks %d\\n", FS_SKIP_POLICY_MAX_TICKS);',
             'printf("abi %d\\n", FS_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "skip_selfplay.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "skip_selfplay"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["kernel"] == _abi.FS_KERNEL_SKIP_SELFPLAY == 64
    assert c["kernel"] & (_abi.FS_KERNEL_HASHED | _abi.FS_KERNEL_POLICY | _abi.FS_KERNEL_PACKED |
                          _abi.FS_KERNEL_SKIP_POLICY | _abi.FS_KERNEL_SELFPLAY | 8) == 0
    assert c["max_ticks"] == _abi.FS_SKIP_POLICY_MAX_TICKS
    assert c["abi"] == _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed


def test_step_skip_selfplay_is_exported_with_the_declared_arguments():
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert hasattr(lib, "fs_step_skip_selfplay")
    text = open(HEADER).read()
    m = re.search(r"^int fs_step_skip_selfplay\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/footsies.h does not declare fs_step_skip_selfplay"
    ctype = {"fs_handle": C.c_void_p, "int": C.c_int, "const fs_policy*": C.POINTER(_abi.fs_policy),
             "const fs_outputs*": C.POINTER(_abi.fs_outputs), "const fs_skip_traj*": C.POINTER(_abi.fs_skip_traj)}
    declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS["fs_step_skip_selfplay"]
    assert restype is C.c_int and argtypes == declared and len(declared) == 8
    # without a handle the call is refused before anything else is looked at
    f = lib.fs_step_skip_selfplay
    f.restype, f.argtypes = restype, argtypes
    pol = _abi.fs_policy()
    assert f(None, 4, C.byref(pol), C.byref(pol), _abi.FS_SELFPLAY_MIRROR, 8, None, None) == _abi.FS_E_INVALID
    k = lib.fs_step_kernel
    k.restype, k.argtypes = _abi.LIB_FUNCTIONS["fs_step_kernel"]
    assert k(None, 8, _abi.FS_KERNEL_SKIP_SELFPLAY) is None
    assert lib.fs_abi_version() == 8


def test_ppo_trainer_checks_decisions_self_play_before_the_device():
    import types
    from footsies_gym_amd.ppo import PPOTrainer
    bot = types.SimpleNamespace(p2_mode="bot")
    ext = types.SimpleNamespace(p2_mode="external")
    for bad in ("nonsense", "decision", "ticks", ""):
        with pytest.raises(ValueError, match="self_play"):
            PPOTrainer(ext, self_play=bad)
    with pytest.raises(ValueError, match="external"):
        PPOTrainer(bot, self_play="decisions")
    for k in (0, -2):
        with pytest.raises(ValueError, match="opponent_refresh"):
            PPOTrainer(ext, self_play="decisions", opponent_refresh=k)
    for cap in (0, _abi.FS_SKIP_POLICY_MAX_TICKS + 1):
        with pytest.raises(ValueError, match="max_skip_ticks"):
            PPOTrainer(ext, self_play="decisions", max_skip_ticks=cap)
    # per-tick self-play keeps refusing frame_skip, and now names the way through
    with pytest.raises(ValueError, match="frame_skip") as e:
        PPOTrainer(ext, self_play=True, frame_skip=True)
    assert "decisions" in str(e.value)


def test_rollout_skipped_is_built():
    import inspect
    from footsies_gym_amd.rollout import FusedSelfPlayRollout
    sig = inspect.signature(FusedSelfPlayRollout.rollout_skipped)
    assert list(sig.parameters) == ["self", "n", "actions", "logp", "ticks", "capped", "p2_actions", "p2_logp",
                                    "trajectory", "max_ticks"]
    assert sig.parameters["p2_actions"].default is False and sig.parameters["p2_logp"].default is False
    assert sig.parameters["max_ticks"].default == _abi.FS_SKIP_DEFAULT_MAX_TICKS
