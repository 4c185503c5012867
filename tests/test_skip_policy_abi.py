"""fs_step_skip_policy's host side without a GPU: fs_skip_traj and the call in the C-ABI (gcc on the
header against the ctypes mirror, the exported symbol) and the Python arguments that are refused
before any device is touched.  The kernel is checked in test_gpu_skip_policy.py."""
import ctypes as C
import os
import re
import subprocess
import types

import pytest

from footsies_gym_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "footsies.h")


def test_skip_traj_layout_matches_ctypes(tmp_path):
    cls = _abi.fs_skip_traj
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "footsies.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(fs_skip_traj));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(fs_skip_traj, %s));' % (f, f))
    lines.append('printf("max %d\\n", FS_SKIP_POLICY_MAX_TICKS); printf("cap %d\\n", FS_SKIP_DEFAULT_MAX_TICKS);')
    lines.append('printf("kernel %d\\n", FS_KERNEL_SKIP_POLICY); printf("abi %d\\n", FS_ABI_VERSION);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert [f for f, _ in cls._fields_] == ["ticks", "capped"]
    assert c["size"] == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert c[f] == getattr(cls, f).offset, f
    assert c["max"] == _abi.FS_SKIP_POLICY_MAX_TICKS >= c["cap"] == _abi.FS_SKIP_DEFAULT_MAX_TICKS
    assert c["kernel"] == _abi.FS_KERNEL_SKIP_POLICY
    assert c["kernel"] & (_abi.FS_KERNEL_HASHED | _abi.FS_KERNEL_POLICY | _abi.FS_KERNEL_PACKED) == 0
    assert c["abi"] == _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed


def test_step_skip_policy_is_exported_with_the_declared_arguments():
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert hasattr(lib, "fs_step_skip_policy")
    text = open(HEADER).read()
    m = re.search(r"^int fs_step_skip_policy\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/footsies.h does not declare fs_step_skip_policy"
    ctype = {"fs_handle": C.c_void_p, "int": C.c_int, "const fs_policy*": C.POINTER(_abi.fs_policy),
             "const fs_outputs*": C.POINTER(_abi.fs_outputs), "const fs_skip_traj*": C.POINTER(_abi.fs_skip_traj)}
    declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS["fs_step_skip_policy"]
    assert restype is C.c_int and argtypes == declared
    # without a handle the call is refused before anything else is looked at
    f = lib.fs_step_skip_policy
    f.restype, f.argtypes = restype, argtypes
    assert f(None, 4, None, 64, None, None) == _abi.FS_E_INVALID
    pol = _abi.fs_policy()
    assert f(None, 0, C.byref(pol), 0, None, None) == _abi.FS_E_INVALID
    assert lib.fs_abi_version() == 8


def test_rollout_skipped_refuses_bad_counts_before_the_device():
    import torch
    from footsies_gym_amd.rollout import FusedPolicyRollout, make_actor
    sim = types.SimpleNamespace(device=torch.device("cpu"), num_envs=4, handle=None)  # never reached
    ro = FusedPolicyRollout(sim, make_actor(seed=1))
    for kw in (dict(n=0), dict(n=-3), dict(n=2, max_ticks=0), dict(n=2, max_ticks=_abi.FS_SKIP_POLICY_MAX_TICKS + 1)):
        with pytest.raises(ValueError):
            ro.rollout_skipped(**kw)
    assert ro.last_capped is None


def test_ppo_trainer_refuses_a_bad_skip_cap_before_the_device():
    from footsies_gym_amd.ppo import PPOTrainer
    for cap in (0, -1, _abi.FS_SKIP_POLICY_MAX_TICKS + 1):
        with pytest.raises(ValueError, match="max_skip_ticks"):
            PPOTrainer(None, frame_skip=True, max_skip_ticks=cap)
