"""fs_step_n_selfplay's host side without a GPU: the constants and the call in the C-ABI (gcc on the
header against the ctypes mirror, the exported symbol) and the two helpers that restate what the
mirrored P2 actor sees and presses.  The kernel is checked in test_gpu_selfplay.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from footsies_gym_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "footsies.h")

# Left = 1, Right = 2, Attack = 4: index -> the same buttons with Left and Right exchanged
SWAPPED = [0, 2, 1, 3, 4, 6, 5, 7]


def test_header_compiles_as_c_with_the_new_constants(tmp_path):
    # (the prototype is only type-checked against a pointer of the declared shape: nothing links the library)
    lines = ['#include <stdio.h>', '#include "footsies.h"',
             "typedef int (*selfplay_fn)(fs_handle, int, const fs_policy*, const fs_policy*, int, const fs_outputs*);",
             "int main(void){", "selfplay_fn f = 0; if (0) f = fs_step_n_selfplay; (void)f;",
             'printf("mirror %d\\n", FS_SELFPLAY_MIRROR); printf("kernel %d\\n", FS_KERNEL_SELFPLAY);',
             'printf("abi %d\\n", FS_ABI_VERSION);', "return 0;}"]
    src = tmp_path / "selfplay.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "selfplay"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["mirror"] == _abi.FS_SELFPLAY_MIRROR == 1
    assert c["kernel"] == _abi.FS_KERNEL_SELFPLAY == 32
    assert c["kernel"] & (_abi.FS_KERNEL_HASHED | _abi.FS_KERNEL_POLICY | _abi.FS_KERNEL_PACKED |
                          _abi.FS_KERNEL_SKIP_POLICY) == 0
    assert c["abi"] == _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed


def test_step_n_selfplay_is_exported_with_the_declared_arguments():
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert hasattr(lib, "fs_step_n_selfplay")
    text = open(HEADER).read()
    m = re.search(r"^int fs_step_n_selfplay\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/footsies.h does not declare fs_step_n_selfplay"
    ctype = {"fs_handle": C.c_void_p, "int": C.c_int, "const fs_policy*": C.POINTER(_abi.fs_policy),
             "const fs_outputs*": C.POINTER(_abi.fs_outputs)}
    declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS["fs_step_n_selfplay"]
    assert restype is C.c_int and argtypes == declared
    # without a handle the call is refused before anything else is looked at
    f = lib.fs_step_n_selfplay
    f.restype, f.argtypes = restype, argtypes
    pol = _abi.fs_policy()
    assert f(None, 4, C.byref(pol), C.byref(pol), _abi.FS_SELFPLAY_MIRROR, None) == _abi.FS_E_INVALID
    assert lib.fs_abi_version() == 8


def test_swap_left_right_table():
    import torch
    from footsies_gym_amd.rollout import swap_left_right
    a = np.arange(8, dtype=np.uint8)
    assert swap_left_right(a).tolist() == SWAPPED
    assert swap_left_right(swap_left_right(a)).tolist() == a.tolist()
    t = torch.arange(8, dtype=torch.uint8)
    assert swap_left_right(t).tolist() == SWAPPED and swap_left_right(t).dtype == torch.uint8
    assert torch.equal(swap_left_right(swap_left_right(t)), t)
    assert [swap_left_right(i) for i in range(8)] == SWAPPED
    for i, s in enumerate(SWAPPED):  # by buttons: Attack stays, Left and Right trade places
        assert (s & 4) == (i & 4) and bool(s & 1) == bool(i & 2) and bool(s & 2) == bool(i & 1)


def test_mirror_features_row():
    import torch
    from footsies_gym_amd.rollout import mirror_features
    #      g1   g2   m1    m2    mf1   mf2   x1    x2
    row = [1.0, 2/3, 0.25, 0.5, 0.125, 0.0, -0.5, 0.75]
    want = [2/3, 1.0, 0.5, 0.25, 0.0, 0.125, -0.75, 0.5]
    x = np.array([row, [v + 1 for v in row]], dtype=np.float32)
    keep = x.copy()
    y = mirror_features(x)
    assert np.array_equal(y[0], np.array(want, dtype=np.float32))
    assert np.array_equal(x, keep)  # the argument is left alone
    assert np.array_equal(mirror_features(y), x)
    assert np.array_equal(mirror_features(x[None])[0], y)  # leading dimensions pass through
    t = torch.tensor(x)
    assert torch.equal(mirror_features(t), torch.tensor(y)) and torch.equal(t, torch.tensor(keep))
    assert torch.equal(mirror_features(mirror_features(t)), t)


def test_ppo_trainer_refuses_bad_self_play_arguments_before_the_device():
    import types
    from footsies_gym_amd.ppo import PPOTrainer
    bot = types.SimpleNamespace(p2_mode="bot")
    ext = types.SimpleNamespace(p2_mode="external")
    with pytest.raises(ValueError, match="external"):
        PPOTrainer(bot, self_play=True)
    with pytest.raises(ValueError, match="frame_skip"):
        PPOTrainer(ext, self_play=True, frame_skip=True)
    for k in (0, -2):
        with pytest.raises(ValueError, match="opponent_refresh"):
            PPOTrainer(ext, self_play=True, opponent_refresh=k)
