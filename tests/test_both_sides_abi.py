"""Learning from both sides of a self-play game, the host side without a GPU: the two P2 learner calls in the
C-ABI (gcc on the header against the ctypes mirror, the exported symbols and their argument checks, which return
before any launch), ppo.p2_eligible_groups / p2_selection -- pure host functions -- on hand-written cases, and
PPOTrainer(both_sides=True)'s refusals, which raise before the device is touched.  The kernels and the trainer
are checked in test_gpu_both_sides.py."""
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
N_ARGS = {"fs_ppo_features_p2": 10, "fs_ppo_gae_p2": 12}


def test_header_compiles_as_c99_with_the_two_prototypes(tmp_path):
    lines = ['#include <stdio.h>', '#include "footsies.h"',
             "typedef int (*features_fn)(const uint8_t*, const uint8_t*, const float*, const float*, int64_t, int64_t,",
             "                           const int32_t*, int64_t, float*, void*);",
             "typedef int (*gae_fn)(const double*, const uint8_t*, const float*, int, int64_t, const int32_t*, int64_t,",
             "                      float, float, float*, float*, void*);",
             "int main(void){",
             "features_fn f = 0; gae_fn g = 0;",
             "if (0) { f = fs_ppo_features_p2; g = fs_ppo_gae_p2; } (void)f; (void)g;",
             'printf("abi %d\\n", FS_ABI_VERSION);',
             "return 0;}"]
    src = tmp_path / "both.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "both"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    assert out.split() == ["abi", "8"] and _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed


@pytest.mark.parametrize("name", sorted(N_ARGS))
def test_the_calls_are_declared_with_matching_arguments(name):
    m = re.search(r"^int %s\(([^;]*)\);" % name, open(HEADER).read(), re.M | re.S)
    assert m, "include/footsies.h does not declare %s" % name
    declared = [" ".join(a.split()[:-1]) for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS[name]
    assert restype is C.c_int and len(argtypes) == len(declared) == N_ARGS[name]
    kinds = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float}
    for c_type, ctype in zip(declared, argtypes):
        assert ctype is (C.c_void_p if c_type.endswith("*") else kinds[c_type]), (name, c_type, ctype)


def test_the_calls_are_exported_and_check_their_arguments_before_any_launch():
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert lib.fs_abi_version() == 8
    err = lib.fs_last_error
    err.restype, err.argtypes = _abi.LIB_FUNCTIONS["fs_last_error"]
    f, g = lib.fs_ppo_features_p2, lib.fs_ppo_gae_p2
    f.restype, f.argtypes = _abi.LIB_FUNCTIONS["fs_ppo_features_p2"]
    g.restype, g.argtypes = _abi.LIB_FUNCTIONS["fs_ppo_gae_p2"]
    p = 4096  # (an aligned, never dereferenced address: every case below is refused on the host)

    def feat(guard=p, move=p, mf=p, pos=p, rows=3, n=130, sel=p, n_sel=5, out=p):
        return f(guard, move, mf, pos, rows, n, sel, n_sel, out, None)

    def gae(rew=p, done=p, val=p, t=4, n=130, sel=p, n_sel=5, adv=p, ret=p):
        return g(rew, done, val, t, n, sel, n_sel, 0.99, 0.94, adv, ret, None)

    bad_feat = [dict(guard=None), dict(move=None), dict(mf=None), dict(pos=None), dict(out=None), dict(rows=0),
                dict(n=0), dict(n_sel=0), dict(n_sel=-1), dict(out=p + 8), dict(pos=p + 4), dict(sel=p + 2),
                dict(sel=None, n_sel=5), dict(sel=None, n_sel=131), dict(n=2**31)]
    for kw in bad_feat:
        assert feat(**kw) == _abi.FS_E_INVALID, kw
        assert b"fs_ppo_features_p2" in err(None), kw
    bad_gae = [dict(rew=None), dict(done=None), dict(val=None), dict(adv=None), dict(ret=None), dict(t=0), dict(n=0),
               dict(n_sel=0), dict(sel=None, n_sel=129), dict(sel=p + 1), dict(n_sel=2**31)]
    for kw in bad_gae:
        assert gae(**kw) == _abi.FS_E_INVALID, kw
        assert b"fs_ppo_gae_p2" in err(None), kw
    assert feat(sel=None, n_sel=5) == _abi.FS_E_INVALID and b"n_sel == N" in err(None)


def test_p2_eligible_groups_single_opponent():
    from footsies_gym_amd.ppo import p2_eligible_groups
    ok = p2_eligible_groups(None, None, 0, None, groups=3)
    assert ok.dtype == np.bool_ and ok.tolist() == [True, True, True]
    assert p2_eligible_groups(None, None, 1, None, groups=3).tolist() == [False, False, False]
    assert p2_eligible_groups(None, None, 0, None).tolist() == [True]  # (one group unless told otherwise)


def test_p2_eligible_groups_pool_and_league():
    from footsies_gym_amd.ppo import p2_eligible_groups
    slots = np.array([2, 0, 2, 1, 2], dtype=np.uint8)
    ok = p2_eligible_groups(slots, 2, 0, None)
    assert ok.dtype == np.bool_ and ok.tolist() == [True, False, True, False, True]
    assert p2_eligible_groups(slots, 0, 0, None).tolist() == [False, True, False, False, False]
    assert not p2_eligible_groups(slots, 2, 1, None).any()  # the newest snapshot is an update old: nothing
    assert not p2_eligible_groups(slots, 2, 3, None).any()
    bots = np.array([True, False, False, False, True])
    assert p2_eligible_groups(slots, 2, 0, bots).tolist() == [False, False, True, False, False]
    assert not p2_eligible_groups(slots, 2, 1, bots).any()
    # a league around a single opponent (a one-slot pool: every slot byte is 0 = newest)
    assert p2_eligible_groups(np.zeros(5, np.uint8), 0, 0, bots).tolist() == [False, True, True, True, False]
    assert p2_eligible_groups(None, None, 0, bots).tolist() == [False, True, True, True, False]
    with pytest.raises(ValueError, match="bots"):
        p2_eligible_groups(slots, 2, 0, bots[:4])


def test_p2_selection_counts_a_partial_last_group_with_its_real_size():
    from footsies_gym_amd.ppo import p2_selection
    assert p2_selection([True, True], 130) is None and p2_selection([True], 7) is None  # every arena: the identity
    last = p2_selection([False, True], 130)
    assert last.dtype == np.int32 and last.tolist() == [128, 129]
    assert p2_selection([True, False], 130).tolist() == list(range(128))
    mid = p2_selection([True, False, True, False, True], 515)
    assert mid.tolist() == list(range(128)) + list(range(256, 384)) + [512, 513, 514]
    assert p2_selection([False, False], 130).size == 0
    with pytest.raises(ValueError, match="groups"):
        p2_selection([True], 130)


def test_ppo_trainer_refuses_both_sides_before_the_device():
    from footsies_gym_amd.ppo import PPOTrainer
    # (no device, no handle: a check that got past would fail on them)
    ext = types.SimpleNamespace(p2_mode="external")
    with pytest.raises(ValueError, match="both_sides.*self_play=True"):
        PPOTrainer(ext, both_sides=True)
    with pytest.raises(ValueError, match="both_sides.*self_play=True"):
        PPOTrainer(types.SimpleNamespace(p2_mode="bot"), both_sides=True)
    with pytest.raises(ValueError, match="decision process"):
        PPOTrainer(ext, self_play="decisions", both_sides=True)
    with pytest.raises(ValueError, match="decision process"):
        PPOTrainer(ext, self_play="decisions", both_sides=True, opponent_pool=3)
    for extra in (dict(opponent_pool=3), dict(opponent_bot=0.5), dict(opponent_pool=3, opponent_bot=0.5)):
        with pytest.raises(ValueError, match="both_sides.*group"):
            PPOTrainer(ext, self_play=True, both_sides=True, group="default", **extra)
