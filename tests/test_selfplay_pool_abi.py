"""The opponent pool's host side without a GPU: the constants, the struct and the two calls in the C-ABI
(gcc on the header against the ctypes mirror, the exported symbols), OpponentPool.assign -- a pure function
of (seed, iteration, global group index, filled, newest) -- on a stub sim, and PPOTrainer's argument checks.
The kernels are checked in test_gpu_selfplay_pool.py."""
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


def test_header_compiles_as_c99_with_the_new_constants_and_struct(tmp_path):
    fields = [f for f, _ in _abi.fs_policy_pool._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "footsies.h"',
             "typedef int (*pool_n_fn)(fs_handle, int, const fs_policy*, const fs_policy_pool*, int, const fs_outputs*);",
             "typedef int (*pool_skip_fn)(fs_handle, int, const fs_policy*, const fs_policy_pool*, int, int,",
             "                            const fs_outputs*, const fs_skip_traj*);",
             "int main(void){",
             "pool_n_fn f = 0; pool_skip_fn g = 0;",
             "if (0) { f = fs_step_n_selfplay_pool; g = fs_step_skip_selfplay_pool; } (void)f; (void)g;",
             'printf("group %d\\n", FS_SELFPLAY_GROUP); printf("max %d\\n", FS_SELFPLAY_POOL_MAX);',
             'printf("kernel_n %d\\n", FS_KERNEL_SELFPLAY_POOL); printf("kernel_skip %d\\n", FS_KERNEL_SKIP_SELFPLAY_POOL);',
             'printf("params %d\\n", FS_PPO_ACTOR_PARAMS); printf("abi %d\\n", FS_ABI_VERSION);',
             'printf("size %d\\n", (int)sizeof(fs_policy_pool));']
    lines += ['printf("%s %%d\\n", (int)offsetof(fs_policy_pool, %s));' % (f, f) for f in fields]
    lines.append("return 0;}")
    src = tmp_path / "pool.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "pool"
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert c["group"] == _abi.FS_SELFPLAY_GROUP == 128 and c["max"] == _abi.FS_SELFPLAY_POOL_MAX == 256
    assert c["kernel_n"] == _abi.FS_KERNEL_SELFPLAY_POOL == 128 and c["kernel_skip"] == _abi.FS_KERNEL_SKIP_SELFPLAY_POOL == 256
    older = (_abi.FS_KERNEL_HASHED | _abi.FS_KERNEL_POLICY | _abi.FS_KERNEL_PACKED | _abi.FS_KERNEL_SKIP_POLICY |
             _abi.FS_KERNEL_SELFPLAY | _abi.FS_KERNEL_SKIP_SELFPLAY | 8)
    assert c["kernel_n"] & older == 0 and c["kernel_skip"] & older == 0 and c["kernel_n"] & c["kernel_skip"] == 0
    assert c["params"] == _abi.FS_PPO_ACTOR_PARAMS == 5256
    assert c["abi"] == _abi.FS_ABI_VERSION == 8  # an addition: no existing struct or call changed
    assert c["size"] == C.sizeof(_abi.fs_policy_pool)
    for f in fields:
        assert c[f] == getattr(_abi.fs_policy_pool, f).offset, f


@pytest.mark.parametrize("name,n_args", [("fs_step_n_selfplay_pool", 6), ("fs_step_skip_selfplay_pool", 8)])
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
    # without a handle the call is refused before anything else is looked at
    f = getattr(lib, name)
    f.restype, f.argtypes = restype, argtypes
    pol, pool = _abi.fs_policy(), _abi.fs_policy_pool()
    tail = (None,) if n_args == 6 else (8, None, None)
    assert f(None, 4, C.byref(pol), C.byref(pool), _abi.FS_SELFPLAY_MIRROR, *tail) == _abi.FS_E_INVALID
    k = lib.fs_step_kernel
    k.restype, k.argtypes = _abi.LIB_FUNCTIONS["fs_step_kernel"]
    assert k(None, 8, _abi.FS_KERNEL_SELFPLAY_POOL) is None and k(None, 8, _abi.FS_KERNEL_SKIP_SELFPLAY_POOL) is None
    assert lib.fs_abi_version() == 8


def stub(num_envs, arena_base=0):
    import torch
    return types.SimpleNamespace(num_envs=num_envs, arena_base=arena_base, device=torch.device("cpu"), p2_mode="external")


def filled_pool(sim, capacity, pushes):
    from footsies_gym_amd.rollout import OpponentPool, make_actor
    pool = OpponentPool(sim, capacity)
    for i in range(pushes):
        assert pool.push(make_actor(seed=i)) == i % capacity
    return pool


def test_pool_slots_fill_in_order_then_the_oldest_is_overwritten():
    import torch
    from footsies_gym_amd.rollout import _weights, make_actor
    sim = stub(256)
    pool = filled_pool(sim, 3, 0)
    assert pool.filled == 0 and pool.newest is None and pool.weights.shape == (3, _abi.FS_PPO_ACTOR_PARAMS)
    with pytest.raises(ValueError, match="empty"):
        pool.assign(0)
    ptr = pool.weights.data_ptr()
    for i, (slot, filled) in enumerate([(0, 1), (1, 2), (2, 3), (0, 3), (1, 3)]):
        actor = make_actor(seed=10 + i)
        assert pool.push(actor) == slot and pool.newest == slot and pool.filled == filled
        views = pool.params(slot)
        assert [tuple(v.shape) for v in views] == [(64, 8), (64,), (64, 64), (64,), (8, 64), (8,)]
        assert all(torch.equal(v, w) for v, w in zip(views, _weights(actor)))
        # a slot is the six arrays packed in fs_policy order
        flat = torch.cat([w.detach().reshape(-1) for w in _weights(actor)])
        assert torch.equal(pool.weights[slot], flat)
    assert pool.weights.data_ptr() == ptr
    with pytest.raises(ValueError, match="8 -> 64 -> 64 -> 8"):
        pool.push(make_actor(hidden=32))
    for bad in (0, 257):
        with pytest.raises(ValueError, match="capacity"):
            filled_pool(sim, bad, 0)


def test_assign_is_a_pure_counter_based_function():
    import torch
    from footsies_gym_amd.rollout import pool_assignment
    sim = stub(2048 * 128)
    pool = filled_pool(sim, 8, 4)
    a = pool.assign(5, latest=0.5, seed=9)
    assert a.dtype == torch.uint8 and a.shape == (2048,) and a.device == sim.device
    assert torch.equal(a, pool.assign(5, latest=0.5, seed=9))  # deterministic
    assert not torch.equal(a, pool.assign(6, latest=0.5, seed=9))  # a fresh draw per iteration
    assert not torch.equal(a, pool.assign(5, latest=0.5, seed=10))
    assert int(a.max()) < 4  # only filled slots
    # it is the documented function of (seed, iteration, global group, filled, newest)
    assert np.array_equal(a.numpy(), pool_assignment(9, 5, 0, 2048, 4, 3, 0.5))
    # latest = 1: everyone meets the newest snapshot
    assert (pool.assign(0, latest=1.0).numpy() == pool.newest).all() and pool.newest == 3
    # latest = 0: uniform over the filled slots -- each share within four binomial standard deviations of 1/4
    counts = np.bincount(pool.assign(0, latest=0.0).numpy(), minlength=8)
    sd = np.sqrt(2048 * 0.25 * 0.75)
    assert counts[4:].sum() == 0 and (np.abs(counts[:4] - 512) < 4 * sd).all(), counts
    # latest = 0.5: the newest gets its half plus a quarter of the rest (p = 5/8), again within four deviations
    share = int((a.numpy() == 3).sum())
    assert abs(share - 2048 * 0.625) < 4 * np.sqrt(2048 * 0.625 * 0.375), share
    # a partial last group has a slot of its own
    assert filled_pool(stub(289), 3, 3).assign(0).shape == (3,)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="latest"):
            pool.assign(0, latest=bad)


def test_shards_draw_what_the_unsharded_run_draws():
    import torch
    whole = filled_pool(stub(65536), 8, 5).assign(3, seed=1)
    parts = [filled_pool(stub(32768, base), 8, 5).assign(3, seed=1) for base in (0, 32768)]
    assert whole.shape == (512,) and torch.equal(torch.cat(parts), whole)
    assert not torch.equal(parts[0], parts[1])
    with pytest.raises(ValueError, match="arena_base"):
        filled_pool(stub(256, 64), 8, 5).assign(3)


def test_ppo_trainer_checks_the_pool_arguments_before_the_device():
    from footsies_gym_amd.ppo import PPOTrainer
    ext = types.SimpleNamespace(p2_mode="external")  # (no device, no handle: a check that got past would fail on it)
    for mode in (True, "decisions"):
        for k in (1, 0, -3, 257):
            with pytest.raises(ValueError, match="opponent_pool"):
                PPOTrainer(ext, self_play=mode, opponent_pool=k)
        for p in (-0.01, 1.01, float("nan")):
            with pytest.raises(ValueError, match="opponent_latest"):
                PPOTrainer(ext, self_play=mode, opponent_pool=3, opponent_latest=p)
    with pytest.raises(ValueError, match="self_play"):
        PPOTrainer(ext, opponent_pool=3)
    with pytest.raises(ValueError, match="self_play"):
        PPOTrainer(types.SimpleNamespace(p2_mode="bot"), opponent_pool=3)
    with pytest.raises(ValueError, match="arena_base"):
        PPOTrainer(types.SimpleNamespace(p2_mode="external", arena_base=64), self_play=True, opponent_pool=3)


def test_the_pool_rollout_takes_slots_and_the_single_opponent_one_is_unchanged():
    import inspect
    from footsies_gym_amd.rollout import FusedPoolSelfPlayRollout, FusedSelfPlayRollout
    assert issubclass(FusedPoolSelfPlayRollout, FusedSelfPlayRollout)
    for name in ("rollout", "rollout_skipped"):
        base = list(inspect.signature(getattr(FusedSelfPlayRollout, name)).parameters)
        pool = list(inspect.signature(getattr(FusedPoolSelfPlayRollout, name)).parameters)
        assert pool == base + ["slots"], name
