"""The fused frame skip's host side without a GPU: fs_skip_out / fs_step_skip in the C-ABI (gcc on
the header against the ctypes mirror, the exported symbol) and the wrappers' step_skipped plumbing
over a stub environment.  The kernel itself is checked in test_gpu_frame_skip.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd import spaces as sp
from footsies_gym_amd import wrappers as W
from tests.oracle_vector_env import OracleVectorEnv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "footsies.h")


def test_skip_out_layout_matches_ctypes(tmp_path):
    cls = _abi.fs_skip_out
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "footsies.h"', "int main(void){",
             'printf("size %zu\\n", sizeof(fs_skip_out));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(fs_skip_out, %s));' % (f, f))
    lines.append('printf("resume %d\\n", FS_SKIP_RESUME); printf("cap %d\\n", FS_SKIP_DEFAULT_MAX_TICKS);')
    lines.append('printf("abi %d\\n", FS_ABI_VERSION);')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.dirname(HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    c = {k: int(v) for k, v in (line.split() for line in out.strip().splitlines())}
    assert [f for f, _ in cls._fields_] == ["ticks", "pending", "n_pending"]
    assert c["size"] == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert c[f] == getattr(cls, f).offset, f
    assert c["resume"] == _abi.FS_SKIP_RESUME == 2
    assert c["cap"] == _abi.FS_SKIP_DEFAULT_MAX_TICKS == 64
    assert c["abi"] == _abi.FS_ABI_VERSION == 8
    assert _abi.FS_SKIP_RESUME & (_abi.FS_ACT_HOST | _abi.FS_ACT_DEVICE) == 0


def test_step_skip_is_exported_with_the_declared_arguments():
    import torch  # noqa: F401 -- first, as _lib.lib() does: one HIP runtime in the process
    from footsies_gym_amd import build
    build.build()
    lib = C.CDLL(build.LIB)
    assert hasattr(lib, "fs_step_skip")
    text = open(HEADER).read()
    m = re.search(r"^int fs_step_skip\(([^;]*)\);", text, re.M | re.S)
    assert m, "include/footsies.h does not declare fs_step_skip"
    ctype = {"fs_handle": C.c_void_p, "const uint8_t*": C.c_void_p, "int": C.c_int,
             "const fs_skip_out*": C.POINTER(_abi.fs_skip_out)}
    declared = [ctype[" ".join(a.split()[:-1])] for a in m.group(1).split(",")]
    restype, argtypes = _abi.LIB_FUNCTIONS["fs_step_skip"]
    assert restype is C.c_int and argtypes == declared
    # without a handle the call is refused before anything else is looked at
    f = lib.fs_step_skip
    f.restype, f.argtypes = restype, argtypes
    assert f(None, None, None, 0, 64, None) == _abi.FS_E_INVALID


class StubEnv:
    """A base vector env whose step_skipped records its actions and returns a fixed batch."""

    def __init__(self, n=3):
        self.num_envs = n
        self.single_observation_space = sp.single_observation_space()
        self.calls = []
        self.steps = []
        self.obs = {"guard": np.array([[3, 2], [1, 0], [2, 2]], np.int64),
                    "move": np.array([[5, 0], [0, 9], [7, 2]], np.int64),  # N_ATTACK / DAMAGE / N_SPECIAL
                    "move_frame": np.array([[11.0, 0.0], [0.0, 5.0], [22.0, 0.0]], np.float32),
                    "position": np.array([[-2.3, 2.3], [0.0, 4.6], [-4.6, 1.15]], np.float32)}
        final = np.empty(n, dtype=object)
        final[1] = {k: v[1].copy() for k, v in self.obs.items()}
        mask = np.array([False, True, False])
        self.info = {"frame": np.array([7, 8, 9]), "final_observation": final, "_final_observation": mask,
                     "final_info": final.copy(), "_final_info": mask.copy()}

    def _result(self):
        return ({k: v.copy() for k, v in self.obs.items()}, np.array([0.3, -1.0, 0.0]),
                np.array([False, True, False]), np.zeros(3, bool), dict(self.info))

    def step(self, actions):
        self.steps.append(np.asarray(actions))
        return self._result()

    def step_skipped(self, actions):
        self.calls.append(np.asarray(actions))
        return self._result()


def test_fused_needs_a_chain_with_step_skipped(oracle_lib):
    base = OracleVectorEnv(2, oracle_lib)
    W.FootsiesFrameSkipped(base)  # the default is the masked-step loop, which the double serves
    with pytest.raises(ValueError):
        W.FootsiesFrameSkipped(base, fused=True)
    with pytest.raises(ValueError):
        W.FootsiesFrameSkipped(W.FootsiesNormalized(base), fused=True)


def test_fused_refuses_statistics_in_the_chain():
    with pytest.raises(ValueError):
        W.FootsiesFrameSkipped(W.FootsiesStatistics(StubEnv()), fused=True)
    with pytest.raises(TypeError):
        W.FootsiesStatistics(StubEnv()).step_skipped(np.zeros(3, np.int64))


def test_fused_refuses_what_the_env_would_refuse():
    class Refusing(StubEnv):
        def skip_refusal(self):
            return "frame_delay > 0"
    with pytest.raises(ValueError, match="frame_delay"):
        W.FootsiesFrameSkipped(Refusing(), fused=True)


def test_discretized_maps_actions_for_step_skipped():
    stub = StubEnv()
    env = W.FootsiesActionCombinationsDiscretized(stub)
    acts = np.array([5, 2, 7])
    env.step(acts)
    env.step_skipped(acts)
    assert stub.calls[0].dtype == np.bool_ and stub.calls[0].shape == (3, 3)
    assert np.array_equal(stub.calls[0], stub.steps[0])
    assert stub.calls[0].tolist() == [[True, False, True], [False, True, False], [True, True, True]]


def test_normalized_transforms_obs_and_final_observations():
    stub = StubEnv()
    env = W.FootsiesNormalized(stub, exact=True)
    obs, rew, term, trunc, info = env.step_skipped(np.zeros((3, 3), bool))
    want = env.observation(stub.obs)
    for k in want:
        assert np.array_equal(np.asarray(obs[k]), np.asarray(want[k])), k
    assert obs["position"][1, 1] == 1.0 and obs["guard"][0, 0] == 1.0
    assert obs["move_frame"][2, 0] == 22.0 / 44.0  # N_SPECIAL lasts 44 frames
    fo = info["final_observation"][1]
    assert fo["position"][1] == 1.0 and fo["move_frame"][1] == 5.0 / 17.0  # DAMAGE lasts 17
    assert info["final_observation"][0] is None
    assert rew.tolist() == [0.3, -1.0, 0.0] and term.tolist() == [False, True, False]


def test_frame_skipped_fused_drops_p1_move_frame():
    stub = StubEnv()
    env = W.FootsiesFrameSkipped(stub, fused=True)
    acts = np.ones((3, 3), bool)
    obs, rew, term, trunc, info = env.step(acts)
    assert len(stub.calls) == 1 and not stub.steps and np.array_equal(stub.calls[0], acts)
    assert obs["move_frame"].shape == (3, 1) and obs["move_frame"][:, 0].tolist() == [0.0, 5.0, 0.0]
    assert info["final_observation"][1]["move_frame"].tolist() == [5.0]
    assert np.array_equal(obs["move"], stub.obs["move"])
    assert rew.tolist() == [0.3, -1.0, 0.0]
    # unfused, the same stub is stepped tick by tick instead
    plain = W.FootsiesFrameSkipped(StubEnv())
    assert plain.fused is False
