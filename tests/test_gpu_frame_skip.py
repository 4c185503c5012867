"""The fused frame skip (fs_step_skip / k_step_skip, FootsiesFrameSkipped(fused=True)) against the
reference wrapper's own fixtures and, step by step, against the unfused wrapper over the CPU
oracle.  Every comparison is bitwise."""
import functools

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd import spaces as sp
from footsies_gym_amd import wrappers as W
from footsies_gym_amd.simulator import encode_actions
from footsies_gym_amd.vector_env import obs_info_from_outputs, step_result_from_outputs
from tests import wrapper_replay as wr
from tests.parity_utils import OBS_KEYS, FINAL_KEYS, assert_same, compare_states, random_states

pytestmark = pytest.mark.gpu

P2 = {"bot": _abi.FS_P2_BOT, "noop": _abi.FS_P2_NOOP}
FLOAT = {"strict": _abi.FS_FLOAT_STRICT32, "double": _abi.FS_FLOAT_DOUBLE}
AR = {"same_step": _abi.FS_AUTORESET_SAME_STEP, "next_step": _abi.FS_AUTORESET_NEXT_STEP}
N, STEPS, SEED = 130, 300, 11  # a partial wave and an odd pair count
OBS = ("guard", "move", "move_frame", "position")


class OracleEnv:
    """The FootsiesVectorEnv surface the unfused wrapper needs (reset / step / step_masked) over the
    CPU oracle, counting each arena's ticks since the last step()."""

    def __init__(self, n, oracle_lib, p2="bot", autoreset="same_step", dense=True, float_mode="strict", seed=0):
        self.num_envs = n
        self.autoreset_mode = autoreset
        self.ora = oracle_lib.Oracle(n, p2_mode=P2[p2], dense_reward=dense, float_mode=FLOAT[float_mode],
                                     autoreset_mode=AR[autoreset], base_seed=seed)
        self.single_observation_space = sp.single_observation_space()
        self.ticks = np.zeros(n, np.int64)

    def reset(self, *, seed=None, options=None):
        return obs_info_from_outputs(self.ora.reset())

    def step(self, actions):
        self.ticks[:] = 1
        return step_result_from_outputs(self.ora.step(encode_actions(np.asarray(actions))), self.autoreset_mode)

    def step_masked(self, actions, active):
        active = np.asarray(active, dtype=bool)
        self.ticks += active
        out = self.ora.step(encode_actions(np.asarray(actions)), active=active.astype(np.uint8))
        out["reward"][~active] = 0.0
        out["terminated"][~active] = 0
        out["truncated"][~active] = 0
        return step_result_from_outputs(out, self.autoreset_mode)


def actions_for(n, steps, seed=5):
    return np.random.default_rng(seed).integers(0, 8, (steps, n)).astype(np.uint8)


def gpu_env(n, p2="bot", autoreset="same_step", dense=True, float_mode="strict", seed=0, output="numpy"):
    from footsies_gym_amd.vector_env import FootsiesVectorEnv
    return FootsiesVectorEnv(n, opponent=None if p2 == "bot" else "noop", dense_reward=dense, autoreset_mode=autoreset,
                             float_mode=float_mode, seed=seed, output=output)


def compare_step(exp, got, t):
    """One wrapped step's 5-tuples: obs, reward bits, terminated / truncated, every info array and
    the per-arena final_observation / final_info dicts."""
    eo, er, et, etr, ei = exp
    go, gr, gt, gtr, gi = got
    for k in OBS:
        assert_same("obs." + k, eo[k], go[k], t)
    assert_same("reward", np.asarray(er, np.float64), np.asarray(gr, np.float64), t)
    assert_same("terminated", np.asarray(et, bool), np.asarray(gt, bool), t)
    assert_same("truncated", np.asarray(etr, bool), np.asarray(gtr, bool), t)
    assert set(ei) == set(gi), (t, sorted(ei), sorted(gi))
    for k, v in ei.items():
        if k in ("final_observation", "final_info"):
            for i in np.nonzero(ei["_" + k])[0]:
                assert set(v[i]) == set(gi[k][i]), (t, k, i)
                for f, x in v[i].items():
                    assert_same("%s[%d].%s" % (k, i, f), x, gi[k][i][f], t)
            assert all(gi[k][i] is None for i in np.nonzero(~np.asarray(ei["_" + k]))[0]), (t, k)
        else:
            assert_same("info." + k, v, gi[k], t)


def lockstep(oracle_lib, n, steps, cfg, state=None, bars=None):
    """The unfused wrapper over the oracle and the fused wrapper on the GPU, step by step."""
    base_o = OracleEnv(n, oracle_lib, **cfg)
    base_g = gpu_env(n, **cfg)
    if state is not None:
        base_o.ora.set_state(state)
        base_g.load_battle_state(state)
    exp_env = W.FootsiesFrameSkipped(base_o)
    got_env = W.FootsiesFrameSkipped(base_g, fused=True)
    if state is None:
        eo, _ = exp_env.reset()
        go, _ = got_env.reset()
        for k in OBS:
            assert_same("reset." + k, eo[k], go[k])
    acts = actions_for(n, steps)
    max_ticks, ended, skipped = 0, 0, 0
    for t in range(steps):
        a = W.FootsiesActionCombinationsDiscretized.action(acts[t])
        exp = exp_env.step(a)
        got = got_env.step(a)
        compare_step(exp, got, t)
        assert_same("last_skip_ticks", base_o.ticks, np.asarray(base_g.last_skip_ticks, np.int64), t)
        max_ticks = max(max_ticks, int(base_o.ticks.max()))
        ended += int(np.asarray(exp[2]).sum())
        skipped += int((base_o.ticks > 1).sum())
    compare_states(base_o.ora.state(), base_g.sim.get_state(), steps)
    base_g.close()
    base_o.ora.close()
    stats = {"max_ticks": max_ticks, "ended": ended, "skipped": skipped / float(steps * n)}
    if bars is not None:  # the rollout reached the hard ground: long skips, episodes ending inside them
        assert max_ticks >= bars[0] and ended >= bars[1] and stats["skipped"] >= bars[2], stats
    return stats


# -- 1. the reference's own fixtures ----------------------------------------------------------------
FUSED_STACKS = {
    "skip_norm": lambda b: W.FootsiesFrameSkipped(W.FootsiesNormalized(b, exact=True), fused=True),
    "skip_raw": lambda b: W.FootsiesFrameSkipped(b, fused=True),
}


@pytest.mark.parametrize("name", sorted(FUSED_STACKS))
def test_fused_wrapper_replays_the_reference_fixtures(name):
    z = wr.load()
    n, steps, seed, dense = (int(v) for v in z[name + "/config"])
    env = FUSED_STACKS[name](gpu_env(n, autoreset="next_step", dense=bool(dense), seed=seed))
    obs, _ = env.reset()
    wr._check_obs(name, obs, lambda k: z["%s/first/%s" % (name, k)], -1)
    acts = z[name + "/actions"]
    for t in range(steps):
        obs, rew, term, trunc, _ = env.step(W.FootsiesActionCombinationsDiscretized.action(acts[t]))
        wr._check_obs(name, obs, lambda k: z["%s/%s" % (name, k)][t], t)
        assert np.array_equal(np.asarray(rew, np.float64).view(np.uint64),
                              z[name + "/reward"][t].view(np.uint64)), (name, "reward", t)
        assert np.array_equal(np.asarray(term).astype(np.uint8), z[name + "/terminated"][t]), (name, "term", t)
        assert not np.asarray(trunc).any()
    env.close()


# -- 2. lockstep with the oracle ----------------------------------------------------------------------
# The bars (most ticks one arena ran in a step, arenas that ended, share of (step, arena) pairs that
# skipped) are 40 / 100 / 10 % wherever the oracle side alone clears them.  It gives, at this shape and
# these actions: bot same_step 51 / 631 / 17.1 %, bot next_step 50 / 633-634 / 17.6 %; against an idle P2
# 22 / 80 (same_step) and 22 / 78 (next_step) / 32 % -- nothing there outlasts P1's own longest
# move and few rounds end, so those two cases are held to what the oracle gives.
LOCKSTEP = {
    "bot-same_step": (dict(p2="bot", autoreset="same_step"), (40, 100, 0.10)),
    "bot-next_step-double": (dict(p2="bot", autoreset="next_step", float_mode="double"), (40, 100, 0.10)),
    "noop-same_step": (dict(p2="noop", autoreset="same_step"), (22, 80, 0.10)),
    "noop-next_step": (dict(p2="noop", autoreset="next_step"), (22, 78, 0.10)),
    "bot-next_step-sparse": (dict(p2="bot", autoreset="next_step", dense=False), (40, 100, 0.10)),
}


@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_fused_wrapper_in_lockstep_with_the_oracle(oracle_lib, name):
    cfg, bars = LOCKSTEP[name]
    lockstep(oracle_lib, N, STEPS, dict(cfg, seed=SEED), bars=bars)


# -- 3. cap and resume ----------------------------------------------------------------------------------
def decide(sim, actions, cap):
    """One decision of every arena through the raw calls: (outputs, ticks, pending count of the
    first call, the first call's pending flags and outputs)."""
    sim.step_skip(actions, max_ticks=cap)
    first = sim.skip_pending_count()
    pend = sim.skip_pending.cpu().numpy().copy()
    first_out = sim.outputs_numpy()
    left = first
    while left:
        sim.step_skip(None, active=sim.skip_pending, max_ticks=cap, resume=True)
        left = sim.skip_pending_count()
    return sim.outputs_numpy(), sim.skip_ticks.cpu().numpy().copy(), first, pend, first_out


@functools.lru_cache(maxsize=None)
def uncapped_rollout(autoreset):
    """The rollout at the default cap (one call per decision: no arena skips 64 ticks), computed once."""
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(N, p2_mode="bot", autoreset_mode=autoreset, seed=SEED)
    acts = actions_for(N, STEPS)
    rows = []
    for t in range(STEPS):
        out, ticks, first, _, _ = decide(sim, acts[t], 64)
        assert first == 0, t
        rows.append((out, ticks))
    state = sim.get_state()
    sim.close()
    return rows, state


@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
@pytest.mark.parametrize("cap", [8, 1])
def test_any_cap_gives_the_uncapped_results(cap, autoreset):
    from footsies_gym_amd.simulator import FootsiesSim
    rows, state = uncapped_rollout(autoreset)
    sim = FootsiesSim(N, p2_mode="bot", autoreset_mode=autoreset, seed=SEED)
    acts = actions_for(N, STEPS)
    resumed = 0
    for t in range(STEPS):
        out, ticks, first, pend, first_out = decide(sim, acts[t], cap)
        exp, exp_ticks = rows[t]
        for k in OBS_KEYS:
            assert_same(k, exp[k], out[k], t)
        term = exp["terminated"].astype(bool)
        if autoreset == "same_step":
            for k in FINAL_KEYS:
                assert_same(k, exp[k][term], out[k][term], t)
        assert_same("ticks", exp_ticks, ticks, t)
        resumed += first > 0
        assert first == int(pend.sum())
        if cap == 1:  # one tick per call: pending is the wrapper's own test on that tick's observation
            want = W.is_skippable(first_out) & ~(first_out["terminated"].astype(bool))
            assert_same("pending", want.astype(np.uint8), pend, t)
    compare_states(state, sim.get_state(), STEPS)
    sim.close()
    assert resumed >= 0.1 * STEPS, resumed  # the cap was hit: resume calls carried the sums on


# -- 4. mask -----------------------------------------------------------------------------------------------
def test_masked_call_leaves_inactive_arenas_untouched():
    from footsies_gym_amd.simulator import FootsiesSim
    sims = [FootsiesSim(N, p2_mode="bot", seed=SEED) for _ in range(2)]
    acts = actions_for(N, 41)
    for t in range(39):  # into the middle of episodes, the same on both
        for s in sims:
            s.step_skip(acts[t])
    full, part = sims
    active = (np.arange(N) % 3 == 0)
    for s in sims:  # (a capped call: arenas stay pending, so both extra arrays hold both kinds of value)
        s.step_skip(acts[39], max_ticks=2)
    before, out_before = part.get_state(), part.outputs_numpy()
    ticks_before, pend_before = part.skip_ticks.cpu().numpy().copy(), part.skip_pending.cpu().numpy().copy()
    taken = part.steps_taken
    full.step_skip(acts[40], max_ticks=3)
    part.step_skip(acts[40], active=active, max_ticks=3)
    assert part.steps_taken == taken + 1
    after, out_after = part.get_state(), part.outputs_numpy()
    ticks_after, pend_after = part.skip_ticks.cpu().numpy(), part.skip_pending.cpu().numpy()
    compare_states(before[~active], after[~active])
    for k in out_before:
        assert_same(k, out_before[k][~active], out_after[k][~active])
    assert_same("ticks", ticks_before[~active], ticks_after[~active])
    assert_same("pending", pend_before[~active], pend_after[~active])
    assert pend_before[~active].any() and (ticks_before[~active] > 1).any()
    compare_states(full.get_state()[active], after[active])
    out_full = full.outputs_numpy()
    for k in OBS_KEYS:
        assert_same(k, out_full[k][active], out_after[k][active])
    assert_same("ticks", full.skip_ticks.cpu().numpy()[active], ticks_after[active])
    assert_same("pending", full.skip_pending.cpu().numpy()[active], pend_after[active])
    assert part.skip_pending_count() == int(pend_after[active].sum())
    for s in sims:
        s.close()


# -- 5. general geometry -------------------------------------------------------------------------------
def test_fused_wrapper_on_loaded_airborne_and_flipped_fighters(oracle_lib):
    state = random_states(66, np.random.default_rng(3), p2="bot", geom_frac=0.3)
    lockstep(oracle_lib, 66, 40, dict(p2="bot", autoreset="same_step", seed=4), state=state)


# -- 6. refusals ---------------------------------------------------------------------------------------
def test_refusals_and_step_counter():
    from footsies_gym_amd._lib import lib
    from footsies_gym_amd.simulator import FootsiesSim
    L = lib()
    a = np.zeros(8, np.uint8)

    def call(sim, p1=a, flags=_abi.FS_ACT_HOST, cap=64):
        rc = L.fs_step_skip(sim.handle, None if p1 is None else p1.ctypes.data, None, flags, cap, None)
        return rc, (L.fs_last_error(sim.handle) or b"").decode()

    ext = FootsiesSim(8, p2_mode="external")
    rc, msg = call(ext)
    assert rc == _abi.FS_E_UNSUPPORTED and msg
    ext.set_p2_mode("bot")
    rc, msg = call(ext)
    assert rc == _abi.FS_E_UNSUPPORTED and msg
    ext.close()
    for kw in ({"p1_mode": "bot"}, {"frame_delay": 3}):
        sim = FootsiesSim(8, p2_mode="bot", **kw)
        rc, msg = call(sim)
        assert rc == _abi.FS_E_UNSUPPORTED and msg, kw
        sim.close()
    sim = FootsiesSim(8, p2_mode="bot")
    assert call(sim, cap=0)[0] == _abi.FS_E_INVALID
    assert call(sim, p1=None)[0] == _abi.FS_E_INVALID
    assert call(sim, flags=4)[0] == _abi.FS_E_INVALID
    before = sim.steps_taken
    assert call(sim)[0] == _abi.FS_OK
    assert call(sim, p1=None, flags=_abi.FS_ACT_HOST | _abi.FS_SKIP_RESUME)[0] == _abi.FS_OK
    sim.sync()
    assert sim.steps_taken == before + 2
    sim.close()
    from footsies_gym_amd.vector_env import FootsiesVectorEnv
    for kw in ({"opponent": lambda obs, info: np.zeros(8, np.uint8)}, {"by_example": True}, {"frame_delay": 2}):
        env = FootsiesVectorEnv(8, **kw)
        with pytest.raises(ValueError):
            env.step_skipped(np.zeros(8, np.int64))
        with pytest.raises(ValueError):
            W.FootsiesFrameSkipped(env, fused=True)
        env.close()


# -- 7. torch output -----------------------------------------------------------------------------------
def test_torch_output_equals_numpy_output():
    import torch
    envs = [gpu_env(N, seed=SEED, output=o) for o in ("numpy", "torch")]
    for e in envs:
        e.reset()
    acts = actions_for(N, 50, seed=9)
    for t in range(50):
        obs, rew, term, trunc, info = envs[0].step_skipped(acts[t])
        tobs, trew, tterm, ttrunc, tout = envs[1].step_skipped(torch.as_tensor(acts[t], device="cuda"))
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (trew, tterm, ttrunc, *tobs.values()))
        for k in OBS:
            assert_same(k, np.asarray(obs[k]), tobs[k].cpu().numpy().astype(np.asarray(obs[k]).dtype), t)
        assert_same("reward", rew, trew.cpu().numpy(), t)
        assert_same("terminated", term, tterm.cpu().numpy().astype(bool), t)
        assert not ttrunc.any()
        assert_same("frame", info["frame"], tout["frame"].cpu().numpy().astype(np.int64), t)
        assert_same("ticks", envs[0].last_skip_ticks, envs[1].last_skip_ticks.cpu().numpy(), t)
    for e in envs:
        e.close()


# -- 8. without torch ----------------------------------------------------------------------------------
NATIVE_CHILD = r'''
import sys
sys.modules["torch"] = None  # torch is not importable in this process
sys.path.insert(0, %(root)r)
import numpy as np
from footsies_gym_amd.vector_env import FootsiesVectorEnv
env = FootsiesVectorEnv(%(n)d, seed=%(seed)d)
assert env.sim.backend == "native", env.sim.backend
env.reset()
acts = np.random.default_rng(9).integers(0, 8, (%(steps)d, %(n)d)).astype(np.uint8)
rec = {"obs": [], "rew": [], "term": [], "ticks": []}
for t in range(%(steps)d):
    obs, rew, term, trunc, info = env.step_skipped(acts[t], max_ticks=8)  # (a cap: resume calls too)
    rec["obs"].append(np.concatenate([obs[k].reshape(%(n)d, -1).astype(np.float64) for k in sorted(obs)], axis=1))
    rec["rew"].append(rew.copy())
    rec["term"].append(term.copy())
    rec["ticks"].append(env.last_skip_ticks.copy())
env.close()
np.savez(%(out)r, **{k: np.stack(v) for k, v in rec.items()})
'''


def test_step_skipped_without_torch(tmp_path):
    """The torch-free backend (outputs and the skip arrays in pinned host memory, the pending count
    summed on the host) against the torch-backed numpy env: a child process, as torch cannot be
    unloaded from this one."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "native_skip.npz")
    steps = 60
    r = subprocess.run([sys.executable, "-c", NATIVE_CHILD % dict(root=root, n=N, seed=SEED, steps=steps, out=out)],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    env = gpu_env(N, seed=SEED)
    env.reset()
    acts = actions_for(N, steps, seed=9)
    for t in range(steps):
        obs, rew, term, trunc, info = env.step_skipped(acts[t])
        flat = np.concatenate([obs[k].reshape(N, -1).astype(np.float64) for k in sorted(obs)], axis=1)
        assert_same("obs", flat, z["obs"][t], t)
        assert_same("reward", rew, z["rew"][t], t)
        assert_same("terminated", term, z["term"][t], t)
        assert_same("ticks", env.last_skip_ticks, z["ticks"][t], t)
    assert z["ticks"].max() > 8
    env.close()
