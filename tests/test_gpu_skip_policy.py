"""fs_step_skip_policy / k_step_skip_policy (FusedPolicyRollout.rollout_skipped, PPOTrainer(frame_skip=True)):
n agent decisions per arena in one launch, the actor in the kernel, each arena skipping its own frames.

The simulation is held bitwise to the reference's frame-skip wrapper: the kernel's own actions, fed to the
unfused wrapper of masked steps over the CPU oracle, give the same observation, float64 reward sum, flags,
info, final_* and tick count for every decision, and the same final state.  The actor is held to the bars
of test_gpu_policy (_check_policy: MARGIN, LOGP_TOL) with the uniform counted in decisions."""
import functools

import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd import wrappers as W
from footsies_gym_amd.vector_env import step_result_from_outputs
from tests.parity_utils import FINAL_KEYS, OBS_KEYS, assert_same, compare_states, random_states
from tests.test_gpu_frame_skip import OracleEnv, compare_step
from tests.test_gpu_policy import _check_policy

pytestmark = pytest.mark.gpu

CAP = _abi.FS_SKIP_DEFAULT_MAX_TICKS
POL_SEED, ACTOR_SEED = 0xC0FFEE, 9
WAVE = 32  # arenas per wave (two lanes each)


def make(n, p2="bot", autoreset="same_step", float_mode="strict", dense=True, seed=21, **kw):
    import torch
    from footsies_gym_amd.rollout import FusedPolicyRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    sim = FootsiesSim(n, p2_mode=p2, autoreset_mode=autoreset, float_mode=float_mode, dense_reward=dense, seed=seed, **kw)
    ro = FusedPolicyRollout(sim, make_actor(device=torch.device("cuda", 0), seed=ACTOR_SEED), seed=POL_SEED)
    return sim, ro


def run(sim, ro, n, max_ticks=CAP):
    """One call: every [n][N] output on the host."""
    import torch
    traj = sim.alloc_trajectory(n)
    acts, logps, ticks = ro.rollout_skipped(n, trajectory=traj, max_ticks=max_ticks)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in traj.items()}
    res.update(A=acts.cpu().numpy(), LP=logps.cpu().numpy(), ticks=ticks.cpu().numpy(), capped=ro.last_capped.cpu().numpy())
    return res


def row(res, d):
    return {k: res[k][d] for k in _abi.OUTPUT_SPEC}


def wrapped_row(res, d, autoreset):
    """Decision d's trajectory row as the frame-skip wrapper's 5-tuple (the fused wrapper's own conversion)."""
    obs, rew, term, trunc, info = step_result_from_outputs(row(res, d), autoreset)
    return W.frame_skip_obs(obs), rew, term, trunc, W._map_final(info, W.frame_skip_obs)


class CappedFrameSkipped(W.FootsiesFrameSkipped):
    """FootsiesFrameSkipped's masked-step loop with the cap restated: the action's tick, then input 0
    while the observation is skippable and the episode goes on, at most `cap` ticks; `capped` flags the
    arenas still skippable there.  Without a capped arena this is the reference wrapper's loop."""

    def __init__(self, env, cap):
        super().__init__(env)
        self.cap = cap
        self.capped = None

    def step(self, actions):
        obs, rew, term, trunc, info = self.env.step(actions)
        obs = {k: np.array(v) for k, v in obs.items()}
        total = 0.0 + np.asarray(rew, dtype=np.float64)
        term, trunc = np.array(term), np.array(trunc)
        info = dict(info)
        ran = np.ones(self.num_envs, np.int64)
        more = W.is_skippable(obs) & ~(term | trunc)
        pending = more & (ran < self.cap)
        while pending.any():
            o2, r2, t2, tr2, i2 = self.env.step_masked(self._noop, pending)
            ran += pending
            total[pending] += np.asarray(r2)[pending]
            for k in obs:
                obs[k][pending] = np.asarray(o2[k])[pending]
            term[pending] = np.asarray(t2)[pending]
            trunc[pending] = np.asarray(tr2)[pending]
            for k, v in i2.items():
                if k in ("final_observation", "_final_observation", "final_info", "_final_info"):
                    continue
                info[k] = np.array(info[k])
                info[k][pending] = np.asarray(v)[pending]
            if "final_observation" in i2:
                W._merge_final(info, i2, pending)
            more = W.is_skippable(obs) & ~(term | trunc)
            pending = pending & more & (ran < self.cap)
        self.capped = (more & (ran >= self.cap)).astype(np.uint8)
        self.full_obs = obs  # (P1's move_frame included: the actor's features)
        return W.frame_skip_obs(obs), total, term, trunc, W._map_final(info, W.frame_skip_obs)


def replay(exp_env, base_o, res, autoreset, d0=0):
    """Feed the kernel's actions to the wrapper over the oracle; every decision bitwise.  Returns the
    oracle's tick counts [n][N]."""
    ticks = []
    for d in range(len(res["A"])):
        exp = exp_env.step(W.FootsiesActionCombinationsDiscretized.action(res["A"][d]))
        compare_step(exp, wrapped_row(res, d, autoreset), d0 + d)
        assert_same("ticks", base_o.ticks, res["ticks"][d].astype(np.int64), d0 + d)
        if isinstance(exp_env, CappedFrameSkipped):
            assert_same("capped", exp_env.capped, res["capped"][d], d0 + d)
        ticks.append(base_o.ticks.copy())
    return np.stack(ticks)


# -- 1. / 2. lockstep with the reference wrapper over the oracle, and the actor -----------------------
N1, CALLS = 1057, (40, 25)  # 2 N lanes leave the last wave part-filled, the pair count is odd
LOCKSTEP = {
    "bot-same_step-strict-dense": dict(p2="bot", autoreset="same_step", float_mode="strict", dense=True),
    "noop-next_step-double-dense": dict(p2="noop", autoreset="next_step", float_mode="double", dense=True),
    "bot-next_step-strict-sparse": dict(p2="bot", autoreset="next_step", float_mode="strict", dense=False),
}


@functools.lru_cache(maxsize=None)
def lockstep_runs(name):
    """The two consecutive calls of one configuration, computed once for the replay and the actor test:
    (results per call, outputs before the first decision, actor parameters, final state, steps_taken)."""
    sim, ro = make(N1, **LOCKSTEP[name])
    sim.reset()
    prev0 = sim.outputs_numpy()
    runs, steps = [], []
    for n in CALLS:
        runs.append(run(sim, ro, n))
        steps.append(sim.steps_taken)
    state = sim.get_state()
    params = [p.cpu().numpy() for p in ro.params]
    sim.close()
    return runs, prev0, params, state, steps


@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_decisions_in_lockstep_with_the_reference_wrapper(oracle_lib, name):
    cfg = LOCKSTEP[name]
    runs, prev0, _, state, steps = lockstep_runs(name)
    assert steps == [CALLS[0], CALLS[0] + CALLS[1]]  # fs_steps_taken counts decisions
    base_o = OracleEnv(N1, oracle_lib, seed=21, **cfg)
    exp_env = W.FootsiesFrameSkipped(base_o)
    eo, _ = exp_env.reset()
    for k in ("guard", "move", "position"):
        assert_same("reset." + k, eo[k], prev0[k].astype(eo[k].dtype))
    ticks, d0 = [], 0
    for res in runs:
        ticks.append(replay(exp_env, base_o, res, cfg["autoreset"], d0))
        d0 += len(res["A"])
    compare_states(base_o.ora.state(), state)
    base_o.ora.close()
    ticks = np.concatenate(ticks)
    term = np.concatenate([r["terminated"] for r in runs]).astype(bool)
    capped = np.concatenate([r["capped"] for r in runs])
    # the run reached the ground the kernel is about (else: another seed, not a looser condition)
    assert ticks.max() < CAP and not capped.any(), ticks.max()  # no decision capped: the reference wrapper's results
    assert ticks.max() >= 10, ticks.max()
    if cfg["p2"] == "bot":
        assert (term & (ticks > 1)).any()  # an episode ended inside a skip
    else:
        # Against an idle P2 no seed gives that: only P1's special ends a round there, it comes out of a
        # normal that hit, and P2 is then in DAMAGE -- not skippable -- until the special lands, so every
        # round ends on the first tick of a decision (the oracle alone, 60 actor seeds at this shape: 0
        # of 4 593 endings inside a skip).  Held to what can happen: rounds end, and the decision after
        # one is the next-step reset burst alone (one tick, reward 0, its action ignored).
        assert term.any()
        after = term[:-1]  # (also across the two calls: the pending reset is arena state)
        rew = np.concatenate([r["reward"] for r in runs])
        assert (ticks[1:][after] == 1).all() and (rew[1:][after] == 0.0).all()
    full = ticks[:, :N1 // WAVE * WAVE].reshape(len(ticks), -1, WAVE)
    assert (full.max(axis=2) != full.min(axis=2)).any()  # arenas of one wave left the loop at different ticks


@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_actor_samples_per_decision(name):
    runs, prev0, params, _, _ = lockstep_runs(name)
    t0, seen = 0, set()
    for res in runs:
        n = len(res["A"])
        prev = [prev0] + [row(res, d) for d in range(n - 1)]  # the outputs before each decision
        _check_policy(params, POL_SEED, prev, res["A"], res["LP"], t0, N1)
        prev0 = row(res, n - 1)
        t0 += n
        seen |= set(np.unique(res["A"]).tolist())
    assert seen == set(range(8))


# -- 3. the cap ---------------------------------------------------------------------------------------------
def test_cap_closes_decisions(oracle_lib):
    n, decisions, cap = 257, 30, 4
    sim, ro = make(n)
    sim.reset()
    res = run(sim, ro, decisions, max_ticks=cap)
    base_o = OracleEnv(n, oracle_lib, seed=21)
    exp_env = CappedFrameSkipped(base_o, cap)
    exp_env.reset()
    ticks = replay(exp_env, base_o, res, "same_step")
    compare_states(base_o.ora.state(), sim.get_state())
    assert sim.steps_taken == decisions
    assert res["capped"].any() and ticks.max() == cap and (res["capped"] == 0).any()
    assert (ticks[res["capped"] == 1] == cap).all()
    base_o.ora.close()
    sim.close()


# -- 4. splitting -------------------------------------------------------------------------------------------
def test_split_calls_and_split_launches_give_one_call(monkeypatch):
    n, total = 300, 24
    keys = tuple(_abi.OUTPUT_SPEC) + ("A", "LP", "ticks", "capped")
    sim, ro = make(n)
    whole = run(sim, ro, total)
    state = sim.get_state()
    sim.close()
    # two calls | one call whose launches the host cuts after every 5 decisions (the 32-bit row limit's path)
    for parts, rows in (((7, 17), None), ((total,), 5 * n)):
        if rows:
            monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(rows))
        sim, ro = make(n)
        got = [run(sim, ro, m) for m in parts]
        monkeypatch.delenv("FOOTSIES_MAX_LAUNCH_ROWS", raising=False)
        for k in keys:
            assert_same(k, whole[k], np.concatenate([g[k] for g in got]), extra=str(parts))
        assert sim.steps_taken == total
        compare_states(state, sim.get_state())
        sim.close()
    assert whole["ticks"].max() > 1


# -- 5. general geometry --------------------------------------------------------------------------------
def test_loaded_airborne_and_flipped_fighters(oracle_lib):
    n, decisions = 130, 30
    state = random_states(n, np.random.default_rng(3), p2="bot", geom_frac=0.3)
    sim, ro = make(n, seed=4)
    sim.set_state(state)
    base_o = OracleEnv(n, oracle_lib, seed=4)
    base_o.ora.set_state(state)
    res = run(sim, ro, decisions)
    replay(CappedFrameSkipped(base_o, CAP), base_o, res, "same_step")  # (loaded states may outlast the cap)
    compare_states(base_o.ora.state(), sim.get_state())
    base_o.ora.close()
    sim.close()


# -- 6. refusals ------------------------------------------------------------------------------------------
def test_refusals_and_the_regular_outputs():
    import ctypes as C
    import torch
    from footsies_gym_amd._lib import FootsiesError, lib
    from footsies_gym_amd.rollout import FusedPolicyRollout, make_actor
    from footsies_gym_amd.simulator import FootsiesSim
    L = lib()
    actor = make_actor(device=torch.device("cuda", 0), seed=ACTOR_SEED)

    def call(sim, n=2, cap=CAP, drop=None):
        w = FusedPolicyRollout(sim, actor).params
        ptr = {k: t.data_ptr() for k, t in zip(("w1", "b1", "w2", "b2", "w3", "b3"), w)}
        if drop:
            ptr[drop] = None
        pol = _abi.fs_policy(seed=1, actions_out=None, logp_out=None, **ptr)
        rc = L.fs_step_skip_policy(sim.handle, n, C.byref(pol), cap, None, None)
        return rc, (L.fs_last_error(sim.handle) or b"").decode()

    ext = FootsiesSim(8, p2_mode="external")
    assert call(ext)[0] == _abi.FS_E_UNSUPPORTED and call(ext)[1]
    ext.set_p2_mode("bot")
    assert call(ext)[0] == _abi.FS_E_UNSUPPORTED
    assert L.fs_step_kernel(ext.handle, 2, _abi.FS_KERNEL_SKIP_POLICY) is None
    ext.close()
    for kw in ({"p1_mode": "bot"}, {"frame_delay": 2}):  # (p1_mode="bot": what a by_example environment creates)
        sim = FootsiesSim(8, p2_mode="bot", **kw)
        rc, msg = call(sim)
        assert rc == _abi.FS_E_UNSUPPORTED and msg, kw
        with pytest.raises(FootsiesError):
            FusedPolicyRollout(sim, actor).rollout_skipped(2)
        sim.close()
    from footsies_gym_amd.vector_env import FootsiesVectorEnv
    env = FootsiesVectorEnv(8, by_example=True)
    assert call(env.sim)[0] == _abi.FS_E_UNSUPPORTED
    env.close()
    sim = FootsiesSim(8, p2_mode="bot")
    assert call(sim, n=0)[0] == _abi.FS_E_INVALID
    assert call(sim, cap=0)[0] == _abi.FS_E_INVALID
    assert call(sim, cap=_abi.FS_SKIP_POLICY_MAX_TICKS + 1)[0] == _abi.FS_E_INVALID
    assert call(sim, drop="w2")[0] == _abi.FS_E_INVALID
    assert L.fs_step_skip_policy(sim.handle, 2, None, CAP, None, None) == _abi.FS_E_INVALID
    assert sim.steps_taken == 0
    assert L.fs_step_kernel(sim.handle, 2, _abi.FS_KERNEL_SKIP_POLICY).decode() == "fsk::k_step_skip_policy<0, 1>"
    sim.close()
    # trajectory=None: the last decision stays in the regular outputs
    a, ra = make(300)
    b, rb = make(300)
    want = run(a, ra, 12)
    acts, logps, ticks = rb.rollout_skipped(12, capped=False)
    got = b.outputs_numpy()
    for k in OBS_KEYS:
        assert_same(k, want[k][11], got[k])
    term = want["terminated"][11].astype(bool)
    for k in FINAL_KEYS:
        assert_same(k, want[k][11][term], got[k][term])
    assert_same("actions", want["A"], acts.cpu().numpy())
    assert_same("ticks", want["ticks"], ticks.cpu().numpy())
    compare_states(a.get_state(), b.get_state())
    a.close()
    b.close()


# -- 7. PPO ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", ["hip", "torch"])
def test_ppo_trains_on_decisions(learner):
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.rollout import FusedPolicyRollout
    from footsies_gym_amd.simulator import FootsiesSim
    n, horizon = 2048, 32
    sim = FootsiesSim(n, p2_mode="bot", seed=5)
    tr = PPOTrainer(sim, horizon=horizon, epochs=2, minibatches=4, lr=1e-2, seed=3, learner=learner, frame_skip=True)
    # the first rollout against the launch called directly on a twin handle with the same actor and seed
    twin = FootsiesSim(n, p2_mode="bot", seed=5)
    traj = twin.alloc_trajectory(horizon)
    acts, logps, ticks = FusedPolicyRollout(twin, tr.actor, seed=3).rollout_skipped(horizon, trajectory=traj)
    feats, actions, rewards, dones = tr.collect()
    assert torch.equal(actions, acts) and torch.equal(tr.logp, logps) and torch.equal(tr.ticks, ticks)
    assert torch.equal(rewards, traj["reward"]) and torch.equal(dones, traj["terminated"])  # the per-decision sums
    assert int(ticks.max()) > 1 and bool((rewards != 0).any())
    last = feats[horizon].clone()
    tr.update(feats, actions, rewards, dones)
    twin.close()
    for it in range(3):
        if it:
            feats, actions, rewards, dones = tr.collect()
            if it == 1:
                assert torch.equal(feats[0], last)  # the hand-over: the last row is the next first features
            tr.update(feats, actions, rewards, dones)
        for k, v in tr.stats.items():
            assert bool(torch.isfinite(v.float())), (it, k)
        for a, b in zip(tr.rollout.params, tr.actor.parameters()):
            assert torch.equal(a, b.detach()), it
        assert float(tr.stats["ticks_per_decision"]) > 1.0
        assert int(tr.stats["capped"]) == int(tr.capped.sum())
    assert sim.steps_taken == 3 * horizon
    sim.close()


def test_ppo_without_frame_skip_is_the_per_tick_rollout():
    import torch
    from footsies_gym_amd.ppo import PPOTrainer
    from footsies_gym_amd.rollout import FusedPolicyRollout
    from footsies_gym_amd.simulator import FootsiesSim
    n, horizon = 2048, 32
    sim, twin = (FootsiesSim(n, p2_mode="bot", seed=5) for _ in range(2))
    tr = PPOTrainer(sim, horizon=horizon, seed=3)
    assert tr.frame_skip is False and "ticks_per_decision" not in tr.stats
    traj = twin.alloc_trajectory(horizon)
    acts, logps = FusedPolicyRollout(twin, tr.actor, seed=3).rollout(horizon, trajectory=traj)
    feats, actions, rewards, dones = tr.collect()
    assert torch.equal(actions, acts) and torch.equal(tr.logp, logps)
    assert torch.equal(rewards, traj["reward"]) and torch.equal(dones, traj["terminated"])
    tr.update(feats, actions, rewards, dones)
    assert "ticks_per_decision" not in tr.stats and "capped" not in tr.stats
    sim.close()
    twin.close()
