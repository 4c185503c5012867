"""The delayed-frame queue (fs_delay.hip, frame_delay > 0) where the rest of the suite does not run
it: delays on either side of 256 and at FS_MAX_FRAME_DELAY, launch seams of fused calls, masked
resets and masked steps with a queue, and the surfaces over it -- bit for bit against the CPU
oracle's FE deque (itself held to FE's rule at these delays by tests/test_oracle_delay.py).

Every case asserts, from the oracle's own outputs, that it cannot pass vacuously: real frames come
out of the queue, and episodes end after the queue has filled."""
import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.delay_model import AR, hashed
from tests.parity_utils import FINAL_KEYS, OBS_KEYS, assert_same, compare_outputs, compare_states

pytestmark = pytest.mark.gpu

MODES = ["same_step", "next_step"]
BASE_SEED, ACTION_SEED = 11, 0xD1A


def _sim(n, d, autoreset, p2="external", **kw):
    from footsies_gym_amd.simulator import FootsiesSim
    return FootsiesSim(n, p2_mode=p2, seed=BASE_SEED, frame_delay=d, autoreset_mode=autoreset, **kw)


def _oracle(oracle_lib, n, d, autoreset, p2=_abi.FS_P2_EXTERNAL):
    return oracle_lib.Oracle(n, p2_mode=p2, base_seed=BASE_SEED, frame_delay=d, autoreset_mode=AR[autoreset])


def _device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _oracle_rows(ora, p1, p2):
    """The oracle's outputs after each step of the action rows, stacked [T][N]."""
    rows = [ora.step(p1[t], p2[t]) for t in range(len(p1))]
    return {k: np.stack([r[k] for r in rows]) for k in rows[0]}


def _compare_rows(exp, got, same_step, t0=0, t1=None):
    """Rows t0 .. t1 of stacked oracle outputs against `got` (rows 0 .. t1 - t0), as compare_outputs
    does for one step."""
    sl = slice(t0, t1)
    for k in OBS_KEYS:
        assert_same(k, exp[k][sl], got[k], extra="(row index + %d = step)" % t0)
    if same_step:
        term = exp["terminated"][sl].astype(bool)
        for k in FINAL_KEYS:
            assert_same(k, exp[k][sl][term], np.asarray(got[k])[term], extra="(terminal rows from step %d)" % t0)


def _host(traj):
    import torch
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in traj.items()}


def _not_vacuous(exp, d, n, same_step):
    """Cases 1-3, from the oracle's rows: an episode ends after the queue filled, real frames come out
    of it, and (same-step) some terminal's final_* is a real frame."""
    term = exp["terminated"].astype(bool)
    assert term[d:].any(), "no terminal at a step >= d"
    assert int((exp["frame"] >= 0).sum()) >= n, "too few rows with a real delayed frame"
    if same_step:
        assert (exp["final_frame"][term] >= 0).any(), "no terminal whose final_frame is a real frame"


# -- 1. delays on either side of one byte, step by step ----------------------------------------------

@pytest.mark.parametrize("autoreset", MODES)
@pytest.mark.parametrize("d", [255, 256, 257])
def test_single_steps_across_256(oracle_lib, d, autoreset):
    """fs_step at frame_delay 255 / 256 / 257 over 257 arenas (one arena in a second k_delay block,
    a part-filled wave in the step kernel) for 2 d + 300 calls, then a hard reset whose next d + 3
    observations repeat state(-1)."""
    N, T = 257, 2 * d + 300
    same = autoreset == "same_step"
    sim, ora = _sim(N, d, autoreset), _oracle(oracle_lib, N, d, autoreset)
    p1, p2 = hashed(ACTION_SEED, N, T)
    exp = _oracle_rows(ora, p1, p2)
    _not_vacuous(exp, d, N, same)
    q1, q2 = _device(p1), _device(p2)
    for t in range(T):
        sim.step(q1[t], q2[t])
        compare_outputs({k: v[t] for k, v in exp.items()}, sim.outputs_numpy(), step=t, same_step=same)
    compare_states(ora.state(), sim.get_state())
    sim.reset(hard=True)
    first = ora.reset(flags=_abi.FS_RESET_HARD)
    compare_outputs(first, sim.outputs_numpy(), step=T, same_step=same)
    assert (first["frame"] == -1).all()
    for t in range(d + 3):
        sim.step(q1[t], q2[t])
        e = ora.step(p1[t], p2[t])
        compare_outputs(e, sim.outputs_numpy(), step=T + 1 + t, same_step=same)
        if t < d:
            assert (e["frame"] == -1).all()
    sim.close()


# -- 2. the same delays across launch seams ----------------------------------------------------------

@pytest.mark.parametrize("autoreset", MODES)
@pytest.mark.parametrize("d,split", [(257, 256), (300, 270)])
def test_fused_calls_across_launch_seams(oracle_lib, monkeypatch, d, split, autoreset):
    """The same actions through (a) two consecutive trajectory calls, the first ending with the ring
    head at slot `split` >= 256, (b) fs_step_n without a trajectory (tick by tick) and (c) one
    trajectory call split into launches of 100 ticks: every row, the last outputs and the state."""
    N, T = 33, 2 * d + 300
    same = autoreset == "same_step"
    assert 256 <= split % d
    ora = _oracle(oracle_lib, N, d, autoreset)
    p1, p2 = hashed(ACTION_SEED, N, T)
    exp = _oracle_rows(ora, p1, p2)
    _not_vacuous(exp, d, N, same)
    q1, q2 = _device(p1), _device(p2)
    last = {k: v[T - 1] for k, v in exp.items()}
    a, b, c = (_sim(N, d, autoreset) for _ in range(3))
    t1, t2 = a.alloc_trajectory(split), a.alloc_trajectory(T - split)
    a.step_n(split, q1[:split], q2[:split], trajectory=t1)
    a.step_n(T - split, q1[split:], q2[split:], trajectory=t2)
    _compare_rows(exp, _host(t1), same, 0, split)
    _compare_rows(exp, _host(t2), same, split, T)
    b.step_n(T, q1, q2)
    compare_outputs(last, b.outputs_numpy(), step=T - 1, same_step=same)
    monkeypatch.setenv("FOOTSIES_MAX_LAUNCH_ROWS", str(100 * N))
    t3 = c.alloc_trajectory(T)
    c.step_n(T, q1, q2, trajectory=t3)
    monkeypatch.delenv("FOOTSIES_MAX_LAUNCH_ROWS")
    _compare_rows(exp, _host(t3), same)
    for s in (a, b, c):
        compare_states(ora.state(), s.get_state())
        s.close()


# -- 3. the largest delay ----------------------------------------------------------------------------

@pytest.mark.parametrize("autoreset", MODES)
def test_largest_delay(oracle_lib, autoreset):
    """frame_delay = FS_MAX_FRAME_DELAY.  Random play ends every episode long before 4096 steps and
    each terminal refills the queue, so the opening (4096 + 200 steps) presses no attack -- no
    terminal -- and 1 200 steps of the full stream follow: trajectory calls of 2 000, 2 296 and 1 200
    ticks on one handle; on a second the first and the last 300 steps one at a time."""
    N, d = 33, _abi.FS_MAX_FRAME_DELAY
    quiet, T = d + 200, d + 200 + 1200
    same = autoreset == "same_step"
    ora = _oracle(oracle_lib, N, d, autoreset)
    p1, p2 = hashed(ACTION_SEED, N, T, quiet=quiet)
    exp = _oracle_rows(ora, p1, p2)
    _not_vacuous(exp, d, N, same)
    assert not exp["terminated"][:quiet].any()
    assert int(exp["terminated"][quiet:].sum()) == (103 if same else 99) and int(exp["frame"].max()) == 1399
    q1, q2 = _device(p1), _device(p2)
    a, b = _sim(N, d, autoreset), _sim(N, d, autoreset)
    t0 = 0
    for n in (2000, 2296, 1200):
        traj = a.alloc_trajectory(n)
        a.step_n(n, q1[t0:t0 + n], q2[t0:t0 + n], trajectory=traj)
        _compare_rows(exp, _host(traj), same, t0, t0 + n)
        t0 += n
    assert t0 == T
    for t in list(range(300)) + [None] + list(range(T - 300, T)):
        if t is None:  # the steps between them in one call
            traj = b.alloc_trajectory(T - 600)
            b.step_n(T - 600, q1[300:T - 300], q2[300:T - 300], trajectory=traj)
            _compare_rows(exp, _host(traj), same, 300, T - 300)
            continue
        b.step(q1[t], q2[t])
        compare_outputs({k: v[t] for k, v in exp.items()}, b.outputs_numpy(), step=t, same_step=same)
    for s in (a, b):
        compare_states(ora.state(), s.get_state())
        s.close()


# -- 4. masked resets ----------------------------------------------------------------------------------

@pytest.mark.parametrize("autoreset", MODES)
@pytest.mark.parametrize("d,T,every,need", [(40, 1200, 50, 10), (300, 1500, 200, 1)])
def test_masked_resets_leave_other_queues_alone(oracle_lib, d, T, every, need, autoreset):
    """Before every `every`-th step a reset of a third of the arenas (hard and FS_RESET_IF_NEEDED in
    turn, seeded every fourth time), and once a masked SEED-only call: the arenas outside the mask
    are separate FootsiesEnvs that nobody reset, and keep their queued frames.  A frame_delay = 0
    twin oracle tells at how many resets some arena outside the mask had real frames queued behind
    a state(-1) observation (its own frame in [0, d))."""
    N = 33
    same = autoreset == "same_step"
    sim, ora = _sim(N, d, autoreset), _oracle(oracle_lib, N, d, autoreset)
    twin = _oracle(oracle_lib, N, 0, autoreset)
    p1, p2 = hashed(7, N, T)
    q1, q2 = _device(p1), _device(p2)
    arena = np.arange(N)
    exposed_resets = exposed_arenas = 0
    for t in range(T):
        if t == every // 2:  # SEED alone: no queue changes, no output changes
            seeds, m = arena.astype(np.uint64) + np.uint64(5000), (arena % 2 == 0).astype(np.uint8)
            sim.reset(seeds=seeds, mask=m, seed_only=True)
            for o in (ora, twin):
                o.reset(seeds=seeds, mask=m, flags=_abi.FS_RESET_SEED_ONLY)
            compare_outputs(ora.outputs(), sim.outputs_numpy(), step=t, same_step=False)
        if t and t % every == 0:
            j = t // every
            m = (arena % 3 == j % 3).astype(np.uint8)
            seeds = arena.astype(np.uint64) + np.uint64(1000 * j) if j % 4 == 0 else None
            own = twin.outputs()["frame"]
            hit = (m == 0) & (own >= 0) & (own < d)
            exposed_resets += int(hit.any())
            exposed_arenas += int(hit.sum())
            sim.reset(seeds=seeds, mask=m, hard=bool(j % 2))
            flags = _abi.FS_RESET_HARD if j % 2 else _abi.FS_RESET_IF_NEEDED
            twin.reset(seeds=seeds, mask=m, flags=flags)
            compare_outputs(ora.reset(seeds=seeds, mask=m, flags=flags), sim.outputs_numpy(), step=t, same_step=False)
        sim.step(q1[t], q2[t])
        twin.step(p1[t], p2[t])
        compare_outputs(ora.step(p1[t], p2[t]), sim.outputs_numpy(), step=t, same_step=same)
    print("resets with an exposed arena: %d (%d arenas)" % (exposed_resets, exposed_arenas))
    assert exposed_resets >= need
    compare_states(ora.state(), sim.get_state())
    sim.close()


# -- 5. masked steps -----------------------------------------------------------------------------------

@pytest.mark.parametrize("autoreset", MODES)
@pytest.mark.parametrize("p2", ["bot", "external"])
@pytest.mark.parametrize("d,T", [(5, 300), (300, 900)])
def test_masked_steps_move_each_queue_with_its_own_steps(oracle_lib, d, T, p2, autoreset):
    """fs_step_masked with a queue: an idle arena's ring and head stay, an active one's advance."""
    N = 999
    same = autoreset == "same_step"
    sim = _sim(N, d, autoreset, p2=p2)
    ora = _oracle(oracle_lib, N, d, autoreset, p2=_abi.FS_P2_BOT if p2 == "bot" else _abi.FS_P2_EXTERNAL)
    rng = np.random.default_rng(5)
    a1 = rng.integers(0, 8, (T, N)).astype(np.uint8)
    a2 = rng.integers(0, 8, (T, N)).astype(np.uint8)
    active = np.stack([rng.random(N) < (0.3 if t % 2 else 0.9) for t in range(T)])
    assert not active.all(axis=0).any() and (active.sum(axis=0) >= d + 1).all()
    real = 0
    for t in range(T):
        sim.step(a1[t], a2[t] if p2 == "external" else None, active=active[t])
        exp = ora.step(a1[t], a2[t] if p2 == "external" else None, active=active[t].astype(np.uint8))
        real += int((exp["frame"][active[t]] >= 0).sum())
        compare_outputs(exp, sim.outputs_numpy(), step=t, same_step=same)
    assert real >= N
    compare_states(ora.state(), sim.get_state())
    sim.close()


# -- 6. the surfaces over it ---------------------------------------------------------------------------

def _same_value(path, e, g):
    """Two reset / step results of a vector environment: the same structure, dtypes and bytes."""
    if isinstance(e, tuple):
        assert isinstance(g, tuple) and len(e) == len(g), path
        for i, (x, y) in enumerate(zip(e, g)):
            _same_value(path + (i,), x, y)
    elif isinstance(e, dict):
        assert isinstance(g, dict) and sorted(e) == sorted(g), path
        for k in e:
            _same_value(path + (k,), e[k], g[k])
    elif isinstance(e, np.ndarray) and e.dtype == object:
        assert isinstance(g, np.ndarray) and g.dtype == object and e.shape == g.shape, path
        for i, (x, y) in enumerate(zip(e, g)):
            _same_value(path + (i,), x, y)
    elif e is None:
        assert g is None, path
    else:
        e, g = np.asarray(e), np.asarray(g)
        assert e.dtype == g.dtype and e.shape == g.shape and e.tobytes() == g.tobytes(), (path, e, g)


@pytest.mark.parametrize("autoreset", MODES)
def test_vector_env_with_a_long_queue(oracle_lib, autoreset):
    """FootsiesVectorEnv(64, frame_delay=300), numpy in and out (the ring works on the pinned host
    rows), against the oracle double: steps, masked resets, a seeded masked hard reset and a hard
    reset of every arena in mid-episode."""
    from footsies_gym_amd.vector_env import FootsiesVectorEnv
    from tests.oracle_vector_env import OracleVectorEnv
    N, d, T = 64, 300, 1000
    env = FootsiesVectorEnv(N, frame_delay=d, autoreset_mode=autoreset, seed=3)
    ref = OracleVectorEnv(N, oracle_lib, frame_delay=d, autoreset_mode=autoreset, seed=3)
    twin = OracleVectorEnv(N, oracle_lib, frame_delay=0, autoreset_mode=autoreset, seed=3)
    assert env.sim.host_outputs
    _same_value(("reset",), ref.reset(), env.reset())
    twin.reset()
    rng = np.random.default_rng(17)
    arena = np.arange(N)
    resets = {120: dict(options={"mask": arena % 4 == 1}),
              240: dict(seed=77, options={"mask": arena % 2 == 0, "hard": True}),
              400: dict(options={"hard": True}),
              520: dict(options={"mask": arena % 3 == 0}),
              640: dict(seed=list(range(900, 900 + N)), options={"mask": arena % 5 != 0, "hard": True})}
    exposed = real = late = 0
    for t in range(T):
        if t in resets:
            own = twin.ora.outputs()["frame"]
            m = resets[t]["options"].get("mask")
            if m is not None:  # an arena outside the mask with real frames behind a state(-1) observation
                exposed += int(((own >= 0) & (own < d) & ~m).any())
            twin.reset(**resets[t])
            _same_value(("reset", t), ref.reset(**resets[t]), env.reset(**resets[t]))
        a = rng.integers(0, 8, N)
        twin.step(a)
        want = ref.step(a)
        _same_value(("step", t), want, env.step(a))
        real += int((want[4]["frame"] >= 0).sum())
        late += int(want[2].sum()) if t >= 640 + d else 0
    assert exposed >= 1 and real >= N and late >= 1
    env.close()


def test_single_env_with_a_long_queue(oracle_lib):
    """FootsiesEnv(frame_delay=300): one arena, actions in the kernel arguments, outputs in pinned
    host memory, against a one-arena oracle for 900 steps with FE's reset handshake."""
    from footsies_gym_amd.simulator import encode_actions
    from footsies_gym_amd.vector_env import FootsiesEnv
    d, T = 300, 900
    env = FootsiesEnv(frame_delay=d, seed=5)
    ora = oracle_lib.Oracle(1, p2_mode=_abi.FS_P2_BOT, base_seed=5, frame_delay=d,
                            autoreset_mode=_abi.FS_AUTORESET_NEXT_STEP)
    assert env.reset() == FootsiesEnv._py_host(ora.reset())
    rng = np.random.default_rng(23)
    real = late = 0
    for t in range(T):
        action = tuple(bool(v) for v in rng.random(3) < 0.5)
        o, r, term, trunc, i = env.step(action)
        e = ora.step(encode_actions(np.asarray([action])))
        assert (o, i) == FootsiesEnv._py_host(e), t
        assert (r, term, trunc) == (float(e["reward"][0]), bool(e["terminated"][0]), False), t
        real += int(e["frame"][0] >= 0)
        if e["terminated"][0]:
            late += int(t >= d)
            assert env.reset() == FootsiesEnv._py_host(ora.reset()), t
    assert real >= 100 and late >= 1  # (the oracle's first episode of this play lasts 627 steps)
    env.close()


@pytest.mark.parametrize("autoreset", MODES)
def test_step_rec_equals_step_then_pack_with_a_long_queue(oracle_lib, autoreset):
    """fs_step_rec at frame_delay = 300 == fs_step + fs_pack_outputs on a twin handle, byte for byte,
    and both follow the oracle."""
    import torch
    N, d, T = 513, 300, 900
    same = autoreset == "same_step"
    a, b = _sim(N, d, autoreset), _sim(N, d, autoreset)
    ora = _oracle(oracle_lib, N, d, autoreset)
    p1, p2 = hashed(ACTION_SEED, N, T)
    exp = _oracle_rows(ora, p1, p2)
    _not_vacuous(exp, d, N, same)
    q1, q2 = _device(p1), _device(p2)
    for t in range(T):
        b.step(q1[t], q2[t])
        want = b.pack_outputs()
        got = a.step_records(q1[t], q2[t])
        assert bool(torch.equal(got, want)), (t, (got != want).nonzero()[:4].tolist())
        compare_outputs({k: v[t] for k, v in exp.items()}, a.outputs_numpy(), step=t, same_step=same)
    compare_outputs({k: v[T - 1] for k, v in exp.items()}, b.outputs_numpy(), step=T - 1, same_step=same)
    a.close()
    b.close()
