"""The host references of the GPU tests at values past 2^31, 2^32 and 2^40 (tests/test_gpu_wide_counters.py holds
the kernels to them there): a reference that wrapped, saturated or raised at such a counter, arena index or seed
would make those tests meaningless, so each is held here to a few lines of Python integers, `& M64` after every
operation and nothing else.  Where a kernel could go wrong by dropping the high half of a counter or an arena
index, the same call with that argument reduced mod 2^32 is shown to draw differently somewhere: the GPU tests
would see it."""
import numpy as np
import pytest

from footsies_gym_amd import _abi
from footsies_gym_amd import rollout
from tests import policy_ref
from tests import sampler_ref as S
from tests.parity_utils import compare_outputs, compare_states

M64 = 2**64 - 1
M32 = 2**32 - 1
C1, C2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03
SEED = 0x5A3D1E5

ARENAS = [2**32 + 45 + i for i in range(8)] + [2**63 + i for i in range(8)]
COUNTERS = sorted({2**31 + k for k in range(-3, 4)} | {2**32 + k for k in range(-3, 4)} | {2**40 - 1})
P2_COUNTERS = [(2**40 - 1) + (j << 40) for j in range(4096)]  # the last decision's, every tick a decision can have


def mix64(x):
    """splitmix64 on a Python integer."""
    x = (x + C1) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def uniform_bits(seed, env, t):
    """The 24 bits of policy_uniform (fs_policy.h): the draw is bits / 2^24."""
    return mix64((seed & M64) ^ ((env * C1) & M64) ^ ((t * C2) & M64)) >> 40


def draw(live, seed, env, t):
    """exact_draw on Python numbers: target = u * K rounded to float32 once, the action live[floor(target)]."""
    live = sorted(live)
    target = np.float32(uniform_bits(seed, env, t) * len(live) / 2.0**24)  # (the quotient is exact in a double)
    return live[int(np.floor(target))]


# -- policy_uniform, exact_draw ---------------------------------------------------------------------------------
@pytest.mark.parametrize("counters", [COUNTERS, P2_COUNTERS], ids=["ticks", "p2-decision-ticks"])
def test_policy_uniform_and_exact_draw_at_wide_arenas_and_counters(counters):
    arena = np.array(ARENAS, dtype=np.uint64)
    ctr = np.array(counters, dtype=np.uint64)[:, None]
    u = policy_ref.policy_uniform(SEED, arena, ctr)
    assert u.shape == (len(counters), len(ARENAS)) and u.dtype == np.float32
    exp = np.array([[uniform_bits(SEED, a, c) for a in ARENAS] for c in counters], dtype=np.int64)
    assert np.array_equal(u.astype(np.float64) * 2.0**24, exp.astype(np.float64))  # (24 bits: exact either way)
    assert len(np.unique(exp)) > 0.99 * exp.size  # distinct (arena, counter) pairs draw apart
    for live in ((0, 1, 2, 3, 4, 5, 6, 7), (1, 2, 5), (0, 2, 4, 5, 6), (3,)):
        act, ref, target = S.exact_draw(live, SEED, arena, ctr)
        assert act.shape == u.shape and ref == -np.log(float(len(live)))
        e = np.array([[draw(live, SEED, a, c) for a in ARENAS] for c in counters], dtype=np.uint8)
        assert np.array_equal(act, e), live
    # a kernel that kept the low 32 bits of the counter, or of the arena index, would draw differently
    live = tuple(range(8))
    act = S.exact_draw(live, SEED, arena, ctr)[0]
    high = (ctr >> np.uint64(32)) != 0
    low_ctr = S.exact_draw(live, SEED, arena, ctr & np.uint64(M32))[0]
    low_arena = S.exact_draw(live, SEED, arena & np.uint64(M32), ctr)[0]
    assert (act != low_ctr)[np.broadcast_to(high, act.shape)].any() and high.any()
    assert np.array_equal(act[~high[:, 0]], low_ctr[~high[:, 0]])
    assert (act != low_arena).any()
    if counters is P2_COUNTERS:  # and one that dropped the tick of P2's counter, (j << 40), likewise
        flat = S.exact_draw(live, SEED, arena, ctr & np.uint64(2**40 - 1))[0]
        assert (act[1:] != flat[1:]).any() and np.array_equal(act[0], flat[0])


# -- the synthetic action stream --------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [0, 5, 2**31, 2**32 + 3, 2**40 + 3, 2**62])
@pytest.mark.parametrize("env0", [0, 2**32 + 45, 2**63 + 128])
def test_hash_actions_equals_or_hash_action(oracle_lib, t, env0):
    n, seed = 70, 0x5EED
    L = oracle_lib.lib()
    for player in (0, 1):
        got = oracle_lib.hash_actions(seed, n, t, player, env0=env0)
        assert got.dtype == np.uint8 and got.shape == (n,)
        exp = [L.or_hash_action(seed, (env0 + i) & M64, t, player) for i in range(n)]
        big = [mix64(seed ^ (((env0 + i) * C1) & M64) ^ (((t << 1) | player) & M64)) & 7 for i in range(n)]
        assert got.tolist() == exp == big, (t, env0, player)
    if env0 == 0:  # the default is arena_base 0, what every earlier caller passes
        assert np.array_equal(oracle_lib.hash_actions(seed, n, t, 1), oracle_lib.hash_actions(seed, n, t, 1, env0=0))
    if t >> 31:  # a 32-bit t (or t << 1) would be seen
        assert not np.array_equal(oracle_lib.hash_actions(seed, n, t, 0, env0=env0),
                                  oracle_lib.hash_actions(seed, n, t & (M32 >> 1), 0, env0=env0))
    if env0 >> 32:
        assert not np.array_equal(oracle_lib.hash_actions(seed, n, t, 0, env0=env0),
                                  oracle_lib.hash_actions(seed, n, t, 0, env0=env0 & M32))


# -- the league's host draws -----------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [0, 1, 3, 2**24])
def test_pool_assignment_and_bot_groups_at_wide_groups_and_iterations(k):
    first, groups, iteration, seed = (2**32 + 128 * k) // 128, 64, 2**32 + 1, 0xABCDEF
    filled, newest, latest, fraction = 5, 3, 0.5, 0.25
    slots = rollout.pool_assignment(seed, iteration, first, groups, filled, newest, latest)
    bots = rollout.bot_groups(seed, first, groups, fraction)
    exp_slots, exp_bots = [], []
    for g in range(first, first + groups):
        key = seed ^ ((g * C1) & M64)
        v = [mix64(key ^ (((iteration + (j << 40)) * C2) & M64)) >> 40 for j in (0, 1)]
        exp_slots.append(newest if v[0] < int(round(latest * 2**24)) else (v[1] * filled) >> 24)
        exp_bots.append((mix64(key ^ ((0xB07 * C2) & M64)) >> 40) < int(round(fraction * 2**24)))
    assert slots.dtype == np.uint8 and slots.tolist() == exp_slots
    assert bots.dtype == np.bool_ and bots.tolist() == exp_bots
    assert len(set(exp_slots)) == filled and 0 < sum(exp_bots) < groups
    # the low 32 bits of the iteration, or a group taken from the low 32 bits of the arena index, draw something else
    low = ((2**32 + 128 * k) & M32) // 128
    assert slots.tolist() != rollout.pool_assignment(seed, iteration & M32, first, groups, filled, newest, latest).tolist()
    assert slots.tolist() != rollout.pool_assignment(seed, iteration, low, groups, filled, newest, latest).tolist()
    assert bots.tolist() != rollout.bot_groups(seed, low, groups, fraction).tolist()


# -- seeds: Random.InitState((int32)seed), include/footsies.h ----------------------------------------------------
WIDE_SEEDS = [2**31, 2**32 - 1, 2**32, 2**32 + 5, 2**63, 2**64 - 1, 5, 0]
BOT_TICKS = 60


def _bot_run(ora, ticks=BOT_TICKS):
    """`ticks` ticks of P1 idle against the in-game bot (which consumes the arena's RNG): every tick's outputs."""
    zero = np.zeros(ora.n, np.uint8)
    return [ora.step(zero) for _ in range(ticks)]


def test_oracle_folds_base_seed_plus_arena_index_to_32_bits(oracle_lib):
    seed, base, n = 2**31 + 7, 2**33 + 64, 8
    wide = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_BOT, base_seed=seed, arena_base=base)
    st = wide.state()
    rows = _bot_run(wide)
    for i in range(n):
        low = oracle_lib.Oracle(n, p2_mode=_abi.FS_P2_BOT, base_seed=(seed + base + i) % 2**32)
        compare_states(low.state()[:1], st[i:i + 1])
        for t, r in enumerate(_bot_run(low)):
            compare_outputs({k: v[:1] for k, v in r.items()}, {k: v[i:i + 1] for k, v in rows[t].items()}, step=t)
        compare_states(low.state()[:1], wide.state()[i:i + 1])
        low.close()
    assert len({tuple(r) for r in st["rng"].tolist()}) == n  # eight streams, not one
    wide.close()


def test_oracle_reset_takes_the_low_32_bits_of_a_seed(oracle_lib):
    a = oracle_lib.Oracle(8, p2_mode=_abi.FS_P2_BOT, base_seed=3)
    b = oracle_lib.Oracle(8, p2_mode=_abi.FS_P2_BOT, base_seed=3)
    compare_outputs(a.reset(seeds=WIDE_SEEDS), b.reset(seeds=[s % 2**32 for s in WIDE_SEEDS]))
    compare_states(a.state(), b.state())
    rng = a.state()["rng"]
    # 2^32 and 2^63 are 0, 2^32 + 5 is 5, 2^64 - 1 is 2^32 - 1: four streams in all
    assert np.array_equal(rng[2], rng[7]) and np.array_equal(rng[4], rng[7]) and np.array_equal(rng[3], rng[6])
    assert np.array_equal(rng[5], rng[1]) and len({tuple(r) for r in rng.tolist()}) == 4
    for t, (x, y) in enumerate(zip(_bot_run(a), _bot_run(b))):
        compare_outputs(x, y, step=t)
    compare_states(a.state(), b.state())
    assert not np.array_equal(a.state()["rng"], rng)  # the bot drew
    a.close()
    b.close()
