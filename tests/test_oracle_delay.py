"""The CPU oracle's delayed-frame deque against FootsiesEnv's rule written out in numpy
(tests/delay_model.py), at the delays where the GPU frame-delay tests lean on it: a
frame_delay = d oracle and a frame_delay = 0 twin driven with the same calls."""
import numpy as np
import pytest

from footsies_gym_amd import _abi
from tests.delay_model import AR, DelayRule, check_rule, hashed

N, BASE_SEED, ACTION_SEED = 33, 11, 0xD1A


def drive(oracle_lib, d, autoreset, calls, p2_mode=_abi.FS_P2_EXTERNAL):
    """Make `calls` on both oracles -- ("step", p1, p2, active) or ("reset", mask, flags, seeds) --
    and hold the delayed one to the rule after each."""
    kw = dict(p2_mode=p2_mode, base_seed=BASE_SEED, autoreset_mode=AR[autoreset])
    dly = oracle_lib.Oracle(N, frame_delay=d, **kw)
    twin = oracle_lib.Oracle(N, frame_delay=0, **kw)
    same = autoreset == "same_step"
    rule = DelayRule(d, same, twin.outputs(), len(calls))
    check_rule(dly.outputs(), rule.expected(), -1, same)
    for e, c in enumerate(calls):
        if c[0] == "step":
            _, p1, p2, active = c
            got = dly.step(p1, p2, active=active)
            rule.feed_step(twin.step(p1, p2, active=active), active)
        else:
            _, mask, flags, seeds = c
            got = dly.reset(seeds=seeds, mask=mask, flags=flags)
            rule.feed_reset(twin.reset(seeds=seeds, mask=mask, flags=flags), mask, flags == _abi.FS_RESET_SEED_ONLY)
        check_rule(got, rule.expected(), e, same)
    dly.close()
    twin.close()
    return rule


def _conditions(rule, d, same):
    assert rule.late_terminals >= 1, "no terminal at a step >= d"
    assert rule.real_rows >= N, "too few rows with a real delayed frame"
    if same:
        assert rule.real_finals >= 1, "no terminal whose final_frame is a real frame"


@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
@pytest.mark.parametrize("d", [1, 16, 256, 257])
def test_oracle_deque_follows_the_rule(oracle_lib, d, autoreset):
    """Unmasked steps, T = 2 d + 300, with one masked hard reset in mid-run."""
    T = 2 * d + 300
    p1, p2 = hashed(ACTION_SEED, N, T)
    calls = [("step", p1[t], p2[t], None) for t in range(T)]
    calls.insert(d + 150, ("reset", (np.arange(N) % 3 == 1).astype(np.uint8), _abi.FS_RESET_HARD, None))
    rule = drive(oracle_lib, d, autoreset, calls)
    _conditions(rule, d, autoreset == "same_step")


@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
@pytest.mark.parametrize("d", [1, 16, 256, 257])
def test_oracle_deque_follows_the_rule_under_masked_steps(oracle_lib, d, autoreset):
    """Masked steps (each arena's deque moves with its own steps only) against the in-game bot,
    with a seeded FS_RESET_IF_NEEDED of a third of the arenas and a masked SEED-only call."""
    T = (2 * d + 300) * 2
    p1, _ = hashed(ACTION_SEED, N, T)
    rng = np.random.default_rng(5)
    calls = [("step", p1[t], None, (rng.random(N) < (0.3 if t % 2 else 0.9)).astype(np.uint8)) for t in range(T)]
    seeds = np.arange(N, dtype=np.uint64) + np.uint64(900)
    calls.insert(T // 2, ("reset", (np.arange(N) % 3 == 2).astype(np.uint8), _abi.FS_RESET_IF_NEEDED, seeds))
    calls.insert(T // 3, ("reset", (np.arange(N) % 2 == 0).astype(np.uint8), _abi.FS_RESET_SEED_ONLY, seeds))
    rule = drive(oracle_lib, d, autoreset, calls, p2_mode=_abi.FS_P2_BOT)
    _conditions(rule, d, autoreset == "same_step")
    active = np.array([c[3] for c in calls if c[0] == "step"], bool)
    assert not active.all(axis=0).any() and (active.sum(axis=0) >= d + 1).all()


@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
def test_oracle_deque_at_the_largest_delay(oracle_lib, autoreset):
    """frame_delay = 4096: random play ends every episode long before 4096 steps and each terminal
    refills the deque, so the opening (4096 + 200 steps) presses no attack -- no hit, no terminal --
    and 1 200 steps of the full stream follow; one masked hard reset 600 steps into them."""
    d, quiet, T = 4096, 4296, 4296 + 1200
    p1, p2 = hashed(ACTION_SEED, N, T, quiet=quiet)
    calls = [("step", p1[t], p2[t], None) for t in range(T)]
    rule = drive(oracle_lib, d, autoreset, calls)
    _conditions(rule, d, autoreset == "same_step")
    assert rule.first_terminal >= quiet  # the opening ends no episode
    # (what this input gives: the GPU test of the same run relies on it)
    assert rule.late_terminals == {"same_step": 103, "next_step": 99}[autoreset]
    assert rule.real_rows >= 15000 and rule.max_frame == 1399
    calls.insert(quiet + 600, ("reset", (np.arange(N) % 3 == 0).astype(np.uint8), _abi.FS_RESET_HARD, None))
    drive(oracle_lib, d, autoreset, calls)


@pytest.mark.parametrize("autoreset", ["same_step", "next_step"])
def test_oracle_deque_at_the_largest_delay_under_masked_steps(oracle_lib, autoreset):
    """frame_delay = 4096 with masked steps: the quiet opening lasts until every arena has taken more
    than 4096 steps of its own, then 1 400 calls of the full stream."""
    d, quiet, T = 4096, 5000, 6400
    p1, p2 = hashed(ACTION_SEED, N, T, quiet=quiet)
    rng = np.random.default_rng(5)
    active = np.stack([rng.random(N) < (0.8 if t % 2 else 0.95) for t in range(T)])
    assert not active.all(axis=0).any() and (active[:quiet].sum(axis=0) >= d + 1).all()
    rule = drive(oracle_lib, d, autoreset, [("step", p1[t], p2[t], active[t].astype(np.uint8)) for t in range(T)])
    _conditions(rule, d, autoreset == "same_step")
    assert rule.first_terminal >= quiet
