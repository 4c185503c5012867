"""The dash parser as a table (fs_tables.h ParserTable, fs_kernels.hip take_input).

The specialised row loops no longer run update_input's dash parser over the input history: they
carry the automaton state tools/gen_tables.py derives -- (first direction among input[1..8], its
kind, the run of direction frames from there, capped at 9) -- and read dash and next state from one
table entry per (state, direction).  Checked here, without a GPU:

1. gen_tables.py --check runs check_parser_table: every entry against the arithmetic parser on
   histories of its state;
2. state_of commutes with the shift, exhaustively in the bits the parser reads: all 2^16 masks of
   "some direction on input[i]" x the three kinds at the first direction x the four new directions
   (the frames behind the first direction hold backward: their kind is read by nobody).  The 2^32
   raw histories differ from these only in those kinds, which part 3 samples;
3. 10^6 steps of 1000 walkers that carry only the state, as the kernel does, against a restatement
   of update_input's parser written from the C# (loops over the frames, no bit tricks): sparse,
   dense and held streams, both directions held, runs of 7, 8 and 9 frames;
4. the check rejects a table with one corrupted entry.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables as G  # noqa: E402

ALLOW = G.load()["fighter"]["dash_allow_frame"]
W = ALLOW - 1
CTZ = np.array([W] + [(i & -i).bit_length() - 1 for i in range(1, 1 << W)], dtype=np.uint32)


@pytest.fixture(scope="module")
def table():
    return np.array(G.gen_parser(ALLOW), dtype=np.uint32)


def np_state_of(B, F):
    """G.state_of over arrays."""
    E = (B | F) & 0xFFFF
    lo = E & ((1 << W) - 1)
    j = CTZ[lo]
    kind = ((B >> j) & 1) | (((F >> j) & 1) << 1)
    run = np.zeros_like(E)
    cont = np.ones_like(E)
    for r in range(W + 1):
        cont = cont & ((E >> (j + r)) & 1)
        run = run + cont
    s = ((run - 1) * W + j) * 3 + kind
    return np.where(lo == 0, 0, s).astype(np.uint32)


def dash_by_frames(B, F, r0):
    """The dash of a tick (1 forward, 2 backward), frame by frame as Fighter.cs:569-635 reads the
    history: input[0] = r0 is the tick's direction, input[i + 1] = bit i of (B, F).  A forward dash:
    forward pressed now and not on input[1]; the first input among input[1..W] with a direction is
    forward without backward; some input among the W behind it has no direction.  Backward alike."""
    n = len(B)
    found = np.zeros(n, bool)
    first_f = np.zeros(n, bool)
    first_b = np.zeros(n, bool)
    j = np.zeros(n, np.uint32)
    for i in range(W):
        b, f = ((B >> i) & 1).astype(bool), ((F >> i) & 1).astype(bool)
        first = (b | f) & ~found
        first_f |= first & f
        first_b |= first & b
        j = np.where(first, i, j).astype(np.uint32)
        found |= b | f
    neutral = np.zeros(n, bool)
    for d in range(1, W + 1):
        i = j + d  # (past the 16 kept frames: no direction)
        neutral |= (((B | F) >> i) & 1) == 0
    fwd_now, back_now = ((r0 >> 1) & 1).astype(bool), (r0 & 1).astype(bool)
    fd = found & first_f & ~first_b & neutral & fwd_now & ((F & 1) == 0)
    bd = found & first_b & ~first_f & neutral & back_now & ((B & 1) == 0)
    return fd.astype(np.uint32) | (bd.astype(np.uint32) << 1)


def shift(B, F, r0):
    return ((B << 1) & 0xFFFE) | (r0 & 1), ((F << 1) & 0xFFFE) | (r0 >> 1)


def test_generator_check_includes_the_automaton():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    G.check_parser_table(G.gen_parser(ALLOW), ALLOW)
    header = open(os.path.join(ROOT, "footsies_gym_amd", "csrc", "fs_tables.h")).read()
    assert "constexpr int kParserStates = %d;" % G.parser_num_states(ALLOW) in header
    assert G.parser_num_states(ALLOW) == 217 and len(G.gen_parser(ALLOW)) == 4 * 217


def test_array_helpers_agree_with_the_generator():
    rng = np.random.default_rng(5)
    B = rng.integers(0, 1 << 16, 4000).astype(np.uint32) & rng.integers(0, 1 << 16, 4000).astype(np.uint32)
    F = rng.integers(0, 1 << 16, 4000).astype(np.uint32) & rng.integers(0, 1 << 16, 4000).astype(np.uint32)
    r0 = rng.integers(0, 4, 4000).astype(np.uint32)
    assert np_state_of(B, F).tolist() == [G.state_of(int(b), int(f), ALLOW) for b, f in zip(B, F)]
    assert dash_by_frames(B, F, r0).tolist() == [G.parser_dash(int(b), int(f), int(r), ALLOW) for b, f, r in zip(B, F, r0)]


def test_state_commutes_with_the_shift_exhaustively(table):
    E = np.arange(1 << 16, dtype=np.uint32)
    first = E & (~E + 1)  # the lowest direction frame (0: none)
    seen = set()
    for kind in (1, 2, 3):
        B = (E & ~first) | (first if kind & 1 else 0)
        F = first if kind & 2 else np.zeros_like(E)
        s = np_state_of(B, F)
        seen |= set(s.tolist())
        for r in range(4):
            r0 = np.full_like(E, r)
            ent = table[4 * s + r]
            assert np.array_equal((ent >> 3) & 3, dash_by_frames(B, F, r0))
            assert np.array_equal(ent >> 5, 8 * np_state_of(*shift(B, F, r0)))
            assert np.array_equal(ent & 7, r0 << 1)
    assert seen == set(range(G.parser_num_states(ALLOW)))  # every state has histories


def test_carried_state_against_the_frame_by_frame_parser(table):
    rng = np.random.default_rng(0xDA5)
    n, steps = 1000, 1000  # 10^6 samples
    hist = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    B, F = (hist & 0xFFFF).astype(np.uint32), (hist >> 16).astype(np.uint32)
    state = np_state_of(B, F)  # loop entry; from here on the walkers carry the state alone
    keep = rng.choice([0.0, 0.5, 0.8, 0.9, 0.95], n)  # how likely a walker repeats its direction
    weights = rng.choice(4, n)  # 0 sparse, 1 dense, 2 with both directions held, 3 uniform
    p_new = np.array([[0.85, 0.07, 0.07, 0.01], [0.1, 0.4, 0.4, 0.1], [0.2, 0.2, 0.2, 0.4], [0.25] * 4])[weights]
    cum = np.cumsum(p_new, axis=1)
    r0 = np.zeros(n, np.uint32)
    run_len = np.zeros(n, np.int64)
    runs_seen, both_held, dashes, visited = set(), 0, 0, set()
    for t in range(steps):
        fresh = (rng.random(n)[:, None] > cum).sum(axis=1).astype(np.uint32)
        r0 = np.where(rng.random(n) < keep, r0, fresh).astype(np.uint32)
        ended = (r0 == 0) & (run_len > 0)
        runs_seen |= set(run_len[ended].tolist())
        run_len = np.where(r0 == 0, 0, run_len + 1)
        both_held += int((r0 == 3).sum())
        ent = table[4 * state + r0]
        want = dash_by_frames(B, F, r0)
        assert np.array_equal((ent >> 3) & 3, want), t
        dashes += int((want != 0).sum())
        B, F = shift(B, F, r0)
        state = ent >> 8
        visited |= set(state.tolist())
        if t % 97 == 0 or t == steps - 1:
            assert np.array_equal(state, np_state_of(B, F)), t
    assert {7, 8, 9} <= runs_seen and both_held > 10000 and dashes > 1000
    assert len(visited) >= 200  # (nearly all of the 217; two are unreachable from a shift)


def test_check_rejects_one_corrupted_entry():
    good = G.gen_parser(ALLOW)
    G.check_parser_table(good, ALLOW)
    for idx, flip in ((4 * 37 + 2, 1 << 3), (4 * 100 + 0, 8 << 5), (4 * 216 + 1, 1 << 4), (1, 1 << 1)):
        bad = list(good)
        bad[idx] ^= flip
        with pytest.raises(AssertionError):
            G.check_parser_table(bad, ALLOW)
