"""The fast row loops' invariant set (fs_kernels.hip kLmFast, in_fast_set): hasWon clear, the
action / buffered / reserved action none of DEAD and WIN, action frame below kTickFrames, vital at
most 1.  tools/gen_tables.py proves from the frame data that a Fight tick with its same-step burst
maps the set into itself (prove_fast_loop_closure, run by --check); here the proof is shown to
reject broken tables, and the oracle's rollout from reset is shown to stay inside the set."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables as G  # noqa: E402

DEAD_ID, WIN_ID = 500, 510  # actionIDs (data/f00.json)


def test_check_passes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


@pytest.fixture(scope="module")
def tables():
    return G.closure_inputs()


def fresh(tables):
    return {k: ([dict(x) for x in v] if k == "attacks" else list(v) if isinstance(v, list) else v)
            for k, v in tables.items()}


def test_proof_holds_on_the_generated_tables(tables):
    G.prove_fast_loop_closure(fresh(tables))


def test_attack_into_dead_without_vital_damage_is_rejected(tables):
    c = fresh(tables)
    dead = c["names"].index("DEAD")
    atk = next(a for a in c["attacks"] if a["damage_action"] == dead)
    atk["vital_damage"] = 0  # DEAD without a KO: the fighter would walk to frame 500 inside the fast loop
    with pytest.raises(AssertionError, match="damage action"):
        G.prove_fast_loop_closure(c)


def test_attack_into_win_or_guard_into_dead_is_rejected(tables):
    c = fresh(tables)
    c["attacks"][0]["damage_action"] = c["names"].index("WIN")
    with pytest.raises(AssertionError, match="damage action"):
        G.prove_fast_loop_closure(c)
    c = fresh(tables)
    c["attacks"][0]["guard_action"] = c["names"].index("DEAD")
    with pytest.raises(AssertionError, match="guard action"):
        G.prove_fast_loop_closure(c)


def test_tick_entry_past_the_table_is_rejected(tables):
    c = fresh(tables)
    tf = c["tick_frames"]
    a = c["names"].index("B_SPECIAL")
    i = (a * 2 + 0) * tf + 10
    assert (c["tick"][i] >> 6) & 3 != 2  # (mid-action: the request may keep the action)
    c["tick"][i] = (c["tick"][i] & 0xFF) | (tf << 8)  # next frame 64
    with pytest.raises(AssertionError, match="tick entry leaves the table"):
        G.prove_fast_loop_closure(c)


def test_request_entries_that_leave_the_set_are_rejected(tables):
    names = tables["names"]
    stand, dead, win = names.index("STAND"), names.index("DEAD"), names.index("WIN")
    c = fresh(tables)
    c["req_table"][(stand << 8) | (5 ^ stand)] = win | (31 << 5) | (1 << 11)  # the chain sets WIN
    with pytest.raises(AssertionError, match="request sets"):
        G.prove_fast_loop_closure(c)
    c = fresh(tables)
    c["req_table"][(stand << 8) | (5 ^ stand)] = stand | (dead << 5) | (1 << 10)  # ... buffers DEAD
    with pytest.raises(AssertionError, match="request buffers"):
        G.prove_fast_loop_closure(c)
    c = fresh(tables)
    c["req_table"][c["req_early"] + stand] = dead | (31 << 5) | (1 << 11)  # an early return into DEAD
    with pytest.raises(AssertionError, match="request sets"):
        G.prove_fast_loop_closure(c)
    c = fresh(tables)
    c["req_table"][(stand << 8) | ((18 << 3) ^ stand)] &= ~(1 << 11)  # an ended action kept: frame 64 survives
    with pytest.raises(AssertionError):
        G.prove_fast_loop_closure(c)


def test_oracle_rollout_from_reset_stays_inside_the_set(oracle_lib, tables):
    """4 096 arenas from reset, 3 000 ticks of hashed actions under same-step auto-reset: every
    fighter is inside the set at every step boundary."""
    n, ticks = 4096, 3000
    ora = oracle_lib.Oracle(n, base_seed=7)
    ora.reset()
    kos = 0
    for t in range(ticks):
        ora.step_n_hashed(1, 0x5EED)
        kos += int(np.asarray(ora.outputs(copy=False)["terminated"]).astype(bool).sum())
        f = ora.state()["f"]
        bad = ((f["has_won"] != 0) | (f["vital"] > 1) | (f["action_frame"] >= tables["tick_frames"]) |
               (f["action_frame"] < 0))
        for field in ("action_id", "buffer_action_id", "reserve_action_id"):
            bad |= (f[field] == DEAD_ID) | (f[field] == WIN_ID)
        assert not bad.any(), (t, np.argwhere(bad)[0], f[tuple(np.argwhere(bad)[0])])
    ora.close()
    assert kos > n  # (rounds did end: the burst's side of the closure was exercised)
