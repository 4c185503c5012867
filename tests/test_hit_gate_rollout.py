"""What the specialised row loops' hit gate rests on (fs_kernels.hip wave_has_hit), shown on the CPU
oracle's rollout: an arena-tick on which neither fighter is hit has reward 0, does not end the round
and leaves both fighters' guard and vital as they were.  4 096 arenas from reset over the
benchmark's action stream (splitmix64, seed 0x5EED), 3 000 ticks under same-step auto-reset.

"Hit" is judged from the state before and after the tick: the hit count of the opponent's action
rose (NotifyAttackHit), or the fighter's action became a damage or guard action at frame 0
(NotifyDamaged).  A round-ending hit cannot be judged so -- the same-step burst resets the hit
count and the action before the state is seen -- and the terminal record does not decide it either
(a special's hit leaves no hitstun, and a guard already at 0 does not fall).  So "no termination
without a hit" is not read off a definition of hit; it follows from two facts asserted after every
tick, hit or not, terminated or not: every fighter's vital is 1, and no fighter is DEAD.  A round
ends only on a tick in which a vital reaches 0 (BC:212-213); with every vital at 1 when the tick
starts, that takes a vital falling within the tick, and NotifyDamaged -- a hit -- is the only
writer that lowers it.  A hit that left a fighter at vital 0 or DEAD without ending the round,
which a later no-hit tick would then end, fails the assertion on the tick of that hit.  The share of
32-arena wave-ticks with a hit, the gate's taken rate, is printed; DESIGN.md quotes it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_tables as G  # noqa: E402

STRUCK = (200, 301, 305, 306, 500)  # DAMAGE, GUARD_M / STAND / CROUCH, DEAD (actionIDs, data/f00.json)
DEAD = 500


def test_no_hit_means_no_reward_no_ko_no_guard_or_vital_change(oracle_lib):
    n, ticks, wave = 4096, 3000, 32
    ora = oracle_lib.Oracle(n, base_seed=7)
    ora.reset()
    prev = ora.state()["f"]
    assert (prev["vital"] == 1).all() and not (prev["action_id"] == DEAD).any()
    hit_waves = quiet_waves = kos = 0
    for t in range(ticks):
        ora.step_n_hashed(1, 0x5EED)
        out = ora.outputs(copy=False)
        term = np.asarray(out["terminated"]).astype(bool)
        reward = np.asarray(out["reward"])
        f = ora.state()["f"]
        counted = f["hit_count"] > prev["hit_count"]  # this fighter's attack hit: the opponent was hit
        # (hitstun holds an action on frame 0: "became" means it was not there already; a fresh hit on a
        # fighter still held there is seen on the attacker's hit count)
        struck = np.isin(f["action_id"], STRUCK) & (f["action_frame"] == 0) & \
            ~((prev["action_id"] == f["action_id"]) & (prev["action_frame"] == 0))
        # after every tick: the next one starts with every vital at 1 and nobody on the ground, so it
        # can end the round only by a hit of its own
        assert (f["vital"] == 1).all(), (t, np.argwhere(f["vital"] != 1)[:4])
        assert not (f["action_id"] == DEAD).any(), (t, np.argwhere(f["action_id"] == DEAD)[:4])
        kos += int(term.sum())
        quiet = ~(counted.any(1) | struck.any(1)) & ~term  # (a terminated tick: hit, by the two facts above)
        hit = ~quiet
        assert not (reward[quiet] != 0).any(), (t, np.flatnonzero(quiet & (reward != 0))[:4])
        assert (f["guard"][quiet] == prev["guard"][quiet]).all(), t
        assert (f["vital"][quiet] == prev["vital"][quiet]).all() and (f["vital"][quiet] == 1).all(), t
        w = hit.reshape(n // wave, wave).any(1)
        hit_waves += int(w.sum())
        quiet_waves += int((~w).sum())
        prev = f
    ora.close()
    print("wave-ticks with a hit: %d of %d (%.2f %%)" % (hit_waves, hit_waves + quiet_waves,
                                                       100.0 * hit_waves / (hit_waves + quiet_waves)))
    assert hit_waves > 0 and quiet_waves > 0
    assert kos > n  # (rounds did end: the facts were asserted across KOs and their bursts)


def test_vital_proof_rejects_a_round_ending_action_without_vital_damage():
    """The set's vital == 1 term (prove_fast_loop_closure, part 4): every attack whose damage action is
    DEAD must take a vital, whichever attack it is -- otherwise a fighter would lie DEAD at vital 1
    inside the fast loop, and with the gate no KO test would see it on a no-hit tick."""
    import pytest
    tables = G.closure_inputs()
    dead = tables["names"].index("DEAD")
    lethal = [i for i, a in enumerate(tables["attacks"]) if a["damage_action"] == dead]
    assert lethal
    for i in lethal:
        c = {k: ([dict(x) for x in v] if k == "attacks" else list(v) if isinstance(v, list) else v)
             for k, v in tables.items()}
        c["attacks"][i]["vital_damage"] = 0
        with pytest.raises(AssertionError, match="damage action"):
            G.prove_fast_loop_closure(c)
    c = {k: ([dict(x) for x in v] if k == "attacks" else list(v) if isinstance(v, list) else v)
         for k, v in tables.items()}
    c["attacks"][0]["vital_damage"] = -1  # a "hit" that would raise vital above 1
    with pytest.raises(AssertionError, match="vital damage"):
        G.prove_fast_loop_closure(c)
