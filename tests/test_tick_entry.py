"""The tick-entry table (fs_tables.h Tables::tick): the generator's offline proof and its outputs.

tools/gen_tables.py proves, while it generates, that the word the fused kernels decode -- the
table below kTickFrames, tick_entry_slow's arithmetic at every frame -- gives IncrementActionFrame
(Fighter.cs:140-166) and the window scans (ActionData.cs:87-168) evaluated directly from
data/f00.json, for every action, frame 0..511 and both hitstun cases."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gen_tables():
    spec = importlib.util.spec_from_file_location("gen_tables", os.path.join(ROOT, "tools", "gen_tables.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_check_passes_with_the_proof():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_tables.py"), "--check"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_regenerated_headers_equal_the_committed_ones():
    outs = {os.path.relpath(p, ROOT): text for p, text in gen_tables().outputs().items()}
    assert set(outs) == {os.path.join("oracle", "or_tables.h"), os.path.join("footsies_gym_amd", "csrc", "fs_tables.h")}
    for rel, text in outs.items():
        with open(os.path.join(ROOT, rel)) as f:
            assert f.read() == text, rel


def test_known_entries():
    """Entries worked out by hand from the asset values, read back from the
    generated header: [0,6) frame record | [6,8) class | [8,16) the next tick's frame."""
    import re
    text = gen_tables().outputs()[os.path.join(ROOT, "tools", "..", "footsies_gym_amd", "csrc", "fs_tables.h")]
    names = re.findall(r"constexpr int A_(\w+) = (\d+);", text)
    idx = {n: int(i) for n, i in names}
    body = text[text.index("__constant__ const Tables kTables"):]
    rows = re.findall(r"^      \{((?:0x[0-9a-f]{4}(?:, )?){64})\},$", body, re.M)
    assert len(rows) == 2 * len(idx)
    tick = [[int(x, 16) for x in r.split(", ")] for r in rows]

    def entry(name, frame, stunned):
        e = tick[2 * idx[name] + stunned][frame]
        return e >> 8, (e >> 6) & 3

    assert entry("WIN", 32, 0) == (5, 0)        # frame 33 == frameCount: loops to loopFromFrame 5
    assert entry("WIN", 32, 1) == (32, 0)       # in hitstun the frame stands
    assert entry("DEAD", 63, 0) == (64, 0)      # the table's last frame
    assert entry("STAND", 23, 0) == (24, 2)     # frameCount 24 reached: ended
    assert entry("STAND", 24, 1) == (24, 2)
    assert entry("N_ATTACK", 0, 0) == (1, 1)    # cancel windows [1, 3] (buffer) and [4, 5] (execute)
    assert entry("N_ATTACK", 5, 0) == (6, 0)
    assert entry("N_ATTACK", 4, 1) == (4, 1)
    assert entry("B_ATTACK", 5, 1) == (5, 1)    # [1, 2] and [3, 5]
    assert entry("GUARD_PROXIMITY", 0, 0) == (1, 2)  # frameCount 1
    # the frame record is the one rec_index gives for (action, that frame)
    m = re.search(r"\},\n  \{\n((?:    [0-9, ]+,\n)+)  \},", body)
    ridx = [int(x) for x in m.group(1).replace("\n", " ").split(",") if x.strip()]
    assert len(ridx) == 64 * len(idx)
    for name, a in idx.items():
        for stunned in (0, 1):
            for f in range(64):
                e = tick[2 * a + stunned][f]
                assert e & 63 == ridx[64 * a + min(e >> 8, 63)], (name, f, stunned)
