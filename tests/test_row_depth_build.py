"""The row ring as compiled (fs_kernels.hip row_ring, FS_ROW_DEPTH2 = D): on the gfx950 assembly of
k_step_n_packed<0, 0> and k_step_n<0, 0>, the specialised loop holds D ticks -- D untracked row
loads, D row waits, each `s_waitcnt vmcnt(kRowOps (D - 1))` -- and the generic loop keeps its two
ticks with vmcnt(3) (packed) / vmcnt(11) (per-field) waits.
Build-container test: hipcc cross-compiles, no GPU needed."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
SRC = os.path.join(ROOT, "footsies_gym_amd", "csrc", "fs_kernels.hip")
ROW_OPS = {"_ZN3fsk15k_step_n_packedILi0ELi0EEEvNS_10StepParamsE": 3,  # one tick's stores plus one row load
           "_ZN3fsk8k_step_nILi0ELi0EEEvNS_10StepParamsE": 11}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    import check_async_loads as CA
    from footsies_gym_amd import build as B
    out = str(tmp_path_factory.mktemp("asm") / "k.s")
    subprocess.run([B._hipcc(), "--offload-arch=" + B.ARCH, *B.flags_for(SRC), "-I", os.path.join(ROOT, "include"),
                    "--cuda-device-only", "-S", "-o", out, SRC], check=True, stderr=subprocess.DEVNULL, timeout=900)
    return CA.kernels(open(out).read())


def depth():
    d = int(re.search(r"^#define FS_ROW_DEPTH2 (\d+)", open(SRC).read(), re.M).group(1))
    assert 2 <= d <= 4
    return d


def row_loops(lines):
    """The two row loops of a kernel, as (row loads, [row wait counts]) each: the widest backward-branch
    span that holds row loads and neither a barrier nor the program's end, and the widest apart from
    it (blocks laid out behind a loop branch back into it: narrower spans, which overlap it)."""
    code = [s.strip() for s in lines if s.strip() and not s.strip().startswith(";")]
    label = {m.group(1): i for i, s in enumerate(code) for m in [re.match(r"^(\.LBB\d+_\d+):", s)] if m}
    spans = []
    for i, s in enumerate(code):
        m = re.match(r"^s_c?branch\S*\s+(\.LBB\d+_\d+)", s)
        if m and label.get(m.group(1), i) < i:
            body = code[label[m.group(1)]:i + 1]
            text = "\n".join(body)
            if "global_load_ubyte" in text and not re.search(r"s_endpgm|s_barrier|global_load_dwordx4", text):
                spans.append((label[m.group(1)], i))
    spans.sort(key=lambda sp: sp[0] - sp[1])
    first = spans[0]
    rest = [sp for sp in spans if sp[1] < first[0] or sp[0] > first[1]]
    assert rest, "expected a generic and a specialised row loop"
    out = []
    for lo, hi in (first, rest[0]):
        body = code[lo:hi + 1]
        waits = [int(m.group(1)) for a, b in zip(body, body[1:]) for m in [re.match(r"s_waitcnt vmcnt\((\d+)\)$", a)]
                 if m and b.startswith("v_mov_b32")]
        out.append((sum(s.startswith("global_load_ubyte") for s in body), waits))
    return out


@pytest.mark.parametrize("kernel", sorted(ROW_OPS))
def test_the_specialised_loop_holds_d_ticks_and_the_generic_loop_two(kernels, kernel):
    d, ops = depth(), ROW_OPS[kernel]
    loops = row_loops(kernels[kernel])
    # (a generic tick holds two row waits, one on its reset-pending path: the counts are what is fixed there)
    is_ring = [lp == (d, [ops * (d - 1)] * d) for lp in loops]
    is_generic = [lp[0] == 2 and set(lp[1]) == {ops} for lp in loops]
    assert (is_ring[0] and is_generic[1]) or (is_ring[1] and is_generic[0]), loops
