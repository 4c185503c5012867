"""The fused kernels' launch-mode loops (fs_kernels.hip kLmFast / kLmFastPrio) cost no occupancy.

Each standard fused row kernel holds a second row loop compiled for the common launch (same-step
auto-reset, dense reward, no pending lane); a kernel's register count is the maximum over its
loops.  From the compiler's resource remarks for gfx950, with the library's own flags: no fused
kernel uses scratch, and the standard kernels (remote or idle P2, both float models) stay within
the 128 VGPRs that keep four waves per SIMD.  The compiled standard kernels must hold the extra
row loop: more untracked row loads than the same kernel for the scripted bot, which keeps the
generic loop alone.  Build-container test: hipcc cross-compiles, no GPU needed."""
import functools
import os
import re
import subprocess
import tempfile

from footsies_gym_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOUR_WAVES_VGPRS = 512 // 4  # gfx950: 512 VGPRs per SIMD lane, unified with the AGPRs these kernels do not use


@functools.lru_cache(maxsize=None)
def resources():
    """{kernel symbol: {"VGPRs": .., "ScratchSize": .., "Occupancy": .., "row_loads": ..}} of
    fs_kernels.hip: the compiler's remarks, and the row loads (row_load's global_load_ubyte) counted
    in each kernel's assembly."""
    src = "fs_kernels.hip"
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        cmd = [B._hipcc(), "--offload-arch=" + B.ARCH, *B.flags_for(src), "-I", os.path.join(ROOT, "include"),
               "--cuda-device-only", "-S", "-o", out, os.path.join(B.CSRC, src),
               "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        asm = open(out).read()
    res, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: +(VGPRs|ScratchSize|Occupancy) ?(?:\[[^\]]*\])?: (\d+)", line)
        if m and cur is not None:
            cur[m.group(1)] = int(m.group(2))
    cur = None
    for line in asm.splitlines():
        m = re.match(r"^(_Z\S+):", line)
        if m:
            cur = res.get(m.group(1))
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None and "global_load_ubyte" in line:
            cur["row_loads"] = cur.get("row_loads", 0) + 1
    return res


def fused(res):
    return {k: v for k, v in res.items() if re.search(r"_ZN3fsk\d+k_step_n", k)}


def test_fused_kernels_use_no_scratch():
    f = fused(resources())
    assert len(f) == 56, sorted(f)  # 8 each of k_step_n, _packed, _hashed, _policy; 6 each of _pf, _packed_pf, n1, n1_packed
    assert all(v["ScratchSize"] == 0 for v in f.values()), {k: v for k, v in f.items() if v["ScratchSize"]}


def test_standard_kernels_keep_four_waves_per_simd():
    f = fused(resources())
    std = {k: v for k, v in f.items()
           if re.search(r"_ZN3fsk\d+k_step_n(_packed)?(_pf)?ILi[01]ELi[02]EE", k)}
    assert len(std) == 16, sorted(std)
    over = {k: v for k, v in std.items() if v["VGPRs"] > FOUR_WAVES_VGPRS or v["Occupancy"] < 4}
    assert not over, over
    assert all(v["VGPRs"] > 0 for v in std.values())


def test_standard_kernels_hold_the_specialised_row_loop():
    """Every row loop issues its own row loads.  The bot kernels hold the generic loop (and, outside
    the _pf kernels, the general-geometry one); the standard kernels of the same family and float
    model hold the specialised loop too, so their assembly has more row loads."""
    f = fused(resources())
    pairs = 0
    for k, v in f.items():
        m = re.search(r"(_ZN3fsk\d+k_step_n(?:_packed)?(?:_pf)?ILi[01]ELi)([02])(EE.*)", k)
        if not m:
            continue
        bot = f[m.group(1) + "1" + m.group(3)]
        assert bot["row_loads"] >= 5, (k, bot)  # rows 0 and 1, then three ticks of one loop
        assert v["row_loads"] >= bot["row_loads"] + 3, (k, v["row_loads"], bot["row_loads"])
        pairs += 1
    assert pairs == 16
