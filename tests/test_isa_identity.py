"""tools/isa_identity.py gates every step kernel: fsk::k_step*, fsk::selfplay::k_step*, fsk::league::k_step*
(DESIGN.md "The identity rule").  Two tiny synthetic listings, no compiler."""
import os
import subprocess
import sys

TOOL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "isa_identity.py")

# mangled name -> demangled (c++filt)
STEP = "_ZN3fsk8k_step_nILi0ELi1EEEvv"             # fsk::k_step_n<0, 1>
SELFPLAY = "_ZN3fsk8selfplay8k_step_xILi0EEEvv"   # fsk::selfplay::k_step_x<0>
LEAGUE = "_ZN3fsk6league8k_step_yILi1EEEvv"       # fsk::league::k_step_y<1>
RESET = "_ZN3fsk7k_resetILi0EEEvv"                # fsk::k_reset<0>
ADDED = "_ZN3fsk8selfplay8k_step_zILi0EEEvv"      # fsk::selfplay::k_step_z<0>


def function(name, body):
    return ("\t.section\t.text.%s,\"axG\",@progbits,%s,comdat\n\t.protected\t%s\n\t.globl\t%s\n\t.p2align\t8\n"
            "\t.type\t%s,@function\n%s:\n%s\ts_endpgm\n\t.amdhsa_next_free_vgpr 8\n" % ((name,) * 6 + (body,)))


def listing(path, bodies):
    text = "\t.text\n\t.amdgcn_target \"amdgcn-amd-amdhsa--gfx950\"\n" + "".join(function(n, b) for n, b in bodies.items())
    path.write_text(text + "\t.type\t__hip_cuid_0123,@object\n")
    return str(path)


def run(tmp_path, tree_changes, added=None):
    parent = {STEP: "\tv_mov_b32 v0, 0\n", SELFPLAY: "\tv_mov_b32 v0, 0\n\tv_mov_b32 v1, 0\n",
              LEAGUE: "\tv_mov_b32 v2, 0\n", RESET: "\ts_nop 0\n"}
    tree = dict(parent, **tree_changes)
    if added:
        tree[added] = "\ts_nop 1\n"
    r = subprocess.run([sys.executable, TOOL, listing(tmp_path / "parent.s", parent), listing(tmp_path / "tree.s", tree)],
                       capture_output=True, text=True)
    assert r.stderr == ""
    # {function name: its line}; a line is the name, the two counts and a one- or two-word verdict
    verdict = {}
    for ln in r.stdout.splitlines():
        if not ln.startswith("#"):
            f = ln.split()
            verdict[" ".join(f[:-4] if f[-2:] == ["only", "here"] else f[:-3])] = ln
    return r.returncode, verdict, r.stdout.splitlines()[-1]


def test_identical_listings_pass_and_count_every_namespace(tmp_path):
    code, verdict, summary = run(tmp_path, {})
    assert code == 0
    assert summary == "# 4 functions, 3 step kernels, 0 step kernels differ"
    assert verdict["fsk::selfplay::k_step_x<0>"].endswith("identical")


def test_differing_selfplay_kernel_fails_and_is_counted(tmp_path):
    # the two v_mov lines changing places: equal instruction counts, other text
    code, verdict, summary = run(tmp_path, {SELFPLAY: "\tv_mov_b32 v1, 0\n\tv_mov_b32 v0, 0\n"})
    assert code == 1
    assert summary == "# 4 functions, 3 step kernels, 1 step kernels differ"
    assert verdict["fsk::selfplay::k_step_x<0>"].endswith("differs")
    assert verdict["fsk::k_step_n<0, 1>"].endswith("identical") and verdict["fsk::league::k_step_y<1>"].endswith("identical")


def test_differing_league_kernel_fails(tmp_path):
    code, _, summary = run(tmp_path, {LEAGUE: "\tv_mov_b32 v3, 0\n"})
    assert code == 1
    assert summary == "# 4 functions, 3 step kernels, 1 step kernels differ"


def test_differing_reset_kernel_does_not_fail(tmp_path):
    code, verdict, summary = run(tmp_path, {RESET: "\ts_nop 7\n"})
    assert code == 0
    assert summary == "# 4 functions, 3 step kernels, 0 step kernels differ"
    assert verdict["fsk::k_reset<0>"].endswith("differs")


def test_kernel_only_in_the_tree_changes_nothing(tmp_path):
    code, verdict, summary = run(tmp_path, {}, added=ADDED)
    assert code == 0
    assert summary == "# 4 functions, 3 step kernels, 0 step kernels differ"
    assert verdict["fsk::selfplay::k_step_z<0>"].endswith("only here")
