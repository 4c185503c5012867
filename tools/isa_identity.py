#!/usr/bin/env python3
"""Compare two device-assembly listings of fs_kernels.hip function by function (text only).

  hipcc --offload-arch=gfx950 <build.flags_for("fs_kernels.hip")> -I include --cuda-device-only -S \
        footsies_gym_amd/csrc/fs_kernels.hip -o tree.s          # the same in a checkout of the parent
  python tools/isa_identity.py parent.s tree.s > profiles/<name>.txt

A function's text runs from its first directive to the next function's: the instruction stream, the
labels, the .amdhsa_* block and the resource comments.  Labels an inline-asm statement numbers with
`%=` (prio_slice's .Lprio_lo<N> / .Lprio_end<N>) count statements over the whole listing, so a kernel
behind one that gained or lost such a statement carries other numbers around the same bytes: they are
renumbered per function, in order of appearance, before the comparison.  One line per function: the two instruction
counts and `identical`, `differs`, or `only here` for a kernel one listing lacks (an added kernel changes
none).  A step kernel is a function named fsk::k_step*, fsk::selfplay::k_step* or fsk::league::k_step*.
Exit status 1 if a step kernel of the parent differs in the tree or is missing there: a refactor
of the tick must leave those byte for byte (DESIGN.md "The identity rule").
"""
import re
import subprocess
import sys


def functions(path):
    """{demangled name: text} of every function in the listing, in order."""
    text = open(path).read()
    text = text[:text.find("\t.type\t__hip_cuid_")] if "\t.type\t__hip_cuid_" in text else text
    # (the code's end padding and the data objects follow the last function: not part of it,
    # whichever function comes last)
    end = re.search(r"^\t\.text\n\t\.p2alignl [^\n]*\n\t\.fill [^\n]*\n\t\.section\t\.AMDGPU\.gpr_maximums", text, re.M)
    text = text[:end.start()] if end else text
    starts = list(re.finditer(r"^(?:\t\.section\t\.text\.\S*\n)?(?:\t\.protected\t[^\n]*\n)?\t\.globl\t(\S+)\n"
                              r"(?:\t\.p2align\t\d+\n)?\t\.type\t\1,@function\n", text, re.M))
    out = {}
    for m, nxt in zip(starts, starts[1:] + [None]):
        out[m.group(1)] = text[m.start():nxt.start() if nxt else len(text)]
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void |\(.*$", "", n): local_labels(t) for n, t in zip(names, out.values())}


def local_labels(text):
    """`text` with its %=-numbered inline-asm labels renumbered from 0 in order of appearance."""
    order = {}
    return re.sub(r"(\.L[A-Za-z_]+?)(\d+)\b(?=:|\s|$)", lambda m: m.group(0) if m.group(1).startswith((".LBB", ".Lfunc", ".Ltmp"))
                  else "%s#%d" % (m.group(1), order.setdefault(m.group(2), len(order))), text, flags=re.M)


def is_step_kernel(name):
    return re.match(r"fsk::(?:selfplay::|league::)?k_step", name) is not None


def count(text):
    return len(re.findall(r"^\t[a-z][a-z0-9_]*(?:\s|$)", text, re.M))


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    print("# %-46s %8s %8s" % ("function", "parent", "tree"))
    for name in list(a) + [n for n in b if n not in a]:
        same = a.get(name) == b.get(name)
        bad += (not same) and name in a and is_step_kernel(name)  # (a kernel the tree adds is no change)
        print("%-48s %8s %8s  %s" % (name, count(a[name]) if name in a else "-", count(b[name]) if name in b else "-",
                                     "identical" if same else "differs" if name in a and name in b else "only here"))
    steps = [n for n in a if is_step_kernel(n)]
    print("# %d functions, %d step kernels, %d step kernels differ" % (len(a), len(steps), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
