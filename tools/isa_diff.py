#!/usr/bin/env python3
"""Instruction streams of the kernels of two builds of libmfpa.so, side by side.

usage: isa_diff.py LIB_A LIB_B [symbol-regex] [--rename OLD=NEW ...] [--lines N]

Kernels are paired by demangled name without the argument list (`ns::kernel<true>`; a second copy of a shared header's kernel is `... #2`).
Per kernel whose name matches the regex: the instruction count in both libraries (csrc/isa_scan.disassemble, trailing padding
dropped), VGPRs / SGPRs / scratch / static LDS from the code objects' metadata notes, and the differing instructions after label
normalisation (a branch's offset becomes `L`, so that one inserted instruction does not show up again at every branch across it).
--rename rewrites A's names before the two sides are paired (a kernel that changed its name or its template arguments);
--lines bounds the differing lines printed per kernel (default: all).
"""
import argparse
import difflib
import os
import re
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from musicfpaugment_amd.csrc import isa_scan
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from same_kernels import PAD, demangle, resources      # the two tools read code objects the same way

_BRANCH = re.compile(r"^(s_cbranch_\w+|s_branch)\s+\S+")


def kernels(lib):
    """demangled name -> (normalised instruction lines, resources or None for a device function)"""
    bodies, last = [], None                                        # a symbol's instructions are one contiguous run of rows; the same
    for sym, ins in isa_scan.disassemble(lib):                     # name again later is another file's copy (a shared header's kernel)
        if sym != last:
            bodies.append((sym, []))
            last = sym
        bodies[-1][1].append(_BRANCH.sub(lambda m: m.group(1) + " L", " ".join(ins.split())))
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for k, co in enumerate(isa_scan.code_objects(lib)):        # the same order as disassemble walks them
            f = os.path.join(tmp, f"{k}.co")
            with open(f, "wb") as fh:
                fh.write(co)
            for sym, r in resources(f).items():
                res.setdefault(sym, []).append(r)
    names = demangle(sorted({s for s, _ in bodies}))
    out = {}
    for sym, ins in bodies:
        while ins and PAD.match(ins[-1]):
            ins.pop()
        nm, n = _short(names[sym]), 1
        while (nm if n == 1 else f"{nm} #{n}") in out:
            n += 1
        out[nm if n == 1 else f"{nm} #{n}"] = (ins, res[sym].pop(0) if res.get(sym) else None)
    return out


def _short(name):
    """a demangled name without its return type and argument list: `ns::kernel<true>`"""
    name = re.sub(r"^void ", "", name)
    if name.endswith(")"):
        depth = 0
        for i in range(len(name) - 1, -1, -1):
            depth += (name[i] == ")") - (name[i] == "(")
            if depth == 0:
                return name[:i]
    return name


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("lib_a")
    ap.add_argument("lib_b")
    ap.add_argument("regex", nargs="?", default=".")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    ap.add_argument("--lines", type=int, default=None)
    args = ap.parse_args()
    a, b = kernels(args.lib_a), kernels(args.lib_b)
    for r in args.rename:
        old, new = r.split("=", 1)
        a = {(new if k == old else k): v for k, v in a.items()}
    pat = re.compile(args.regex)
    fmt = lambda r: "vgpr %d sgpr %d scratch %d lds %d" % (r["vgpr"], r["sgpr"], r["scratch"], r["lds"]) if r else "(function)"
    for nm in sorted(k for k in set(a) | set(b) if pat.search(k)):
        if nm not in a or nm not in b:
            ins, r = (a if nm in a else b)[nm]
            print(f"only {'A' if nm in a else 'B'}: {len(ins):6d} ins  {fmt(r)}  {nm}")
            continue
        (ia, ra), (ib, rb) = a[nm], b[nm]
        diff = [d for d in difflib.unified_diff(ia, ib, lineterm="", n=0) if not d.startswith(("+++", "---"))]
        nd = sum(1 for d in diff if d[:1] in "+-")
        print(f"{nm}\n  A {len(ia):6d} ins  {fmt(ra)}\n  B {len(ib):6d} ins  {fmt(rb)}\n  {'identical' if nd == 0 else f'{nd} differing lines'}")
        for d in diff[:args.lines]:
            print("    " + d)
    return 0


if __name__ == "__main__":
    sys.exit(main())
