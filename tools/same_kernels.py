"""Are the gfx950 kernels of two builds the same machine code?   same_kernels.py OLD.o... -- NEW.o...

Each side is any number of hipcc-built .o / .so files.  Their gfx950 code objects are extracted as tools/disasm_obj.py does, and the
kernels of the two sides are compared by demangled name:
  * the instruction text of `llvm-objdump -d`, addresses and encodings stripped, branch offsets kept, trailing padding dropped; the
    literal of a pc-relative address (the s_add_u32 / s_addc_u32 pair behind s_getpc_b64: where a called device function lies in
    ITS file) is an address too and is stripped -- the called functions are compared like kernels, by name;
  * VGPR / AGPR / SGPR counts, scratch, static LDS and kernarg size from the code object's notes.
One line per kernel, `identical` or `differs (n lines)`, with the resource counts; kernels that only one side has are listed.  The exit
status is 0 only when both sides have the same kernels and every one is identical.  The tool diffs text; it searches for nothing.
"""
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from musicfpaugment_amd.csrc import isa_scan

_LABEL = re.compile(r"^[0-9a-f]+ <([^>]+)>:")
PAD = re.compile(r"^(s_nop|s_code_end|v_nop|\.\.\.)")
_GETPC = re.compile(r"^s_getpc_b64 s\[(\d+):(\d+)\]")
_NOTE_KEYS = {".vgpr_count": "vgpr", ".agpr_count": "agpr", ".sgpr_count": "sgpr", ".private_segment_fixed_size": "scratch",
              ".group_segment_fixed_size": "lds", ".kernarg_segment_size": "kernarg"}


def _tool(name):
    return os.path.join(os.path.dirname(isa_scan._objdump()), name)


def demangle(names):
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not filt or not names:             # no demangler: the mangled names compare just as well
        return {n: n for n in names}
    out = subprocess.run([filt] + list(names), capture_output=True, text=True, check=True).stdout.splitlines()
    return dict(zip(names, out))


def resources(path):
    """kernel symbol -> {vgpr, agpr, sgpr, scratch, lds, kernarg} from the AMDGPU metadata note"""
    txt = subprocess.run([_tool("llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    res, cur = {}, {}
    for line in txt.splitlines() + ["  - .end:"]:
        if line.startswith("  - ") and ".name" in cur:          # the next kernel's map begins
            res[cur[".name"]] = {v: int(cur.get(k, 0)) for k, v in _NOTE_KEYS.items()}
            cur = {}
        m = re.match(r"^  [ -] (\.[a-z_]+):\s+'?([^']+)'?$", line)   # a kernel's own keys: four columns in (its arguments sit deeper)
        if m:
            cur[m.group(1)] = m.group(2)
    return res


def kernels(paths):
    """demangled kernel name -> (instruction lines, resources) over every gfx950 code object of `paths`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for p in paths:
            for k, co in enumerate(isa_scan.code_objects(p)):
                f = os.path.join(tmp, f"{len(out)}_{k}.co")
                with open(f, "wb") as fh:
                    fh.write(co)
                res = resources(f)
                txt = subprocess.run([isa_scan._objdump(), "-d", f], capture_output=True, text=True, check=True).stdout
                body, sym = {}, None
                for line in txt.splitlines():
                    m = _LABEL.match(line)
                    if m:
                        sym = m.group(1)
                        body[sym] = []
                    elif sym and line.startswith("\t"):
                        body[sym].append(" ".join(line.split("//")[0].split()))
                names = demangle(list(body))
                for s, nm in names.items():
                    ins = body[s]
                    while ins and PAD.match(ins[-1]):
                        ins.pop()
                    for j, line in enumerate(ins):
                        m = _GETPC.match(line)
                        if m:
                            for k, (op, reg) in enumerate((("s_add_u32", m.group(1)), ("s_addc_u32", m.group(2))), 1):
                                if j + k < len(ins) and ins[j + k].startswith(f"{op} s{reg}, s{reg}, "):
                                    ins[j + k] = f"{op} s{reg}, s{reg}, <pc-relative>"
                    if nm in out and out[nm] == (ins, None):        # a device function may sit in several files, the same text in each
                        continue
                    n = 1                                           # so may an internal kernel of a shared header: #2, #3 ... in file order
                    while (nm if n == 1 else f"{nm} #{n}") in out:
                        n += 1
                    out[nm if n == 1 else f"{nm} #{n}"] = (ins, res.get(s))         # no resources: a device function, not a kernel
    return out


def main(argv):
    if "--" not in argv:
        raise SystemExit(__doc__)
    i = argv.index("--")
    old, new = kernels(argv[:i]), kernels(argv[i + 1:])
    same = 0
    for nm in sorted(set(old) | set(new)):
        if nm not in old or nm not in new:
            print(f"only {'old' if nm in old else 'new'}: {nm}")
            continue
        (io, ro), (inw, rn) = old[nm], new[nm]
        n = sum(1 for d in difflib.unified_diff(io, inw, lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---"))
        rs = " ".join(f"{k}={v}" for k, v in rn.items()) if rn else "(function)"
        if n == 0 and ro == rn:
            same += 1
            print(f"identical  {len(inw):6d} ins  {rs}  {nm}")
        else:
            was = "" if ro == rn else f"  (was {ro})"
            print(f"differs ({n} lines)  {rs}{was}  {nm}")
    print(f"{sum(1 for v in old.values() if v[1])} | {sum(1 for v in new.values() if v[1])} kernels, "
          f"{len(old)} | {len(new)} symbols, {same} identical")
    return 0 if same == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
