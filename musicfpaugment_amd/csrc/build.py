"""Build libmfpa.so (all HIP kernels + the C ABI of include/mfpa.h) for gfx950 with hipcc.

In-tree, no torch dependency: `python -m musicfpaugment_amd.csrc.build`.  hipcc cross-compiles
without a GPU; the resulting musicfpaugment_amd/libmfpa.so travels to the GPU box as is.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OUT = os.path.join(PKG, "libmfpa.so")
RECORD = os.path.join(PKG, "libmfpa.build.json")     # identity of the library in the tree (git-ignored like the library itself)
OBJ = os.path.join(HERE, "build")
ARCH = "gfx950"

COMMON = ["-O3", f"--offload-arch={ARCH}", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function"]
# The peak pickers compare float64 values that must round exactly like numpy's un-fused
# multiply / add sequence: no FMA contraction there.  The IIR recurrence is restated in numpy operation for operation
# (tests/_iir_oracle.py) and compared bit for bit: none there either.  The room simulator's delays tau = (d fs) / c are the
# oracle's doubles (tests/_rir_oracle.py) only without contraction.  The compressor's recurrences (dynamics.hip) keep the order and the
# roundings of the formula in include/mfpa.h, which tests/_dynamics_oracle.py restates.  The delay lines (delay.hip) likewise: the comb is
# compared with tests/_delay_oracle.py bit for bit, and the fractional delay's staged and direct paths must round alike.  The transform codec (codec.hip) takes discrete decisions (a band coded
# or not, a coefficient's rounding) from sums and products that tests/_codec_oracle.py restates in the order of include/mfpa.h.  The spectral noise suppressor (denoise.hip) is two serial
# recurrences of correctly rounded operations that tests/_denoise_oracle.py restates in numpy and compares bit for bit.  The loudness meter
# (loudness.hip) runs the IIR recurrence of iir.hip (mfpa_sos.h) and sums squares and block powers in the order of include/mfpa.h, which
# tests/_loudness_oracle.py restates bit for bit.
PER_FILE = {
    "audfprint.hip": ["-ffp-contract=off"],
    "codec.hip": ["-ffp-contract=off"],
    "dejavu.hip": ["-ffp-contract=off"],
    "delay.hip": ["-ffp-contract=off"],
    "denoise.hip": ["-ffp-contract=off"],
    "dynamics.hip": ["-ffp-contract=off"],
    "iir.hip": ["-ffp-contract=off"],
    "loudness.hip": ["-ffp-contract=off"],
    "nplog.hip": ["-ffp-contract=off"],
    "rir.hip": ["-ffp-contract=off"],
}


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: libmfpa.so cannot be built")


def _sources():
    return sorted(f for f in os.listdir(HERE) if f.endswith(".hip"))


def _stamp(src: str, flags) -> str:
    h = hashlib.sha1()
    h.update(" ".join(flags).encode())
    for f in [src] + sorted(x for x in os.listdir(HERE) if x.endswith(".h")) + ["../../include/mfpa.h"]:
        with open(os.path.join(HERE, f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    jobs = []
    objs = []
    for src in _sources():
        flags = COMMON + PER_FILE.get(src, [])
        obj = os.path.join(OBJ, src.replace(".hip", ".o"))
        stamp_file = obj + ".stamp"
        stamp = _stamp(src, flags)
        objs.append(obj)
        if not force and os.path.exists(obj) and os.path.exists(stamp_file) and open(stamp_file).read() == stamp:
            continue
        jobs.append((src, [hipcc] + flags + ["-c", os.path.join(HERE, src), "-o", obj], stamp_file, stamp))

    def run(job):
        src, cmd, stamp_file, stamp = job
        if verbose:
            print("[mfpa build]", " ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
        if r.stderr.strip() and verbose:
            print(r.stderr, file=sys.stderr)
        with open(stamp_file, "w") as fh:
            fh.write(stamp)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    if jobs or not os.path.exists(OUT) or force:
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", OUT] + objs
        if verbose:
            print("[mfpa build]", " ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    write_record(record(OUT))
    return OUT


def write_record(rec: dict) -> None:
    with open(RECORD, "w") as fh:
        fh.write(json.dumps(rec, indent=1, sort_keys=True) + "\n")


def record(path: str = None) -> dict:
    """Identity of a built library: sha256, size, hipcc version, flags (build() writes it to RECORD; a round's final one is committed as
    profiles/BUILD_rNN.txt)."""
    path = path or OUT
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 20), b""):
            h.update(blk)
    ver = subprocess.run([_hipcc(), "--version"], capture_output=True, text=True).stdout.strip().splitlines()
    src = hashlib.sha256()
    for f in _sources() + sorted(x for x in os.listdir(HERE) if x.endswith(".h")) + ["../../include/mfpa.h"]:
        with open(os.path.join(HERE, f), "rb") as fh:
            src.update(f.encode() + b"\0" + fh.read())
    return {"library": os.path.relpath(path, os.path.dirname(PKG)), "sha256": h.hexdigest(), "bytes": os.path.getsize(path),
            "sources_sha256": src.hexdigest(), "hipcc": " | ".join(v for v in ver[:2]), "flags": " ".join(COMMON),
            "per_file_flags": {k: " ".join(v) for k, v in PER_FILE.items()}}


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
