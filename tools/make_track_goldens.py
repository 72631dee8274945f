#!/usr/bin/env python3
"""Generate tests/golden/g17_track.npz with the REAL reference's Audfprint_peaks.find_peaks, peaks2landmarks, landmarks2hashes
and the unique / sort of wavfile2hashes (afp/audfprint/peak_extractor.py:236-346, :40-58, :443-460) on inputs LONGER than the
device's clip kernels take: 2041 frames (past 64 chunks of np.mean's reduction) and 1501 frames (past the LDS pruner).
Build-container only, like tools/make_goldens.py, whose import_reference() it reuses; the inputs are rebuilt from
musicfpaugment_amd.synth seeds (tests/_track_cases.py), only peak lists, hash rows and digests are written.

Usage:  python tools/make_track_goldens.py
"""
from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from make_goldens import OUT, import_reference  # noqa: E402
from musicfpaugment_amd import synth  # noqa: E402
from tests import _track_cases as tc  # noqa: E402


def main():
    import scipy
    ref = import_reference()
    pe = ref["pe"]
    analyzer = pe.Audfprint_peaks(ref["afp_settings"]["audfprint"])
    out = {"versions": np.array([f"numpy {np.__version__}", f"scipy {scipy.__version__}"])}
    for name, d in tc.g17_inputs().items():
        with contextlib.redirect_stdout(io.StringIO()):
            pklist, mask, _ = analyzer.find_peaks(d)
        assert mask.shape == (256, tc.G17_FRAMES[name]), mask.shape
        landmarks = analyzer.peaks2landmarks(pklist)
        hashes = pe.landmarks2hashes(landmarks)
        merged = (hashes[:, 0].astype(np.uint64) << 32) + hashes[:, 1].astype(np.uint64)          # wavfile2hashes, :448-458
        u = np.sort(np.unique(merged))
        rows = np.hstack([(u >> 32)[:, np.newaxis], (u & ((1 << 32) - 1))[:, np.newaxis]]).astype(np.int32)
        pk = np.array(pklist, dtype=np.int64).reshape(-1, 2)
        out[f"pklist_{name}"] = pk.astype(np.int16)
        out[f"rows_{name}"] = rows
        out[f"n_landmarks_{name}"] = np.int32(len(landmarks))
        out[f"n_samples_{name}"] = np.int32(len(d))
        out[f"digest_{name}"] = np.array(synth.digest(d))
        per_frame = np.bincount(pk[:, 0], minlength=mask.shape[1])
        print(f"  {name}: {mask.shape[1]} frames, {len(pk)} peaks (most in a frame {per_frame.max()}), {len(landmarks)} landmarks, "
              f"{len(rows)} unique rows")
    path = os.path.join(OUT, "g17_track.npz")
    np.savez_compressed(path, **out)
    print(f"g17_track.npz  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
