"""CPU: the phase-vocoder entry points (mfpa_phase_vocoder, mfpa_vocoder_frames) through ctypes.  mfpa_vocoder_frames is a host
function; mfpa_phase_vocoder checks its arguments before any launch and never dereferences a pointer on the host, so all of this
runs without a GPU (the style of tests/test_capi_istft.py)."""
import ctypes
import os
import re
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import _vocoder_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_phase_vocoder", "mfpa_vocoder_frames")
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _vocoder(h, **kw):
    a = dict(spec=P, B=2, n_frames=4, rates=P, out=P, ld_out=8, n_out=P, stream=None)
    a.update(kw)
    return h.mfpa_phase_vocoder(a["spec"], a["B"], a["n_frames"], a["rates"], a["out"], a["ld_out"], a["n_out"], a["stream"])


def _frames(h, n_frames, rate):
    out = ctypes.c_int(-7)
    return h.mfpa_vocoder_frames(n_frames, rate, ctypes.addressof(out)), out.value


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    from musicfpaugment_amd import ops
    assert int(re.search(r"#define MFPA_VOCODER_MAX_FRAMES (\d+)", header).group(1)) == ops.VOCODER_MAX_FRAMES == ops.TRACK_MAX_FRAMES == 16384


def test_vocoder_frames_is_the_length_of_arange(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    for n in (1, 2, 3, 4, 251, 16384):
        for r in (0.5, 0.7, 1.0, 1.3, 2.0, 300.0):
            want = len(np.arange(0, n, r))
            if want > 16384:
                assert _frames(h, n, r) == (lib.EINVAL, -7), (n, r)
                with pytest.raises(ValueError):
                    ops.vocoder_frames(n, r)
            else:
                assert _frames(h, n, r) == (0, want) and ops.vocoder_frames(n, r) == want == vo.frames(n, r), (n, r)


def test_vocoder_frames_rejects(lib):
    h = lib.lib()
    assert h.mfpa_vocoder_frames(4, 0.9, None) == lib.EINVAL
    for n, r in ((0, 1.0), (-1, 1.0), (16385, 2.0), (4, 0.0), (4, -0.5), (4, float("nan")), (4, float("inf")), (4, -float("inf")),
                 (4, 1e-300), (16384, 0.9999), (2, 1e-4)):
        assert _frames(h, n, r) == (lib.EINVAL, -7), (n, r)
    assert _frames(h, 16384, 1.0) == (0, 16384) and _frames(h, 8192, 0.5) == (0, 16384) and _frames(h, 1, 1e300) == (0, 1)


@pytest.mark.parametrize("change", [dict(spec=None), dict(rates=None), dict(out=None), dict(n_out=None), dict(spec=P + 8), dict(out=P + 8),
                                    dict(rates=P + 4), dict(n_out=P + 2), dict(B=-1), dict(B=65536), dict(n_frames=0), dict(n_frames=-3),
                                    dict(n_frames=16385), dict(ld_out=0), dict(ld_out=-1), dict(ld_out=16385),
                                    dict(n_frames=1 << 30, ld_out=1 << 30)], ids=str)
def test_phase_vocoder_rejects_before_any_launch(lib, change):
    assert _vocoder(lib.lib(), **change) == lib.EINVAL


def test_empty_batch_is_a_no_op_but_a_bad_shape_is_still_an_error(lib):
    h = lib.lib()
    assert _vocoder(h, B=0) == 0 and _vocoder(h, B=0, spec=None, rates=None, out=None, n_out=None) == 0
    assert _vocoder(h, B=0, n_frames=16384, ld_out=16384) == 0 and _vocoder(h, B=0, n_frames=1, ld_out=1) == 0
    assert _vocoder(h, B=0, n_frames=0) == lib.EINVAL and _vocoder(h, B=0, ld_out=16385) == lib.EINVAL


def test_host_side_refusals_need_no_gpu(lib):
    """Constructors check their geometry with host functions only."""
    from musicfpaugment_amd import transforms as tr
    from musicfpaugment_amd.augmentation.transformations.pitch_shift import PitchShift, transpositions
    from musicfpaugment_amd.augmentation.transformations.time_stretch import TimeStretch
    for bad in (dict(n_freq=201), dict(hop_length=128), dict(n_freq=513, hop_length=256)):
        with pytest.raises(NotImplementedError):
            tr.TimeStretch(**bad)
    ts = tr.TimeStretch()
    assert (ts.hop_length, ts.n_freq, ts.fixed_rate) == (256, 257, None)
    with pytest.raises(ValueError, match="If no fixed_rate is specified"):
        ts(torch.zeros(257, 4, dtype=torch.complex128))
    with pytest.raises(ValueError, match="must be complex type"):
        ts(torch.zeros(257, 4), 1.1)
    z = torch.zeros(2, 257, 4, dtype=torch.complex64)
    assert tr.TimeStretch(fixed_rate=1.0)(z) is z and ts(z, 1.0) is z               # rate 1: the input itself, like torchaudio
    a, b = tr.PitchShift(8000, 12), tr.PitchShift(8000, -1)
    assert (a.rate, a.ratio) == (0.5, Fraction(2, 1)) and b.ratio == Fraction(151, 160) and b.rate == 2.0 ** (1 / 12)
    with pytest.raises(ValueError):
        tr.PitchShift(8000, 2)                                                     # 8979 : 8000 -- more than 1024 phases
    s = tr.Speed(8000, 1.1)
    assert (s.source_sample_rate, s.target_sample_rate, s.resampler.orig_freq, s.resampler.new_freq) == (8800, 8000, 11, 10)
    c = transpositions(-4.0, 4.0, 16)
    assert len(c) == len(set(c)) == 36 and c[0] == Fraction(4, 5) and c[-1] == Fraction(5, 4) and Fraction(1) not in c
    assert all(f.denominator <= 16 and -4.0 <= 12 * np.log2(float(f)) <= 4.0 for f in c) and c == sorted(c)
    assert PitchShift(sample_rate=8000).candidates == c
    assert transpositions(-13.0, 13.0, 1) == [Fraction(2)] and transpositions(0.0, 12.0, 2) == [Fraction(3, 2), Fraction(2)]
    with pytest.raises(ValueError):
        PitchShift(min_transpose_semitones=0.05, max_transpose_semitones=0.1)
    with pytest.raises(ValueError):
        PitchShift(min_transpose_semitones=1.0, max_transpose_semitones=-1.0)
    with pytest.raises(ValueError):
        TimeStretch(min_rate=0.0)
    with pytest.raises(ValueError):
        TimeStretch(min_rate=1.2, max_rate=0.8)


def test_no_cpu_fallback():
    from musicfpaugment_amd import ops
    from musicfpaugment_amd import transforms as tr
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.pitch_shift import PitchShift
    from musicfpaugment_amd.augmentation.transformations.time_stretch import TimeStretch
    with pytest.raises(MfpaError):
        ops.phase_vocoder(torch.zeros(1, 257, 4, dtype=torch.complex128), 1.1)
    with pytest.raises(MfpaError):
        ops.time_stretch(torch.zeros(1, 8000), 1.1)
    with pytest.raises(MfpaError):
        ops.pitch_shift(torch.zeros(1, 8000), Fraction(9, 8))
    for t in (PitchShift(p=1.0, sample_rate=8000), TimeStretch(p=1.0, sample_rate=8000)):
        with pytest.raises(MfpaError):
            t(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            tr.TimeStretch(fixed_rate=1.1)(torch.zeros(257, 4, dtype=torch.complex128))
        with pytest.raises(MfpaError):
            tr.PitchShift(8000, 12)(torch.zeros(8000))
        with pytest.raises(MfpaError):
            tr.Speed(8000, 1.1)(torch.zeros(8000))
