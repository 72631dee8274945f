"""CPU: the loudness entry points (mfpa_loudness_segments, mfpa_loudness_work, mfpa_loudness_gate, mfpa_loudness_apply) through ctypes.
They check their arguments before any launch and dereference no device pointer on the host, so all of this runs without a GPU (the
style of tests/test_capi_denoise.py).  The Python refusals of ops.loudness*, functional.loudness* and LoudnessNormalization need none
either."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced
nan, inf = math.nan, math.inf


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _segments(h, **kw):
    a = dict(x=P, x_f64=0, R=2, T=4000, sos=P, S=2, hop=800, work=P, work_len=512, seg=P, peak=None, stream=None)
    a.update(kw)
    return h.mfpa_loudness_segments(a["x"], a["x_f64"], a["R"], a["T"], a["sos"], a["S"], a["hop"], a["work"], a["work_len"], a["seg"], a["peak"],
                                    a["stream"])


def _gate(h, **kw):
    a = dict(seg=P, B=2, C=2, nseg=50, hop=800, win=4, weights=None, p_abs=1e-7, rel=0.1, power=P, counts=P, blocks=None, range=None, stream=None)
    a.update(kw)
    return h.mfpa_loudness_gate(a["seg"], a["B"], a["C"], a["nseg"], a["hop"], a["win"], a["weights"], a["p_abs"], a["rel"], a["power"],
                                a["counts"], a["blocks"], a["range"], a["stream"])


def _apply(h, **kw):
    a = dict(x=P, x_f64=0, B=2, C=2, T=4000, gated=P, target=P, peak=None, peak_limit=0.0, apply=None, y=P, gain=None, stream=None)
    a.update(kw)
    return h.mfpa_loudness_apply(a["x"], a["x_f64"], a["B"], a["C"], a["T"], a["gated"], a["target"], a["peak"], a["peak_limit"], a["apply"],
                                 a["y"], a["gain"], a["stream"])


def test_symbols_header_constants_and_abi_version(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name, nargs in (("mfpa_loudness_segments", 12), ("mfpa_loudness_work", 2), ("mfpa_loudness_gate", 14), ("mfpa_loudness_apply", 13)):
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name)
        assert len(lib._SIGNATURES[name][0]) == nargs
        proto = re.search(r"^int\s+" + name + r"\s*\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == nargs, name
    for macro, value in (("MFPA_LOUDNESS_MAX_CHANNELS", ops.LOUDNESS_MAX_CHANNELS), ("MFPA_LOUDNESS_MAX_WINDOW", ops.LOUDNESS_MAX_WINDOW),
                         ("MFPA_LOUDNESS_MAX_RANGE_BLOCKS", ops.LOUDNESS_MAX_RANGE_BLOCKS)):
        assert int(re.search(r"#define " + macro + r" (\d+)", header).group(1)) == value
    assert ops.LOUDNESS_MAX_RANGE_BLOCKS >= 16384 and ops.LOUDNESS_MAX_CHANNELS == 8 and ops.LOUDNESS_MAX_WINDOW == 64
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    from musicfpaugment_amd.csrc import build as b
    assert b.PER_FILE["loudness.hip"] == ["-ffp-contract=off"] and b.PER_FILE["iir.hip"] == ["-ffp-contract=off"]


def test_work_length(lib):
    h = lib.lib()
    n = ctypes.c_longlong(-1)
    for S in range(9):
        assert h.mfpa_loudness_work(S, ctypes.addressof(n)) == 0 and n.value == S * 256
    m = ctypes.c_longlong(-1)
    assert h.mfpa_sosfilt_work(1, 2, 0, ctypes.addressof(m)) == 0 and m.value == 512          # the same table as mfpa_sosfilt's
    for bad in (-1, 9):
        assert h.mfpa_loudness_work(bad, ctypes.addressof(n)) == lib.EINVAL
    assert h.mfpa_loudness_work(2, None) == lib.EINVAL


SEGMENT_ERRORS = [dict(R=-1), dict(R=65536), dict(T=0), dict(T=-5), dict(T=2 ** 30 + 1), dict(S=-1), dict(S=9, work_len=9 * 256), dict(hop=0),
                  dict(hop=-3), dict(hop=2 ** 24 + 1), dict(x_f64=2), dict(x_f64=-1), dict(work_len=511), dict(x=None), dict(seg=None),
                  dict(sos=None), dict(work=None), dict(x=P + 2), dict(x=P + 4, x_f64=1), dict(sos=P + 4), dict(work=P + 4), dict(seg=P + 4),
                  dict(peak=P + 4)]
GATE_ERRORS = [dict(B=-1), dict(B=65536), dict(C=0), dict(C=9), dict(nseg=-1), dict(nseg=2 ** 30 + 1), dict(hop=0), dict(hop=2 ** 24 + 1),
               dict(win=0), dict(win=65), dict(p_abs=-1.0), dict(p_abs=nan), dict(p_abs=inf), dict(rel=-0.1), dict(rel=nan), dict(rel=inf),
               dict(range=P, nseg=16384 + 4), dict(range=P, nseg=16384 + 30, win=30), dict(seg=None), dict(power=None), dict(counts=None),
               dict(seg=P + 4), dict(weights=P + 4), dict(power=P + 4), dict(counts=P + 2), dict(blocks=P + 4), dict(range=P + 4)]
APPLY_ERRORS = [dict(B=-1), dict(B=65536), dict(C=0), dict(C=9), dict(B=32768, C=2), dict(T=0), dict(T=2 ** 30 + 1), dict(x_f64=2),
                dict(peak_limit=-1.0), dict(peak_limit=nan), dict(peak_limit=inf), dict(peak_limit=1.0), dict(peak=P), dict(x=None),
                dict(y=None), dict(gated=None), dict(target=None), dict(x=P + 2), dict(y=P + 2), dict(x=P + 4, x_f64=1), dict(y=P + 4, x_f64=1),
                dict(gated=P + 4), dict(target=P + 4), dict(peak=P + 4, peak_limit=1.0), dict(gain=P + 4)]


def _ids(errors):
    return [str(i) + "-" + ",".join(c) for i, c in enumerate(errors)]


@pytest.mark.parametrize("change", SEGMENT_ERRORS, ids=_ids(SEGMENT_ERRORS))
def test_segments_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _segments(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", GATE_ERRORS, ids=_ids(GATE_ERRORS))
def test_gate_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _gate(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", APPLY_ERRORS, ids=_ids(APPLY_ERRORS))
def test_apply_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _apply(lib.lib(), **change) == lib.EINVAL


def test_empty_batches_are_ok_without_a_launch(lib):
    h = lib.lib()
    assert _segments(h, R=0, x=None, seg=None, sos=None, work=None) == 0
    assert _gate(h, B=0, seg=None, power=None, counts=None) == 0
    assert _apply(h, B=0, x=None, y=None, gated=None, target=None) == 0
    assert _gate(h, B=0, range=P, nseg=16384 + 3) == 0 and _gate(h, B=0, range=P, nseg=16384 + 4) == lib.EINVAL       # the cap is nb = 16384


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation.transformations.loudness import LoudnessNormalization
    x = torch.zeros(2, 2, 8000)
    for bad in (torch.zeros(8000), torch.zeros(2, 9, 100), torch.zeros(2, 2, 0), torch.zeros(2, 2, 100, dtype=torch.float16), np.zeros((2, 100))):
        with pytest.raises(ValueError):
            ops.loudness(bad, 8000)
    for call in (lambda: ops.loudness(x, 0), lambda: ops.loudness(x, nan), lambda: ops.loudness(x, 8000, design="x"),
                 lambda: ops.loudness(x, 8000, weights=[1.0]), lambda: ops.loudness(x, 8000, weights=[1.0, -1.0]),
                 lambda: ops.loudness(x, 8000, weights=[1.0, nan]), lambda: ops.loudness_curve(x, 8000, "long"),
                 lambda: ops.loudness_normalize(x, 8000, nan), lambda: ops.loudness_normalize(x, 8000, [-23.0]),
                 lambda: ops.loudness_normalize(x, 8000, -23.0, peak_limit=0.0), lambda: ops.loudness_normalize(x, 8000, -23.0, peak_limit=inf),
                 lambda: ops.loudness_normalize(x, 8000, -23.0, apply=[True]), lambda: ops.loudness_segments(x, None, 0),
                 lambda: ops.loudness_segments(x, None, 2 ** 24 + 1), lambda: ops.loudness_segments(x, np.zeros((9, 6)), 100),
                 lambda: ops.loudness_segments(x, np.zeros((2, 2, 6)), 100), lambda: ops.loudness_segments(x.half(), None, 100),
                 lambda: ops.loudness_gate(torch.zeros(2, 50), 800), lambda: ops.loudness_gate(torch.zeros(2, 50, dtype=torch.float64), 0),
                 lambda: ops.loudness_gate(torch.zeros(2, 50, dtype=torch.float64), 800, win=65),
                 lambda: ops.loudness_gate(torch.zeros(2, 50, dtype=torch.float64), 800, rel=-1.0),
                 lambda: ops.loudness_gate(torch.zeros(2, 9, 50, dtype=torch.float64), 800),
                 lambda: ops.loudness_gate(torch.zeros(1, 1, 16384 + 30, dtype=torch.float64), 800, win=30, want_range=True),
                 lambda: ops.true_peak(x.double()), lambda: ops.true_peak(x, 0), lambda: F.loudness(torch.zeros(100), 8000),
                 lambda: F.loudness(x, -1), lambda: F.loudness_normalize(x, 8000, nan)):
        with pytest.raises(ValueError):
            call()
    assert ops.loudness_hop(48000) == 4800 and ops.loudness_hop(44100) == 4410 and ops.loudness_hop(22050) == 2205 and ops.loudness_hop(11025) == 1103
    assert ops.loudness_power(-70.0) == 10.0 ** ((-70.0 + 0.691) / 10.0)
    assert ops.loudness_power([-23.0, -14.0]).shape == (2,)
    for bad in (dict(min_lufs=-10.0, max_lufs=-20.0), dict(min_lufs=-inf), dict(max_lufs=nan)):
        with pytest.raises(ValueError):
            LoudnessNormalization(**bad)


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.loudness import LoudnessNormalization
    x = torch.zeros(2, 2, 8000)
    for call in (lambda: ops.loudness(x, 8000), lambda: ops.loudness_curve(x, 8000), lambda: ops.loudness_range(x, 8000),
                 lambda: ops.loudness_normalize(x, 8000, -23.0), lambda: ops.true_peak(x), lambda: ops.loudness_segments(x, None, 800),
                 lambda: ops.loudness_gate(torch.zeros(2, 2, 50, dtype=torch.float64), 800),
                 lambda: LoudnessNormalization(p=1.0)(torch.zeros(2, 1, 8000), 8000)):
        with pytest.raises(MfpaError):
            call()
    if not torch.cuda.is_available():
        for call in (lambda: F.loudness(x, 8000), lambda: F.loudness_range(x, 8000), lambda: F.loudness_normalize(x, 8000, -23.0)):
            with pytest.raises(MfpaError):
                call()


def test_transform_constructs_names_its_parameters_and_composes():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.loudness import LoudnessNormalization
    t = LoudnessNormalization()
    assert (t.min_lufs, t.max_lufs, t.p) == (-31.0, -13.0, 0.5)
    torch.manual_seed(5)
    t.transform_parameters = {"should_apply": torch.tensor([True, False, True, True, False, True])}
    t.randomize_parameters(torch.zeros(6, 2000), 8000)                   # the draw is host work
    assert sorted(k for k in t.transform_parameters if k != "should_apply") == ["lufs"] and len(t.transform_parameters["lufs"]) == 4
    f = t.targets()
    assert f.shape == (6,) and f.dtype == np.float64 and np.all(f >= -31.0) and np.all(f <= -13.0) and len(set(f.tolist())) == 6
    chain = Compose([LoudnessNormalization(p=1.0), SomeOf((1, 2), [LoudnessNormalization(p=1.0), LoudnessNormalization()]),
                     OneOf([LoudnessNormalization(), LoudnessNormalization()])])
    assert len(chain.transforms) == 3
