"""CPU: the lossy-coding entry points (mfpa_transform_codec, mfpa_mulaw) through ctypes.  They check their arguments before any launch
and dereference no device pointer on the host (the band table IS a host array), so all of this runs without a GPU (the style of
tests/test_capi_delay.py).  The Python refusals of ops.transform_codec / mu_law, of the functional fronts and of the LossyCodec /
TelephoneChannel transforms need none either."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced
EDGES = (ctypes.c_int * 20)(0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 88, 104, 124, 148, 176, 208, 256)


def _edges(*values):
    a = (ctypes.c_int * len(values))(*values)
    return a


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _codec(h, **kw):
    a = dict(x=P, x_f64=0, ldx=100, B=2, T=100, rate=100.0, rates=None, edges=EDGES, n_bands=19, up=10.0, down=25.0, apply=None, y=P, y_f64=0,
             lam=None, coded=None, stream=None)
    a.update(kw)
    e = a["edges"]
    e = e if e is None or isinstance(e, int) else ctypes.addressof(e)
    return h.mfpa_transform_codec(a["x"], a["x_f64"], a["ldx"], a["B"], a["T"], a["rate"], a["rates"], e, a["n_bands"], a["up"], a["down"],
                                  a["apply"], a["y"], a["y_f64"], a["lam"], a["coded"], a["stream"])


def _mulaw(h, **kw):
    a = dict(x=P, x_f64=0, B=2, T=100, channels=256, mode=2, apply=None, y=P, y_f64=0, stream=None)
    a.update(kw)
    return h.mfpa_mulaw(a["x"], a["x_f64"], a["B"], a["T"], a["channels"], a["mode"], a["apply"], a["y"], a["y_f64"], a["stream"])


def test_symbols_header_constants_and_abi_version(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name, nargs in (("mfpa_transform_codec", 17), ("mfpa_mulaw", 10)):
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name)
        assert name in lib._SIGNATURES and len(lib._SIGNATURES[name][0]) == nargs
    assert int(re.search(r"#define MFPA_CODEC_FRAMES (\d+)", header).group(1)) == ops.CODEC_FRAMES
    assert int(re.search(r"#define MFPA_CODEC_MAX_BANDS (\d+)", header).group(1)) == ops.CODEC_MAX_BANDS == 32
    assert (ops.CODEC_FRAMES + 1) * 8 == 256                             # eight lanes per frame, four wavefronts
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive


CODEC_ERRORS = [dict(x=None), dict(y=None), dict(edges=None), dict(x=P + 2), dict(y=P + 2), dict(x=P + 4, x_f64=1), dict(y=P + 4, y_f64=1),
                dict(rates=P + 4), dict(lam=P + 4), dict(coded=P + 2), dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-5),
                dict(T=(1 << 30) + 1, ldx=1 << 31), dict(ldx=99), dict(x_f64=2), dict(y_f64=-1), dict(n_bands=0), dict(n_bands=-1), dict(n_bands=33),
                dict(n_bands=18), dict(edges=_edges(1, 256), n_bands=1), dict(edges=_edges(0, 255), n_bands=1), dict(edges=_edges(0, 257), n_bands=1),
                dict(edges=_edges(0, 100, 100, 256), n_bands=3), dict(edges=_edges(0, 100, 50, 256), n_bands=3), dict(edges=_edges(0, -5, 256), n_bands=2),
                dict(edges=_edges(0, 300, 256), n_bands=2), dict(rate=math.nan), dict(up=-1.0), dict(down=-0.5), dict(up=math.nan), dict(down=math.nan),
                dict(up=math.inf), dict(down=math.inf)]


@pytest.mark.parametrize("change", CODEC_ERRORS, ids=[str(i) + "-" + ",".join(c) for i, c in enumerate(CODEC_ERRORS)])
def test_transform_codec_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _codec(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", [dict(x=None), dict(y=None), dict(x=P + 2), dict(y=P + 2), dict(x=P + 4, x_f64=1), dict(y=P + 4, y_f64=1),
                                    dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-1), dict(T=(1 << 30) + 1), dict(channels=1),
                                    dict(channels=0), dict(channels=-256), dict(channels=65537), dict(mode=3), dict(mode=-1), dict(x_f64=2),
                                    dict(y_f64=2), dict(mode=0, y_f64=1), dict(mode=1, x_f64=1), dict(mode=0, apply=P), dict(mode=1, apply=P)],
                         ids=str)
def test_mulaw_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _mulaw(lib.lib(), **change) == lib.EINVAL


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    x = torch.zeros(2, 100)
    nan, inf = float("nan"), float("inf")
    for wav in (torch.zeros(100), torch.zeros(1, 2, 100), x.to(torch.float16), x.to(torch.int32), np.zeros((2, 100))):
        with pytest.raises(ValueError):
            ops.transform_codec(wav, 16.0)
        with pytest.raises(ValueError):
            ops.mu_law(wav)
        with pytest.raises(ValueError):
            ops.mu_law_encode(wav)
    for kw in (dict(kbps=nan), dict(kbps=-inf), dict(kbps=[8.0, nan]), dict(kbps=[8.0, 16.0, 32.0]), dict(kbps=[[8.0, 16.0]]), dict(kbps="fast"),
               dict(kbps=16.0, sample_rate=0), dict(kbps=16.0, sample_rate=nan), dict(kbps=16.0, side_bits=-1), dict(kbps=16.0, up_db=-1.0),
               dict(kbps=16.0, down_db=nan), dict(kbps=16.0, up_db=inf), dict(kbps=16.0, band_edges=[0, 256.5]), dict(kbps=16.0, band_edges=[0, 100]),
               dict(kbps=16.0, band_edges=[1, 256]), dict(kbps=16.0, band_edges=[0, 50, 50, 256]), dict(kbps=16.0, band_edges=[256]),
               dict(kbps=16.0, band_edges=list(range(0, 257, 4))), dict(kbps=16.0, band_edges=[[0, 256]]), dict(kbps=16.0, apply=[True]),
               dict(kbps=16.0, out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            ops.transform_codec(x, **kw)
    for kw in (dict(channels=1), dict(channels=65537), dict(channels=2.5), dict(apply=[True, False, True]), dict(out_dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.mu_law(x, **kw)
    for codes in (torch.zeros(2, 100), torch.zeros(2, 100, dtype=torch.int64), torch.zeros(100, dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.mu_law_decode(codes)
    with pytest.raises(ValueError):
        ops.mu_law_decode(torch.zeros(2, 100, dtype=torch.int32), out_dtype=torch.float16)
    calls = [lambda: F.transform_codec(x, 8000, nan), lambda: F.transform_codec(x, 8000, [8.0, 16.0]), lambda: F.transform_codec(x, 0, 16.0),
             lambda: F.transform_codec(x.to(torch.float16), 8000, 16.0), lambda: F.transform_codec(x, 8000, -inf),
             lambda: F.mu_law_encoding(x, 1), lambda: F.mu_law_encoding(x, 256.0), lambda: F.mu_law_encoding(x.long(), 256),
             lambda: F.mu_law_decoding(x, 256), lambda: F.mu_law_decoding(x.long(), 70000), lambda: F.mu_law_decoding(np.zeros(4, dtype=np.int64), 256)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} did not raise")
    assert ops.codec_bit_budget(8.0) == 256000.0 / 1000.0 - 114.0 and ops.codec_bit_budget(inf) == inf
    assert np.array_equal(ops.codec_bit_budget([8.0, 64.0], 16000, 4, 10), [128.0 - 40.0, 1024.0 - 40.0])
    assert ops.codec_band_edges([0, 128, 256]).dtype == np.int32 and ops.codec_frames(64000) == 251


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.codec import LossyCodec, TelephoneChannel
    x = torch.zeros(2, 100)
    with pytest.raises(MfpaError):
        ops.transform_codec(x, [8.0, math.inf], sample_rate=16000, band_edges=[0, 100, 256], apply=[True, False], return_stats=True)
    with pytest.raises(MfpaError):
        ops.mu_law(x.double(), 16, apply=[True, False], return_codes=True)
    with pytest.raises(MfpaError):
        ops.mu_law_encode(x)
    with pytest.raises(MfpaError):
        ops.mu_law_decode(torch.zeros(2, 100, dtype=torch.int32))
    for t in (LossyCodec(p=1.0, sample_rate=8000), TelephoneChannel(p=1.0, sample_rate=8000)):
        with pytest.raises(MfpaError):
            t(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        x3 = torch.zeros(3, 1, 100)
        for call in (lambda: F.transform_codec(x3, 8000, 16.0), lambda: F.mu_law_encoding(x3[0, 0]), lambda: F.mu_law_decoding(x3.long())):
            with pytest.raises(MfpaError):
                call()


def test_transforms_construct_name_their_parameters_and_compose():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.codec import LossyCodec, TelephoneChannel
    c, t = LossyCodec(), TelephoneChannel()
    assert (c.min_kbps, c.max_kbps, c.p, t.p) == (8.0, 64.0, 0.5, 0.5)
    assert (t.low_hz, t.high_hz, t.channels) == (300.0, 3400.0, 256) and t.cutoffs(8000) == (0.0375, 0.425)
    with pytest.raises(ValueError):
        t.cutoffs(6000)
    x = torch.zeros(6, 2000)
    torch.manual_seed(5)
    c.transform_parameters = {"should_apply": torch.tensor([True, False, True, True, False, True])}
    c.randomize_parameters(x, 8000)                                       # the draws are host work
    assert sorted(k for k in c.transform_parameters if k != "should_apply") == ["kbps"] and len(c.transform_parameters["kbps"]) == 4
    r = c.rates()
    assert r.shape == (6,) and r.dtype == np.float64 and np.all(r >= 8.0 * (1 - 1e-6)) and np.all(r <= 64.0 * (1 + 1e-6))
    torch.manual_seed(0)
    wide = LossyCodec(1.0, 1000.0)
    wide.transform_parameters = {"should_apply": torch.ones(4000, dtype=torch.bool)}
    wide.randomize_parameters(torch.zeros(4000, 10), 8000)
    assert abs(float(np.median(wide.rates())) - math.sqrt(1000.0)) < 4.0   # log-uniform: the median is the geometric mean
    for bad in (dict(min_kbps=0.0), dict(min_kbps=-1.0), dict(min_kbps=100.0), dict(max_kbps=math.inf)):
        with pytest.raises(ValueError):
            LossyCodec(**bad)
    chain = Compose([LossyCodec(p=1.0), SomeOf((1, 2), [TelephoneChannel(p=1.0), LossyCodec(p=1.0)]), OneOf([TelephoneChannel(), LossyCodec()])])
    assert len(chain.transforms) == 3
