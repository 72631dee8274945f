"""CPU: the entry points of csrc/transforms.hip through ctypes (mfpa_rfft_plan and mfpa_rfft_twiddles are host functions; the two
launchers check their arguments before any launch and never dereference a pointer on the host), the ops wrappers without a GPU,
and the combinators with stub transforms."""
import ctypes
import os
import random
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_bandpass_taps", "mfpa_rfft_plan", "mfpa_rfft_twiddles", "mfpa_colored_noise")
CAP = 16384                                   # MFPA_RFFT_MAX_N: 8 bytes per complex point, N/2 points, one 64 KiB LDS buffer


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _plan(h, N):
    radices = (ctypes.c_int * 16)(*([-1] * 16))
    n, lds = ctypes.c_int(-1), ctypes.c_int(-1)
    rc = h.mfpa_rfft_plan(N, ctypes.addressof(radices), ctypes.addressof(n), ctypes.addressof(lds))
    return rc, list(radices), n.value, lds.value


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive


def test_the_cap_is_the_lds_buffer(lib):
    from musicfpaugment_amd import ops
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    assert int(re.search(r"#define MFPA_RFFT_MAX_N (\d+)", header).group(1)) == CAP == ops.RFFT_MAX_N
    assert int(re.search(r"#define MFPA_RFFT_MAX_RADICES (\d+)", header).group(1)) == 16 == ops.RFFT_MAX_RADICES
    rc, _, _, lds = _plan(lib.lib(), CAP)
    assert rc == 0 and lds == (CAP // 2) * 8 + 64 and (CAP // 2) * 8 == 64 * 1024
    assert lds <= 160 * 1024                                            # what one workgroup of a CDNA4 compute unit may hold


@pytest.mark.parametrize("N", [4, 6, 8, 10, 12, 20, 30, 600, 1000, 8000, 16000, CAP])
def test_plan_accepts_and_its_radices_multiply_to_half_n(lib, N):
    rc, radices, n, lds = _plan(lib.lib(), N)
    assert rc == 0 and 1 <= n <= 16 and lds > 0
    assert all(r in (2, 3, 4, 5) for r in radices[:n]) and all(r == 0 for r in radices[n:])
    assert int(np.prod(radices[:n])) == N // 2
    assert radices[:n] == sorted(radices[:n], key=lambda r: {5: 0, 3: 1, 4: 2, 2: 3}[r]) and radices[:n].count(2) <= 1


def test_plan_covers_every_radix_alone_and_in_pairs(lib):
    got = {N: tuple(_plan(lib.lib(), N)[1][:_plan(lib.lib(), N)[2]]) for N in (4, 6, 8, 10, 12, 20, 30, 24, 40)}
    assert got == {4: (2,), 6: (3,), 8: (4,), 10: (5,), 12: (3, 2), 20: (5, 2), 30: (5, 3), 24: (3, 4), 40: (5, 4)}


@pytest.mark.parametrize("N", [2, 0, 9, 14, 22, 8001, CAP + 2, 2 * CAP, -8, -16000, 44100])
def test_plan_refuses(lib, N):
    rc, radices, n, lds = _plan(lib.lib(), N)
    assert rc == lib.EINVAL and n == -1 and lds == -1 and radices == [-1] * 16        # nothing written


def test_plan_outputs_are_optional_and_ops_wraps_it(lib):
    from musicfpaugment_amd import ops
    assert lib.lib().mfpa_rfft_plan(8000, None, None, None) == 0
    assert ops.rfft_plan(8000) == ((5, 5, 5, 4, 4, 2), 65600)
    assert ops.rfft_plan(16000)[0] == (5, 5, 5, 4, 4, 4)
    for bad in (9, 14, 44100, CAP + 2, -4, 1 << 40):
        with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
            ops.rfft_plan(bad)


@pytest.mark.parametrize("N", [8, 30, 1000, 16000])
def test_twiddles_are_float64_values_rounded_once(lib, N):
    buf = np.full(2 * N + 4, np.nan, dtype=np.float32)
    assert lib.lib().mfpa_rfft_twiddles(N, buf.ctypes.data_as(ctypes.c_void_p)) == 0
    q = np.arange(N, dtype=np.float64)
    want = np.stack([np.cos(2 * np.pi * q / N), -np.sin(2 * np.pi * q / N)], axis=1).reshape(-1)
    assert np.all(np.abs(buf[:2 * N].astype(np.float64) - want) <= 2.0 ** -24 * np.abs(want) + 1e-15)
    assert buf[0] == 1.0 and buf[1] == 0.0 and np.all(np.isnan(buf[2 * N:]))
    assert lib.lib().mfpa_rfft_twiddles(N, None) == lib.EINVAL and lib.lib().mfpa_rfft_twiddles(14, buf.ctypes.data_as(ctypes.c_void_p)) == lib.EINVAL


def _noise(h, **kw):
    a = dict(white=8, B=3, N=8000, f_decay=8, T=16000, tw=8, out=8, stream=None)
    a.update(kw)
    return h.mfpa_colored_noise(a["white"], a["B"], a["N"], a["f_decay"], a["T"], a["tw"], a["out"], a["stream"])


@pytest.mark.parametrize("change", [dict(white=None), dict(f_decay=None), dict(tw=None), dict(out=None), dict(B=-1), dict(T=0),
                                    dict(T=-5), dict(N=9), dict(N=14), dict(N=2), dict(N=0), dict(N=-8000), dict(N=CAP + 2),
                                    dict(N=44100), dict(tw=12), dict(B=0, N=9), dict(B=0, T=0)], ids=str)
def test_colored_noise_rejects_before_any_launch(lib, change):
    assert _noise(lib.lib(), **change) == lib.EINVAL


def _taps(h, **kw):
    a = dict(lo=8, hi=8, half=8, off=8, B=3, taps=8, stream=None)
    a.update(kw)
    return h.mfpa_bandpass_taps(a["lo"], a["hi"], a["half"], a["off"], a["B"], a["taps"], a["stream"])


def test_bandpass_taps_rejects_and_empty_batches_are_no_ops(lib):
    h = lib.lib()
    for change in (dict(lo=None), dict(hi=None), dict(half=None), dict(off=None), dict(taps=None), dict(B=-1)):
        assert _taps(h, **change) == lib.EINVAL, change
    assert _taps(h, B=0) == 0 and _noise(h, B=0) == 0 and _noise(h, B=0, T=1, N=4) == 0


def test_no_cpu_fallback(lib):
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    with pytest.raises(MfpaError):                                         # host tensors are refused with or without a GPU
        ops.colored_noise(torch.zeros(2, 8000), torch.zeros(2), 100)
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    with pytest.raises(MfpaError):
        Gain(p=1.0)(torch.zeros(2, 1, 100))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            ops.bandpass_taps([0.1], [0.2])
        with pytest.raises(MfpaError):
            ops.rfft_twiddles(8000, "cuda")


# ----------------------------------------------------------------------------- the Python surface, no GPU
def test_every_import_path_of_the_reference_package():
    from musicfpaugment_amd.augmentation.composition import BaseCompose, Compose, OneOf, SomeOf  # noqa: F401
    from musicfpaugment_amd.augmentation.transform import (BaseWaveformTransform, EmptyPathException,  # noqa: F401
                                                           ModeNotSupportedException, MultichannelAudioNotSupportedException,
                                                           ObjectDict)
    from musicfpaugment_amd.augmentation.transformations.background_noise import AddBackgroundNoise  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.band_filters import BandPassFilter, BandStopFilter  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.colored_noise import AddColoredNoise  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.gain import Gain  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.impulse_response import ApplyImpulseResponse  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.pass_filters import HighPassFilter, LowPassFilter  # noqa: F401
    from musicfpaugment_amd.augmentation.transformations.peak_normalization import PeakNormalization  # noqa: F401
    d = ObjectDict(samples=1, sample_rate=2)
    assert d.samples == 1 and d["sample_rate"] == 2 and dict(**d) == {"samples": 1, "sample_rate": 2}
    d.samples = 5
    assert d["samples"] == 5
    with pytest.raises(AttributeError):
        d.missing


def test_constructors_validate_like_the_reference(lib):
    from musicfpaugment_amd.augmentation.transformations.band_filters import BandPassFilter, BandStopFilter
    from musicfpaugment_amd.augmentation.transformations.clipping import Clipping
    from musicfpaugment_amd.augmentation.transformations.colored_noise import AddColoredNoise
    from musicfpaugment_amd.augmentation.transformations.gain import Gain
    from musicfpaugment_amd.augmentation.transformations.pass_filters import HighPassFilter
    for make in (lambda: BandPassFilter(max_bandwidth_fraction=2.0), lambda: BandStopFilter(min_bandwidth_fraction=0.0),
                 lambda: BandPassFilter(min_center_frequency=500, max_center_frequency=400), lambda: Gain(3.0, 3.0),
                 lambda: Clipping(scope="song"), lambda: HighPassFilter(200.0, 100.0), lambda: AddColoredNoise(min_f_decay=3.0, sample_rate=8000),
                 lambda: AddColoredNoise(), lambda: AddColoredNoise(sample_rate=44100), lambda: AddColoredNoise(sample_rate=8001)):
        with pytest.raises(ValueError):
            make()
    with pytest.raises(ValueError, match="2\\^a 3\\^b 5\\^c"):
        AddColoredNoise(sample_rate=None)                                  # None means 44100 = 2 * 3^2 5^2 7^2
    t = AddColoredNoise(sample_rate=16000, p=0.25)
    assert t.p == 0.25 and t.noise_period == 16000
    t.p = 1.0
    assert t.p == 1.0 and float(t.bernoulli_distribution.probs) == 1.0     # p is a settable property
    with pytest.raises(RuntimeError, match="three-dimensional input tensors"):
        t(torch.zeros(4, 100), 16000)
    with pytest.warns(UserWarning, match="empty samples tensor"):
        empty = torch.zeros(0, 1, 100)
        assert t(empty, 16000).samples is empty
    from musicfpaugment_amd.augmentation.transform import MultichannelAudioNotSupportedException
    with pytest.raises(MultichannelAudioNotSupportedException, match="only supports mono audio"):
        t(torch.zeros(2, 2, 100), 16000)


def _stubs(n):
    from musicfpaugment_amd.augmentation.transform import BaseWaveformTransform, ObjectDict
    log = []

    class Stub(BaseWaveformTransform):
        def __init__(self, k):
            super().__init__(p=1.0)
            self.k = k

        def forward(self, samples, sample_rate=None):
            log.append(self.k)
            return ObjectDict(samples=samples * 10 + self.k, sample_rate=sample_rate)

    return [Stub(k) for k in range(1, n + 1)], log


def test_compose_applies_in_order_and_shuffle_permutes():
    from musicfpaugment_amd.augmentation.composition import Compose
    ts, log = _stubs(4)
    x = torch.zeros(1, 1, 2)
    out = Compose(ts)(x, sample_rate=8000)
    assert log == [1, 2, 3, 4] and out.samples.tolist() == [[[1234.0, 1234.0]]] and out.sample_rate == 8000
    c = Compose(ts, shuffle=True)
    seen = set()
    for seed in range(6):
        del log[:]
        random.seed(seed)
        c(x, 8000)
        want = [1, 2, 3, 4]
        random.seed(seed)
        random.shuffle(want)
        assert log == want
        seen.add(tuple(log))
    assert len(seen) > 1
    state = random.getstate()
    Compose(ts, p=0.0)(x)                                     # like the reference's, Compose stores p and draws nothing
    assert random.getstate() == state
    Compose(ts + [torch.nn.Identity()])(x)                    # not a transform: skipped


def test_some_of_and_one_of_pick_what_random_says():
    from musicfpaugment_amd.augmentation.composition import OneOf, SomeOf
    ts, log = _stubs(5)
    x = torch.zeros(1, 1, 2)
    counts = set()
    for seed in range(12):
        for comp, lo, hi in ((SomeOf((1, 3), ts, p=0.9), 1, 3), (OneOf(ts, p=0.9), 1, 1), (SomeOf((2, None), ts), 2, 5), (SomeOf(2, ts), 2, 2)):
            del log[:]
            random.seed(seed)
            out = comp(x, 8000)
            random.seed(seed)
            want = []
            if random.random() < comp.p:
                n = random.randint(lo, hi)
                want = sorted(random.sample(range(5), n))
                assert comp.transform_indexes == want
            assert log == [i + 1 for i in want]
            assert (out.samples is x) == (not want)
            counts.add((lo, hi, len(want)))
    assert {(1, 3, 1), (1, 3, 2), (1, 3, 3), (1, 1, 1), (1, 1, 0)} <= counts


def test_p_zero_returns_the_input_untouched_and_freeze_reaches_the_members():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    ts, log = _stubs(3)
    x = torch.ones(1, 1, 2)
    for comp in (SomeOf((1, 3), ts, p=0.0), OneOf(ts, p=0.0)):
        out = comp(x, 8000)
        assert out.samples is x and out.sample_rate == 8000 and log == [] and torch.equal(x, torch.ones(1, 1, 2))
    c = Compose([SomeOf(1, ts), ts[0]])
    c.freeze_parameters(7)
    a, b = random.random(), float(torch.rand(()))
    assert c.are_parameters_frozen and all(t.are_parameters_frozen for t in ts) and c.transforms[0].are_parameters_frozen
    c.freeze_parameters(7)
    assert (random.random(), float(torch.rand(()))) == (a, b)              # freeze reseeds `random` and torch
    c.unfreeze_parameters()
    assert not c.are_parameters_frozen and not any(t.are_parameters_frozen for t in ts)
