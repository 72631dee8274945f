"""CPU: the room-simulator entry points (mfpa_rir_shoebox, mfpa_rir_image_count) through ctypes.  mfpa_rir_image_count is a host
function; mfpa_rir_shoebox checks its arguments before any launch and never dereferences a pointer on the host, so all of this runs
without a GPU (the style of tests/test_capi_iir.py).  The Python refusals of ops.simulate_rir, functional and RoomReverb need none
either."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_rir_shoebox", "mfpa_rir_image_count")
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced
ROOM, SRC, MIC = [5.2, 4.1, 2.7], [1.3, 2.9, 1.1], [3.7, 0.8, 1.6]


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _shoebox(h, **kw):
    a = dict(geom=P, B=2, max_order=3, length=100, fs=8000.0, c=343.0, filter_len=81, reversed=0, out_f64=0, out=P, ldo=100, stream=None)
    a.update(kw)
    return h.mfpa_rir_shoebox(a["geom"], a["B"], a["max_order"], a["length"], a["fs"], a["c"], a["filter_len"], a["reversed"], a["out_f64"],
                              a["out"], a["ldo"], a["stream"])


def _count(h, N):
    out = ctypes.c_longlong(-7)
    return h.mfpa_rir_image_count(N, ctypes.addressof(out)), out.value


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive


def test_image_count(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    for N, want in ((0, 1), (1, 7), (2, 25), (7, 575), (17, 7175), (16, 6017), (32, 45825), (47, 142975), (128, 2829313)):
        assert _count(h, N) == (0, want) and ops.rir_image_count(N) == want, N
        i = np.arange(-N, N + 1)
        if N <= 32:
            assert want == int(np.count_nonzero(np.abs(i)[:, None, None] + np.abs(i)[None, :, None] + np.abs(i)[None, None, :] <= N))
    assert h.mfpa_rir_image_count(3, None) == lib.EINVAL
    for N in (-1, 129, 1 << 20):
        assert _count(h, N) == (lib.EINVAL, -7), N
        with pytest.raises(ValueError):
            ops.rir_image_count(N)
    with pytest.raises(ValueError):
        ops.rir_image_count(2.5)


@pytest.mark.parametrize("change", [dict(geom=None), dict(out=None), dict(geom=P + 4), dict(out=P + 2), dict(out=P + 4, out_f64=1), dict(B=-1),
                                    dict(B=65536), dict(max_order=-1), dict(max_order=129), dict(length=0), dict(length=-3),
                                    dict(length=262145, ldo=262145), dict(ldo=99), dict(ldo=-1), dict(filter_len=80), dict(filter_len=1),
                                    dict(filter_len=2), dict(filter_len=257), dict(filter_len=-81), dict(fs=0.0), dict(fs=-8000.0),
                                    dict(fs=math.inf), dict(fs=math.nan), dict(c=0.0), dict(c=-343.0), dict(c=math.inf), dict(c=math.nan),
                                    dict(reversed=2), dict(reversed=-1), dict(out_f64=2), dict(out_f64=-1)], ids=str)
def test_shoebox_rejects_before_any_launch(lib, change):
    assert _shoebox(lib.lib(), **change) == lib.EINVAL


def test_empty_batch_is_a_no_op_but_a_bad_shape_is_still_an_error(lib):
    h = lib.lib()
    assert _shoebox(h, B=0) == 0 and _shoebox(h, B=0, geom=None, out=None) == 0
    assert _shoebox(h, B=0, max_order=128, length=262144, ldo=262144, filter_len=255, reversed=1, out_f64=1) == 0
    for bad in (dict(max_order=129), dict(length=0), dict(ldo=99), dict(filter_len=82), dict(fs=0.0), dict(c=math.nan), dict(reversed=2)):
        assert _shoebox(h, B=0, **bad) == lib.EINVAL, bad
    from musicfpaugment_amd import ops
    if not torch.cuda.is_available():
        return
    assert ops.simulate_rir(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3)), 0.5, 3, 100, 8000).shape == (0, 100)


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation.transformations.room_reverb import RoomReverb

    def sim(room=ROOM, source=SRC, mic=MIC, absorption=0.3, max_order=3, length=100, sample_rate=8000, **kw):
        return ops.simulate_rir(room, source, mic, absorption, max_order, length, sample_rate, **kw)

    bad_calls = [dict(source=[0.0, 2.9, 1.1]), dict(source=[5.2, 2.9, 1.1]), dict(source=[1.3, 4.5, 1.1]), dict(mic=[3.7, 0.8, 2.7]),
                 dict(mic=[3.7, -0.1, 1.6]), dict(mic=SRC), dict(absorption=-0.01), dict(absorption=1.01),
                 dict(absorption=[0.1, 0.2, 0.3, 0.4, 0.5, 1.5]), dict(absorption=[0.1, 0.2, 0.3]), dict(absorption=math.nan),
                 dict(room=[5.2, 4.1]), dict(room=[5.2, 0.0, 2.7]), dict(room=[5.2, math.inf, 2.7]), dict(source=[[1.3, 2.9, 1.1]] * 2),
                 dict(room=[ROOM, ROOM], source=[SRC, [6.0, 1.0, 1.0]], mic=[MIC, MIC]), dict(max_order=-1), dict(max_order=129),
                 dict(max_order=2.5), dict(length=0), dict(length=262145), dict(sample_rate=0), dict(sample_rate=math.inf),
                 dict(sound_speed=0.0), dict(sound_speed=math.nan), dict(filter_len=80), dict(filter_len=1), dict(filter_len=257),
                 dict(out_dtype=torch.float16), dict(room=np.tile(ROOM, (65536, 1)), source=np.tile(SRC, (65536, 1)), mic=np.tile(MIC, (65536, 1)))]
    for bad in bad_calls:
        with pytest.raises(ValueError):
            sim(**bad)
    g = ops.rir_geometry([ROOM, ROOM], [SRC, SRC], MIC, 0.25)
    assert g.shape == (2, 15) and g.dtype == np.float64
    np.testing.assert_array_equal(g[1], ROOM + SRC + MIC + [0.25] * 6)
    np.testing.assert_array_equal(ops.rir_geometry(ROOM, SRC, MIC, [0.3, 0.25, 0.4, 0.15, 0.5, 0.2])[0, 9:], [0.3, 0.25, 0.4, 0.15, 0.5, 0.2])

    with pytest.raises(ValueError):
        F.simulate_rir_ism(ROOM, [0.0, 1.0, 1.0], MIC, 3, 0.3, 100, sample_rate=8000)
    with pytest.raises(ValueError):
        F.simulate_rir_ism(ROOM, SRC, MIC, 3, 0.3, 100, sample_rate=8000, delay_filter_length=80)
    with pytest.raises(TypeError):
        F.simulate_rir_ism(ROOM, SRC, MIC, 3, 0.3, 100)                                # the sample rate has no default
    V, S = 5.2 * 4.1 * 2.7, 2 * (5.2 * 4.1 + 4.1 * 2.7 + 5.2 * 2.7)
    assert F.eyring_absorption(ROOM, 0.3) == pytest.approx(1 - math.exp(-0.161 * V / (S * 0.3)), rel=1e-14)
    a = F.eyring_absorption([ROOM, [3.0, 2.5, 2.2]], [0.3, 0.1])
    assert a.shape == (2,) and a[0] == F.eyring_absorption(ROOM, 0.3) and a[1] == F.eyring_absorption([3.0, 2.5, 2.2], 0.1)
    assert [F.rir_max_order([3.0, 2.5, 2.2], t) for t in (0.1, 0.2, 0.3)] == [16, 32, 47]
    assert F.rir_max_order(ROOM, 0.3, sound_speed=270.0) == math.ceil(270.0 * 0.3 / 2.7)
    assert F.rir_max_order([ROOM, [3.0, 2.5, 2.2]], 0.3).tolist() == [39, 47]
    for bad in (0.0, -0.3, math.inf, math.nan, [0.1, 0.2, 0.3]):
        with pytest.raises(ValueError):
            F.eyring_absorption(ROOM, bad)
        with pytest.raises(ValueError):
            F.rir_max_order(ROOM, bad)
    for bad in ([5.2, 4.1], [5.2, -4.1, 2.7], [[ROOM]]):
        with pytest.raises(ValueError):
            F.eyring_absorption(bad, 0.3)
    with pytest.raises(ValueError):
        F.rir_max_order(ROOM, 0.3, sound_speed=0.0)

    RoomReverb()
    for bad in (dict(min_rt60=0.0), dict(min_rt60=0.4, max_rt60=0.3), dict(max_rt60=math.inf), dict(min_room_dim=(3.0, 2.5)),
                dict(min_room_dim=(3.0, 2.5, 5.0)), dict(min_room_dim=(0.0, 2.5, 2.2)), dict(min_wall_distance=0.0),
                dict(min_wall_distance=1.1), dict(max_order=-1), dict(max_order=129), dict(max_order=2.5)):
        with pytest.raises(ValueError):
            RoomReverb(**bad)


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.room_reverb import RoomReverb
    with pytest.raises(MfpaError):
        RoomReverb(p=1.0, sample_rate=8000)(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            ops.simulate_rir(ROOM, SRC, MIC, 0.3, 3, 100, 8000)
        with pytest.raises(MfpaError):
            F.simulate_rir_ism(ROOM, SRC, MIC, 3, 0.3, 100, sample_rate=8000)
