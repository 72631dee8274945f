"""CPU: argument checks of the whole-track entry points (mfpa_audfprint_pick_track, mfpa_audfprint_landmarks_track) through
ctypes.  Invalid arguments are rejected on the host before any launch and pointers are never dereferenced, so this runs without a
GPU (the style of tests/test_capi_abi.py)."""
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _pick(h, **kw):
    a = dict(spec=8, clip_max=8, B=1, F=257, T=2041, pole=0.98, gauss=8, a_dec=0.99, maxpks=5, logs=8, sums=8, events=8, mask=16,
             npeaks=8, stream=None)
    a.update(kw)
    return h.mfpa_audfprint_pick_track(a["spec"], a["clip_max"], a["B"], a["F"], a["T"], a["pole"], a["gauss"], a["a_dec"], a["maxpks"],
                                       a["logs"], a["sums"], a["events"], a["mask"], a["npeaks"], a["stream"])


def _landmarks(h, **kw):
    a = dict(mask=8, B=1, R=256, T=2041, cap=4096, mindt=2, targetdt=63, targetdf=31, maxpairs=3, tiles=8, landmarks=None, hashes=None,
             uniq=8, counts=8, stream=None)
    a.update(kw)
    return h.mfpa_audfprint_landmarks_track(a["mask"], a["B"], a["R"], a["T"], a["cap"], a["mindt"], a["targetdt"], a["targetdf"],
                                            a["maxpairs"], a["tiles"], a["landmarks"], a["hashes"], a["uniq"], a["counts"], a["stream"])


def test_abi_version_and_symbols(lib):
    h = lib.lib()
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47
    assert "mfpa_audfprint_pick_track" in lib.exported_symbols() and "mfpa_audfprint_landmarks_track" in lib.exported_symbols()


def test_empty_batch_is_a_no_op(lib):
    h = lib.lib()
    assert _pick(h, B=0) == 0 and _landmarks(h, B=0) == 0
    # ... whatever else is wrong: B == 0 comes first, as for every entry point
    assert _pick(h, B=0, spec=None, T=0, F=3) == 0
    assert _landmarks(h, B=0, mask=None, T=0, cap=0) == 0


@pytest.mark.parametrize("change", [dict(spec=None), dict(clip_max=None), dict(gauss=None), dict(logs=None), dict(sums=None),
                                    dict(events=None), dict(mask=None), dict(npeaks=None), dict(B=-1),
                                    dict(T=0), dict(T=-5), dict(T=16385), dict(T=1 << 20),
                                    dict(F=140), dict(F=258), dict(F=2), dict(F=256), dict(F=255), dict(F=254),   # (F - 1) % 4 != 0 inside [141, 257]
                                    dict(maxpks=0), dict(maxpks=9), dict(maxpks=-1), dict(events=12)],
                         ids=str)
def test_pick_track_rejects(lib, change):
    assert _pick(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", [dict(mask=None), dict(tiles=None), dict(uniq=None), dict(counts=None), dict(B=-1),
                                    dict(landmarks=8), dict(hashes=8),                                 # one list without the other
                                    dict(T=0), dict(T=16385), dict(R=0), dict(R=257), dict(R=260), dict(R=255), dict(R=254), dict(R=2),
                                    dict(cap=0), dict(cap=-1), dict(maxpairs=0), dict(maxpairs=5), dict(mindt=-1), dict(targetdt=0),
                                    dict(targetdt=257), dict(targetdf=-1)],
                         ids=str)
def test_landmarks_track_rejects(lib, change):
    assert _landmarks(lib.lib(), **change) == lib.EINVAL


def test_python_wrappers_refuse_cpu_tensors_and_bad_shapes(lib):
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    with pytest.raises(MfpaError):
        ops.audfprint_pick_track(torch.zeros(1, 257, 1600, dtype=torch.float64), torch.ones(1, dtype=torch.float64))
    with pytest.raises(MfpaError):
        ops.audfprint_landmarks_track(torch.zeros(1, 256, 1600, dtype=torch.uint8), 64)
    assert ops.TRACK_MAX_FRAMES == 16384


def test_switch_defaults_to_off_and_limits_are_named():
    import inspect

    import numpy as np
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.testing import audfprint_exps as ex
    assert inspect.signature(Audfprint_peaks.__init__).parameters["whole_tracks"].default is False
    assert inspect.signature(ex.create_fp_database_batch).parameters["whole_tracks"].default is False
    assert inspect.signature(ex.create_fp_database).parameters["whole_tracks"].default is False
    a = Audfprint_peaks(None, device="cpu")
    assert a.whole_tracks is False and not a._track_path(1 << 24)          # off: nothing changes, whatever the length
    a = Audfprint_peaks(None, device="cpu", whole_tracks=True)
    assert not a._track_path(64000) and not a._track_path(1433 * 256 + 255)   # up to 1434 frames: the clip kernels
    assert a._track_path(1434 * 256) and a._track_path(1500 * 256) and a._track_path(16383 * 256 + 255)
    with pytest.raises(ValueError, match="16384.*14 time bits"):
        a._track_path(16384 * 256)
    with pytest.raises(ValueError, match="1500"):
        ex._check_track_length(1500 * 256, "t")
    ex._check_track_length(16383 * 256, "t", whole_tracks=True)
    with pytest.raises(ValueError, match="16384.*14 time bits"):
        ex._check_track_length(16384 * 256, "t", whole_tracks=True)
    with pytest.raises(ValueError, match="16384"):                          # checked before any device work
        ex.create_fp_database_batch([np.zeros(16384 * 256, np.float32)], ["long"], device="cpu", whole_tracks=True)
