"""CPU: the complex-STFT / inverse-STFT entry points (mfpa_stft_complex, mfpa_istft, mfpa_istft_envelope_min) through ctypes.
mfpa_istft_envelope_min is a host function; the other two check their arguments before any launch and never dereference a pointer
on the host, so all of this runs without a GPU (the style of tests/test_capi_resample.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import _istft_oracle as io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mfpa_stft_complex", "mfpa_istft", "mfpa_istft_envelope_min")
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _istft(h, **kw):
    a = dict(spec=P, mag=None, mag_dtype=0, denom=None, flags=0, B=2, n_frames=4, length=800, tables=P, out=P, out_dtype=0, stream=None)
    a.update(kw)
    return h.mfpa_istft(a["spec"], a["mag"], a["mag_dtype"], a["denom"], a["flags"], a["B"], a["n_frames"], a["length"], a["tables"],
                        a["out"], a["out_dtype"], a["stream"])


def _envelope_min(h, win, n_frames, length):
    out = ctypes.c_double(-1.0)
    rc = h.mfpa_istft_envelope_min(None if win is None else win.ctypes.data_as(ctypes.c_void_p), n_frames, length, ctypes.addressof(out))
    return rc, out.value


def test_symbols_header_and_abi_version(lib):
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name in NEW:
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name), name
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive
    from musicfpaugment_amd import ops
    assert int(re.search(r"#define MFPA_ISTFT_CLAMP (\d+)", header).group(1)) == ops.ISTFT_CLAMP == 1


def test_envelope_minimum(lib):
    h = lib.lib()
    w = io.window()
    rc, m = _envelope_min(h, w, 251, 64000)
    assert rc == 0 and m == pytest.approx(0.5030853576634366, rel=1e-15) and m == io.envelope_min(w, 251, 64000)
    rc, m = _envelope_min(h, w, 2, 511)          # the last hop lies under one frame only: the window's thin tail, squared
    assert rc == 0 and m == pytest.approx(2.2501246633972162e-08, rel=1e-15) and m == io.envelope_min(w, 2, 511)
    for nF, length in ((2, 256), (2, 257), (3, 600), (4, 1000), (34, 8548), (94, 24000)):
        rc, m = _envelope_min(h, w, nF, length)
        assert rc == 0 and m == io.envelope_min(w, nF, length), (nF, length)
    assert _envelope_min(h, np.zeros(512), 3, 600) == (0, 0.0)
    from musicfpaugment_amd import ops
    assert ops.istft_envelope_min(w, 251, 64000) == io.envelope_min(w, 251, 64000)


def test_envelope_minimum_rejects(lib):
    h = lib.lib()
    w = io.window()
    assert _envelope_min(h, None, 3, 600)[0] == lib.EINVAL
    assert h.mfpa_istft_envelope_min(w.ctypes.data_as(ctypes.c_void_p), 3, 600, None) == lib.EINVAL
    for nF, length in ((1, 100), (0, 0), (-1, 10), (3, 511), (3, 768), (3, -1), (2, 255), (2, 512)):
        assert _envelope_min(h, w, nF, length)[0] == lib.EINVAL, (nF, length)


@pytest.mark.parametrize("change", [dict(spec=None), dict(tables=None), dict(out=None), dict(spec=P + 8), dict(n_frames=1, length=100),
                                    dict(n_frames=0, length=0), dict(length=767), dict(length=1024), dict(length=-1),
                                    dict(n_frames=1 << 23, length=-(1 << 31)), dict(mag=P, mag_dtype=2), dict(mag_dtype=-1),
                                    dict(out_dtype=2), dict(out_dtype=-1), dict(flags=2), dict(flags=3), dict(flags=-1), dict(B=-1),
                                    dict(B=65536)], ids=str)
def test_istft_rejects_before_any_launch(lib, change):
    assert _istft(lib.lib(), **change) == lib.EINVAL


def test_istft_takes_every_length_of_its_frame_count_and_empty_batches(lib):
    h = lib.lib()
    for length in (768, 769, 1023):
        assert _istft(h, B=0, length=length) == 0
    assert _istft(h, B=0, spec=None, tables=None, out=None) == 0 and _istft(h, B=0, mag=P, mag_dtype=1, denom=P, flags=1, out_dtype=1) == 0
    assert _istft(h, B=0, length=1024) == lib.EINVAL and _istft(h, B=0, flags=2) == lib.EINVAL      # ... but a bad shape is still an error


def test_stft_complex_argument_rules_are_those_of_stft_mag(lib):
    h = lib.lib()
    assert h.mfpa_stft_complex(P, 2, 100, P, P, None, 0, None, None) == lib.EINVAL        # T_w <= 256
    assert h.mfpa_stft_complex(P, 2, 256, P, P, None, 0, None, None) == lib.EINVAL
    assert h.mfpa_stft_complex(None, 2, 8000, P, P, None, 0, None, None) == lib.EINVAL
    assert h.mfpa_stft_complex(P, 2, 8000, None, P, None, 0, None, None) == lib.EINVAL
    assert h.mfpa_stft_complex(P, 2, 8000, P, None, None, 0, None, None) == lib.EINVAL
    assert h.mfpa_stft_complex(P, 2, 8000, P, P + 8, None, 0, None, None) == lib.EINVAL    # complex128 elements are 16-byte aligned
    assert h.mfpa_stft_complex(P, -1, 8000, P, P, None, 0, None, None) == lib.EINVAL
    assert h.mfpa_stft_complex(P, 2, 8000, P, P, P, 2, None, None) == lib.EINVAL          # dtype
    assert h.mfpa_stft_complex(None, 0, 8000, None, None, None, 0, None, None) == 0       # empty batch is a no-op


def test_no_cpu_fallback():
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.training.unet import UNet
    with pytest.raises(MfpaError):
        ops.stft_complex(torch.zeros(1, 8000))
    with pytest.raises(MfpaError):
        ops.istft(torch.zeros(1, 257, 4, dtype=torch.complex128))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            UNet(1, 1).eval().denoise_waveform(torch.zeros(1, 8000))
