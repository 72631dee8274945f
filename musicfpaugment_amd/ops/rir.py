"""Room impulse responses of shoebox rooms by the image-source method (csrc/rir.hip)."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .._lib import check, lib, ptr, stream
from ._args import _current_gpu, _host_f64, _out_dtype, _sample_rate, _upload


RIR_MAX_ORDER = 128
RIR_MAX_LENGTH = 262144
RIR_MAX_FILTER = 255
RIR_MAX_ROOMS = 65535


def rir_image_count(max_order: int) -> int:
    """Images of a shoebox room up to reflection order N = max_order: (2N + 1)(2N^2 + 2N + 3) / 3 (host arithmetic, no GPU).
    ValueError: an order outside [0, 128]."""
    if int(max_order) != max_order:
        raise ValueError(f"max_order must be an integer, got {max_order}")
    n = ctypes.c_longlong(0)
    check(lib().mfpa_rir_image_count(int(max_order), ctypes.addressof(n)), "mfpa_rir_image_count")
    return n.value


def rir_geometry(room, source, mic, absorption) -> np.ndarray:
    """(B, 15) float64 on the host: room, source, mic, absorption, what mfpa_rir_shoebox reads.  room, source and mic are (B, 3) (or
    (3,) for one room), absorption (B, 6), (6,) or a scalar: energy coefficients of the walls x0 x1 y0 y1 z0 z1.  ValueError: another
    shape, a value that is not finite, a room side that is not positive, a point not strictly inside its room, a coefficient outside
    [0, 1], source and microphone at the same point."""
    room, source, mic, absorption = (_host_f64(v, n) for v, n in ((room, "room"), (source, "source"), (mic, "mic"),
                                                                   (absorption, "absorption")))
    if room.ndim == 1:
        room = room[None]
    if room.ndim != 2 or room.shape[1] != 3:
        raise ValueError(f"room must be (B, 3), got {room.shape}")
    B = room.shape[0]
    try:
        source, mic = np.broadcast_to(source, (B, 3)), np.broadcast_to(mic, (B, 3))
        absorption = np.broadcast_to(absorption, (B, 6))
    except ValueError:
        raise ValueError(f"source and mic must be ({B}, 3) and absorption ({B}, 6), (6,) or a scalar, got {source.shape}, {mic.shape}, "
                         f"{absorption.shape}") from None
    geom = np.ascontiguousarray(np.concatenate([room, source, mic, absorption], axis=1))
    if not np.all(np.isfinite(geom)):
        raise ValueError("the geometry holds a value that is not finite")
    if not np.all(room > 0.0):
        raise ValueError("every room side must be positive")
    for name, pt in (("source", source), ("microphone", mic)):
        if not np.all((pt > 0.0) & (pt < room)):
            raise ValueError(f"the {name} must lie strictly inside its room")
    if not np.all((absorption >= 0.0) & (absorption <= 1.0)):
        raise ValueError("absorption coefficients must lie in [0, 1]")
    if np.any(np.all(source == mic, axis=1)):
        raise ValueError("source and microphone at the same point")
    return geom


def simulate_rir(room, source, mic, absorption, max_order: int, length: int, sample_rate: float, *, sound_speed: float = 343.0,
                 filter_len: int = 81, reversed: bool = False, out_dtype=torch.float32, device="cuda") -> torch.Tensor:
    """Impulse responses of B shoebox rooms by the image-source method (Allen and Berkley), (B, length) of `out_dtype` (float32 or
    float64; float32 is the float64 result rounded once) on the GPU, in one launch.  The geometry is given on the host (see
    rir_geometry) and uploaded once.  Every image with |ix| + |iy| + |iz| <= max_order adds amp w(k - tau) sinc(k - tau) with
    amp = gain / (4 pi d), tau = d sample_rate / sound_speed and a Hann window of `filter_len` (odd) taps; taps outside
    [0, length) are dropped.  reversed=True returns every row time-reversed: the taps mfpa_fir wants for this response.
    ValueError: the geometry's, max_order outside [0, 128], length outside [1, 262144], filter_len even or outside [3, 255], a
    sample_rate or sound_speed that is not finite and positive, more than 65535 rooms."""
    geom = rir_geometry(room, source, mic, absorption)
    B = geom.shape[0]
    if int(max_order) != max_order or not 0 <= max_order <= RIR_MAX_ORDER:
        raise ValueError(f"max_order must be an integer in [0, {RIR_MAX_ORDER}], got {max_order}")
    if int(length) != length or not 1 <= length <= RIR_MAX_LENGTH:
        raise ValueError(f"length must be an integer in [1, {RIR_MAX_LENGTH}], got {length}")
    if int(filter_len) != filter_len or not 3 <= filter_len <= RIR_MAX_FILTER or filter_len % 2 == 0:
        raise ValueError(f"filter_len must be an odd integer in [3, {RIR_MAX_FILTER}], got {filter_len}")
    fs, c = _sample_rate(sample_rate), float(sound_speed)
    if not (np.isfinite(c) and c > 0.0):
        raise ValueError(f"sound_speed must be finite and positive, got {sound_speed}")
    if B > RIR_MAX_ROOMS:
        raise ValueError(f"at most {RIR_MAX_ROOMS} rooms per call, got {B}")
    _out_dtype(out_dtype)
    dev = _current_gpu(device)
    out = torch.empty((B, int(length)), dtype=out_dtype, device=dev)
    if B == 0:
        return out
    geom_d = _upload(torch.from_numpy(geom), dev)
    check(lib().mfpa_rir_shoebox(ptr(geom_d), B, int(max_order), int(length), fs, c, int(filter_len), int(bool(reversed)),
                                 int(out_dtype == torch.float64), ptr(out), int(length), stream()), "mfpa_rir_shoebox")
    return out
