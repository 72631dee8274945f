"""Programme loudness: BS.1770 metering, range, normalisation (csrc/loudness.hip)."""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _apply_mask, _check_apply, _dtype_code, _host_f64, _row_limit, _row_values, _sample_rate, _upload
from .iir import sos_normalized
from .resampler import resample


LOUDNESS_MAX_CHANNELS = 8              # MFPA_LOUDNESS_MAX_CHANNELS
LOUDNESS_MAX_WINDOW = 64               # MFPA_LOUDNESS_MAX_WINDOW
LOUDNESS_MAX_RANGE_BLOCKS = 16384      # MFPA_LOUDNESS_MAX_RANGE_BLOCKS
LOUDNESS_MAX_SAMPLES = 1 << 30
LOUDNESS_MAX_HOP = 1 << 24
LOUDNESS_OFFSET = -0.691               # BS.1770: LUFS = -0.691 + 10 log10(power)
LOUDNESS_WINDOWS = {"momentary": 4, "short": 30}


class LoudnessGate(tuple):
    """(power, abs_power, n_abs, n_rel, blocks, range) of ops.loudness_gate, also by name."""
    __slots__ = ()
    _fields = ("power", "abs_power", "n_abs", "n_rel", "blocks", "range")

    def __new__(cls, *values):
        return tuple.__new__(cls, values)

    power = property(lambda self: self[0])
    abs_power = property(lambda self: self[1])
    n_abs = property(lambda self: self[2])
    n_rel = property(lambda self: self[3])
    blocks = property(lambda self: self[4])
    range = property(lambda self: self[5])


def loudness_hop(sample_rate) -> int:
    """The 100 ms hop in samples: floor(0.1 fs + 0.5)."""
    fs = _sample_rate(sample_rate)
    hop = int(math.floor(0.1 * fs + 0.5))
    if not 1 <= hop <= LOUDNESS_MAX_HOP:
        raise ValueError(f"sample_rate {sample_rate} gives a hop of {hop} samples, outside 1 to {LOUDNESS_MAX_HOP}")
    return hop


def loudness_power(lufs):
    """The mean-square power of a loudness in LUFS, 10^((lufs + 0.691) / 10), in float64 on the host: a float, or an array for an
    array.  This is the absolute gate (at -70) and the target of loudness_normalize as the kernels receive them."""
    v = np.asarray(lufs, dtype=np.float64)
    out = np.array([10.0 ** ((float(t) - LOUDNESS_OFFSET) / 10.0) for t in v.reshape(-1)], dtype=np.float64).reshape(v.shape)
    return float(out) if out.ndim == 0 else out


def loudness_lufs(power: torch.Tensor) -> torch.Tensor:
    """-0.691 + 10 log10(power) with torch on float64 results; -inf at 0."""
    return LOUDNESS_OFFSET + 10.0 * torch.log10(power)


def _loudness_sos(sos) -> Optional[np.ndarray]:
    if sos is None:
        return None
    s = _host_f64(sos, "sos")
    if s.ndim == 2 and s.shape[0] == 0:
        return None
    if s.ndim != 2:
        raise ValueError(f"sos must be (S, 6), shared by all rows, got {s.shape}")
    return sos_normalized(s)


def loudness_segments(wav: torch.Tensor, sos, hop: int, *, return_peak: bool = False):
    """Segment energies of (..., T) float32 or float64 samples on the GPU: every row is filtered by the sections `sos` ((S, 6), S <= 8,
    shared by all rows; None or (0, 6): unweighted) in float64 exactly as ops.sosfilt does, squared, and summed over consecutive
    segments of `hop` samples -> (..., T // hop) float64.  The filtered signal is never stored.  return_peak=True: also (...,) float64,
    the largest |sample| of the unfiltered rows."""
    s = _loudness_sos(sos)
    if not isinstance(wav, torch.Tensor) or wav.dim() < 1 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a (..., T) float32 or float64 tensor")
    hop = int(hop)
    if not 1 <= hop <= LOUDNESS_MAX_HOP:
        raise ValueError(f"hop must lie in 1 to {LOUDNESS_MAX_HOP}, got {hop}")
    lead, T = tuple(wav.shape[:-1]), wav.shape[-1]
    R = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if T < 1 or T > LOUDNESS_MAX_SAMPLES or R > 65535:
        raise ValueError(f"at most 65535 rows of 1 to {LOUDNESS_MAX_SAMPLES} samples per call, got {R} rows of {T}")
    require_gpu(wav, "waveform")
    dev = wav.device
    rows = wav.contiguous().reshape(R, T)
    nseg = T // hop
    seg = torch.empty((R, nseg), dtype=torch.float64, device=dev)
    peak = torch.empty((R,), dtype=torch.float64, device=dev) if return_peak else None
    if R > 0:
        S = 0 if s is None else s.shape[0]
        need = ctypes.c_longlong(0)
        check(lib().mfpa_loudness_work(S, ctypes.addressof(need)), "mfpa_loudness_work")
        work = torch.empty((need.value,), dtype=torch.float64, device=dev) if S else None
        sos_d = _upload(torch.from_numpy(s), dev) if S else None
        check(lib().mfpa_loudness_segments(ptr(rows), _dtype_code(rows), R, T, ptr(sos_d), S, hop, ptr(work), need.value,
                                           ptr(seg) if nseg else 0, ptr(peak), stream()), "mfpa_loudness_segments")
    seg = seg.reshape(*lead, nseg)
    return (seg, peak.reshape(lead)) if return_peak else seg


def _loudness_weights(weights, C: int) -> Optional[np.ndarray]:
    if weights is None:
        return None
    w = _host_f64(weights, "weights")
    if w.shape != (C,) or not np.all(np.isfinite(w)) or np.any(w < 0.0):
        raise ValueError(f"weights must be {C} finite, non-negative channel weights, got {w!r}")
    return np.ascontiguousarray(w)


def loudness_gate(seg: torch.Tensor, hop: int, *, win: int = 4, rel: float = 0.1, weights=None, abs_lufs: float = -70.0,
                  return_blocks: bool = False, want_range: bool = False) -> LoudnessGate:
    """The two-stage gate of BS.1770 on segment energies (B, C, nseg) or (B, nseg) float64 (ops.loudness_segments with the same
    `hop`).  A block is `win` segments and advances by one; its power is the weighted sum over the channels of its mean squares.
    Blocks above the absolute gate `abs_lufs`, then above `rel` times their mean power, are averaged.  Returns a LoudnessGate of
    float64 / int32 tensors on the device: power (B,) (0 when no block passes), abs_power (B,), n_abs, n_rel (B,), blocks (B, nb)
    with return_blocks, range (B, 2) with want_range: the powers at the nearest ranks of 10 % and 95 % of the gated blocks."""
    if not isinstance(seg, torch.Tensor) or seg.dim() not in (2, 3) or seg.dtype != torch.float64:
        raise ValueError("seg must be a (B, C, nseg) or (B, nseg) float64 tensor")
    if seg.dim() == 2:
        seg = seg[:, None, :]
    B, C, nseg = seg.shape
    hop, win = int(hop), int(win)
    if not 1 <= hop <= LOUDNESS_MAX_HOP:
        raise ValueError(f"hop must lie in 1 to {LOUDNESS_MAX_HOP}, got {hop}")
    if not 1 <= win <= LOUDNESS_MAX_WINDOW:
        raise ValueError(f"win must lie in 1 to {LOUDNESS_MAX_WINDOW}, got {win}")
    if not 1 <= C <= LOUDNESS_MAX_CHANNELS or B > 65535:
        raise ValueError(f"1 to {LOUDNESS_MAX_CHANNELS} channels and at most 65535 examples, got {C} and {B}")
    rel, p_abs = float(rel), loudness_power(float(abs_lufs))
    if not (math.isfinite(rel) and rel >= 0.0) or not math.isfinite(p_abs):
        raise ValueError(f"rel must be finite and not negative and abs_lufs finite, got {rel} and {abs_lufs}")
    w = _loudness_weights(weights, C)
    nb = max(0, nseg - win + 1)
    if want_range and nb > LOUDNESS_MAX_RANGE_BLOCKS:
        raise ValueError(f"the range ranks take at most {LOUDNESS_MAX_RANGE_BLOCKS} blocks, got {nb}")
    require_gpu(seg, "seg")
    dev = seg.device
    seg = seg.contiguous()
    power = torch.zeros((B, 2), dtype=torch.float64, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    blocks = torch.empty((B, nb), dtype=torch.float64, device=dev) if return_blocks else None
    rng = torch.zeros((B, 2), dtype=torch.float64, device=dev) if want_range else None
    if B > 0:
        w_d = _upload(torch.from_numpy(w), dev) if w is not None else None
        check(lib().mfpa_loudness_gate(ptr(seg) if nseg else 0, B, C, nseg, hop, win, ptr(w_d), p_abs, rel, ptr(power), ptr(counts),
                                       ptr(blocks) if nb else 0, ptr(rng), stream()), "mfpa_loudness_gate")
    return LoudnessGate(power[:, 0].contiguous(), power[:, 1].contiguous(), counts[:, 0].contiguous(), counts[:, 1].contiguous(), blocks, rng)


def _loudness_input(wav, name: str = "waveform") -> torch.Tensor:
    if not isinstance(wav, torch.Tensor) or wav.dim() not in (2, 3) or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be a (B, C, T) or (B, T) float32 or float64 tensor")
    x = wav[:, None, :] if wav.dim() == 2 else wav
    if not 1 <= x.shape[1] <= LOUDNESS_MAX_CHANNELS:
        raise ValueError(f"1 to {LOUDNESS_MAX_CHANNELS} channels, got {x.shape[1]}")
    if x.shape[2] < 1:
        raise ValueError("the waveform holds no sample")
    return x


def _loudness_meter(wav, sample_rate, *, design="bs1770", weights=None, win=4, rel=0.1, return_blocks=False, want_range=False,
                    return_peak=False):
    from ..functional import k_weighting_sos                                  # host design; functional imports this package
    x = _loudness_input(wav)
    hop = loudness_hop(sample_rate)
    sos = k_weighting_sos(sample_rate, design)
    _loudness_weights(weights, x.shape[1])
    out = loudness_segments(x, sos, hop, return_peak=return_peak)
    seg, peak = out if return_peak else (out, None)
    return loudness_gate(seg, hop, win=win, rel=rel, weights=weights, return_blocks=return_blocks, want_range=want_range), peak


def loudness(wav: torch.Tensor, sample_rate, *, design: str = "bs1770", weights=None) -> torch.Tensor:
    """Integrated programme loudness (ITU-R BS.1770-4) of (B, C, T) or (B, T) float32 or float64 samples on the GPU -> (B,) float64
    LUFS; -inf where no 400 ms block passes the gates (silence, or less than 400 ms).  `weights`: one per channel, default 1 (the
    standard gives the surround pair 1.41).  `design`: functional.k_weighting_sos."""
    gate, _ = _loudness_meter(wav, sample_rate, design=design, weights=weights)
    return loudness_lufs(gate.power)


def loudness_curve(wav: torch.Tensor, sample_rate, window: str = "momentary") -> torch.Tensor:
    """Momentary (400 ms) or short-term (window="short", 3 s) loudness every 100 ms -> (B, nb) float64 LUFS, ungated."""
    if window not in LOUDNESS_WINDOWS:
        raise ValueError(f"window must be one of {tuple(LOUDNESS_WINDOWS)}, got {window!r}")
    gate, _ = _loudness_meter(wav, sample_rate, win=LOUDNESS_WINDOWS[window], return_blocks=True)
    return loudness_lufs(gate.blocks)


def loudness_range(wav: torch.Tensor, sample_rate) -> torch.Tensor:
    """Loudness range (EBU Tech 3342) -> (B,) float64 LU: short-term blocks every 100 ms, the absolute gate at -70 LUFS, the relative
    gate at -20 LU, the spread between the nearest ranks at 10 % and 95 %.  0 where no block passes.  At most 16384 blocks (27 min)."""
    gate, _ = _loudness_meter(wav, sample_rate, win=LOUDNESS_WINDOWS["short"], rel=0.01, want_range=True)
    lra = 10.0 * torch.log10(gate.range[:, 1] / gate.range[:, 0])
    return torch.where(gate.n_rel > 0, lra, torch.zeros_like(lra))


def loudness_normalize(wav: torch.Tensor, sample_rate, target_lufs, *, peak_limit: Optional[float] = None, apply=None,
                       return_gain: bool = False):
    """Scale every example of (B, C, T) or (B, T) to the integrated loudness `target_lufs` (a number, or one per example), same
    shape and dtype.  peak_limit: the gain is reduced where the sample peak would exceed it (linear, e.g. 1.0).  An example comes back
    bit for bit when it has no gated loudness (silence), when its gain is not finite, or when `apply` (B,) is false for it.  The
    meter, the gain and the multiply run on the device without a host synchronisation.  return_gain=True: also (B,) float64."""
    x = _loudness_input(wav)
    B, C, T = x.shape
    t = _row_values(target_lufs, B, "target_lufs", "example")
    limit = 0.0 if peak_limit is None else float(peak_limit)
    if peak_limit is not None and not (math.isfinite(limit) and limit > 0.0):
        raise ValueError(f"peak_limit must be positive and finite, got {peak_limit}")
    _check_apply(apply, B, "example")
    _row_limit(B * C, T, LOUDNESS_MAX_SAMPLES)
    gate, peak = _loudness_meter(x, sample_rate, return_peak=peak_limit is not None)
    dev = x.device
    x = x.contiguous()
    y = torch.empty_like(x)
    gain = torch.ones((B,), dtype=torch.float64, device=dev) if return_gain else None
    if B > 0:
        target_d = _upload(torch.from_numpy(loudness_power(t)), dev)
        check(lib().mfpa_loudness_apply(ptr(x), _dtype_code(x), B, C, T, ptr(gate.power), ptr(target_d), ptr(peak), limit,
                                        ptr(_apply_mask(apply, dev)), ptr(y), ptr(gain), stream()), "mfpa_loudness_apply")
    y = y.reshape(wav.shape)
    return (y, gain) if return_gain else y


def true_peak(wav: torch.Tensor, oversample: int = 4) -> torch.Tensor:
    """An estimate of the inter-sample peak of (B, C, T) or (B, T) float32 samples -> (B, C) or (B,) float32, linear: the largest
    |sample| of ops.resample(wav, 1, oversample).  It has no kernel of its own and is NOT the interpolation filter of BS.1770 Annex 2:
    the interpolator is the resampler's windowed sinc (width 6, roll-off 0.99), which reads a sine at fs / 4 within 0.1 dB."""
    x = _loudness_input(wav)
    if wav.dtype != torch.float32:
        raise ValueError("true_peak takes float32 samples (ops.resample)")
    oversample = int(oversample)
    if not 1 <= oversample <= 16:
        raise ValueError(f"oversample must lie in 1 to 16, got {oversample}")
    require_gpu(wav, "waveform")
    B, C, T = x.shape
    up = resample(x.reshape(B * C, T), 1, oversample)
    return up.abs().amax(dim=1).reshape(wav.shape[:-1])
