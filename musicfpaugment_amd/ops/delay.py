"""Delay lines: the time-varying fractional delay, the comb and the delay curves they take (csrc/delay.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._lib import check, lib, ptr, require_gpu, stream
from ._args import (_apply_mask, _check_apply, _current_gpu, _dtype_code, _host_f64, _out_dtype, _row_values, _rows, _sample_rate,
                    _upload)


DELAY_MAX_VOICES = 8                   # MFPA_DELAY_MAX_VOICES
VARIDELAY_TILE = 256                   # MFPA_VARIDELAY_TILE
VARIDELAY_WINDOW = 1024                # MFPA_VARIDELAY_WINDOW
COMB_MAX_DELAY = 1 << 24
DELAY_MAX_SAMPLES = 1 << 30


def variable_delay(wav: torch.Tensor, delay, gains=1.0, *, dry=0.0, filter_len: int = 81, apply=None, out_dtype=None) -> torch.Tensor:
    """A time-varying fractional delay without feedback along the rows of (B, T) float32 or float64 samples on the GPU, in one launch
    (the formula: include/mfpa.h, mfpa_varidelay):  y[n] = dry * x[n] + sum over the voices of gains[v] * x(n - delay[v][n]),  x(.)
    the row read through a Hann-windowed sinc of `filter_len` taps (odd, 3 to 255), zero outside the row.  `delay` is in samples,
    negative values read ahead: (B, T) for one voice, (B, V, T), or (B, V, 1) / (B, V) for voices of constant delay, V up to
    DELAY_MAX_VOICES (a two-dimensional delay of shape (B, T) is one voice).  It is float64; float32 is upcast, and its 24 bits lose
    interpolation accuracy once the delay exceeds a few hundred samples.  A tensor whose time stride is 0 or 1 is passed as it
    is, so a constant delay costs no (B, V, T) tensor; a host array is uploaded.  A delay that is not finite, or one that puts
    the window wholly outside the row, contributes exactly 0.  `gains` a number, (V,) or (B, V), `dry` a number or (B,): finite,
    read on the host.  `apply` (B,) of booleans: a row with a false entry is copied through.  Returns (B, T) in `out_dtype`
    (the samples' dtype without it), the float64 value rounded once."""
    B, T = _rows(wav, "waveform", DELAY_MAX_SAMPLES)
    out_dtype = _out_dtype(out_dtype, wav.dtype)
    if int(filter_len) != filter_len or not 3 <= filter_len <= 255 or not int(filter_len) & 1:
        raise ValueError(f"filter_len must be odd and lie in [3, 255], got {filter_len}")
    d = delay if isinstance(delay, torch.Tensor) else torch.from_numpy(np.array(_host_f64(delay, "delay")))
    if d.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"delay must be float64 (float32 is upcast), got {d.dtype}")
    if d.dim() == 2 and tuple(d.shape) == (B, T):
        d = d.unsqueeze(1)
    elif d.dim() == 2 and d.shape[0] == B:
        d = d.unsqueeze(2)
    if d.dim() != 3 or d.shape[0] != B or d.shape[2] not in (1, T):
        raise ValueError(f"delay must be ({B}, {T}), ({B}, V, {T}), ({B}, V, 1) or ({B}, V), got {tuple(delay.shape) if hasattr(delay, 'shape') else d.shape}")
    V = d.shape[1]
    if not 1 <= V <= DELAY_MAX_VOICES:
        raise ValueError(f"1 to {DELAY_MAX_VOICES} voices, got {V}")
    g, g0 = _host_f64(gains, "gains"), _host_f64(dry, "dry")
    if g.ndim > 2 or (g.ndim == 1 and g.shape != (V,)) or (g.ndim == 2 and g.shape != (B, V)):
        raise ValueError(f"gains must be a number, ({V},) or ({B}, {V}), got {g.shape}")
    if g0.ndim > 1 or (g0.ndim == 1 and g0.shape != (B,)):
        raise ValueError(f"dry must be a number or ({B},), got {g0.shape}")
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(g0))):
        raise ValueError("gains and dry must be finite")
    _check_apply(apply, B)
    require_gpu(wav, "waveform")
    dev = wav.device
    y = torch.empty((B, T), dtype=out_dtype, device=dev)
    if B == 0 or T == 0:
        return y
    wav = wav.contiguous()
    d = d.to(torch.float64)
    d = d.to(dev) if d.is_cuda else _upload(d, dev)
    constant = d.shape[2] == 1 or d.stride(2) == 0
    if not (d.stride(0) >= 0 and d.stride(1) >= 0 and (constant or d.stride(2) == 1 or T == 1)):
        d = d.contiguous()
    if d.device.index != torch.cuda.current_device():
        raise _lib.MfpaError(f"delay on {d.device} but the current device is cuda:{torch.cuda.current_device()}")
    g_d = _upload(torch.from_numpy(np.array(np.broadcast_to(g, (B, V)))), dev)
    g0_d = _upload(torch.from_numpy(np.array(np.broadcast_to(g0, (B,)))), dev)
    apply_d = _apply_mask(apply, dev)
    check(lib().mfpa_varidelay(ptr(wav), _dtype_code(wav), T, B, T, d.data_ptr(), d.stride(0) if B > 1 else 0,
                               d.stride(1) if V > 1 else 0, 0 if constant or T == 1 else 1, V, ptr(g_d), ptr(g0_d), ptr(apply_d),
                               int(filter_len), ptr(y), _dtype_code(y), stream()), "mfpa_varidelay")
    return y


def comb_params(delay, b0=1.0, bD=0.0, aD=0.0) -> np.ndarray:
    """The comb's parameters as float64 on the host (no GPU): (4,) for numbers, (N, 4) when any value has N entries; columns D, b0,
    bD, aD.  ValueError: a delay that is not an integer in [1, 2^24], |aD| >= 1, a value that is not finite, lengths that do not
    agree."""
    vals = [_host_f64(v, n) for v, n in ((delay, "delay"), (b0, "b0"), (bD, "bD"), (aD, "aD"))]
    if any(v.ndim > 1 for v in vals):
        raise ValueError("every comb parameter must be a number or have one entry per row")
    try:
        D, c0, cD, cA = np.broadcast_arrays(*vals)
    except ValueError:
        raise ValueError(f"per-row comb parameters must agree in length, got {[v.shape for v in vals]}") from None
    q = np.stack([D, c0, cD, cA], axis=-1)
    if not np.all(np.isfinite(q)):
        raise ValueError("the comb's parameters must be finite")
    if np.any(D < 1) or np.any(D > COMB_MAX_DELAY) or np.any(D != np.floor(D)):
        raise ValueError(f"delay must be an integer number of samples in [1, {COMB_MAX_DELAY}], got {delay}")
    if np.any(np.abs(cA) >= 1.0):
        raise ValueError(f"|aD| must be below 1, got {aD}")
    return np.ascontiguousarray(q)


def comb(wav: torch.Tensor, delay, b0=1.0, bD=0.0, aD=0.0, *, apply=None, out_dtype=None) -> torch.Tensor:
    """y[n] = b0 x[n] + (bD x[n - D] + aD y[n - D]) along the rows of (B, T) float32 or float64 samples on the GPU, in one launch
    (include/mfpa.h, mfpa_comb): float64 state and arithmetic without fused multiply-adds, the same bits as the formula evaluated
    sample by sample, rounded once for a float32 output; zeros before the row's start, no state across calls.  b0 = 1, bD = 0: a
    regenerating echo; aD = 0: a feed-forward comb; b0 = -g, bD = 1, aD = g: Schroeder's all-pass.  `delay` D an integer number
    of samples in [1, 2^24], |aD| < 1; every parameter a number, or a (B,) tensor or sequence with one value per row.  `apply`
    (B,) of booleans: a row with a false entry is copied through."""
    B, T = _rows(wav, "waveform", DELAY_MAX_SAMPLES)
    out_dtype = _out_dtype(out_dtype, wav.dtype)
    q = comb_params(delay, b0, bD, aD)
    if q.ndim == 2 and q.shape[0] != B:
        raise ValueError(f"per-row parameters must have one entry per row ({B}), got {q.shape[0]}")
    _check_apply(apply, B)
    require_gpu(wav, "waveform")
    dev = wav.device
    y = torch.empty((B, T), dtype=out_dtype, device=dev)
    if B == 0 or T == 0:
        return y
    wav = wav.contiguous()
    q_d = _upload(torch.from_numpy(q), dev)
    apply_d = _apply_mask(apply, dev)
    check(lib().mfpa_comb(ptr(wav), _dtype_code(wav), T, B, T, ptr(q_d), int(q.ndim == 2), int(np.max(q[..., 0])), ptr(apply_d), ptr(y),
                          _dtype_code(y), stream()), "mfpa_comb")
    return y


def _column(a: np.ndarray, dev) -> torch.Tensor:
    return _upload(torch.from_numpy(a), dev).unsqueeze(1)


def _delay_grid(B: int, T: int, sample_rate) -> float:
    if int(B) != B or int(T) != T or B < 0 or T < 0:
        raise ValueError(f"B and T must be non-negative integers, got {B}, {T}")
    return _sample_rate(sample_rate)


def lfo_delay(B: int, T: int, sample_rate, *, base_ms, depth_ms, rate_hz, phase=0.0, device="cuda") -> torch.Tensor:
    """(B, T) float64 on the GPU: the delay in samples  (base_ms + depth_ms sin(2 pi rate_hz n / sample_rate + phase)) sample_rate / 1000
    of a sine oscillator, what vibrato, chorus and flanger give ops.variable_delay.  Every parameter a number or one per row.
    Elementwise torch on the device, not a kernel of the library."""
    rate = _delay_grid(B, T, sample_rate)
    host = [_row_values(v, B, n) for v, n in ((base_ms, "base_ms"), (depth_ms, "depth_ms"), (rate_hz, "rate_hz"), (phase, "phase"))]
    dev = _current_gpu(device)
    base, depth, hz, ph = (_column(a, dev) for a in host)
    n = torch.arange(T, dtype=torch.float64, device=dev)
    return (base + depth * torch.sin(2.0 * np.pi * hz * n / rate + ph)) * (rate / 1000.0)


def speed_drift_delay(B: int, T: int, sample_rate, components, *, device="cuda") -> torch.Tensor:
    """(B, T) float64 on the GPU: the delay in samples whose derivative is minus the relative speed deviation
    sum_i depth_i sin(2 pi f_i t + phi_i)  of a playback chain (wow: slow, flutter: fast), in closed form
        d[n] = sum_i depth_i sample_rate / (2 pi f_i) (cos(2 pi f_i n / sample_rate + phi_i) - cos(phi_i)),
    so d[0] = 0 and the read position n - d[n] advances by 1 + deviation per sample.  `components` is a sequence of
    (depth, hz, phase), each a number or one per row; a component with depth 0 or hz 0 adds nothing.  Elementwise torch on the device."""
    rate = _delay_grid(B, T, sample_rate)
    comps = []
    for c in components:
        if len(c) != 3:
            raise ValueError("a component is (depth, hz, phase)")
        depth, hz, phase = (_row_values(v, B, n) for v, n in zip(c, ("depth", "hz", "phase")))
        if np.any(hz < 0.0):
            raise ValueError("hz must not be negative")
        comps.append((depth, hz, phase))
    dev = _current_gpu(device)
    n = torch.arange(T, dtype=torch.float64, device=dev)
    d = torch.zeros((B, T), dtype=torch.float64, device=dev)
    for depth, hz, phase in comps:
        on = (hz > 0.0) & (depth != 0.0)
        if not on.any():
            continue
        scale = np.where(on, depth * rate / (2.0 * np.pi * np.where(on, hz, 1.0)), 0.0)
        k, f, ph = (_column(a, dev) for a in (scale, np.where(on, hz, 0.0), phase))
        d += k * (torch.cos(2.0 * np.pi * f * n / rate + ph) - torch.cos(ph))
    return d
