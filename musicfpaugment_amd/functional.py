"""Substitutes for torchaudio.functional's filtering: `lfilter`, `biquad` and the `*_biquad` family, with torchaudio's signatures,
(..., T) in and out on the input's device like transforms.Resample.  The recurrence runs in csrc/iir.hip (ops.sosfilt); there is no
CPU fallback.

Two things differ from torchaudio, on purpose:
  * torchaudio filters in the input's dtype; this filters in float64 whatever the input and rounds a float32 output once.  Parity
    with torchaudio itself is therefore unpinned (torchaudio is not installed where this is tested);
  * the pinned reference is scipy: the output is scipy.signal.sosfilt's in float64 within a few of scipy's own rounding errors
    (tests/test_gpu_iir.py), and the designs meet their defining gains under scipy.signal.freqz (tests/test_iir_oracle.py).

The coefficient designs are the public Audio-EQ-Cookbook formulas (R. Bristow-Johnson) in the form torchaudio uses, as pure host
functions in float64: `biquad_coefficients(kind, sample_rate, freq, Q, gain_db)`.  Orders above 2 go through ops.sosfilt as
second-order sections; there is no tf2sos here.

Beside the filters: `simulate_rir_ism` (torchaudio.prototype.functional's name; the shoebox image-source simulator of csrc/rir.hip,
ops.simulate_rir) with the host helpers `eyring_absorption` and `rir_max_order`.  Parity with torchaudio and pyroomacoustics is
unpinned there too; the pinned reference is tests/_rir_oracle.py.

And `compressor` / `limiter` with the host helper `compressor_params`: the dynamic range compressor of csrc/dynamics.hip
(ops.compressor); the pinned reference is the definition restated in tests/_dynamics_oracle.py.

And the delay-line effects of csrc/delay.hip: `echo`, `vibrato`, `chorus`, `flanger` and `wow_flutter` over ops.variable_delay,
`comb`, `feedback_echo` and `allpass_comb` over ops.comb; the pinned reference is tests/_delay_oracle.py.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np
import torch

from . import ops
from ._lib import MfpaError
from .ops._args import _host_f64, _sample_rate as _rate

BIQUAD_KINDS = ("lowpass", "highpass", "bandpass", "bandpass_skirt", "bandreject", "allpass", "peaking", "lowshelf", "highshelf")


def biquad_coefficients(kind: str, sample_rate: float, freq: float, Q: float, gain_db: Optional[float] = None) -> np.ndarray:
    """(b0, b1, b2, a0, a1, a2) of one cookbook biquad, float64, not normalised (a0 is the cookbook's).  `kind` is one of
    BIQUAD_KINDS: "bandpass" has a 0 dB peak, "bandpass_skirt" a constant skirt gain (peak gain Q); "peaking", "lowshelf" and
    "highshelf" need gain_db.  ValueError: an unknown kind, a frequency outside (0, sample_rate / 2), Q <= 0, a missing or
    non-finite gain."""
    if kind not in BIQUAD_KINDS:
        raise ValueError(f"kind must be one of {BIQUAD_KINDS}, got {kind!r}")
    sample_rate, freq, Q = float(sample_rate), float(freq), float(Q)
    if not (math.isfinite(sample_rate) and sample_rate > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    if not 0.0 < freq < sample_rate / 2:
        raise ValueError(f"the frequency must lie in (0, sample_rate / 2 = {sample_rate / 2}), got {freq}")
    if not (math.isfinite(Q) and Q > 0.0):
        raise ValueError(f"Q must be positive, got {Q}")
    w0 = 2.0 * math.pi * freq / sample_rate
    cs, sn = math.cos(w0), math.sin(w0)
    alpha = sn / (2.0 * Q)
    if kind in ("peaking", "lowshelf", "highshelf"):
        if gain_db is None or not math.isfinite(float(gain_db)):
            raise ValueError(f"{kind} needs a finite gain_db")
        A = math.exp(float(gain_db) / 40.0 * math.log(10.0))
    if kind == "lowpass":
        c = ((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "highpass":
        c = ((1.0 + cs) / 2.0, -1.0 - cs, (1.0 + cs) / 2.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind in ("bandpass", "bandpass_skirt"):
        t = sn / 2.0 if kind == "bandpass_skirt" else alpha
        c = (t, 0.0, -t, 1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "bandreject":
        c = (1.0, -2.0 * cs, 1.0, 1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "allpass":
        c = (1.0 - alpha, -2.0 * cs, 1.0 + alpha, 1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "peaking":
        c = (1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A, 1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)
    else:
        t1, t2, t3 = 2.0 * math.sqrt(A) * alpha, (A - 1.0) * cs, (A + 1.0) * cs
        if kind == "lowshelf":
            c = (A * ((A + 1.0) - t2 + t1), 2.0 * A * ((A - 1.0) - t3), A * ((A + 1.0) - t2 - t1),
                 (A + 1.0) + t2 + t1, -2.0 * ((A - 1.0) + t3), (A + 1.0) + t2 - t1)
        else:
            c = (A * ((A + 1.0) + t2 + t1), -2.0 * A * ((A - 1.0) + t3), A * ((A + 1.0) + t2 - t1),
                 (A + 1.0) - t2 + t1, 2.0 * ((A - 1.0) - t3), (A + 1.0) - t2 - t1)
    return np.array(c, dtype=np.float64)


def _filter(waveform: torch.Tensor, sos: np.ndarray, clamp: bool, who: str) -> torch.Tensor:
    """sos (S, 6) for every row or (F, S, 6) for the F rows of the last but one dimension."""
    sos = ops.sos_normalized(sos)                                            # the refusals need no GPU
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 1 or waveform.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a float32 or float64 tensor (..., T)")
    x = waveform
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError(f"{who} computes on the MI355X and none is present; no CPU fallback")
        x = x.cuda()
    lead, T = x.shape[:-1], x.shape[-1]
    rows = x.reshape(-1, T)
    if sos.ndim == 3:
        sos = np.ascontiguousarray(np.broadcast_to(sos, (rows.shape[0] // sos.shape[0],) + sos.shape).reshape(-1, *sos.shape[1:]))
    with torch.cuda.device(x.device):
        y = ops.sosfilt(rows, sos, clamp=clamp)
    return y.reshape(*lead, T).to(waveform.device)


def _coeff_rows(c, name: str) -> np.ndarray:
    c = np.array(_host_f64(c, name))
    if c.ndim not in (1, 2) or c.shape[-1] < 1:
        raise ValueError(f"{name} must be (num_order + 1,) or (num_filters, num_order + 1), got {c.shape}")
    return c


def lfilter(waveform: torch.Tensor, a_coeffs, b_coeffs, clamp: bool = True, batching: bool = True) -> torch.Tensor:
    """torchaudio.functional.lfilter (note its order: the DENOMINATOR first) for filters of order up to 2, lower delays first.
    Coefficients (num_order + 1,) filter every row; (num_filters, num_order + 1) with batching=True filter the rows of a
    (..., num_filters, T) waveform each with its own filter, and with batching=False every input row with every filter:
    (..., T) -> (..., num_filters, T).  Longer coefficient vectors are a NotImplementedError: give them to ops.sosfilt as
    second-order sections."""
    a, b = _coeff_rows(a_coeffs, "a_coeffs"), _coeff_rows(b_coeffs, "b_coeffs")
    if a.shape != b.shape:
        raise ValueError(f"a_coeffs and b_coeffs must have the same shape, got {a.shape} and {b.shape}")
    if a.shape[-1] > 3:
        raise NotImplementedError(f"lfilter takes orders up to 2 (3 coefficients), got {a.shape[-1]}: factor the filter into "
                                  "second-order sections and call ops.sosfilt")
    pad = [(0, 0)] * (a.ndim - 1) + [(0, 3 - a.shape[-1])]
    sos = np.concatenate([np.pad(b, pad), np.pad(a, pad)], axis=-1)           # (6,) or (F, 6)
    if sos.ndim == 1:
        return _filter(waveform, sos[None], clamp, "lfilter")
    sos = sos[:, None, :]                                                     # (F, 1, 6)
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 1:
        raise ValueError("waveform must be a float32 or float64 tensor (..., T)")
    if not batching:
        waveform = waveform.unsqueeze(-2).expand(*waveform.shape[:-1], sos.shape[0], waveform.shape[-1])
    elif waveform.dim() < 2 or waveform.shape[-2] != sos.shape[0]:
        raise ValueError(f"with batching, {sos.shape[0]} filters need a waveform (..., {sos.shape[0]}, T)")
    return _filter(waveform, sos, clamp, "lfilter")


def biquad(waveform: torch.Tensor, b0: float, b1: float, b2: float, a0: float, a1: float, a2: float) -> torch.Tensor:
    """torchaudio.functional.biquad: lfilter of one second-order section, clamped to [-1, 1] like torchaudio's."""
    return _filter(waveform, np.array([[float(b0), float(b1), float(b2), float(a0), float(a1), float(a2)]]), True, "biquad")


def _design(waveform, who: str, kind: str, sample_rate, freq, Q, gain_db=None) -> torch.Tensor:
    return _filter(waveform, biquad_coefficients(kind, sample_rate, freq, Q, gain_db)[None], True, who)


def lowpass_biquad(waveform: torch.Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> torch.Tensor:
    return _design(waveform, "lowpass_biquad", "lowpass", sample_rate, cutoff_freq, Q)


def highpass_biquad(waveform: torch.Tensor, sample_rate: int, cutoff_freq: float, Q: float = 0.707) -> torch.Tensor:
    return _design(waveform, "highpass_biquad", "highpass", sample_rate, cutoff_freq, Q)


def bandpass_biquad(waveform: torch.Tensor, sample_rate: int, central_freq: float, Q: float = 0.707,
                    const_skirt_gain: bool = False) -> torch.Tensor:
    return _design(waveform, "bandpass_biquad", "bandpass_skirt" if const_skirt_gain else "bandpass", sample_rate, central_freq, Q)


def bandreject_biquad(waveform: torch.Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> torch.Tensor:
    return _design(waveform, "bandreject_biquad", "bandreject", sample_rate, central_freq, Q)


def allpass_biquad(waveform: torch.Tensor, sample_rate: int, central_freq: float, Q: float = 0.707) -> torch.Tensor:
    return _design(waveform, "allpass_biquad", "allpass", sample_rate, central_freq, Q)


def equalizer_biquad(waveform: torch.Tensor, sample_rate: int, center_freq: float, gain: float, Q: float = 0.707) -> torch.Tensor:
    """A peaking equaliser: `gain` dB at center_freq."""
    return _design(waveform, "equalizer_biquad", "peaking", sample_rate, center_freq, Q, gain)


def bass_biquad(waveform: torch.Tensor, sample_rate: int, gain: float, central_freq: float = 100, Q: float = 0.707) -> torch.Tensor:
    """A low shelf: `gain` dB below central_freq."""
    return _design(waveform, "bass_biquad", "lowshelf", sample_rate, central_freq, Q, gain)


def treble_biquad(waveform: torch.Tensor, sample_rate: int, gain: float, central_freq: float = 3000, Q: float = 0.707) -> torch.Tensor:
    """A high shelf: `gain` dB above central_freq."""
    return _design(waveform, "treble_biquad", "highshelf", sample_rate, central_freq, Q, gain)


# ----------------------------------------------------------------------------- room impulse responses (csrc/rir.hip)
def _rooms(room) -> np.ndarray:
    room = _host_f64(room, "room")
    if room.ndim not in (1, 2) or room.shape[-1] != 3:
        raise ValueError(f"room must be (3,) or (B, 3), got {room.shape}")
    if not (np.all(np.isfinite(room)) and np.all(room > 0.0)):
        raise ValueError("every room side must be finite and positive")
    return room


def _rt60s(rt60, rooms: np.ndarray) -> np.ndarray:
    rt60 = np.asarray(rt60, dtype=np.float64)
    if not (np.all(np.isfinite(rt60)) and np.all(rt60 > 0.0)):
        raise ValueError(f"rt60 must be finite and positive, got {rt60}")
    try:
        return np.broadcast_to(rt60, rooms.shape[:-1])
    except ValueError:
        raise ValueError(f"rt60 must be a scalar or one value per room, got {rt60.shape} for {rooms.shape[:-1]} rooms") from None


def eyring_absorption(room, rt60):
    """The uniform energy absorption coefficient that Eyring's formula gives a shoebox room (3,) or rooms (B, 3) for the decay time
    rt60 in seconds: 1 - exp(-0.161 V / (S rt60)), V the volume, S the wall area.  A float, or (B,) float64; host arithmetic."""
    room = _rooms(room)
    rt60 = _rt60s(rt60, room)
    V = room[..., 0] * room[..., 1] * room[..., 2]
    S = 2.0 * (room[..., 0] * room[..., 1] + room[..., 1] * room[..., 2] + room[..., 0] * room[..., 2])
    a = 1.0 - np.exp(-0.161 * V / (S * rt60))
    return float(a) if a.ndim == 0 else a


def rir_max_order(room, rt60, sound_speed: float = 343.0):
    """The reflection order whose images reach past rt60 along the room's shortest side: ceil(c rt60 / min(L)).  An int, or (B,)
    int64; host arithmetic."""
    room = _rooms(room)
    rt60 = _rt60s(rt60, room)
    if not (math.isfinite(float(sound_speed)) and sound_speed > 0.0):
        raise ValueError(f"sound_speed must be finite and positive, got {sound_speed}")
    n = np.ceil(float(sound_speed) * rt60 / room.min(axis=-1)).astype(np.int64)
    return int(n) if n.ndim == 0 else n


def simulate_rir_ism(room, source, mic, max_order: int, absorption, output_length: int, *, sample_rate: float,
                     sound_speed: float = 343.0, delay_filter_length: int = 81) -> torch.Tensor:
    """torchaudio.prototype.functional.simulate_rir_ism for one microphone and frequency-independent walls: the image-source impulse
    response of a shoebox room, (1, output_length) float32 on the GPU for room, source and mic of shape (3,), (B, output_length) for
    (B, 3).  absorption is a scalar, (6,) or (B, 6), the walls in the order x0 x1 y0 y1 z0 z1 (west east south north floor ceiling).
    Unlike torchaudio's, the length and the sample rate have no defaults, every image with |ix| + |iy| + |iz| <= max_order is summed
    in float64, and the result is not normalised.  Parity with torchaudio and with pyroomacoustics is unpinned (neither is installed
    where this is tested); the pinned reference is the numpy restatement in tests/_rir_oracle.py."""
    return ops.simulate_rir(room, source, mic, absorption, max_order, output_length, sample_rate, sound_speed=sound_speed,
                            filter_len=delay_filter_length)


# ----------------------------------------------------------------------------- dynamic range compression (csrc/dynamics.hip)
def compressor_params(sample_rate, threshold_db=-20.0, ratio=4.0, attack_ms=5.0, release_ms=100.0, knee_db=6.0,
                      makeup_db=0.0) -> np.ndarray:
    """What ops.compressor takes, from a compressor's front panel: (6,) float64 for numbers, (N, 6) when any value is a sequence of
    N (the others are repeated).  slope = 1 - 1 / ratio (ratio >= 1, float("inf") is a limiter), the coefficients are
    ops.time_coef(ms / 1000, sample_rate).  Host arithmetic.  ValueError: a ratio below 1 or NaN, a negative knee or time, a value
    that is not finite, lengths that do not agree."""
    vals = [_host_f64(v, n) for v, n in ((threshold_db, "threshold_db"), (ratio, "ratio"), (knee_db, "knee_db"), (attack_ms, "attack_ms"),
                                         (release_ms, "release_ms"), (makeup_db, "makeup_db"))]
    if any(v.ndim > 1 for v in vals):
        raise ValueError("every compressor parameter must be a number or have one entry per row")
    try:
        th, ratio, knee, attack, release, makeup = np.broadcast_arrays(*vals)
    except ValueError:
        raise ValueError(f"per-row compressor parameters must agree in length, got {[v.shape for v in vals]}") from None
    if np.any(np.isnan(ratio)) or np.any(ratio < 1.0):
        raise ValueError(f"ratio must be at least 1 (float('inf') for a limiter), got {ratio}")
    q = np.empty(th.shape + (6,))
    q[..., 0], q[..., 1], q[..., 2], q[..., 5] = th, 1.0 - 1.0 / ratio, knee, makeup
    q[..., 3], q[..., 4] = ops.time_coef(attack / 1000.0, sample_rate), ops.time_coef(release / 1000.0, sample_rate)
    return ops.dynamics_params(q)


def _compress(waveform: torch.Tensor, q: np.ndarray, who: str) -> torch.Tensor:
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 1 or waveform.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a float32 or float64 tensor (..., T)")
    lead, T = waveform.shape[:-1], waveform.shape[-1]
    n = int(np.prod(lead, dtype=np.int64))
    if q.ndim == 2 and q.shape[0] != n:
        raise ValueError(f"per-row parameters must have one entry per row ({n}), got {q.shape[0]}")
    x = waveform
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError(f"{who} computes on the MI355X and none is present; no CPU fallback")
        x = x.cuda()
    with torch.cuda.device(x.device):
        y = ops.compressor(x.reshape(-1, T), q)
    return y.reshape(*lead, T).to(waveform.device)


def compressor(waveform: torch.Tensor, sample_rate: int, threshold_db=-20.0, ratio=4.0, attack_ms=5.0, release_ms=100.0, knee_db=6.0,
               makeup_db=0.0) -> torch.Tensor:
    """A feed-forward dynamic range compressor (log-domain, smooth decoupled peak detector: Giannoulis, Massberg and Reiss, JAES
    2012) along the last dimension of a (..., T) float32 or float64 waveform, in and out on the input's device, computed on the GPU
    in float64 and rounded once.  Every parameter is a number or has one entry per row of the flattened leading dimensions."""
    return _compress(waveform, compressor_params(sample_rate, threshold_db, ratio, attack_ms, release_ms, knee_db, makeup_db), "compressor")


def limiter(waveform: torch.Tensor, sample_rate: int, threshold_db=-1.0, release_ms=50.0) -> torch.Tensor:
    """A peak limiter: the compressor with slope 1 (ratio infinity), no knee and no attack time, so no output sample exceeds
    10^(threshold_db / 20)."""
    return _compress(waveform, compressor_params(sample_rate, threshold_db, float("inf"), 0.0, release_ms, 0.0, 0.0), "limiter")


# ----------------------------------------------------------------------------- delay-line effects (csrc/delay.hip)
def _numbers(who: str, **values) -> None:
    """Each value one finite real number, a Python or numpy scalar."""
    for name, v in values.items():
        if not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{who}: {name} must be one finite real number (a Python or numpy scalar), got {v!r}")


def _on_rows(waveform: torch.Tensor, who: str, run) -> torch.Tensor:
    """run(rows (N, T) on the GPU) for a (..., T) waveform on any device; the result goes back in the waveform's shape, on its device."""
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 1 or waveform.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a float32 or float64 tensor (..., T)")
    lead, T = waveform.shape[:-1], waveform.shape[-1]
    x = waveform
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError(f"{who} computes on the MI355X and none is present; no CPU fallback")
        x = x.cuda()
    with torch.cuda.device(x.device):
        y = run(x.reshape(-1, T))
    return y.reshape(*lead, T).to(waveform.device)


def comb_delay_samples(sample_rate, delay_ms) -> int:
    """The comb's integer delay: delay_ms in samples rounded to the nearest, at least 1."""
    rate = _rate(sample_rate)
    _numbers("comb", delay_ms=delay_ms)
    if delay_ms < 0.0:
        raise ValueError(f"delay_ms must not be negative, got {delay_ms}")
    return max(1, int(round(delay_ms * rate / 1000.0)))


def echo(waveform: torch.Tensor, sample_rate, delays_ms, decays, gain_in: float = 1.0, gain_out: float = 1.0) -> torch.Tensor:
    """sox `echo`, feed-forward: gain_out (gain_in x[n] + sum_k decays[k] x(n - delays_ms[k])) along the last dimension of a
    (..., T) float32 or float64 waveform, up to ops.DELAY_MAX_VOICES echoes, the delays fractional (81-tap windowed sinc).  It is
    ops.variable_delay(rows, [delays_ms[k] * sample_rate / 1000] as (N, V, 1) constant voices, gains=[gain_out * decays[k]],
    dry=gain_out * gain_in): one launch, no (N, V, T) tensor."""
    rate = _rate(sample_rate)
    dl, dc = np.atleast_1d(np.asarray(delays_ms, dtype=np.float64)), np.atleast_1d(np.asarray(decays, dtype=np.float64))
    if dl.ndim != 1 or dl.shape != dc.shape or not 1 <= dl.size <= ops.DELAY_MAX_VOICES:
        raise ValueError(f"delays_ms and decays must have the same length, 1 to {ops.DELAY_MAX_VOICES}, got {dl.shape} and {dc.shape}")
    _numbers("echo", gain_in=gain_in, gain_out=gain_out)
    if not (np.all(np.isfinite(dl)) and np.all(np.isfinite(dc))) or np.any(dl < 0.0):
        raise ValueError("delays_ms must be finite and not negative, decays finite")
    return _on_rows(waveform, "echo", lambda rows: ops.variable_delay(
        rows, np.broadcast_to((dl * rate / 1000.0)[:, None], (rows.shape[0], dl.size, 1)), gain_out * dc, dry=gain_out * gain_in))


def comb(waveform: torch.Tensor, sample_rate, delay_ms, b0: float = 1.0, bD: float = 0.0, aD: float = 0.0) -> torch.Tensor:
    """y[n] = b0 x[n] + (bD x[n - D] + aD y[n - D]), D = comb_delay_samples(sample_rate, delay_ms), |aD| < 1: it is
    ops.comb(rows, D, b0, bD, aD)."""
    D = comb_delay_samples(sample_rate, delay_ms)
    q = ops.comb_params(D, b0, bD, aD)
    if q.ndim != 1:
        raise ValueError("b0, bD and aD must be numbers")
    return _on_rows(waveform, "comb", lambda rows: ops.comb(rows, D, b0, bD, aD))


def feedback_echo(waveform: torch.Tensor, sample_rate, delay_ms, feedback, mix: float = 1.0) -> torch.Tensor:
    """A regenerating echo: wet[n] = x[n] + feedback wet[n - D], y = (1 - mix) x + mix wet, |feedback| < 1, D as in `comb`.  It is
    ops.comb(rows, D, 1.0, -(1.0 - mix) * feedback, feedback); with mix = 1 the comb's pure feedback corner."""
    _numbers("feedback_echo", feedback=feedback, mix=mix)
    return comb(waveform, sample_rate, delay_ms, 1.0, -(1.0 - mix) * feedback, feedback)


def allpass_comb(waveform: torch.Tensor, sample_rate, delay_ms, gain) -> torch.Tensor:
    """Schroeder's all-pass: y[n] = -g x[n] + (x[n - D] + g y[n - D]), |g| < 1, unit magnitude at every frequency.  It is
    ops.comb(rows, D, -gain, 1.0, gain)."""
    _numbers("allpass_comb", gain=gain)
    return comb(waveform, sample_rate, delay_ms, -gain, 1.0, gain)


def vibrato(waveform: torch.Tensor, sample_rate, rate_hz: float = 5.0, depth_ms: float = 1.0) -> torch.Tensor:
    """Pitch modulation: the row read at a delay of depth_ms (1 + sin(2 pi rate_hz t)), nothing dry.  It is
    ops.variable_delay(rows, ops.lfo_delay(N, T, sample_rate, base_ms=depth_ms, depth_ms=depth_ms, rate_hz=rate_hz))."""
    rate = _rate(sample_rate)
    _numbers("vibrato", rate_hz=rate_hz, depth_ms=depth_ms)
    if rate_hz < 0.0 or depth_ms < 0.0:
        raise ValueError("rate_hz and depth_ms must not be negative")
    return _on_rows(waveform, "vibrato", lambda rows: ops.variable_delay(
        rows, ops.lfo_delay(rows.shape[0], rows.shape[1], rate, base_ms=depth_ms, depth_ms=depth_ms, rate_hz=rate_hz, device=rows.device)))


def chorus_phases(voices: int) -> np.ndarray:
    """The voices' oscillator phases, spread evenly over a period."""
    return 2.0 * np.pi * np.arange(voices) / voices


def chorus(waveform: torch.Tensor, sample_rate, voices: int = 3, base_ms: float = 20.0, depth_ms: float = 2.0, rate_hz: float = 0.8,
           mix: float = 0.5) -> torch.Tensor:
    """(1 - mix) x + mix / voices * sum_v x(n - d_v[n]), d_v = base_ms + depth_ms sin(2 pi rate_hz t + 2 pi v / voices).  It is
    ops.variable_delay(rows, delay (N, voices, T), gains=mix / voices, dry=1 - mix) with delay[:, v] =
    ops.lfo_delay(N, T, sample_rate, base_ms=base_ms, depth_ms=depth_ms, rate_hz=rate_hz, phase=chorus_phases(voices)[v])."""
    rate = _rate(sample_rate)
    if not isinstance(voices, int) or not 1 <= voices <= ops.DELAY_MAX_VOICES:
        raise ValueError(f"voices must be an integer from 1 to {ops.DELAY_MAX_VOICES}, got {voices!r}")
    _numbers("chorus", base_ms=base_ms, depth_ms=depth_ms, rate_hz=rate_hz, mix=mix)
    if rate_hz < 0.0 or depth_ms < 0.0 or base_ms < depth_ms:
        raise ValueError("rate_hz and depth_ms must not be negative and base_ms not below depth_ms")

    def run(rows):
        N, T = rows.shape
        delay = torch.stack([ops.lfo_delay(N, T, rate, base_ms=base_ms, depth_ms=depth_ms, rate_hz=rate_hz, phase=float(ph), device=rows.device)
                             for ph in chorus_phases(voices)], dim=1)
        return ops.variable_delay(rows, delay, mix / voices, dry=1.0 - mix)
    return _on_rows(waveform, "chorus", run)


def flanger(waveform: torch.Tensor, sample_rate, base_ms: float = 1.0, depth_ms: float = 2.0, rate_hz: float = 0.5,
            mix: float = 0.7) -> torch.Tensor:
    """A feed-forward flanger: x[n] + mix x(n - d[n]), d sweeping from base_ms to base_ms + depth_ms at rate_hz.  It is
    ops.variable_delay(rows, ops.lfo_delay(N, T, sample_rate, base_ms=base_ms + depth_ms / 2, depth_ms=depth_ms / 2,
    rate_hz=rate_hz), gains=mix, dry=1.0).  torchaudio.functional.flanger's `regen` (feedback through the moving delay) is not
    offered, its interpolation and wave shapes differ, and parity with torchaudio is unpinned."""
    rate = _rate(sample_rate)
    _numbers("flanger", base_ms=base_ms, depth_ms=depth_ms, rate_hz=rate_hz, mix=mix)
    if rate_hz < 0.0 or depth_ms < 0.0 or base_ms < 0.0:
        raise ValueError("base_ms, depth_ms and rate_hz must not be negative")
    return _on_rows(waveform, "flanger", lambda rows: ops.variable_delay(
        rows, ops.lfo_delay(rows.shape[0], rows.shape[1], rate, base_ms=base_ms + depth_ms / 2, depth_ms=depth_ms / 2, rate_hz=rate_hz,
                            device=rows.device), mix, dry=1.0))


def wow_flutter(waveform: torch.Tensor, sample_rate, wow_hz: float = 0.8, wow_depth: float = 0.002, flutter_hz: float = 8.0,
                flutter_depth: float = 0.0008, phase=(0.0, 0.0)) -> torch.Tensor:
    """The speed drift of an analogue playback chain: the row played at the relative speed
    1 + wow_depth sin(2 pi wow_hz t + phase[0]) + flutter_depth sin(2 pi flutter_hz t + phase[1]).  It is
    ops.variable_delay(rows, ops.speed_drift_delay(N, T, sample_rate, [(wow_depth, wow_hz, phase[0]), (flutter_depth, flutter_hz,
    phase[1])])); with both depths 0 the delay is 0 and finite samples come back with their bits, up to the sign of a zero
    (a sample that is not finite spreads over the filter's length as NaN, as in any FIR).  The interpolator does not band-limit,
    which is negligible at these depths; for a large constant speed change use transforms.Speed."""
    rate = _rate(sample_rate)
    if len(phase) != 2:
        raise ValueError("phase is (wow phase, flutter phase)")
    _numbers("wow_flutter", wow_hz=wow_hz, wow_depth=wow_depth, flutter_hz=flutter_hz, flutter_depth=flutter_depth, wow_phase=phase[0],
             flutter_phase=phase[1])
    if wow_hz < 0.0 or flutter_hz < 0.0 or not (abs(wow_depth) + abs(flutter_depth) < 1.0):
        raise ValueError("the frequencies must not be negative and the depths must sum to less than 1")
    return _on_rows(waveform, "wow_flutter", lambda rows: ops.variable_delay(
        rows, ops.speed_drift_delay(rows.shape[0], rows.shape[1], rate, [(wow_depth, wow_hz, phase[0]), (flutter_depth, flutter_hz, phase[1])],
                                    device=rows.device)))


# ----------------------------------------------------------------------------- lossy coding (csrc/codec.hip)
def transform_codec(waveform: torch.Tensor, sample_rate, kbps) -> torch.Tensor:
    """A (..., T) float32 or float64 waveform through the simulated transform codec at `kbps` kbit/s (one number; math.inf is
    lossless): ops.transform_codec(rows, kbps, sample_rate=sample_rate).  It simulates transform coding; parity with a real MP3,
    AAC or GSM encoder is unpinned."""
    rate = _rate(sample_rate)
    if not isinstance(kbps, (int, float, np.integer, np.floating)) or math.isnan(kbps) or kbps == -math.inf:
        raise ValueError(f"transform_codec: kbps must be one number, got {kbps!r}")
    return _on_rows(waveform, "transform_codec", lambda rows: ops.transform_codec(rows, kbps, sample_rate=rate))


def _channels(quantization_channels) -> int:
    if not isinstance(quantization_channels, (int, np.integer)) or not 2 <= quantization_channels <= 65536:
        raise ValueError(f"quantization_channels must be an integer in [2, 65536], got {quantization_channels!r}")
    return int(quantization_channels)


def mu_law_encoding(x: torch.Tensor, quantization_channels: int = 256) -> torch.Tensor:
    """torchaudio.functional.mu_law_encoding on the device, in float64 (parity with torchaudio's float32 unpinned): a (..., T)
    float32 or float64 tensor, clamped to [-1, 1], to int64 codes in [0, quantization_channels - 1]."""
    ch = _channels(quantization_channels)
    if not isinstance(x, torch.Tensor) or x.dim() < 1 or x.dtype not in (torch.float32, torch.float64):
        raise ValueError("x must be a float32 or float64 tensor (..., T)")
    lead, T = x.shape[:-1], x.shape[-1]
    g = x
    if not g.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError("mu_law_encoding computes on the MI355X and none is present; no CPU fallback")
        g = g.cuda()
    with torch.cuda.device(g.device):
        codes = ops.mu_law_encode(g.reshape(-1, T), ch)
    return codes.reshape(*lead, T).to(torch.int64).to(x.device)


def mu_law_decoding(x_mu: torch.Tensor, quantization_channels: int = 256) -> torch.Tensor:
    """torchaudio.functional.mu_law_decoding on the device, in float64 rounded once to float32: a (..., T) integer tensor of codes
    (int64 as mu_law_encoding returns them, or int32) to float32 samples in [-1, 1]."""
    ch = _channels(quantization_channels)
    if not isinstance(x_mu, torch.Tensor) or x_mu.dim() < 1 or x_mu.dtype not in (torch.int32, torch.int64):
        raise ValueError("x_mu must be an int32 or int64 tensor (..., T)")
    lead, T = x_mu.shape[:-1], x_mu.shape[-1]
    g = x_mu
    if not g.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError("mu_law_decoding computes on the MI355X and none is present; no CPU fallback")
        g = g.cuda()
    with torch.cuda.device(g.device):
        y = ops.mu_law_decode(g.reshape(-1, T).to(torch.int32), ch)
    return y.reshape(*lead, T).to(x_mu.device)


# ----------------------------------------------------------------------------- spectral noise suppression (csrc/denoise.hip)
def spectral_denoise(waveform: torch.Tensor, sample_rate, **kw) -> torch.Tensor:
    """A (..., T) float32 waveform through the model-free spectral suppressor: the pipeline's STFT (512 / 256, whatever the rate),
    ops.spectral_suppress(mag, **kw) on its magnitudes, the inverse STFT on the input's phase -- denoisers.SpectralDenoiser's
    denoise_waveform.  `kw`: alpha, back, ahead, bias, dd, xi_min_db, floor_db.  T must exceed 256."""
    from .denoisers import SpectralDenoiser
    _rate(sample_rate)
    net = SpectralDenoiser(**kw)
    if not isinstance(waveform, torch.Tensor) or waveform.dtype != torch.float32:
        raise ValueError("waveform must be a float32 tensor (..., T)")
    return _on_rows(waveform, "spectral_denoise", net.denoise_waveform)


# ----------------------------------------------------------------------------- programme loudness (csrc/loudness.hip)
K_WEIGHTING_DESIGNS = ("bs1770", "torchaudio")


def _k_stage(sample_rate: float, f0: float, Q: float):
    K = math.tan(math.pi * f0 / sample_rate)
    return K, 1.0 + K / Q + K * K


def k_weighting_sos(sample_rate, design: str = "bs1770") -> np.ndarray:
    """(2, 6) float64, a0 == 1: the K-weighting of ITU-R BS.1770 as two second-order sections, the shelf and the high-pass, at any
    rate; host arithmetic.
      "bs1770"      the analogue prototypes behind the standard's 48 kHz table, bilinear-transformed at `sample_rate` (the
                    re-derivation open-source meters use); at 48 kHz it gives the table to 9e-16;
      "torchaudio"  torchaudio.functional.loudness' own pair: a cookbook high shelf (1500 Hz, Q 1/sqrt 2, +4 dB) and high-pass (38 Hz,
                    Q 0.5).  Up to 0.043 dB from the table at 48 kHz and 0.18 dB low at 997 Hz at 8 kHz, so it is not the default;
                    parity with torchaudio itself is unpinned."""
    fs = _rate(sample_rate)
    if design not in K_WEIGHTING_DESIGNS:
        raise ValueError(f"design must be one of {K_WEIGHTING_DESIGNS}, got {design!r}")
    if design == "torchaudio":
        return ops.sos_normalized(np.stack([biquad_coefficients("highshelf", fs, 1500.0, 1.0 / math.sqrt(2.0), 4.0),
                                            biquad_coefficients("highpass", fs, 38.0, 0.5)]))
    if fs <= 2.0 * 1681.974450955533:
        raise ValueError(f"the K-weighting shelf sits at 1682 Hz: sample_rate must exceed 3364 Hz, got {sample_rate}")
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K, a0 = _k_stage(fs, f0, Q)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 1.0, 2.0 * (K * K - 1.0) / a0,
             (1.0 - K / Q + K * K) / a0]
    Q = 0.5003270373238773
    K, a0 = _k_stage(fs, 38.13547087602444, Q)
    highpass = [1.0, -2.0, 1.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array([shelf, highpass], dtype=np.float64)


def _on_examples(waveform: torch.Tensor, who: str, run):
    """run(x (N, C, T) on the GPU) for a (..., C, T) waveform on any device -> (tensor on the GPU, lead shape, the input's device)."""
    if not isinstance(waveform, torch.Tensor) or waveform.dim() < 2 or waveform.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a float32 or float64 tensor (..., channels, T)")
    x = waveform
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise MfpaError(f"{who} computes on the MI355X and none is present; no CPU fallback")
        x = x.cuda()
    with torch.cuda.device(x.device):
        return run(x.reshape(-1, *x.shape[-2:]))


def loudness(waveform: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """torchaudio.functional.loudness: integrated loudness (ITU-R BS.1770-4) of (..., channels, T) -> (...) float64 LUFS, on the
    input's device.  Every channel has weight 1 and the K-weighting is k_weighting_sos(sample_rate, "bs1770"), not torchaudio's pair
    (ops.loudness takes weights and the design)."""
    _rate(sample_rate)
    out = _on_examples(waveform, "loudness", lambda x: ops.loudness(x, sample_rate))
    return out.reshape(waveform.shape[:-2]).to(waveform.device)


def loudness_range(waveform: torch.Tensor, sample_rate: int) -> torch.Tensor:
    """Loudness range (EBU Tech 3342) of (..., channels, T) -> (...) float64 LU (ops.loudness_range)."""
    _rate(sample_rate)
    out = _on_examples(waveform, "loudness_range", lambda x: ops.loudness_range(x, sample_rate))
    return out.reshape(waveform.shape[:-2]).to(waveform.device)


def loudness_normalize(waveform: torch.Tensor, sample_rate: int, target_lufs: float, peak_limit: Optional[float] = None) -> torch.Tensor:
    """(..., channels, T) with every example scaled to `target_lufs` integrated loudness (ops.loudness_normalize), same shape, dtype and
    device.  Silence comes back unchanged."""
    _rate(sample_rate)
    _numbers("loudness_normalize", target_lufs=target_lufs)
    out = _on_examples(waveform, "loudness_normalize", lambda x: ops.loudness_normalize(x, sample_rate, float(target_lufs), peak_limit=peak_limit))
    return out.reshape(waveform.shape).to(waveform.device)
