"""Dynamic range compression and the envelope follower (csrc/dynamics.hip)."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _apply_mask, _check_apply, _dtype_code, _host_f64, _rows, _sample_rate, _upload


DYNAMICS_MAX_SAMPLES = 1 << 30
DYNAMICS_PARAMS = ("threshold_db", "slope", "knee_db", "attack_coef", "release_coef", "makeup_db")


def time_coef(seconds, sample_rate):
    """The one-pole coefficient of a time constant: exp(-1 / (seconds * sample_rate)) in float64 on the host, 0 for a time of 0.  A
    float for a number, an array for an array.  ValueError: a time that is negative or not finite, a rate that is not positive."""
    s = _host_f64(seconds, "seconds")
    rate = _sample_rate(sample_rate)
    if not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
        raise ValueError(f"a time constant must be finite and not negative, got {seconds}")
    c = np.zeros_like(s)
    np.divide(-1.0, s * rate, out=c, where=s > 0.0)
    c = np.where(s > 0.0, np.exp(c), 0.0)
    return float(c) if c.ndim == 0 else c


def dynamics_params(params, B: Optional[int] = None) -> np.ndarray:
    """Compressor parameters (6,) or (B, 6), columns DYNAMICS_PARAMS, as float64 on the host (no GPU).  ValueError: another shape,
    a value that is not finite, a slope outside [0, 1], a knee below 0, a coefficient outside [0, 1)."""
    q = np.array(_host_f64(params, "params"))                                # a copy: the caller may write into it
    if q.ndim not in (1, 2) or q.shape[-1] != 6 or (q.ndim == 2 and B is not None and q.shape[0] != B):
        raise ValueError(f"params must be (6,) or ({'B' if B is None else B}, 6): {', '.join(DYNAMICS_PARAMS)}; got {q.shape}")
    if not np.all(np.isfinite(q)):
        raise ValueError("params holds a value that is not finite")
    if np.any(q[..., 1] < 0.0) or np.any(q[..., 1] > 1.0):
        raise ValueError("slope = 1 - 1 / ratio must lie in [0, 1]")
    if np.any(q[..., 2] < 0.0):
        raise ValueError("knee_db must not be negative")
    if np.any(q[..., 3:5] < 0.0) or np.any(q[..., 3:5] >= 1.0):
        raise ValueError("attack_coef and release_coef must lie in [0, 1)")
    return np.ascontiguousarray(q)


def _dynamics(wav: torch.Tensor, q: np.ndarray, apply, zi, level_in: bool, want_gr: bool, name: str):
    """The launch of mfpa_dynamics: (y, gr or None, zf (B, 2) float64)."""
    B, T = _rows(wav, name, DYNAMICS_MAX_SAMPLES)
    if q.ndim == 2 and q.shape[0] != B:
        raise ValueError(f"per-row parameters must have one entry per row ({B}), got {q.shape[0]}")
    _check_apply(apply, B)
    if zi is not None and (not isinstance(zi, torch.Tensor) or tuple(zi.shape) != (B, 2)):
        raise ValueError(f"zi must be a ({B}, 2) tensor: y1 and yL of every row")
    require_gpu(wav, name)
    dev = wav.device
    wav = wav.contiguous()
    y = torch.empty_like(wav)
    gr = torch.empty_like(wav) if want_gr else None
    zi_d = None if zi is None else zi.to(device=dev, dtype=torch.float64).contiguous()
    zf = torch.zeros((B, 2), dtype=torch.float64, device=dev) if zi_d is None else zi_d.clone()
    if B == 0 or T == 0:
        return y, gr, zf
    apply_d = _apply_mask(apply, dev)
    q_d = _upload(torch.from_numpy(q), dev)
    check(lib().mfpa_dynamics(ptr(wav), _dtype_code(wav), B, T, ptr(q_d), int(q.ndim == 2), ptr(apply_d), ptr(zi_d), ptr(zf),
                              int(level_in), ptr(y), ptr(gr), stream()), "mfpa_dynamics")
    return y, gr, zf


def envelope_follow(level: torch.Tensor, attack_coef, release_coef, *, zi=None, return_state: bool = False):
    """The smooth decoupled peak detector along the rows of a (B, T) float32 or float64 level on the GPU, in one launch:
        y1 = max(level, release_coef * y1 + (1 - release_coef) * level);   yL = attack_coef * yL + (1 - attack_coef) * y1
    (instant attack and smooth release, then attack smoothing), float64 state and arithmetic, yL returned in the level's dtype.
    The coefficients are numbers or one value per row (time_coef(seconds, sample_rate)), in [0, 1).  `zi` (B, 2): the state
    (y1, yL), zeros without it; with return_state the return value is (yL, zf), zf (B, 2) float64 on the device."""
    a, r = _host_f64(attack_coef, "attack_coef"), _host_f64(release_coef, "release_coef")
    if a.ndim > 1 or r.ndim > 1:
        raise ValueError("attack_coef and release_coef must be numbers or have one entry per row")
    try:
        a, r = np.broadcast_arrays(a, r)
    except ValueError:
        raise ValueError(f"attack_coef {a.shape} and release_coef {r.shape} must be numbers or have one entry per row") from None
    q = np.zeros(a.shape + (6,))
    q[..., 3], q[..., 4] = a, r
    y, _, zf = _dynamics(level, dynamics_params(q), None, zi, True, False, "level")
    return (y, zf) if return_state else y


def compressor(wav: torch.Tensor, params, *, apply=None, zi=None, return_gain_reduction: bool = False, return_state: bool = False):
    """A feed-forward, log-domain dynamic range compressor along the rows of (B, T) float32 or float64 samples on the GPU, in one
    launch (the formula: include/mfpa.h, mfpa_dynamics).  `params` (6,) for the batch or (B, 6), columns DYNAMICS_PARAMS:
    threshold_db, slope = 1 - 1 / ratio (1 is a limiter), knee_db, attack_coef and release_coef (time_coef(seconds, sample_rate)),
    makeup_db; read and checked on the host.  `apply` (B,) of booleans: a row with a false entry comes back bit for bit, with no
    gain reduction and its state unchanged.  `zi` (B, 2): the detector's state (y1, yL), zeros without it.  Returns y, or a tuple
    of y, then the gain reduction in dB (B, T) in the samples' dtype with return_gain_reduction, then zf (B, 2) float64 with
    return_state."""
    q = dynamics_params(params)
    y, gr, zf = _dynamics(wav, q, apply, zi, False, bool(return_gain_reduction), "waveform")
    out = (y,) + ((gr,) if return_gain_reduction else ()) + ((zf,) if return_state else ())
    return out[0] if len(out) == 1 else out
