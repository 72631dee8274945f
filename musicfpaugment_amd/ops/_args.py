"""What every wrapper does to its arguments on the host before a launch, written once: conversion to float64, the refusals
that many wrappers share, and the uploads that do not synchronise.  Plain functions; every refusal is a ValueError raised before
the GPU is asked for, so it is the same on a machine without one."""
from __future__ import annotations

import numpy as np
import torch

from .. import _lib
from .._lib import F32, F64, lib

MAX_ROWS = 65535                       # a grid dimension of the row kernels


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError(f"float32 or float64 expected, got {t.dtype}")


def _current_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.MfpaError("no GPU: libmfpa has no CPU fallback")
    lib()
    device = torch.device("cuda" if device is None else device)
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device through a pinned buffer, without a stream synchronisation."""
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def _host_f64(v, name: str) -> np.ndarray:
    """A number, a sequence, an array or a tensor as float64 on the host (a device tensor is read back: one synchronisation).  The
    result may share the argument's memory: a caller that writes into it copies it first."""
    try:
        return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, a sequence of numbers or a tensor") from None


def _host_tensor(v, name: str) -> torch.Tensor:
    """_host_f64 as a flat torch tensor, what _upload takes."""
    return torch.from_numpy(_host_f64(v, name).reshape(-1))


def _row_limit(n_rows: int, T: int, max_samples: int) -> None:
    if n_rows > MAX_ROWS or T > max_samples:
        raise ValueError(f"at most {MAX_ROWS} rows of {max_samples} samples per call")


def _rows(wav, name: str, max_samples: int):
    """(B, T) of a two-dimensional float32 or float64 tensor within the row kernels' limits."""
    if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be a (B, T) float32 or float64 tensor")
    B, T = wav.shape
    _row_limit(B, T, max_samples)
    return B, T


def _check_apply(apply, B: int, noun: str = "row") -> None:
    """The host half of `apply`: None, or one entry per row (clip, example)."""
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per {noun} ({B})")


def _apply_mask(apply, dev):
    """The device half of `apply`: (B,) uint8 of 0 and 1 on `dev`, None for None.  A host value goes through the pinned buffer, a
    device tensor is used where it is."""
    if apply is None:
        return None
    a = torch.as_tensor(apply)
    return (a if a.is_cuda else _upload(a.to(torch.uint8), dev)).ne(0).to(torch.uint8).contiguous()


def _out_dtype(out_dtype, default=None):
    """float32 or float64; `default` (the input's dtype) stands in for None."""
    out_dtype = default if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    return out_dtype


def _sample_rate(sample_rate) -> float:
    rate = float(sample_rate)
    if not (np.isfinite(rate) and rate > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    return rate


def _is_number(v) -> bool:
    """A real number that is not a tensor or an array."""
    return isinstance(v, (int, float, np.integer, np.floating))


def _row_values(v, B: int, name: str, noun: str = "row") -> np.ndarray:
    """A number or one finite value per row (clip, example) as (B,) float64 on the host."""
    a = _host_f64(v, name)
    if a.ndim > 1 or (a.ndim == 1 and a.shape != (B,)):
        raise ValueError(f"{name} must be a number or have one entry per {noun} ({B}), got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return np.array(np.broadcast_to(a, (B,)))
