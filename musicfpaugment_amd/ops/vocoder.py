"""The phase vocoder, time stretching and pitch shifting (csrc/vocoder.hip)."""
from __future__ import annotations

import ctypes
from fractions import Fraction
from typing import Optional, Tuple

import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import _host_tensor, _out_dtype, _upload
from .resampler import resample, resample_kernel_for
from .stft import N_BINS, N_HOP, istft, stft_complex, stft_frames


VOCODER_MAX_FRAMES = 16384             # MFPA_VOCODER_MAX_FRAMES (= TRACK_MAX_FRAMES)


def vocoder_frames(n_frames: int, rate: float) -> int:
    """ceil(n_frames / rate) by the kernel's double arithmetic: the frames phase_vocoder makes of n_frames at `rate`
    (mfpa_vocoder_frames: host arithmetic).  ValueError for a rate that is not finite or not positive, or too many frames."""
    n = ctypes.c_int(0)
    if not 1 <= int(n_frames) <= VOCODER_MAX_FRAMES:
        raise ValueError(f"n_frames must be in [1, {VOCODER_MAX_FRAMES}], got {n_frames}")
    check(lib().mfpa_vocoder_frames(int(n_frames), float(rate), ctypes.addressof(n)), f"mfpa_vocoder_frames({n_frames}, {rate})")
    return n.value


def _host_rates(rates, B: int) -> torch.Tensor:
    r = _host_tensor(rates, "rates")
    if r.numel() == 1 and not (isinstance(rates, torch.Tensor) and rates.dim() == 1):
        r = r.expand(B)
    if r.shape != (B,):
        raise ValueError(f"rates must be one number or have one entry per clip ({B}), got {tuple(r.shape)}")
    return r.contiguous()


def phase_vocoder(spec: torch.Tensor, rates, ld_out: Optional[int] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """torchaudio.functional.phase_vocoder of a (B, 257, n_frames) complex128 spectrum at hop 256 with one rate per clip, in one
    launch: -> (out (B, 257, max n_out) complex128, n_out (B,) int32 on the device).  Clip b has n_out[b] = ceil(n_frames / rate[b])
    frames, zeros behind them; a clip at rate exactly 1.0 is copied through.  `rates` is a number or B of them (list, array, tensor);
    they are checked on the host (ValueError) and size the output.  With `ld_out` given and the rates a (B,) float64 tensor on the
    device nothing is read back: the output has ld_out frames, and a clip whose rate the kernel refuses (not finite, not positive,
    more than ld_out frames) comes back as zeros with n_out[b] = -1."""
    require_gpu(spec, "spectrum")
    if spec.dim() != 3 or spec.shape[1] != N_BINS or spec.dtype != torch.complex128:
        raise ValueError("spectrum must be (B, 257, n_frames) complex128")
    B, _, nF = spec.shape
    if not 1 <= nF <= VOCODER_MAX_FRAMES:
        raise ValueError(f"n_frames must be in [1, {VOCODER_MAX_FRAMES}], got {nF}")
    if B > 65535:
        raise ValueError("at most 65535 clips per call")
    if ld_out is None:
        host = _host_rates(rates, B)
        ld_out = max([vocoder_frames(nF, r) for r in host.tolist()], default=1)
        rates_d = _upload(host, spec.device)
    else:
        require_gpu(rates, "rates")
        if rates.shape != (B,) or rates.dtype != torch.float64:
            raise ValueError("with ld_out, rates must be (B,) float64 on the device")
        rates_d = rates.contiguous()
        if not 1 <= int(ld_out) <= VOCODER_MAX_FRAMES:
            raise ValueError(f"ld_out must be in [1, {VOCODER_MAX_FRAMES}], got {ld_out}")
    spec = spec.contiguous()
    out = torch.empty((B, N_BINS, int(ld_out)), dtype=torch.complex128, device=spec.device)
    n_out = torch.empty((B,), dtype=torch.int32, device=spec.device)
    check(lib().mfpa_phase_vocoder(ptr(spec), B, nF, ptr(rates_d), ptr(out), int(ld_out), ptr(n_out), stream()), "mfpa_phase_vocoder")
    return out, n_out


def _stretched_length(T: int, rate: float) -> int:
    return int(round(T / rate))


def time_stretch(wav: torch.Tensor, rates, out_dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """Change the tempo of (B, T) float32 clips without changing their pitch: clip b becomes L_b = round(T / rate[b]) samples long
    (rate > 1 is faster).  One stft_complex, one phase_vocoder and one istft launch for the batch, whatever the rates.
    -> (stretched (B, max L_b) of out_dtype, lengths (B,) int64 on the host).  The inverse transform runs at its natural length,
    256 (n_out - 1) samples per clip, and each row is cropped or zero-padded to L_b: samples at and beyond L_b are zero.
    For rates below 1 torchaudio's algorithm repeats frame 0 and loses level."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    _out_dtype(out_dtype)
    B, T = wav.shape
    if T <= N_HOP:
        raise ValueError("reflect padding needs more than 256 samples per clip")
    host = _host_rates(rates, B)
    nF = stft_frames(T)
    frames = [vocoder_frames(nF, r) for r in host.tolist()]                  # refuses a bad rate before any launch
    lengths = torch.tensor([_stretched_length(T, r) for r in host.tolist()], dtype=torch.int64)
    L_max = int(lengths.max()) if B else 0
    out = torch.zeros((B, L_max), dtype=out_dtype, device=wav.device)
    n_max = max(frames, default=0)
    if B == 0 or L_max == 0 or n_max < 2:                                    # one frame has no hop to give back
        return out, lengths
    voc, _ = phase_vocoder(stft_complex(wav), host)
    y = istft(voc, out_dtype=out_dtype)                                      # (B, 256 (n_max - 1))
    # a clip with fewer frames than the longest ends under zero frames: what lies before 256 (n_out - 1) is its own natural-length
    # inverse, what lies behind is not kept
    keep = torch.minimum(lengths, torch.tensor([N_HOP * (n - 1) for n in frames], dtype=torch.int64))
    W = min(L_max, y.shape[1])
    mask = torch.arange(W, device=wav.device)[None, :] < _upload(keep, wav.device)[:, None]
    out[:, :W] = torch.where(mask, y[:, :W], torch.zeros((), dtype=out_dtype, device=wav.device))
    return out, lengths


def _host_ratios(ratios, B: int):
    if isinstance(ratios, Fraction):
        ratios = [ratios] * B
    ratios = list(ratios) if isinstance(ratios, (list, tuple)) else None
    if ratios is None or len(ratios) != B or not all(isinstance(f, Fraction) for f in ratios):
        raise ValueError(f"ratios must be one fractions.Fraction or one per clip ({B})")
    if any(f <= 0 for f in ratios):
        raise ValueError("a pitch ratio must be positive")
    return ratios


def pitch_shift(wav: torch.Tensor, ratios, rates: Optional[float] = None, *, any_ratio: bool = False) -> torch.Tensor:
    """Multiply the pitch of (B, T) float32 clips by p/q (`ratios`: one fractions.Fraction, or one per clip) at unchanged length:
    time_stretch by the rate q/p (the clip gets p/q times longer), then resample(., p, q) -- one launch per distinct ratio in the
    batch --, cropped or zero-padded to T.  A clip at ratio 1 comes back bit for bit.  A ratio whose filter bank the resampler does
    not take (resample_geometry(p, q)) is a ValueError before any launch.  `rates`: one stretch rate for every clip in place of
    q/p (transforms.PitchShift: torchaudio stretches by 2^(-steps/12) itself and resamples by the integer pair next to it).
    any_ratio=True: a ratio the dense resampler refuses goes to the sparse-tap one (resample(..., any_ratio=True)), which takes p
    up to 2^20 and q up to 65536 -- 8979/8000, two semitones at 8 kHz, for one."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    B, T = wav.shape
    ratios = _host_ratios(ratios, B)
    for f in set(ratios):
        if f != 1:
            resample_kernel_for(f.numerator, f.denominator, any_ratio)
    out = wav.contiguous().clone()
    moved = [b for b in range(B) if ratios[b] != 1]
    if not moved or T == 0:
        return out
    sel = _upload(torch.tensor(moved, dtype=torch.int64), wav.device)
    stretched, lengths = time_stretch(wav.index_select(0, sel), [float(1 / ratios[b]) if rates is None else float(rates) for b in moved])
    for f in sorted(set(ratios[b] for b in moved)):
        rows = [i for i, b in enumerate(moved) if ratios[b] == f]
        L = int(lengths[rows[0]])                                            # one ratio, one length
        x = stretched[:, :L] if len(rows) == len(moved) else stretched.index_select(0, _upload(torch.tensor(rows), wav.device))[:, :L]
        y = resample(x.contiguous(), f.numerator, f.denominator, any_ratio=any_ratio) if L > 0 else x
        dst = _upload(torch.tensor([moved[i] for i in rows], dtype=torch.int64), wav.device)
        W = min(T, y.shape[1])
        fitted = torch.zeros((len(rows), T), dtype=torch.float32, device=wav.device)
        fitted[:, :W] = y[:, :W]
        out.index_copy_(0, dst, fitted)
    return out
