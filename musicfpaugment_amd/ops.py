"""Thin, typed wrappers over the C ABI (include/mfpa.h): torch tensors in, torch tensors out.

Each function allocates its outputs with torch on the input's device, checks shapes on the
host (a kernel must never see a shape its grid does not assume) and enqueues on torch's
current HIP stream.  Nothing here computes on the CPU.
"""
from __future__ import annotations

import ctypes
import math
from fractions import Fraction
from functools import lru_cache
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from ._lib import F32, F64, check, lib, ptr, require_gpu, stream

N_FFT, N_HOP, N_BINS = 512, 256, 257


FLOAT32_LOGS = ("rounded", "numpy")


def _float32_log_code(float32_log: str) -> int:
    """The logarithm of the pickers' FLOAT32 (denoised) branch: "rounded" = the float64 log rounded once to float32 (the default),
    "numpy" = numpy's own float32 log bit for bit (csrc/mfpa_nplog.h), what the reference computes at
    afp/audfprint/peak_extractor.py:265-276 and afp/dejavu/fingerprint.py:70-79."""
    if float32_log not in FLOAT32_LOGS:
        raise ValueError(f"float32_log must be 'rounded' or 'numpy', got {float32_log!r}")
    return FLOAT32_LOGS.index(float32_log)


def _dtype_code(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float64:
        return F64
    raise TypeError(f"float32 or float64 expected, got {t.dtype}")


# ----------------------------------------------------------------------------- STFT
def audfprint_window() -> np.ndarray:
    """np.hanning(514)[1:-1]  (training/visualisation.py:18, afp/audfprint/peak_extractor.py:257)."""
    return np.hanning(N_FFT + 2)[1:-1]


def dejavu_window() -> np.ndarray:
    """mlab.window_hanning on 512 samples = np.hanning(512)  (afp/dejavu/fingerprint.py:64)."""
    return np.hanning(N_FFT)


@lru_cache(maxsize=16)
def _tables_cached(kind: str, device_index: int) -> torch.Tensor:
    win = audfprint_window() if kind == "audfprint" else dejavu_window()
    return stft_tables(win, torch.device("cuda", device_index))


def stft_tables(window: np.ndarray, device) -> torch.Tensor:
    """Host-side table build (mfpa_stft_tables) + upload: window and FFT twiddles, float64."""
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (N_FFT,):
        raise ValueError("window must have 512 points")
    out = np.empty(_lib.STFT_TABLE_LEN, dtype=np.float64)
    check(lib().mfpa_stft_tables(w.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p)),
          "mfpa_stft_tables")
    return torch.from_numpy(out).to(device)


def default_tables(device, kind: str = "audfprint") -> torch.Tensor:
    device = torch.device(device)
    return _tables_cached(kind, device.index if device.index is not None else torch.cuda.current_device())


def stft_frames(n_samples: int) -> int:
    return 1 + n_samples // N_HOP


def stft_mag(wav: torch.Tensor, out_dtype=torch.float64, tables: Optional[torch.Tensor] = None,
             want_max: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(B, T_w) float32 -> |STFT| (B, 257, 1 + T_w//256) and per-clip float64 maxima."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w <= N_HOP:
        raise ValueError("reflect padding needs more than 256 samples per clip")
    if tables is None:
        tables = default_tables(wav.device)
    nF = stft_frames(T_w)
    mag = torch.empty((B, N_BINS, nF), dtype=out_dtype, device=wav.device)
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device) if want_max else None
    check(lib().mfpa_stft_mag(ptr(wav), B, T_w, ptr(tables), ptr(mag), _dtype_code(mag), ptr(cmax), stream()),
          "mfpa_stft_mag")
    return mag, cmax


def stft_complex(wav: torch.Tensor, tables: Optional[torch.Tensor] = None, want_mag: bool = False, mag_dtype=torch.float64):
    """(B, T_w) float32 -> torch.stft(wav.double(), 512, 256, window=w, return_complex=True): (B, 257, 1 + T_w//256) complex128.
    want_mag=True returns (spec, mag, clip_max) from the one transform, mag and clip_max bit for bit stft_mag(wav, mag_dtype)'s."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    if mag_dtype not in (torch.float32, torch.float64):
        raise ValueError("mag_dtype must be torch.float32 or torch.float64")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w <= N_HOP:
        raise ValueError("reflect padding needs more than 256 samples per clip")
    if tables is None:
        tables = default_tables(wav.device)
    nF = stft_frames(T_w)
    spec = torch.empty((B, N_BINS, nF), dtype=torch.complex128, device=wav.device)
    mag = torch.empty((B, N_BINS, nF), dtype=mag_dtype, device=wav.device) if want_mag else None
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device) if want_mag else None
    check(lib().mfpa_stft_complex(ptr(wav), B, T_w, ptr(tables), ptr(spec), ptr(mag), F32 if mag_dtype == torch.float32 else F64,
                                  ptr(cmax), stream()), "mfpa_stft_complex")
    return (spec, mag, cmax) if want_mag else spec


ISTFT_CLAMP = 1                        # MFPA_ISTFT_CLAMP
ISTFT_ENVELOPE_MIN = 1e-11             # torch.istft refuses a smaller overlap-added squared window


def istft_envelope_min(window: np.ndarray, n_frames: int, length: int) -> float:
    """Minimum of the overlap-added squared window over the samples istft keeps (mfpa_istft_envelope_min: host arithmetic)."""
    w = np.ascontiguousarray(window, dtype=np.float64)
    if w.shape != (N_FFT,):
        raise ValueError("window must have 512 points")
    out = ctypes.c_double(0.0)
    check(lib().mfpa_istft_envelope_min(w.ctypes.data_as(ctypes.c_void_p), int(n_frames), int(length), ctypes.addressof(out)),
          "mfpa_istft_envelope_min")
    return out.value


@lru_cache(maxsize=64)
def _default_envelope_min(n_frames: int, length: int) -> float:
    return istft_envelope_min(audfprint_window(), n_frames, length)


def istft(spec: torch.Tensor, length: Optional[int] = None, mag: Optional[torch.Tensor] = None,
          denom: Optional[torch.Tensor] = None, clamp: bool = False, out_dtype=torch.float32,
          tables: Optional[torch.Tensor] = None) -> torch.Tensor:
    """torch.istft(Z, 512, 256, window=w, center=True, length=length) of a (B, 257, n_frames) complex128 spectrum -> (B, length).
    mag=None: Z = spec.  Otherwise Z = m * spec / |spec| with m = mag * denom[b] (mag (B, 257, n_frames) float32 or float64, denom
    (B,) float64 or None), phase 0 where spec is 0; clamp=True turns a negative m into 0.  length=None is 256 * (n_frames - 1), as in
    torch; any length an STFT with n_frames frames can have come from is taken.  With `tables` given, its window is read back from
    the device for torch's "window overlap add min" check (the default tables need no copy)."""
    require_gpu(spec, "spectrum")
    if spec.dim() != 3 or spec.shape[1] != N_BINS or spec.dtype != torch.complex128:
        raise ValueError("spectrum must be (B, 257, n_frames) complex128")
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("out_dtype must be torch.float32 or torch.float64")
    B, _, nF = spec.shape
    if nF < 2:
        raise ValueError("istft needs at least 2 frames")
    if length is None:
        length = N_HOP * (nF - 1)
    length = int(length)
    if not N_HOP * (nF - 1) <= length < N_HOP * nF:
        raise ValueError(f"length must be in [{N_HOP * (nF - 1)}, {N_HOP * nF}) for {nF} frames, got {length}")
    if B > 65535:
        raise ValueError("at most 65535 clips per call")
    if mag is not None:
        require_gpu(mag, "magnitude")
        if mag.shape != spec.shape or mag.dtype not in (torch.float32, torch.float64):
            raise ValueError("magnitude must be (B, 257, n_frames) float32 or float64")
        mag = mag.contiguous()
        if denom is not None:
            require_gpu(denom, "denominator")
            if denom.shape != (B,) or denom.dtype != torch.float64:
                raise ValueError("denom must be (B,) float64")
            denom = denom.contiguous()
    elif denom is not None or clamp:
        raise ValueError("denom and clamp belong to mag")
    if tables is None:
        tables = default_tables(spec.device)
        env_min = _default_envelope_min(nF, length)
    else:
        require_gpu(tables, "tables")
        if tables.shape != (_lib.STFT_TABLE_LEN,) or tables.dtype != torch.float64:
            raise ValueError(f"tables must be ({_lib.STFT_TABLE_LEN},) float64 (stft_tables)")
        env_min = istft_envelope_min(tables[:N_FFT].cpu().numpy(), nF, length)
    if not env_min >= ISTFT_ENVELOPE_MIN:
        raise RuntimeError(f"istft: window overlap add min: {env_min}")      # torch's refusal (its message ends "window overlap add min: 1")
    spec = spec.contiguous()
    out = torch.empty((B, length), dtype=out_dtype, device=spec.device)
    check(lib().mfpa_istft(ptr(spec), ptr(mag), _dtype_code(mag) if mag is not None else F32, ptr(denom),
                           ISTFT_CLAMP if clamp else 0, B, nF, length, ptr(tables), ptr(out), _dtype_code(out), stream()),
          "mfpa_istft")
    return out


def specgram_psd(wav: torch.Tensor, scale_in: float = 1.0, tables: Optional[torch.Tensor] = None):
    """(B, T_w) float32 -> mlab.specgram-style PSD (B, 257, (T_w-256)//256) float64 (unscaled) + clip maxima."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    wav = wav.contiguous()
    B, T_w = wav.shape
    if T_w < N_FFT:
        raise ValueError("need at least one full 512-sample frame")
    if tables is None:
        tables = default_tables(wav.device, "dejavu")
    nF = (T_w - 256) // 256
    psd = torch.empty((B, N_BINS, nF), dtype=torch.float64, device=wav.device)
    cmax = torch.empty((B,), dtype=torch.float64, device=wav.device)
    check(lib().mfpa_specgram_psd(ptr(wav), B, T_w, float(scale_in), ptr(tables), ptr(psd), ptr(cmax), stream()),
          "mfpa_specgram_psd")
    return psd, cmax


def normalize_(data: torch.Tensor, clip_max: torch.Tensor, per_clip: bool) -> torch.Tensor:
    """In-place data[b] /= (clip_max[b] if per_clip else max(clip_max))."""
    require_gpu(data, "data")
    B = data.shape[0]
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    n = data[0].numel() if B else 0
    check(lib().mfpa_normalize(ptr(data), _dtype_code(data), B, n, ptr(clip_max), int(per_clip), stream()),
          "mfpa_normalize")
    return data


def nplog_f32(x: torch.Tensor) -> torch.Tensor:
    """Element-wise numpy float32 log (mfpa_nplog_f32): float32 tensor of any shape -> np.log(x) as numpy's SIMD kernel returns it,
    bit for bit (csrc/mfpa_nplog.h).  For callers that post-process float32 spectrograms themselves."""
    require_gpu(x)
    if x.dtype != torch.float32:
        raise TypeError("float32 expected")
    x = x.contiguous()
    out = torch.empty_like(x)
    check(lib().mfpa_nplog_f32(ptr(x), ptr(out), x.numel(), stream()), "mfpa_nplog_f32")
    return out


def f64_to_f32(x: torch.Tensor) -> torch.Tensor:
    require_gpu(x)
    if x.dtype != torch.float64:
        raise TypeError("float64 expected")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    check(lib().mfpa_f64_to_f32(ptr(x), ptr(out), x.numel(), stream()), "mfpa_f64_to_f32")
    return out


# ----------------------------------------------------------------------------- resampling (csrc/resample.hip)
RESAMPLE_LOWPASS_FILTER_WIDTH = 6      # torchaudio.transforms.Resample's defaults (sinc_interp_hann); torchaudio is not in the
RESAMPLE_ROLLOFF = 0.99                # reference tree, so parity with it is unpinned
RESAMPLE_TAP_ALIGN = 16                # MFPA_RESAMPLE_TAP_ALIGN


def resample_geometry(orig_freq: int, new_freq: int, T: int = 0) -> Tuple[int, int, int, int, int]:
    """(o, n, width, taps per phase, Tout) of torchaudio.transforms.Resample(orig_freq, new_freq) for T input samples
    (mfpa_resample_geometry: host arithmetic)."""
    o, n, width, ntaps = (ctypes.c_int(0) for _ in range(4))
    tout = ctypes.c_longlong(0)
    check(lib().mfpa_resample_geometry(int(orig_freq), int(new_freq), RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, int(T),
                                       ctypes.addressof(o), ctypes.addressof(n), ctypes.addressof(width), ctypes.addressof(ntaps),
                                       ctypes.addressof(tout)), "mfpa_resample_geometry")
    return o.value, n.value, width.value, ntaps.value, int(tout.value)


def resample_tile(orig_freq: int, new_freq: int) -> int:
    """Frames (groups of n output / o input samples) one workgroup of the resampling kernel owns for this pair of rates."""
    o, n, width, _, _ = resample_geometry(orig_freq, new_freq)
    tile = lib().mfpa_resample_tile(o, n, width)
    check(min(tile, 0), "mfpa_resample_tile")
    return tile


@lru_cache(maxsize=256)                 # augmentation PitchShift's default set alone is 36 ratios (q <= 16 within +-4 semitones)
def _resample_taps_cached(o: int, n: int, device_index: int) -> torch.Tensor:
    _, _, width, ntaps, _ = resample_geometry(o, n)
    taps = np.empty((n, resample_tap_pitch(ntaps)), dtype=np.float32)
    check(lib().mfpa_resample_taps(o, n, width, RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF,
                                   taps.ctypes.data_as(ctypes.c_void_p)), "mfpa_resample_taps")
    return torch.from_numpy(taps).to(torch.device("cuda", device_index))


def resample_tap_pitch(ntaps: int) -> int:
    """MFPA_RESAMPLE_TAP_PITCH: floats from the taps of one phase to the next in the bank."""
    return (ntaps + RESAMPLE_TAP_ALIGN - 1) // RESAMPLE_TAP_ALIGN * RESAMPLE_TAP_ALIGN


def resample_taps(orig_freq: int, new_freq: int, device) -> torch.Tensor:
    """The filter bank of the pair of rates, phase-major (n, resample_tap_pitch(taps per phase)) float32 on `device`, zero behind
    the taps of each row (mfpa_resample_taps: built on the host in float64, uploaded once per (o, n, device))."""
    o, n, _, _, _ = resample_geometry(orig_freq, new_freq)
    device = torch.device(device)
    return _resample_taps_cached(o, n, device.index if device.index is not None else torch.cuda.current_device())


RESAMPLE_ANY_RATIO_HINT = ("the dense resampling kernel does not take this pair of rates (at most 1024 phases and 8192 taps per phase after "
                           "reduction by the gcd); pass any_ratio=True for the sparse-tap kernel, which takes every pair below 65536 Hz")


def resample_sparse_geometry(orig_freq: int, new_freq: int, T: int = 0) -> Tuple[int, int, int, int, int]:
    """(o, n, width, support, Tout) of the sparse-tap resampler for T input samples (mfpa_resample_sparse_geometry: host arithmetic).
    support = 2 * width + 1 rounded up to a multiple of 4: the taps it keeps per phase."""
    o, n, width, support = (ctypes.c_int(0) for _ in range(4))
    tout = ctypes.c_longlong(0)
    check(lib().mfpa_resample_sparse_geometry(int(orig_freq), int(new_freq), RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, int(T),
                                              ctypes.addressof(o), ctypes.addressof(n), ctypes.addressof(width), ctypes.addressof(support),
                                              ctypes.addressof(tout)), "mfpa_resample_sparse_geometry")
    return o.value, n.value, width.value, support.value, int(tout.value)


def resample_sparse_tile(orig_freq: int, new_freq: int) -> int:
    """Consecutive output samples one workgroup of the sparse-tap resampling kernel owns for this pair of rates."""
    o, n, width, _, _ = resample_sparse_geometry(orig_freq, new_freq)
    tile = lib().mfpa_resample_sparse_tile(o, n, width)
    check(min(tile, 0), "mfpa_resample_sparse_tile")
    return tile


@lru_cache(maxsize=64)                  # 8979 : 8000 is 512 KB; the largest table (65536 phases of 512 taps) is 128 MB
def _resample_sparse_taps_cached(o: int, n: int, device_index: int) -> Tuple[torch.Tensor, torch.Tensor]:
    _, _, width, support, _ = resample_sparse_geometry(o, n)
    taps = np.empty((n, support), dtype=np.float32)
    first = np.empty((n,), dtype=np.int32)
    check(lib().mfpa_resample_sparse_taps(o, n, width, RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, taps.ctypes.data_as(ctypes.c_void_p),
                                          first.ctypes.data_as(ctypes.c_void_p)), "mfpa_resample_sparse_taps")
    dev = torch.device("cuda", device_index)
    return torch.from_numpy(taps).to(dev), torch.from_numpy(first).to(dev)


def resample_sparse_taps(orig_freq: int, new_freq: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(taps (n, support) float32, first (n,) int32) on `device`: row i holds taps first[i] .. first[i] + support - 1 of phase i of the
    dense bank, every tap it leaves out being 0.0f (mfpa_resample_sparse_taps proves it; built on the host, uploaded once per
    (o, n, device))."""
    o, n, _, _, _ = resample_sparse_geometry(orig_freq, new_freq)
    device = torch.device(device)
    return _resample_sparse_taps_cached(o, n, device.index if device.index is not None else torch.cuda.current_device())


def resample_kernel_for(orig_freq: int, new_freq: int, any_ratio: bool = False, kernel: Optional[str] = None) -> str:
    """"dense" or "sparse": the kernel a pair of rates takes -- the dense one unless kernel="sparse" forces the sparse one, or
    any_ratio=True and the dense kernel refuses the pair.  A pair that is left without a kernel is a ValueError; without any_ratio
    its text names the flag."""
    if kernel not in (None, "dense", "sparse"):
        raise ValueError(f'kernel must be None, "dense" or "sparse", got {kernel!r}')
    if kernel == "sparse":
        resample_sparse_geometry(orig_freq, new_freq)
        return "sparse"
    try:
        resample_geometry(orig_freq, new_freq)
        return "dense"
    except ValueError:
        if kernel == "dense" or not any_ratio:
            raise ValueError(f"resample({orig_freq}, {new_freq}): {RESAMPLE_ANY_RATIO_HINT}") from None
    resample_sparse_geometry(orig_freq, new_freq)
    return "sparse"


def resample(wav: torch.Tensor, orig_freq: int, new_freq: int, *, any_ratio: bool = False, kernel: Optional[str] = None) -> torch.Tensor:
    """torchaudio.transforms.Resample(orig_freq, new_freq) of (B, T) float32 on the GPU -> (B, ceil(T * new / orig)).  Equal rates
    return `wav` itself, like torchaudio.  any_ratio=True: a pair of rates the dense kernel refuses (more than 1024 phases or 8192
    taps per phase) takes the sparse-tap kernel, which walks only the taps that are not zero; a pair the dense kernel takes still
    takes it.  kernel="sparse" forces the sparse kernel for any pair it accepts (same float32 values as the dense kernel, up to the
    sign of a zero); kernel="dense" and None are the default routing."""
    require_gpu(wav, "waveform")
    if wav.dim() != 2 or wav.dtype != torch.float32:
        raise ValueError("waveform must be (B, T) float32")
    if int(orig_freq) <= 0 or int(new_freq) <= 0:
        raise ValueError("Original frequency and desired frequecy should be positive")       # torchaudio's own message
    if int(orig_freq) == int(new_freq):
        return wav
    wav = wav.contiguous()
    B, T = wav.shape
    if resample_kernel_for(orig_freq, new_freq, any_ratio, kernel) == "sparse":
        o, n, width, support, Tout = resample_sparse_geometry(orig_freq, new_freq, T)
        out = torch.empty((B, Tout), dtype=torch.float32, device=wav.device)
        if B == 0 or Tout == 0:
            return out
        taps, first = resample_sparse_taps(orig_freq, new_freq, wav.device)
        check(lib().mfpa_resample_sparse(ptr(wav), B, T, T, o, n, width, support, ptr(taps), ptr(first), ptr(out), Tout, Tout, stream()),
              "mfpa_resample_sparse")
        return out
    o, n, width, _, Tout = resample_geometry(orig_freq, new_freq, T)
    out = torch.empty((B, Tout), dtype=torch.float32, device=wav.device)
    if B == 0 or Tout == 0:
        return out
    taps = resample_taps(orig_freq, new_freq, wav.device)
    check(lib().mfpa_resample(ptr(wav), B, T, T, o, n, width, ptr(taps), ptr(out), Tout, Tout, stream()), "mfpa_resample")
    return out


# ----------------------------------------------------------------------------- training segments (csrc/segments.hip)
SEGMENT_MAX_PER_TRACK = 8192           # MFPA_SEGMENT_MAX_PER_TRACK
SEGMENT_DBS_THRESHOLD = -7.5           # training/dataset.py:89


def segment_geometry(lengths, L: int, S: int) -> np.ndarray:
    """Exclusive prefix (n_tracks + 1 int32, on the HOST) of the segments per track, 1 + (N - L) // S or 0 when N < L
    (tf.signal.frame without end padding, training/dataset.py:78-82).  mfpa_segment_geometry: host integers only."""
    lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int64).reshape(-1))
    seg_off = np.empty(lens.size + 1, dtype=np.int32)
    check(lib().mfpa_segment_geometry(lens.ctypes.data_as(ctypes.c_void_p), int(lens.size), int(L), int(S),
                                      seg_off.ctypes.data_as(ctypes.c_void_p)), "mfpa_segment_geometry")
    return seg_off


def segment_threshold(dbs_threshold: float = SEGMENT_DBS_THRESHOLD) -> float:
    """thr of mfpa_segment_select: 10 * ln(rms_seg / rms_ref) > dbs  <=>  meansq_seg > exp(dbs / 5) * meansq_ref."""
    return float(np.exp(np.float64(dbs_threshold) / 5.0))


def _segment_meta(off: torch.Tensor, lens: torch.Tensor, seg_off: torch.Tensor) -> int:
    for t, dt, name in ((off, torch.int64, "off"), (lens, torch.int64, "lens"), (seg_off, torch.int32, "seg_off")):
        require_gpu(t, name)
        if t.dtype != dt or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D {dt} tensor")
    if off.numel() != lens.numel() or seg_off.numel() != lens.numel() + 1:
        raise ValueError("off and lens hold one entry per track, seg_off one more")
    return int(lens.numel())


def segment_stats(bank: torch.Tensor, off: torch.Tensor, lens: torch.Tensor, seg_off: torch.Tensor, n_seg: int, L: int,
                  S: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(seg_sumsq (n_seg,) float64, trk_sumsq (n_tracks,) float64, trk_peak (n_tracks,) float32) of the tracks
    bank[off[i] : off[i] + lens[i]]; off / lens (int64) and seg_off (int32, segment_geometry's, uploaded) are device tensors and
    n_seg = seg_off[-1] is the host's copy of it.  Each value is bit for bit a function of its own samples."""
    require_gpu(bank, "bank")
    if bank.dtype != torch.float32 or bank.dim() != 1:
        raise ValueError("bank must be a 1-D float32 tensor")
    n = _segment_meta(off, lens, seg_off)
    seg_sumsq = torch.empty((int(n_seg),), dtype=torch.float64, device=bank.device)
    trk_sumsq = torch.empty((n,), dtype=torch.float64, device=bank.device)
    trk_peak = torch.empty((n,), dtype=torch.float32, device=bank.device)
    # an empty bank has no address: hand the kernel a valid one it never reads (every track is then empty)
    check(lib().mfpa_segment_stats(ptr(bank) if bank.numel() else ptr(trk_peak), ptr(off), ptr(lens), ptr(seg_off), n, int(L), int(S),
                                   ptr(seg_sumsq) if n_seg else ptr(trk_sumsq), ptr(trk_sumsq), ptr(trk_peak), stream()),
          "mfpa_segment_stats")
    return seg_sumsq, trk_sumsq, trk_peak


def segment_select(seg_sumsq: torch.Tensor, trk_sumsq: torch.Tensor, trk_peak: torch.Tensor, off: torch.Tensor, lens: torch.Tensor,
                   seg_off: torch.Tensor, L: int, S: int, keys: torch.Tensor, dbs_threshold: float = SEGMENT_DBS_THRESHOLD,
                   n_keep: int = 1, do_norm: bool = True, with_mask: bool = False):
    """The reference's select_no_silence_frames + shuffle(...)[:n_keep] per track (training/dataset.py:86-122): returns
    (sel (n_tracks * n_keep,) int32, src (...) int64, div (...) float32, kept (n_tracks,) int32[, mask (n_seg,) uint8]).
    `keys`: one uint32 per segment (an int32 tensor holding the bit patterns is taken as such), drawn before the mask is known;
    the winners of a track are its kept segments in ascending (key, index) order."""
    n = _segment_meta(off, lens, seg_off)
    require_gpu(keys, "keys")
    if keys.dim() != 1 or keys.element_size() != 4 or keys.numel() != seg_sumsq.numel():
        raise ValueError("keys must hold one 32-bit integer per segment")
    if int(n_keep) < 1:
        raise ValueError("n_keep must be at least 1")
    dev = seg_sumsq.device
    rows = n * int(n_keep)
    sel = torch.empty((rows,), dtype=torch.int32, device=dev)
    src = torch.empty((rows,), dtype=torch.int64, device=dev)
    div = torch.empty((rows,), dtype=torch.float32, device=dev)
    kept = torch.empty((n,), dtype=torch.int32, device=dev)
    mask = torch.empty((seg_sumsq.numel(),), dtype=torch.uint8, device=dev) if with_mask else None
    ns = seg_sumsq.numel()
    check(lib().mfpa_segment_select(ptr(seg_sumsq) if ns else ptr(trk_sumsq), ptr(trk_sumsq), ptr(trk_peak), ptr(off), ptr(lens),
                                    ptr(seg_off), n, int(L), int(S), ptr(keys) if ns else ptr(trk_peak),
                                    segment_threshold(dbs_threshold), int(n_keep), 1 if do_norm else 0, ptr(sel), ptr(src), ptr(div),
                                    ptr(kept), ptr(mask) if ns else 0, stream()), "mfpa_segment_select")
    return (sel, src, div, kept, mask) if with_mask else (sel, src, div, kept)


def segment_gather(bank: torch.Tensor, src: torch.Tensor, div: Optional[torch.Tensor], L: int,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[r] = bank[src[r] : src[r] + L] / div[r] (float32 division; a copy without `div`); rows with src[r] < 0 keep what `out`
    held (a fresh `out` is zero there).  The caller guarantees src[r] + L <= len(bank): nothing here reads the device to check."""
    require_gpu(bank, "bank")
    require_gpu(src, "src")
    if bank.dtype != torch.float32 or bank.dim() != 1 or src.dtype != torch.int64 or src.dim() != 1:
        raise ValueError("bank must be 1-D float32 and src 1-D int64")
    if div is not None and (div.dtype != torch.float32 or div.shape != src.shape):
        raise ValueError("div must be float32, one per row")
    rows, L = int(src.numel()), int(L)
    if out is None:
        out = torch.zeros((rows, L), dtype=torch.float32, device=bank.device)
    elif (out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != rows or out.shape[1] < L or out.stride(1) != 1
          or (rows > 1 and out.stride(0) < L)):
        raise ValueError("out must be (rows, >= L) float32 with unit stride along a row and a row pitch of at least L")
    if rows == 0 or bank.numel() == 0:
        return out
    first = out.as_strided((1,), (1,))                                   # `out` may be the first L columns of a wider buffer
    check(lib().mfpa_segment_gather(ptr(bank), ptr(src), ptr(div), rows, L, ptr(first), int(out.stride(0)) if rows > 1 else L,
                                    stream()), "mfpa_segment_gather")
    return out


# ----------------------------------------------------------------------------- Audfprint picker
# testing/parameters.py:17-26 (afp_settings["audfprint"])
AUDFPRINT_DENSITY = 20
AUDFPRINT_MAX_PKS = 5
AUDFPRINT_F_SD = 30.0
AUDFPRINT_POLE = 0.98


def audfprint_a_dec(density: float = AUDFPRINT_DENSITY, n_hop: int = N_HOP) -> float:
    """peak_extractor.py:295."""
    return float(1 - 0.01 * (density * np.sqrt(n_hop / 352.8) / 35))


@lru_cache(maxsize=16)
def _gauss_cached(npoints: int, width: float, device_index: int) -> torch.Tensor:
    # peak_extractor.py:163-165 -- computed with numpy on the host so the table is numpy's, bit for bit
    tab = np.exp(-0.5 * ((np.arange(-npoints, npoints + 1) / width) ** 2))
    return torch.from_numpy(tab).to(torch.device("cuda", device_index))


def gauss_table(npoints: int, width: float, device) -> torch.Tensor:
    device = torch.device(device)
    return _gauss_cached(int(npoints), float(width),
                         device.index if device.index is not None else torch.cuda.current_device())


def audfprint_prepare(spec: torch.Tensor, denom: Optional[torch.Tensor] = None, mean_order: int = 0,
                      log_input: bool = False, pole: float = AUDFPRINT_POLE, denom_is_clip_max: bool = False,
                      float32_log: str = "rounded") -> torch.Tensor:
    """(B, F, T) spectrogram -> frame-major filtered log-spectrogram (B, T, F-1) float64.  `denom_is_clip_max`: denom[b] is the
    maximum of the float64 spec[b] itself (what stft_mag returned with it), so the kernel skips its max pass.  `float32_log`
    ("rounded" | "numpy", float32 spectrograms without `log_input` only): which float32 logarithm, see _float32_log_code."""
    nplog = 4 * _float32_log_code(float32_log)
    require_gpu(spec, "spectrogram")
    if spec.dim() != 3:
        raise ValueError("spectrogram must be (B, F, T)")
    spec = spec.contiguous()
    B, F, T = spec.shape
    if F < 2 or F - 1 > 256 or T < 1:
        raise ValueError("need 2 <= F <= 257 bins and T >= 1 frames")
    if denom is not None and (denom.shape != (B,) or denom.dtype != torch.float64):
        raise ValueError("denom must be (B,) float64")
    filtered = torch.empty((B, T, F - 1), dtype=torch.float64, device=spec.device)
    scratch = torch.empty((B, F * T), dtype=torch.float64, device=spec.device)
    check(lib().mfpa_audfprint_prepare(ptr(spec), _dtype_code(spec), B, F, T, ptr(denom), int(mean_order),
                                       int(bool(log_input)) | (2 if (denom_is_clip_max and denom is not None and spec.dtype == torch.float64) else 0) | nplog,
                                       float(pole), ptr(filtered), ptr(scratch), stream()),
          "mfpa_audfprint_prepare")
    return filtered


def audfprint_prune(filtered: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                    f_sd: float = AUDFPRINT_F_SD):
    """Frame-major filtered (B, T, R) float64 -> (mask (B, R, T) uint8, npeaks (B,) int32)."""
    require_gpu(filtered, "filtered spectrogram")
    if filtered.dim() != 3 or filtered.dtype != torch.float64:
        raise ValueError("filtered must be (B, T, R) float64")
    filtered = filtered.contiguous()
    B, T, R = filtered.shape
    if R % 4 or R < 4 or R > 256 or T < 1 or T > 1500 or not (1 <= maxpks <= 8):
        raise ValueError("unsupported pruner shape (R % 4 == 0, R <= 256, T <= 1500, maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    gauss = gauss_table(R, f_sd, filtered.device)
    mask = torch.empty((B, R, T), dtype=torch.uint8, device=filtered.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=filtered.device)
    check(lib().mfpa_audfprint_prune(ptr(filtered), B, R, T, ptr(gauss), float(a_dec), int(maxpks), ptr(mask),
                                     ptr(npeaks), stream()), "mfpa_audfprint_prune")
    return mask, npeaks


def audfprint_pick(mag: torch.Tensor, clip_max: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                   f_sd: float = AUDFPRINT_F_SD, pole: float = AUDFPRINT_POLE):
    """find_peaks without a denoiser, stages 1 + 2 in one call (mfpa_audfprint_pick): raw float64 |STFT| (B, F, T) and its per-clip
    maxima (what stft_mag returned) -> (mask (B, F-1, T) uint8, npeaks (B,) int32).  Same arithmetic as
    audfprint_prepare(mag, clip_max, mean_order=1, denom_is_clip_max=True) + audfprint_prune; the filtered spectrogram is never
    written (the pruner filters the frames as it walks them)."""
    require_gpu(mag, "spectrogram")
    if mag.dim() != 3 or mag.dtype != torch.float64:
        raise ValueError("spectrogram must be (B, F, T) float64")
    mag = mag.contiguous()
    B, F, T = mag.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    if F < 141 or F > 257 or (F - 1) % 4 or T < 1 or T > 512 or ((F - 1) * T) % 16 or not (1 <= maxpks <= 8):
        raise ValueError("unsupported shape for the fused picker (141 <= F <= 257, (F - 1) % 4 == 0, T <= 512, maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    gauss = gauss_table(F - 1, f_sd, mag.device)
    work = torch.empty(B * F * T + B * 128, dtype=torch.float64, device=mag.device)
    mask = torch.empty((B, F - 1, T), dtype=torch.uint8, device=mag.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=mag.device)
    check(lib().mfpa_audfprint_pick(ptr(mag), ptr(clip_max), B, F, T, float(pole), ptr(gauss), float(a_dec), int(maxpks), ptr(work),
                                    ptr(mask), ptr(npeaks), stream()), "mfpa_audfprint_pick")
    return mask, npeaks


TRACK_MAX_FRAMES = 16384          # HashTable keeps 14 time bits (hash_table.py:55 of the reference): frame times below 2^14 do not wrap


def audfprint_pick_track(mag: torch.Tensor, clip_max: torch.Tensor, a_dec: Optional[float] = None, maxpks: int = AUDFPRINT_MAX_PKS,
                         f_sd: float = AUDFPRINT_F_SD, pole: float = AUDFPRINT_POLE):
    """audfprint_pick for whole tracks (mfpa_audfprint_pick_track): raw float64 |STFT| (B, F, T) with 1 <= T <= 16384 frames and its
    per-clip maxima -> (mask (B, F-1, T) uint8, npeaks (B,) int32).  The same arithmetic, value for value; the pruner's event list
    lives in a workspace allocated here (T * maxpks * 12 + 4 * (T + 2) bytes per clip) instead of LDS."""
    require_gpu(mag, "spectrogram")
    if mag.dim() != 3 or mag.dtype != torch.float64:
        raise ValueError("spectrogram must be (B, F, T) float64")
    mag = mag.contiguous()
    B, F, T = mag.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    if F < 141 or F > 257 or (F - 1) % 4 or T < 1 or T > TRACK_MAX_FRAMES or not (1 <= maxpks <= 8):
        raise ValueError(f"unsupported shape for the track picker (141 <= F <= 257, (F - 1) % 4 == 0, 1 <= T <= {TRACK_MAX_FRAMES}, "
                         "maxpks <= 8)")
    if a_dec is None:
        a_dec = audfprint_a_dec()
    dev = mag.device
    gauss = gauss_table(F - 1, f_sd, dev)
    nchunks = (F * T + 8191) // 8192
    logs = torch.empty((B, T, F), dtype=torch.float64, device=dev)
    sums = torch.empty((B, 2 * nchunks), dtype=torch.float64, device=dev)
    events = torch.empty(max(1, (B * (T * maxpks * 12 + 4 * (T + 2)) + 7) // 8), dtype=torch.float64, device=dev)
    mask = torch.empty((B, F - 1, T), dtype=torch.uint8, device=dev)
    npeaks = torch.empty((B,), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_pick_track(ptr(mag), ptr(clip_max), B, F, T, float(pole), ptr(gauss), float(a_dec), int(maxpks),
                                          ptr(logs), ptr(sums), ptr(events), ptr(mask), ptr(npeaks), stream()),
          "mfpa_audfprint_pick_track")
    return mask, npeaks


# ----------------------------------------------------------------------------- Dejavu picker
DEJAVU_RADIUS = 10   # afp/dejavu/variables.py:19 PEAK_NEIGHBORHOOD_SIZE
DEJAVU_AMP_MIN = 50  # testing/parameters.py:32


def dejavu_prepare(psd: torch.Tensor, denom: Optional[torch.Tensor], scale: float = 10.0,
                   mean_order: int = 1) -> torch.Tensor:
    require_gpu(psd, "psd")
    if psd.dim() != 3 or psd.dtype != torch.float64:
        raise ValueError("psd must be (B, F, T) float64")
    psd = psd.contiguous()
    B, F, T = psd.shape
    arr = torch.empty_like(psd)
    check(lib().mfpa_dejavu_prepare(ptr(psd), B, F, T, ptr(denom), float(scale), int(mean_order), ptr(arr), stream()),
          "mfpa_dejavu_prepare")
    return arr


def dejavu_pick(psd: torch.Tensor, clip_max: torch.Tensor, scale: float = 10.0, mean_order: int = 1, radius: int = DEJAVU_RADIUS,
                amp_min: float = DEJAVU_AMP_MIN):
    """The un-denoised Dejavu chain after the spectrogram in one call (mfpa_dejavu_pick): PSD (B, F, T) float64 and its per-clip
    maxima (what specgram_psd returned) -> (mask (B, F, T) uint8, npeaks (B,) int32).  Same arithmetic as
    dejavu_prepare(psd, clip_max, scale, mean_order) + localmax2d; the mean-subtracted array is never written."""
    require_gpu(psd, "psd")
    if psd.dim() != 3 or psd.dtype != torch.float64:
        raise ValueError("psd must be (B, F, T) float64")
    psd = psd.contiguous()
    B, F, T = psd.shape
    if clip_max.shape != (B,) or clip_max.dtype != torch.float64:
        raise ValueError("clip_max must be (B,) float64")
    per = ctypes.c_longlong(0)
    check(lib().mfpa_dejavu_pick_work_doubles(F, T, ctypes.byref(per)), "mfpa_dejavu_pick_work_doubles")
    work = torch.empty(max(B, 1) * per.value, dtype=torch.float64, device=psd.device)
    mask = torch.empty((B, F, T), dtype=torch.uint8, device=psd.device)
    npeaks = torch.empty(B, dtype=torch.int32, device=psd.device)
    check(lib().mfpa_dejavu_pick(ptr(psd), ptr(clip_max), B, F, T, float(scale), int(mean_order), int(radius), float(amp_min),
                                 ptr(work), ptr(mask), ptr(npeaks), stream()), "mfpa_dejavu_pick")
    return mask, npeaks


def dejavu_prepare_f32(x: torch.Tensor, square: bool = True, scale: float = 10.0, mean_order: int = 0,
                       float32_log: str = "rounded") -> torch.Tensor:
    """The denoised branch of Dejavu's pre-processing (fingerprint.py:70-79): float32 (B, F, T) network output -> x**2 ->
    10*log(max(., max/1e6)) - mean in float32, widened to float64 for the picker.  `float32_log` ("rounded" | "numpy"): which
    float32 logarithm, see _float32_log_code."""
    log_mode = _float32_log_code(float32_log)
    require_gpu(x, "x")
    if x.dim() != 3 or x.dtype != torch.float32:
        raise ValueError("x must be (B, F, T) float32")
    x = x.contiguous()
    B, F, T = x.shape
    arr = torch.empty((B, F, T), dtype=torch.float64, device=x.device)
    check(lib().mfpa_dejavu_prepare_f32_ex(ptr(x), B, F, T, int(bool(square)), float(scale), int(mean_order), log_mode, ptr(arr),
                                           stream()), "mfpa_dejavu_prepare_f32_ex")
    return arr


def localmax2d(arr: torch.Tensor, radius: int = DEJAVU_RADIUS, amp_min: float = DEJAVU_AMP_MIN):
    require_gpu(arr, "arr2D")
    if arr.dim() != 3 or arr.dtype != torch.float64:
        raise ValueError("arr must be (B, F, T) float64")
    arr = arr.contiguous()
    B, F, T = arr.shape
    if not (0 <= radius <= 16) or F < 1 or T < 1:
        raise ValueError("radius must be in [0, 16]")
    mask = torch.empty((B, F, T), dtype=torch.uint8, device=arr.device)
    npeaks = torch.empty((B,), dtype=torch.int32, device=arr.device)
    check(lib().mfpa_localmax2d(ptr(arr), B, F, T, int(radius), float(amp_min), ptr(mask), ptr(npeaks), stream()),
          "mfpa_localmax2d")
    return mask, npeaks


# ----------------------------------------------------------------------------- metrics
def peak_metrics_counts(predicted: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """0/1 uint8 masks (B, N1, N2) -> (B, 4) int64 [hits_p, n_pred, hits_r, n_gt]."""
    require_gpu(predicted, "predicted")
    require_gpu(gt, "gt")
    if predicted.shape != gt.shape or predicted.dim() != 3:
        raise ValueError("masks must both be (B, N1, N2)")
    if predicted.dtype != torch.uint8 or gt.dtype != torch.uint8:
        raise TypeError("masks must be uint8")
    predicted, gt = predicted.contiguous(), gt.contiguous()
    B, N1, N2 = predicted.shape
    if N1 < 2 or N2 < 2:
        raise ValueError("mask axes must have length >= 2")
    counts = torch.empty((B, 4), dtype=torch.int64, device=predicted.device)
    check(lib().mfpa_peak_metrics(ptr(predicted), ptr(gt), B, N1, N2, ptr(counts), stream()), "mfpa_peak_metrics")
    return counts


# ----------------------------------------------------------------------------- landmarks / hashes
def audfprint_landmarks(mask: torch.Tensor, cap: int = 4096, mindt: int = 2, targetdt: int = 63, targetdf: int = 31,
                        maxpairs: int = 3):
    """Peak masks (B, R, T) uint8 -> (landmarks (B,cap,4), hashes (B,cap,2), unique sorted hashes (B,cap,2),
    counts (B,2) = [n_landmarks, n_unique]); all int32 on the device.  peak_extractor.py:313-346, :40-58, :443-460."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, R, T) uint8")
    mask = mask.contiguous()
    B, R, T = mask.shape
    if not (1 <= cap <= 8192) or R > 256:
        raise ValueError("cap must be in [1, 8192] and R <= 256")
    dev = mask.device
    lm = torch.zeros((B, cap, 4), dtype=torch.int32, device=dev)
    hs = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    uq = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_landmarks(ptr(mask), B, R, T, cap, mindt, targetdt, targetdf, maxpairs, ptr(lm), ptr(hs),
                                         ptr(uq), ptr(counts), stream()), "mfpa_audfprint_landmarks")
    return lm, hs, uq, counts


def audfprint_landmarks_track(mask: torch.Tensor, cap: int, mindt: int = 2, targetdt: int = 63, targetdf: int = 31, maxpairs: int = 3,
                              want_lists: bool = False):
    """audfprint_landmarks for whole tracks (mfpa_audfprint_landmarks_track): peak masks (B, R, T) uint8 with T <= 16384 and any
    capacity `cap` -> (landmarks (B,cap,4) | None, hashes (B,cap,2) | None, unique sorted hashes (B,cap,2), counts (B,2)); the two
    list-order outputs only with `want_lists`.  counts is [-1, -1] for a clip with more than 8 peaks in a frame or more than `cap`
    landmarks."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, R, T) uint8")
    mask = mask.contiguous()
    B, R, T = mask.shape
    if cap < 1 or R > 256 or R % 4 or T < 1 or T > TRACK_MAX_FRAMES:
        raise ValueError(f"cap must be >= 1, R <= 256 with R % 4 == 0 and 1 <= T <= {TRACK_MAX_FRAMES}")
    dev = mask.device
    lm = torch.zeros((B, cap, 4), dtype=torch.int32, device=dev) if want_lists else None
    hs = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev) if want_lists else None
    uq = torch.zeros((B, cap, 2), dtype=torch.int32, device=dev)
    counts = torch.zeros((B, 2), dtype=torch.int32, device=dev)
    tiles = torch.empty((B, (T + 255) // 256, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_landmarks_track(ptr(mask), B, R, T, int(cap), mindt, targetdt, targetdf, maxpairs, ptr(tiles), ptr(lm),
                                               ptr(hs), ptr(uq), ptr(counts), stream()), "mfpa_audfprint_landmarks_track")
    return lm, hs, uq, counts


def dejavu_hashes(mask: torch.Tensor, cap: int = 4096, peak_cap: int = 4096, fan_value: int = 3, min_dt: int = 0,
                  max_dt: int = 200):
    """Peak masks (B, F, T) uint8 -> (digests (B,cap,10) uint8 = sha1("f1|f2|dt")[:20 hex], t1 (B,cap) int32,
    counts (B,) int32).  afp/dejavu/fingerprint.py:174-213."""
    require_gpu(mask, "mask")
    if mask.dim() != 3 or mask.dtype != torch.uint8:
        raise ValueError("mask must be (B, F, T) uint8")
    mask = mask.contiguous()
    B, F, T = mask.shape
    dev = mask.device
    dig = torch.zeros((B, cap, 10), dtype=torch.uint8, device=dev)
    t1 = torch.zeros((B, cap), dtype=torch.int32, device=dev)
    counts = torch.zeros((B,), dtype=torch.int32, device=dev)
    check(lib().mfpa_dejavu_hashes(ptr(mask), B, F, T, cap, peak_cap, fan_value, min_dt, max_dt, ptr(dig), ptr(t1),
                                   ptr(counts), stream()), "mfpa_dejavu_hashes")
    return dig, t1, counts


def psnr_stats(pred: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """(B, ...) pred (float32|float64) vs float64 target -> (B, 3) float64 [sse, min(target), max(target)]."""
    require_gpu(pred, "pred")
    require_gpu(target, "target")
    if pred.shape != target.shape or target.dtype != torch.float64:
        raise ValueError("pred/target must have the same shape, target float64")
    pred, target = pred.contiguous(), target.contiguous()
    B = pred.shape[0]
    n = pred[0].numel() if B else 0
    out = torch.empty((B, 3), dtype=torch.float64, device=pred.device)
    check(lib().mfpa_psnr_stats(ptr(pred), _dtype_code(pred), ptr(target), B, n, ptr(out), stream()), "mfpa_psnr_stats")
    return out


# ----------------------------------------------------------------------------- Audfprint hash table / matcher
def audfprint_store(table: torch.Tensor, counts: torch.Tensor, rows: torch.Tensor, ids: torch.Tensor, seed: int = 0,
                    timebits: int = 14) -> None:
    """HashTable.store (hash_table.py:72-113) of N entries in arrival order, in place: table (2^hashbits, depth) int32
    (bit pattern of the reference's uint32), counts (2^hashbits,) int32, rows (N, 2) int32 (time, hash), ids (N,) int32.
    Torch only groups the entries by bucket (a stable sort); the slot assignment and the reservoir step run in the kernel."""
    for t, name in ((table, "table"), (counts, "counts"), (rows, "rows"), (ids, "ids")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if nb != 1 << hashbits or counts.shape != (nb,):
        raise ValueError("table must have 2^hashbits rows and counts one entry per row")
    N = rows.shape[0]
    if rows.shape != (N, 2) or ids.shape != (N,):
        raise ValueError("rows must be (N, 2) and ids (N,)")
    if N == 0:
        return
    bucket = rows[:, 1].to(torch.int64) & (nb - 1)
    sb, order = torch.sort(bucket, stable=True)
    _, seg_counts = torch.unique_consecutive(sb, return_counts=True)
    seg = torch.zeros(seg_counts.numel() + 1, dtype=torch.int32, device=rows.device)
    seg[1:] = torch.cumsum(seg_counts, 0)
    check(lib().mfpa_audfprint_store(ptr(rows.contiguous()), ptr(ids.contiguous()), ptr(order.contiguous()), ptr(seg),
                                     int(seg_counts.numel()), hashbits, timebits, depth, int(seed) & ((1 << 64) - 1),
                                     ptr(table), ptr(counts), stream()), "mfpa_audfprint_store")


def match_scratch_bytes(hcap: int, extended: bool = False) -> int:
    n = ctypes.c_longlong(0)
    name = "mfpa_audfprint_match_ex_scratch_bytes" if extended else "mfpa_audfprint_match_scratch_bytes"
    check(getattr(lib(), name)(int(hcap), ctypes.addressof(n)), name)
    return int(n.value)


def pow2_roundup_mask() -> int:
    """Bit k is set when encpowerof2(2^k) (audfprint_match.py:17-21: int(ceil(log(v) / log(2))) in numpy's float64) is
    k + 1, not k; the extended matcher reproduces encpowerof2 on the device from this mask."""
    mask = 0
    for k in range(32):
        if int(np.ceil(np.log(np.int64(1) << k) / np.log(2))) > k:
            mask |= 1 << k
    return mask


def audfprint_match(table: torch.Tensor, counts: torch.Tensor, hashesperid: torch.Tensor, hashes: torch.Tensor,
                    nq: torch.Tensor, k: int = 1, threshcount: int = 5, search_depth: int = 100, window: int = 2,
                    max_alignments_per_id: int = 100, hcap: int = 1 << 15, timebits: int = 14,
                    scratch_budget: int = 1 << 30, exact_count: bool = False, find_time_range: bool = False,
                    time_quantile: float = 0.05, hashesfor: Optional[int] = None, hashes_cap: int = 2048,
                    extended: Optional[bool] = None):
    """Matcher.match_hashes (audfprint_match.py:322-346) for B queries: hashes (B, cap, 2) int32 (time, hash) with nq (B,)
    valid rows each -> (rows (B, k, 7) int32 sorted by filtered count, info (B, 3) int32 [n_hits, rows written, rows in
    total], the hit capacity used).  A query with more hits than the scratch capacity is reported by the kernel and the
    batch runs again with a capacity that holds it: nothing is truncated.

    exact_count, find_time_range (with time_quantile) and hashesfor go through mfpa_audfprint_match_ex (`extended` forces
    that entry point, or the default one, regardless); they need cap <= 32768.  With hashesfor = r the
    result has two more members: (B, n, 2) int32 rows [time, hash] of the matching hashes of result row r, and (B,) int32
    their number per query (-1: the query has no row r); the buffer grows from hashes_cap until every list fits."""
    for t, name in ((table, "table"), (counts, "counts"), (hashesperid, "hashesperid"), (hashes, "hashes"), (nq, "nq")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if hashes.dim() != 3 or hashes.shape[2] != 2 or nq.shape != (hashes.shape[0],):
        raise ValueError("hashes must be (B, cap, 2) and nq (B,)")
    flags = (1 if exact_count else 0) | (2 if find_time_range else 0)
    if extended is None:
        extended = bool(flags) or hashesfor is not None
    elif not extended and (flags or hashesfor is not None):
        raise ValueError("exact_count, find_time_range and hashesfor need the extended entry point")
    if exact_count and threshcount < 1:
        raise ValueError("exact_count needs threshcount >= 1: with less, empty bins of the dt histogram would be modes")
    if not 0.0 <= time_quantile < 1.0:
        raise ValueError("time_quantile must lie in [0, 1)")
    if hashesfor is not None and hashesfor < 0:
        raise ValueError("hashesfor must be a row index >= 0")
    B, cap = hashes.shape[0], hashes.shape[1]
    if extended and cap > 1 << 15:
        raise ValueError(f"the extended matcher takes at most 32768 rows per query, not {cap}")
    dev = hashes.device
    out = torch.zeros((B, k, 7), dtype=torch.int32, device=dev)
    info = torch.zeros((B, 3), dtype=torch.int32, device=dev)
    want_hashes = hashesfor is not None
    hf = torch.zeros((B, hashes_cap, 2), dtype=torch.int32, device=dev) if want_hashes else None
    hf_n = torch.full((B,), -1, dtype=torch.int32, device=dev) if want_hashes else None

    def done():
        if not want_hashes:
            return out, info, hcap
        return out, info, hcap, hf[:, :max(0, int(hf_n.max())) if B else 0], hf_n

    if B == 0:
        return done()
    hashes, nq = hashes.contiguous(), nq.contiguous()
    p2mask = pow2_roundup_mask() if extended else 0
    while True:
        per_q = match_scratch_bytes(hcap, extended)
        chunk = max(1, min(B, scratch_budget // per_q))
        scratch = torch.empty(chunk * per_q, dtype=torch.uint8, device=dev)
        for s in range(0, B, chunk):
            e = min(B, s + chunk)
            head = (ptr(table), ptr(counts), ptr(hashesperid), hashesperid.numel(), hashbits, timebits, depth, ptr(hashes[s:e]),
                    ptr(nq[s:e]), e - s, cap, threshcount, search_depth, window, max_alignments_per_id)
            tail = (hcap, ptr(scratch), k, ptr(out[s:e]), ptr(info[s:e]), stream())
            if extended:
                check(lib().mfpa_audfprint_match_ex(*head, flags, float(time_quantile), p2mask, hashesfor if want_hashes else -1,
                                                    hf.shape[1] if want_hashes else 0, ptr(hf[s:e]) if want_hashes else None,
                                                    ptr(hf_n[s:e]) if want_hashes else None, *tail), "mfpa_audfprint_match_ex")
            else:
                check(lib().mfpa_audfprint_match(*head, *tail), "mfpa_audfprint_match")
        del scratch
        need = int(info[:, 0].max())
        if need > hcap:
            if need > 1 << 26:
                raise ValueError(f"a query has {need} table hits: more than the matcher's limit of 2^26 per query")
            while hcap < need:
                hcap <<= 1
            continue
        if want_hashes and int(hf_n.max()) > hf.shape[1]:              # a list longer than the buffer: reported, run again
            hf = torch.zeros((B, int(hf_n.max()), 2), dtype=torch.int32, device=dev)
            continue
        return done()


MAINTAIN_FULL_ROWS = 1          # MFPA_MAINTAIN_FULL_ROWS


def _maintain_table(table: torch.Tensor, counts: torch.Tensor):
    for t, name in ((table, "table"), (counts, "counts")):
        require_gpu(t, name)
        if t.dtype != torch.int32:
            raise TypeError(f"{name} must be int32")
    if table.dim() != 2:
        raise ValueError("table must be (2^hashbits, depth)")
    nb, depth = table.shape
    hashbits = nb.bit_length() - 1
    if nb != 1 << hashbits or counts.shape != (nb,):
        raise ValueError("table must have 2^hashbits rows and counts one entry per row")
    return hashbits, depth


def _maintain_ids(ids, limit: Optional[int]) -> np.ndarray:
    a = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
    if a.size and a.dtype.kind not in "iu":
        raise TypeError("ids must be integers")
    a = a.astype(np.int64).reshape(-1)
    if a.size and (int(a.min()) < 0 or (limit is not None and int(a.max()) >= limit)):
        raise ValueError("ids must lie in [0, n_ids)" if limit is not None else "ids must not be negative")
    return a


def audfprint_remove(table: torch.Tensor, counts: torch.Tensor, ids, n_ids: int, timebits: int = 14,
                     full_rows: bool = False) -> torch.Tensor:
    """HashTable.remove (hash_table.py:277-295) of a SET of ids in one pass over the table, in place -> removed (n_ids,)
    int32, the entries each id had.  The same table and counts as the reference's remove called once per id, in any order
    (mfpa_audfprint_remove; tables whose slots at or beyond min(counts, depth) are zero).  ids: integers in [0, n_ids)."""
    hashbits, depth = _maintain_table(table, counts)
    n_ids = int(n_ids)
    if n_ids < 0:
        raise ValueError("n_ids must not be negative")
    a = _maintain_ids(ids, n_ids)
    removed = torch.zeros(n_ids, dtype=torch.int32, device=table.device)
    if a.size == 0:
        return removed
    in_set = np.zeros(n_ids, np.uint8)
    in_set[a] = 1
    in_set = torch.from_numpy(in_set).to(table.device)
    check(lib().mfpa_audfprint_remove(ptr(table), ptr(counts), hashbits, int(timebits), depth, ptr(in_set), n_ids,
                                      MAINTAIN_FULL_ROWS if full_rows else 0, ptr(removed), stream()), "mfpa_audfprint_remove")
    return removed


def audfprint_retrieve(table: torch.Tensor, counts: torch.Tensor, ids, timebits: int = 14, full_rows: bool = False):
    """HashTable.retrieve (hash_table.py:297-316) of K distinct ids -> (rows (N, 2) int32 (time, hash) of all of them in
    request order, each id's by bucket then slot; offsets (K + 1,) int32: rows[offsets[k]:offsets[k + 1]] are ids[k]'s).
    Both stay on the device; the table is never copied, one integer (N) is read back to size `rows`."""
    hashbits, depth = _maintain_table(table, counts)
    a = _maintain_ids(ids, None)
    K = int(a.size)
    dev = table.device
    if len(np.unique(a)) != K:
        raise ValueError("ids must be distinct")
    if K == 0:
        return torch.zeros((0, 2), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    n_ids = int(a.max()) + 1
    rank = np.full(n_ids, -1, np.int32)
    rank[a] = np.arange(K, dtype=np.int32)
    rank = torch.from_numpy(rank).to(dev)
    n = ctypes.c_longlong(0)
    check(lib().mfpa_audfprint_retrieve_work_ints(hashbits, K, ctypes.addressof(n)), "mfpa_audfprint_retrieve_work_ints")
    work = torch.empty(int(n.value), dtype=torch.int32, device=dev)
    offsets = torch.empty(K + 1, dtype=torch.int32, device=dev)
    flags = MAINTAIN_FULL_ROWS if full_rows else 0
    head = (ptr(table), ptr(counts), hashbits, int(timebits), depth, ptr(rank), n_ids, K, flags, ptr(work), ptr(offsets))
    check(lib().mfpa_audfprint_retrieve_count(*head, stream()), "mfpa_audfprint_retrieve_count")
    n_rows = int(offsets[K])
    rows = torch.empty((n_rows, 2), dtype=torch.int32, device=dev)
    check(lib().mfpa_audfprint_retrieve(*head, ptr(rows), n_rows, stream()), "mfpa_audfprint_retrieve")
    return rows, offsets


# ----------------------------------------------------------------------------- Dejavu fingerprint store / matcher
DEJAVU_MAX_SID = (1 << 24) - 1        # song ids are packed into 24 bits of the matcher's sort key
DEJAVU_DIRBITS = 20


def _dejavu_dirbits(directory: torch.Tensor) -> int:
    nd = directory.numel() - 1
    dirbits = nd.bit_length() - 1
    if nd < 2 or nd != 1 << dirbits or directory.dtype != torch.int32:
        raise ValueError("directory must be (2^dirbits + 1,) int32")
    return dirbits


def dejavu_store(digests: torch.Tensor, sids: torch.Tensor, offsets: torch.Tensor, dirbits: int = DEJAVU_DIRBITS):
    """The fingerprints table of the SET of rows (digest (N,10) uint8, song id (N,) int32, offset (N,) int32):
    INSERT ... ON CONFLICT DO NOTHING under UNIQUE(song_id, offset, hash) (postgres_database.py:266-295) -> (table (M,5) int32
    sorted by (hash, sid, offset), directory (2^dirbits + 1,) int32).  Torch orders the rows (three stable sorts, least
    significant key first); deduplication, placement and the directory run in mfpa_dejavu_store."""
    for t, name, dt in ((digests, "digests", torch.uint8), (sids, "sids", torch.int32), (offsets, "offsets", torch.int32)):
        require_gpu(t, name)
        if t.dtype != dt:
            raise TypeError(f"{name} must be {dt}")
    N = digests.shape[0]
    if digests.shape != (N, 10) or sids.shape != (N,) or offsets.shape != (N,):
        raise ValueError("digests must be (N, 10), sids and offsets (N,)")
    dev = digests.device
    if N:
        if int(sids.min()) < 1 or int(sids.max()) > DEJAVU_MAX_SID:
            raise ValueError(f"song ids must lie in [1, {DEJAVU_MAX_SID}] (24 bits of the matcher's sort key)")
        if int(offsets.min()) < 0:
            raise ValueError("offsets must be >= 0")
    d = digests.to(torch.int64)
    hi = (d[:, 0] - 128) * (1 << 56)                       # bytes 0-7 in signed order = their unsigned byte order
    for i in range(1, 8):
        hi = hi + (d[:, i] << (56 - 8 * i))
    mid = (((d[:, 8] << 8) | d[:, 9]) << 24) | sids.to(torch.int64)
    order = torch.sort(offsets.to(torch.int64), stable=True).indices
    order = order[torch.sort(mid[order], stable=True).indices]
    order = order[torch.sort(hi[order], stable=True).indices]
    work = torch.empty(max(1, (N + 255) // 256), dtype=torch.int32, device=dev)
    table = torch.empty((max(N, 1), 5), dtype=torch.int32, device=dev)
    n_rows = torch.zeros(1, dtype=torch.int32, device=dev)
    directory = torch.empty((1 << dirbits) + 1, dtype=torch.int32, device=dev)
    check(lib().mfpa_dejavu_store(ptr(digests.contiguous()), ptr(sids.contiguous()), ptr(offsets.contiguous()), ptr(order),
                                  N, int(dirbits), ptr(work), ptr(table), ptr(n_rows), ptr(directory), stream()),
          "mfpa_dejavu_store")
    return table[: int(n_rows)].clone(), directory


def dejavu_table_digests(table: torch.Tensor) -> torch.Tensor:
    """(M,5) table rows -> their (M,10) uint8 digests (the words are big-endian, the tensors little-endian)."""
    M = table.shape[0]
    return table[:, :3].contiguous().view(torch.uint8).view(M, 3, 4).flip(-1).reshape(M, 12)[:, :10].contiguous()


def dejavu_lookup(table: torch.Tensor, directory: torch.Tensor, digests: torch.Tensor) -> torch.Tensor:
    """Row ranges (n, 2) int32 [first, end) of the table rows carrying each of the (n, 10) uint8 digests."""
    require_gpu(table, "table")
    require_gpu(directory, "directory")
    require_gpu(digests, "digests")
    dirbits = _dejavu_dirbits(directory)
    if digests.dtype != torch.uint8 or digests.dim() != 2 or digests.shape[1] != 10:
        raise ValueError("digests must be (n, 10) uint8")
    n = digests.shape[0]
    ranges = torch.zeros((n, 2), dtype=torch.int32, device=digests.device)
    check(lib().mfpa_dejavu_lookup(ptr(table.contiguous()), ptr(directory), dirbits, ptr(digests.contiguous()), n, ptr(ranges),
                                   stream()), "mfpa_dejavu_lookup")
    return ranges


def dejavu_match_scratch_bytes(cap: int, hcap: int) -> int:
    n = ctypes.c_longlong(0)
    check(lib().mfpa_dejavu_match_scratch_bytes(int(cap), int(hcap), ctypes.addressof(n)), "mfpa_dejavu_match_scratch_bytes")
    return int(n.value)


def dejavu_match(table: torch.Tensor, directory: torch.Tensor, digests: torch.Tensor, t1: torch.Tensor, nq: torch.Tensor,
                 k: int = 1, hcap: int = 1 << 15, scratch_budget: int = 1 << 30) -> Tuple[torch.Tensor, torch.Tensor, int]:
    """return_matches + align_matches (postgres_database.py:180-229, dejavu.py:312-378) for B queries, each the SET of its
    (digest, t1) pairs: digests (B,cap,10) uint8, t1 (B,cap) int32, nq (B,) int32 as mfpa_dejavu_hashes writes them ->
    (rows (B,k,4) int32 [sid, offset, count of the song's best offset, hashes_matched], info (B,4) int32 [n_hits,
    n_distinct_pairs, rows written, songs hit], the hit capacity used).  A query with more hits than the scratch capacity is
    reported by the kernel and the batch runs again with a capacity that holds it: nothing is truncated."""
    for t, name in ((table, "table"), (directory, "directory"), (digests, "digests"), (t1, "t1"), (nq, "nq")):
        require_gpu(t, name)
    dirbits = _dejavu_dirbits(directory)
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 5:
        raise ValueError("table must be (M, 5) int32")
    if digests.dtype != torch.uint8 or digests.dim() != 3 or digests.shape[2] != 10:
        raise ValueError("digests must be (B, cap, 10) uint8")
    B, cap = digests.shape[0], digests.shape[1]
    if t1.shape != (B, cap) or t1.dtype != torch.int32 or nq.shape != (B,) or nq.dtype != torch.int32:
        raise ValueError("t1 must be (B, cap) int32 and nq (B,) int32")
    dev = digests.device
    out = torch.zeros((B, k, 4), dtype=torch.int32, device=dev)
    info = torch.zeros((B, 4), dtype=torch.int32, device=dev)
    if B == 0:
        return out, info, hcap
    table = table if table.numel() else torch.zeros((1, 5), dtype=torch.int32, device=dev)   # never read: the directory is empty
    digests, t1, nq = digests.contiguous(), t1.contiguous(), nq.contiguous()
    while True:
        per_q = dejavu_match_scratch_bytes(cap, hcap)
        chunk = max(1, min(B, scratch_budget // per_q))
        scratch = torch.empty(chunk * per_q, dtype=torch.uint8, device=dev)
        for s in range(0, B, chunk):
            e = min(B, s + chunk)
            check(lib().mfpa_dejavu_match(ptr(table), ptr(directory), dirbits, ptr(digests[s:e]), ptr(t1[s:e]), ptr(nq[s:e]),
                                          e - s, cap, hcap, ptr(scratch), k, ptr(out[s:e]), ptr(info[s:e]), stream()),
                  "mfpa_dejavu_match")
        del scratch
        need = int(info[:, 0].max())
        if need <= hcap:
            return out, info, hcap
        if need > 1 << 26:
            raise ValueError(f"a query has {need} table hits: more than the matcher's limit of 2^26 per query")
        while hcap < need:
            hcap <<= 1


# ----------------------------------------------------------------------------- composable transforms (csrc/transforms.hip)
RFFT_MAX_N = 16384                     # MFPA_RFFT_MAX_N: N/2 complex points in one 64 KiB LDS buffer
RFFT_MAX_RADICES = 16                  # MFPA_RFFT_MAX_RADICES
FILTER_ZEROS = 8                       # julius' default; half = int(zeros / cutoff / 2)


def _current_gpu(device=None) -> torch.device:
    if not torch.cuda.is_available():
        raise _lib.MfpaError("no GPU: libmfpa has no CPU fallback")
    lib()
    device = torch.device("cuda" if device is None else device)
    return torch.device("cuda", device.index if device.index is not None else torch.cuda.current_device())


def _host_f64(v) -> torch.Tensor:
    return (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float64)).to(torch.float64).reshape(-1)


def _upload(t: torch.Tensor, dev) -> torch.Tensor:
    """Host tensor -> device through a pinned buffer, without a stream synchronisation."""
    return t.contiguous().pin_memory().to(dev, non_blocking=True)


def bandpass_taps(cut_lo, cut_hi, device=None):
    """Band-pass taps (julius 0.2.7 BandPassFilter restated; parity unpinned) for B pairs of cut-offs, fractions of the sample
    rate with 0 < lo <= hi <= 0.5, given on the host.  Returns the arguments mfpa_fir wants, on the device:
    (taps, tap_off int64 (B,), ntaps int32 (B,), half int32 (B,)); example b owns taps[tap_off[b] : tap_off[b] + ntaps[b]],
    ntaps = 2 * half + 1, half = int(8 / lo / 2) from the cut-off as given (a float32 tensor's values, or Python floats in
    double); the taps themselves are float32 arithmetic on the float32 cut-offs."""
    dev = _current_gpu(device)
    lo, hi = _host_f64(cut_lo), _host_f64(cut_hi)
    if lo.shape != hi.shape:
        raise ValueError("cut_lo and cut_hi must have one entry per example")
    half = []
    for l, h in zip(lo.tolist(), hi.tolist()):
        if h > 0.5 or l > 0.5:
            raise ValueError("A cutoff above 0.5 does not make sense.")                  # julius' own message
        if not (0.0 < l <= h):
            raise ValueError(f"band cut-offs must satisfy 0 < low <= high, got ({l}, {h})")
        if FILTER_ZEROS / l / 2 >= 2 ** 30:
            raise ValueError(f"low cut-off {l}: more than 2^31 taps")
        half.append(int(FILTER_ZEROS / l / 2))
    B = len(half)
    ntaps = [2 * h + 1 for h in half]
    off = np.concatenate([[0], np.cumsum(ntaps)]).astype(np.int64)
    taps = torch.empty((int(off[-1]),), dtype=torch.float32, device=dev)
    off_d = _upload(torch.from_numpy(off[:-1].copy()), dev)
    ntaps_d, half_d = _upload(torch.tensor(ntaps, dtype=torch.int32), dev), _upload(torch.tensor(half, dtype=torch.int32), dev)
    lo_d, hi_d = _upload(lo.to(torch.float32), dev), _upload(hi.to(torch.float32), dev)
    if B:
        with torch.cuda.device(dev):
            check(lib().mfpa_bandpass_taps(ptr(lo_d), ptr(hi_d), ptr(half_d), ptr(off_d), B, ptr(taps),
                                           stream()), "mfpa_bandpass_taps")
    return taps, off_d, ntaps_d, half_d


def rfft_plan(N: int) -> Tuple[Tuple[int, ...], int]:
    """(radices of the N/2-point complex passes, LDS bytes of the workgroup) of the device real FFT, or ValueError for an N it
    does not take (mfpa_rfft_plan: host integers only)."""
    radices = (ctypes.c_int * RFFT_MAX_RADICES)()
    n, lds = ctypes.c_int(0), ctypes.c_int(0)
    N = int(N)
    if not -2 ** 31 <= N < 2 ** 31 or lib().mfpa_rfft_plan(N, ctypes.addressof(radices), ctypes.addressof(n),
                                                           ctypes.addressof(lds)) != 0:
        raise ValueError(f"the device FFT takes an even N with 4 <= N <= {RFFT_MAX_N} and N/2 = 2^a 3^b 5^c, not {N}")
    return tuple(radices[:n.value]), lds.value


@lru_cache(maxsize=16)
def _rfft_twiddles_cached(N: int, device_index: int) -> torch.Tensor:
    tw = np.empty(2 * N, dtype=np.float32)
    check(lib().mfpa_rfft_twiddles(N, tw.ctypes.data_as(ctypes.c_void_p)), "mfpa_rfft_twiddles")
    return torch.from_numpy(tw).to(torch.device("cuda", device_index))


def rfft_twiddles(N: int, device) -> torch.Tensor:
    """exp(-2 pi i q / N), q < N, as (2N,) float32 on `device` (mfpa_rfft_twiddles: float64 on the host, rounded once, uploaded
    once per (N, device))."""
    rfft_plan(N)
    return _rfft_twiddles_cached(int(N), _current_gpu(device).index)


def colored_noise(white: torch.Tensor, f_decay: torch.Tensor, num_samples: int) -> torch.Tensor:
    """AddColoredNoise._gen_noise for a batch: white (B, N) float32 normal draws and f_decay (B,) on the GPU -> (B, num_samples)
    unit-RMS noise with a 1/f^f_decay amplitude profile, one period of N samples tiled to num_samples."""
    _current_gpu()
    require_gpu(white, "white noise")
    require_gpu(f_decay, "f_decay")
    if white.dim() != 2 or white.dtype != torch.float32:
        raise ValueError("white must be (B, N) float32")
    B, N = white.shape
    rfft_plan(N)
    if f_decay.shape != (B,) or f_decay.dtype != torch.float32:
        raise ValueError("f_decay must be (B,) float32")
    T = int(num_samples)
    if not 1 <= T < 2 ** 31:
        raise ValueError("num_samples must be at least 1")
    white, f_decay = white.contiguous(), f_decay.contiguous()
    out = torch.empty((B, T), dtype=torch.float32, device=white.device)
    if B == 0:
        return out
    check(lib().mfpa_colored_noise(ptr(white), B, N, ptr(f_decay), T, ptr(rfft_twiddles(N, white.device)), ptr(out), stream()),
          "mfpa_colored_noise")
    return out


# ----------------------------------------------------------------------------- phase vocoder (csrc/vocoder.hip)
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
    r = _host_f64(rates)
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
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("out_dtype must be torch.float32 or torch.float64")
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


# ----------------------------------------------------------------------------- recursive filters (csrc/iir.hip)
SOS_MAX_SECTIONS = 8                   # MFPA_SOS_MAX_SECTIONS
SOS_MAX_SAMPLES = 1 << 30


def sos_normalized(sos) -> np.ndarray:
    """Second-order sections (S, 6) or (B, S, 6), rows b0 b1 b2 a0 a1 a2, as float64 on the host with every row divided by its a0
    (host arithmetic, no GPU).  ValueError: another shape, more than SOS_MAX_SECTIONS sections, a coefficient that is not finite,
    a0 == 0."""
    s = np.array(sos.detach().cpu().numpy() if isinstance(sos, torch.Tensor) else sos, dtype=np.float64)
    if s.ndim not in (2, 3) or s.shape[-1] != 6:
        raise ValueError(f"sos must be (S, 6) or (B, S, 6), got {s.shape}")
    if not 1 <= s.shape[-2] <= SOS_MAX_SECTIONS:
        raise ValueError(f"1 to {SOS_MAX_SECTIONS} sections per filter, got {s.shape[-2]}")
    if not np.all(np.isfinite(s)):
        raise ValueError("sos holds a coefficient that is not finite")
    if np.any(s[..., 3] == 0.0):
        raise ValueError("a section with a0 == 0")
    s = s / s[..., 3:4]
    s[..., 3] = 1.0
    if not np.all(np.isfinite(s)):
        raise ValueError("sos holds a coefficient that is not finite once divided by a0")
    return np.ascontiguousarray(s)


def sosfilt(wav: torch.Tensor, sos, *, apply=None, zi=None, clamp: bool = False):
    """scipy.signal.sosfilt along the rows of (B, T) float32 or float64 samples on the GPU: a cascade of up to 8 second-order
    sections in transposed direct form II, one filter for the batch (sos (S, 6)) or one per row ((B, S, 6)), in one launch.  State
    and arithmetic are float64; a float32 output is the float64 result rounded once.  `sos` (rows b0 b1 b2 a0 a1 a2) is read on the
    host and divided by a0.  `apply` (B,) of booleans: a row with a false entry comes back bit for bit.  `zi` (B, S, 2): scipy's
    initial state; with it the return value is (y, zf), zf (B, S, 2) float64 on the device.  clamp=True limits the output to
    [-1, 1] (torchaudio.functional.lfilter's default)."""
    s = sos_normalized(sos)
    if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError("waveform must be a (B, T) float32 or float64 tensor")
    B, T = wav.shape
    S = s.shape[-2]
    if s.ndim == 3 and s.shape[0] != B:
        raise ValueError(f"per-row sections must be ({B}, S, 6), got {s.shape}")
    if B > 65535 or T > SOS_MAX_SAMPLES:
        raise ValueError(f"at most 65535 rows of {SOS_MAX_SAMPLES} samples per call")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
    if zi is not None and (not isinstance(zi, torch.Tensor) or tuple(zi.shape) != (B, S, 2)):
        raise ValueError(f"zi must be a ({B}, {S}, 2) tensor")
    require_gpu(wav, "waveform")
    dev = wav.device
    wav = wav.contiguous()
    y = torch.empty_like(wav)
    zi_d = zf = None
    if zi is not None:
        zi_d = zi.to(device=dev, dtype=torch.float64).contiguous()
        zf = zi_d.clone()
    if B == 0 or T == 0:
        return y if zi is None else (y, zf)
    apply_d = None
    if apply is not None:
        a = torch.as_tensor(apply)
        apply_d = (a if a.is_cuda else _upload(a.to(torch.uint8), dev)).ne(0).to(torch.uint8).contiguous()
    per_row = int(s.ndim == 3)
    need = ctypes.c_longlong(0)
    check(lib().mfpa_sosfilt_work(B, S, per_row, ctypes.addressof(need)), "mfpa_sosfilt_work")
    work = torch.empty((need.value,), dtype=torch.float64, device=dev)
    sos_d = _upload(torch.from_numpy(s), dev)
    check(lib().mfpa_sosfilt(ptr(wav), _dtype_code(wav), B, T, ptr(sos_d), S, per_row, ptr(apply_d), ptr(zi_d), ptr(zf), int(bool(clamp)),
                             ptr(work), need.value, ptr(y), stream()), "mfpa_sosfilt")
    return y if zi is None else (y, zf)


# ----------------------------------------------------------------------------- room impulse responses (csrc/rir.hip)
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
    def host(v):
        return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    room, source, mic, absorption = host(room), host(source), host(mic), host(absorption)
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
    fs, c = float(sample_rate), float(sound_speed)
    if not (np.isfinite(fs) and fs > 0.0 and np.isfinite(c) and c > 0.0):
        raise ValueError(f"sample_rate and sound_speed must be finite and positive, got {sample_rate}, {sound_speed}")
    if B > RIR_MAX_ROOMS:
        raise ValueError(f"at most {RIR_MAX_ROOMS} rooms per call, got {B}")
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError("out_dtype must be torch.float32 or torch.float64")
    dev = _current_gpu(device)
    out = torch.empty((B, int(length)), dtype=out_dtype, device=dev)
    if B == 0:
        return out
    geom_d = _upload(torch.from_numpy(geom), dev)
    check(lib().mfpa_rir_shoebox(ptr(geom_d), B, int(max_order), int(length), fs, c, int(filter_len), int(bool(reversed)),
                                 int(out_dtype == torch.float64), ptr(out), int(length), stream()), "mfpa_rir_shoebox")
    return out


# ----------------------------------------------------------------------------- dynamic range compression (csrc/dynamics.hip)
DYNAMICS_MAX_SAMPLES = 1 << 30
DYNAMICS_PARAMS = ("threshold_db", "slope", "knee_db", "attack_coef", "release_coef", "makeup_db")


def time_coef(seconds, sample_rate):
    """The one-pole coefficient of a time constant: exp(-1 / (seconds * sample_rate)) in float64 on the host, 0 for a time of 0.  A
    float for a number, an array for an array.  ValueError: a time that is negative or not finite, a rate that is not positive."""
    s = np.asarray(seconds.detach().cpu().numpy() if isinstance(seconds, torch.Tensor) else seconds, dtype=np.float64)
    rate = float(sample_rate)
    if not (np.isfinite(rate) and rate > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    if not (np.all(np.isfinite(s)) and np.all(s >= 0.0)):
        raise ValueError(f"a time constant must be finite and not negative, got {seconds}")
    c = np.zeros_like(s)
    np.divide(-1.0, s * rate, out=c, where=s > 0.0)
    c = np.where(s > 0.0, np.exp(c), 0.0)
    return float(c) if c.ndim == 0 else c


def dynamics_params(params, B: Optional[int] = None) -> np.ndarray:
    """Compressor parameters (6,) or (B, 6), columns DYNAMICS_PARAMS, as float64 on the host (no GPU).  ValueError: another shape,
    a value that is not finite, a slope outside [0, 1], a knee below 0, a coefficient outside [0, 1)."""
    q = np.array(params.detach().cpu().numpy() if isinstance(params, torch.Tensor) else params, dtype=np.float64)
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
    if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be a (B, T) float32 or float64 tensor")
    B, T = wav.shape
    if q.ndim == 2 and q.shape[0] != B:
        raise ValueError(f"per-row parameters must have one entry per row ({B}), got {q.shape[0]}")
    if B > 65535 or T > DYNAMICS_MAX_SAMPLES:
        raise ValueError(f"at most 65535 rows of {DYNAMICS_MAX_SAMPLES} samples per call")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
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
    apply_d = None
    if apply is not None:
        a = torch.as_tensor(apply)
        apply_d = (a if a.is_cuda else _upload(a.to(torch.uint8), dev)).ne(0).to(torch.uint8).contiguous()
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
    a, r = (np.asarray(c.detach().cpu().numpy() if isinstance(c, torch.Tensor) else c, dtype=np.float64) for c in (attack_coef, release_coef))
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


# ----------------------------------------------------------------------------- delay lines (csrc/delay.hip)
DELAY_MAX_VOICES = 8                   # MFPA_DELAY_MAX_VOICES
VARIDELAY_TILE = 256                   # MFPA_VARIDELAY_TILE
VARIDELAY_WINDOW = 1024                # MFPA_VARIDELAY_WINDOW
COMB_MAX_DELAY = 1 << 24
DELAY_MAX_SAMPLES = 1 << 30


def _host_values(v, name: str) -> np.ndarray:
    """A number, a sequence or a tensor as float64 on the host (a device tensor is read back: one synchronisation)."""
    try:
        return np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number, a sequence of numbers or a tensor") from None


def _delay_rows(wav, name: str):
    if not isinstance(wav, torch.Tensor) or wav.dim() != 2 or wav.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be a (B, T) float32 or float64 tensor")
    B, T = wav.shape
    if B > 65535 or T > DELAY_MAX_SAMPLES:
        raise ValueError(f"at most 65535 rows of {DELAY_MAX_SAMPLES} samples per call")
    return B, T


def _delay_out_dtype(wav, out_dtype):
    out_dtype = wav.dtype if out_dtype is None else out_dtype
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    return out_dtype


def _apply_mask(apply, B: int, dev):
    if apply is None:
        return None
    a = torch.as_tensor(apply)
    return (a if a.is_cuda else _upload(a.to(torch.uint8), dev)).ne(0).to(torch.uint8).contiguous()


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
    B, T = _delay_rows(wav, "waveform")
    out_dtype = _delay_out_dtype(wav, out_dtype)
    if int(filter_len) != filter_len or not 3 <= filter_len <= 255 or not int(filter_len) & 1:
        raise ValueError(f"filter_len must be odd and lie in [3, 255], got {filter_len}")
    d = delay if isinstance(delay, torch.Tensor) else torch.from_numpy(np.array(_host_values(delay, "delay")))
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
    g, g0 = _host_values(gains, "gains"), _host_values(dry, "dry")
    if g.ndim > 2 or (g.ndim == 1 and g.shape != (V,)) or (g.ndim == 2 and g.shape != (B, V)):
        raise ValueError(f"gains must be a number, ({V},) or ({B}, {V}), got {g.shape}")
    if g0.ndim > 1 or (g0.ndim == 1 and g0.shape != (B,)):
        raise ValueError(f"dry must be a number or ({B},), got {g0.shape}")
    if not (np.all(np.isfinite(g)) and np.all(np.isfinite(g0))):
        raise ValueError("gains and dry must be finite")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
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
    apply_d = _apply_mask(apply, B, dev)
    check(lib().mfpa_varidelay(ptr(wav), _dtype_code(wav), T, B, T, d.data_ptr(), d.stride(0) if B > 1 else 0,
                               d.stride(1) if V > 1 else 0, 0 if constant or T == 1 else 1, V, ptr(g_d), ptr(g0_d), ptr(apply_d),
                               int(filter_len), ptr(y), _dtype_code(y), stream()), "mfpa_varidelay")
    return y


def comb_params(delay, b0=1.0, bD=0.0, aD=0.0) -> np.ndarray:
    """The comb's parameters as float64 on the host (no GPU): (4,) for numbers, (N, 4) when any value has N entries; columns D, b0,
    bD, aD.  ValueError: a delay that is not an integer in [1, 2^24], |aD| >= 1, a value that is not finite, lengths that do not
    agree."""
    vals = [_host_values(v, n) for v, n in ((delay, "delay"), (b0, "b0"), (bD, "bD"), (aD, "aD"))]
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
    B, T = _delay_rows(wav, "waveform")
    out_dtype = _delay_out_dtype(wav, out_dtype)
    q = comb_params(delay, b0, bD, aD)
    if q.ndim == 2 and q.shape[0] != B:
        raise ValueError(f"per-row parameters must have one entry per row ({B}), got {q.shape[0]}")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
    require_gpu(wav, "waveform")
    dev = wav.device
    y = torch.empty((B, T), dtype=out_dtype, device=dev)
    if B == 0 or T == 0:
        return y
    wav = wav.contiguous()
    q_d = _upload(torch.from_numpy(q), dev)
    apply_d = _apply_mask(apply, B, dev)
    check(lib().mfpa_comb(ptr(wav), _dtype_code(wav), T, B, T, ptr(q_d), int(q.ndim == 2), int(np.max(q[..., 0])), ptr(apply_d), ptr(y),
                          _dtype_code(y), stream()), "mfpa_comb")
    return y


def _row_values(v, B: int, name: str) -> np.ndarray:
    """A number or one finite value per row as (B,) float64 on the host."""
    a = _host_values(v, name)
    if a.ndim > 1 or (a.ndim == 1 and a.shape != (B,)):
        raise ValueError(f"{name} must be a number or have one entry per row ({B}), got {a.shape}")
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{name} must be finite")
    return np.array(np.broadcast_to(a, (B,)))


def _column(a: np.ndarray, dev) -> torch.Tensor:
    return _upload(torch.from_numpy(a), dev).unsqueeze(1)


def _delay_grid(B: int, T: int, sample_rate) -> float:
    if int(B) != B or int(T) != T or B < 0 or T < 0:
        raise ValueError(f"B and T must be non-negative integers, got {B}, {T}")
    rate = float(sample_rate)
    if not (np.isfinite(rate) and rate > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    return rate


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


# ----------------------------------------------------------------------------- lossy coding (csrc/codec.hip)
CODEC_FRAMES = 31                      # MFPA_CODEC_FRAMES: blocks of 256 outputs per workgroup
CODEC_MAX_BANDS = 32                   # MFPA_CODEC_MAX_BANDS
CODEC_BAND_EDGES = (0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 88, 104, 124, 148, 176, 208, 256)
MULAW_ENCODE, MULAW_DECODE, MULAW_ROUNDTRIP = 0, 1, 2


def codec_frames(T: int) -> int:
    """Frames of 512 samples at hop 256 that cover a row of T samples standing behind 256 zeros: ceil(T / 256) + 1."""
    return (int(T) + 255) // 256 + 1


def codec_band_edges(band_edges=None) -> np.ndarray:
    """The band table as int32 on the host: n_bands + 1 integers ascending strictly from 0 to 256, at most CODEC_MAX_BANDS bands;
    CODEC_BAND_EDGES (19 bands, roughly a quarter octave wide above 750 Hz at 8 kHz) without an argument."""
    e = np.asarray(CODEC_BAND_EDGES if band_edges is None else band_edges)
    if e.ndim != 1 or e.size < 2 or e.size > CODEC_MAX_BANDS + 1 or not np.issubdtype(e.dtype, np.integer):
        raise ValueError(f"band_edges must be 2 to {CODEC_MAX_BANDS + 1} integers")
    if e[0] != 0 or e[-1] != 256 or np.any(np.diff(e) <= 0):
        raise ValueError(f"band_edges must ascend strictly from 0 to 256, got {e.tolist()}")
    return np.ascontiguousarray(e, dtype=np.int32)


def codec_bit_budget(kbps, sample_rate=8000, side_bits=6, n_bands: int = len(CODEC_BAND_EDGES) - 1) -> np.ndarray:
    """R = kbps * 1000 * 256 / sample_rate - side_bits * n_bands: the bits a frame of 256 new samples may spend on coefficients, as
    float64 on the host (no GPU).  kbps a number or one per row, not NaN; +inf is lossless."""
    k = _host_values(kbps, "kbps")
    rate = float(sample_rate)
    if not (np.isfinite(rate) and rate > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
    if k.ndim > 1 or np.any(np.isnan(k)) or np.any(np.isneginf(k)):
        raise ValueError(f"kbps must be a number or one per row, not NaN, got {kbps}")
    if not (np.isfinite(side_bits) and side_bits >= 0):
        raise ValueError(f"side_bits must not be negative, got {side_bits}")
    return k * 1000.0 * 256.0 / rate - float(side_bits * n_bands)


def transform_codec(wav: torch.Tensor, kbps, *, sample_rate=8000, side_bits=6, band_edges=None, up_db: float = 10.0, down_db: float = 25.0,
                    apply=None, return_stats: bool = False, out_dtype=None):
    """What a transform codec does to the rows of (B, T) float32 or float64 samples at `kbps` kbit/s, in one launch (the definition:
    include/mfpa.h, mfpa_transform_codec): an MDCT of 512-sample sine-windowed frames at hop 256, a masking threshold per band
    (a band's variance spread `up_db` dB per band upwards and `down_db` downwards), reverse water-filling of the frame's budget
    codec_bit_budget(kbps, sample_rate, side_bits, n_bands) over the bands relative to that threshold, a uniform quantiser per coded
    band, bands below the water line set to zero, and the inverse MDCT.  It SIMULATES transform coding: the rate is the
    high-resolution estimate 1/2 log2(variance / noise) per coefficient, not an entropy-coded file size, and parity with any real
    MP3, AAC or GSM encoder is unpinned.  `kbps` a number or one value per row; math.inf reconstructs the input (to rounding), a
    budget that is not positive gives silence.  `apply` (B,) of booleans: a row with a false entry is copied through.  Returns
    (B, T) in `out_dtype` (the samples' dtype without it), the float64 value rounded once; with return_stats also lambda (B, F)
    float64, the water line per frame (NaN where nothing is coded, -inf when lossless), and coded (B, F) int32, the coefficients
    that did not quantise to zero, F = codec_frames(T)."""
    B, T = _delay_rows(wav, "waveform")
    out_dtype = _delay_out_dtype(wav, out_dtype)
    edges = codec_band_edges(band_edges)
    R = codec_bit_budget(kbps, sample_rate, side_bits, edges.size - 1)
    if R.ndim == 1 and R.shape != (B,):
        raise ValueError(f"kbps must be a number or have one entry per row ({B}), got {R.shape}")
    for name, v in (("up_db", up_db), ("down_db", down_db)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number that is not negative, got {v!r}")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
    require_gpu(wav, "waveform")
    dev = wav.device
    F = codec_frames(T)
    y = torch.empty((B, T), dtype=out_dtype, device=dev)
    lam = torch.empty((B, F), dtype=torch.float64, device=dev) if return_stats else None
    coded = torch.empty((B, F), dtype=torch.int32, device=dev) if return_stats else None
    if B == 0 or T == 0:
        return (y, lam, coded) if return_stats else y
    wav = wav.contiguous()
    R_d = _upload(torch.from_numpy(np.array(R)), dev) if R.ndim == 1 else None
    apply_d = _apply_mask(apply, B, dev)
    check(lib().mfpa_transform_codec(ptr(wav), _dtype_code(wav), T, B, T, float(R) if R.ndim == 0 else 0.0, ptr(R_d),
                                     edges.ctypes.data, int(edges.size - 1), float(up_db), float(down_db), ptr(apply_d), ptr(y),
                                     _dtype_code(y), ptr(lam), ptr(coded), stream()), "mfpa_transform_codec")
    return (y, lam, coded) if return_stats else y


def _mulaw(x: torch.Tensor, channels, mode: int, apply, out_dtype) -> torch.Tensor:
    if int(channels) != channels or not 2 <= channels <= 65536:
        raise ValueError(f"channels must be an integer in [2, 65536], got {channels}")
    B, T = x.shape
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per row ({B})")
    require_gpu(x, "input")
    y = torch.empty((B, T), dtype=out_dtype, device=x.device)
    if B == 0 or T == 0:
        return y
    x = x.contiguous()
    apply_d = _apply_mask(apply, B, x.device)
    check(lib().mfpa_mulaw(ptr(x), int(x.dtype == torch.float64), B, T, int(channels), mode, ptr(apply_d), ptr(y),
                           int(out_dtype == torch.float64), stream()), "mfpa_mulaw")
    return y


def mu_law(wav: torch.Tensor, channels: int = 256, *, apply=None, return_codes: bool = False, out_dtype=None):
    """Mu-law companding of (B, T) float32 or float64 samples on the GPU and back, in one pass (include/mfpa.h, mfpa_mulaw;
    torchaudio's mu_law_encoding / mu_law_decoding formulas in float64, parity with torchaudio's float32 unpinned): the samples are
    clamped to [-1, 1], quantised to `channels` levels on the logarithmic scale and expanded again; 256 is G.711's 8 bits.
    `apply` (B,) of booleans: a row with a false entry is copied through.  With return_codes also the codes (B, T) int32 of every
    row (a second launch)."""
    B, T = _delay_rows(wav, "waveform")
    out_dtype = _delay_out_dtype(wav, out_dtype)
    y = _mulaw(wav, channels, MULAW_ROUNDTRIP, apply, out_dtype)
    return (y, mu_law_encode(wav, channels)) if return_codes else y


def mu_law_encode(wav: torch.Tensor, channels: int = 256) -> torch.Tensor:
    """(B, T) float32 or float64 samples -> int32 codes in [0, channels - 1] on the GPU."""
    _delay_rows(wav, "waveform")
    return _mulaw(wav, channels, MULAW_ENCODE, None, torch.int32)


def mu_law_decode(codes: torch.Tensor, channels: int = 256, *, out_dtype=torch.float32) -> torch.Tensor:
    """(B, T) int32 codes -> samples in [-1, 1] on the GPU, float32 (the float64 value rounded once) or float64."""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.dtype != torch.int32:
        raise ValueError("codes must be a (B, T) int32 tensor")
    if codes.shape[0] > 65535 or codes.shape[1] > DELAY_MAX_SAMPLES:
        raise ValueError(f"at most 65535 rows of {DELAY_MAX_SAMPLES} samples per call")
    if out_dtype not in (torch.float32, torch.float64):
        raise ValueError(f"out_dtype must be torch.float32 or torch.float64, got {out_dtype}")
    return _mulaw(codes, channels, MULAW_DECODE, None, out_dtype)


# ----------------------------------------------------------------------------- spectral noise suppression (csrc/denoise.hip)
DENOISE_MAX_WINDOW = 128               # MFPA_DENOISE_MAX_WINDOW: back + ahead + 1 at most
DENOISE_MAX_FRAMES = 16384


def suppress_thresholds(xi_min_db: float = -25.0, floor_db: float = -20.0) -> Tuple[float, float]:
    """(xi_min, g_floor) = (10^(xi_min_db / 10), 10^(floor_db / 20)) as Python floats (host arithmetic, `**`): the a-priori SNR is a
    power ratio, the gain floor an amplitude ratio.  The C entry point takes these two numbers."""
    for name, v in (("xi_min_db", xi_min_db), ("floor_db", floor_db)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
            raise ValueError(f"{name} must be a finite number, got {v!r}")
    if floor_db > 0:
        raise ValueError(f"floor_db must not be positive (a gain floor above 1), got {floor_db}")
    return 10.0 ** (float(xi_min_db) / 10.0), 10.0 ** (float(floor_db) / 20.0)


def _row_floors(floor_db, B: int):
    """floor_db one value per clip -> (B,) float64 gain floors on the host, each suppress_thresholds's."""
    f = _host_values(floor_db, "floor_db")
    if f.shape != (B,) or not np.all(np.isfinite(f)) or np.any(f > 0):
        raise ValueError(f"floor_db must be a number or one finite value per clip ({B}) that is not positive")
    return np.array([suppress_thresholds(-25.0, float(v))[1] for v in f], dtype=np.float64)


def spectral_suppress(mag: torch.Tensor, *, alpha: float = 0.7, back: int = 48, ahead: int = 48, bias: float = 3.0, dd: float = 0.9,
                      xi_min_db: float = -25.0, floor_db: float = -20.0, noise_psd=None, denom=None, apply=None, out_dtype=None,
                      return_gain: bool = False, return_noise: bool = False):
    """A model-free noise suppressor on (B, F, nF) float32 or float64 STFT magnitudes with the frames contiguous (the layout of
    stft_mag), in one launch (the definition: include/mfpa.h, mfpa_spectral_suppress): the periodogram smoothed with `alpha`, its
    minimum over the frames [t - back, t + ahead] times `bias` as the noise PSD (minimum statistics, Martin 2001, plain windowed
    form), the decision-directed a-priori SNR with weight `dd` (Ephraim and Malah 1984) floored at `xi_min_db` dB, and the Wiener
    gain xi / (1 + xi) floored at `floor_db` dB, a number or one value per clip (suppress_thresholds turns the two dB values into numbers).  At the pipeline's hop
    of 256 samples at 8 kHz the default window is 3.1 s; dd = 0.9, not the usual 0.98, because a frame is 32 ms here.
    `noise_psd` (B, F) float64 replaces the tracker (no bias); `denom` (B,) float64 divides each clip's output; `apply` (B,) of
    booleans: a clip with a false entry has gain 1.  back + ahead + 1 <= DENOISE_MAX_WINDOW, nF <= DENOISE_MAX_FRAMES.  Float64
    arithmetic without contraction: the result equals tests/_denoise_oracle.py bit for bit.  Returns y (B, F, nF) in `out_dtype`
    (the input's dtype without it; float32 is the float64 value rounded once), then g and n as float64 (B, F, nF) when
    return_gain / return_noise ask for them."""
    if not isinstance(mag, torch.Tensor) or mag.dim() != 3 or mag.dtype not in (torch.float32, torch.float64):
        raise ValueError("magnitudes must be a (B, F, nF) float32 or float64 tensor")
    B, F, nF = mag.shape
    out_dtype = _delay_out_dtype(mag, out_dtype)
    per_row = not isinstance(floor_db, (int, float, np.integer, np.floating))
    floors = _row_floors(floor_db, B) if per_row else None
    xi_min, g_floor = suppress_thresholds(xi_min_db, -20.0 if per_row else floor_db)
    for name, v in (("alpha", alpha), ("dd", dd)):
        if not isinstance(v, (int, float, np.integer, np.floating)) or not 0.0 <= v < 1.0:
            raise ValueError(f"{name} must be a number in [0, 1), got {v!r}")
    if not isinstance(bias, (int, float, np.integer, np.floating)) or not (bias > 0.0 and math.isfinite(bias)):
        raise ValueError(f"bias must be positive and finite, got {bias!r}")
    for name, v in (("back", back), ("ahead", ahead)):
        if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{name} must be an integer that is not negative, got {v!r}")
    if back + ahead + 1 > DENOISE_MAX_WINDOW:
        raise ValueError(f"back + ahead + 1 must not exceed {DENOISE_MAX_WINDOW}, got {back + ahead + 1}")
    if B < 1 or F < 1 or nF < 1 or B > 65535 or F > (1 << 20) or nF > DENOISE_MAX_FRAMES:
        raise ValueError(f"1 <= B <= 65535, 1 <= F <= 2^20, 1 <= nF <= {DENOISE_MAX_FRAMES}, got {tuple(mag.shape)}")
    for name, t, shape in (("noise_psd", noise_psd, (B, F)), ("denom", denom, (B,))):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float64):
            raise ValueError(f"{name} must be a {shape} float64 tensor")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per clip ({B})")
    require_gpu(mag, "magnitudes")
    dev = mag.device
    for name, t in (("noise_psd", noise_psd), ("denom", denom)):
        if t is not None:
            require_gpu(t, name)
    mag = mag.contiguous()
    noise_psd = noise_psd.contiguous() if noise_psd is not None else None
    denom = denom.contiguous() if denom is not None else None
    y = torch.empty((B, F, nF), dtype=out_dtype, device=dev)
    g = torch.empty((B, F, nF), dtype=torch.float64, device=dev) if return_gain else None
    n = torch.empty((B, F, nF), dtype=torch.float64, device=dev) if return_noise else None
    apply_d = _apply_mask(apply, B, dev)
    floors_d = _upload(torch.from_numpy(floors), dev) if per_row else None
    check(lib().mfpa_spectral_suppress(ptr(mag), _dtype_code(mag), B, F, nF, float(alpha), int(back), int(ahead), float(bias), float(dd),
                                       xi_min, g_floor, ptr(floors_d), ptr(noise_psd), ptr(denom), ptr(apply_d), ptr(y), _dtype_code(y), ptr(g), ptr(n),
                                       stream()), "mfpa_spectral_suppress")
    out = (y,) + ((g,) if return_gain else ()) + ((n,) if return_noise else ())
    return out if len(out) > 1 else y


# ----------------------------------------------------------------------------- programme loudness (csrc/loudness.hip)
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
    fs = float(sample_rate)
    if not (math.isfinite(fs) and fs > 0.0):
        raise ValueError(f"sample_rate must be positive, got {sample_rate}")
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
    s = np.asarray(sos.detach().cpu().numpy() if isinstance(sos, torch.Tensor) else sos, dtype=np.float64)
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
    w = np.asarray(weights.detach().cpu().numpy() if isinstance(weights, torch.Tensor) else weights, dtype=np.float64)
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
    from .functional import k_weighting_sos                                   # host design; functional imports this module
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
    t = np.asarray(target_lufs.detach().cpu().numpy() if isinstance(target_lufs, torch.Tensor) else target_lufs, dtype=np.float64)
    if t.ndim == 0:
        t = np.full((B,), float(t))
    if t.shape != (B,) or not np.all(np.isfinite(t)):
        raise ValueError(f"target_lufs must be a finite number or one per example ({B}), got {target_lufs!r}")
    limit = 0.0 if peak_limit is None else float(peak_limit)
    if peak_limit is not None and not (math.isfinite(limit) and limit > 0.0):
        raise ValueError(f"peak_limit must be positive and finite, got {peak_limit}")
    if apply is not None and tuple(torch.as_tensor(apply).shape) != (B,):
        raise ValueError(f"apply must have one entry per example ({B})")
    if B * C > 65535 or T > LOUDNESS_MAX_SAMPLES:
        raise ValueError(f"at most 65535 rows of {LOUDNESS_MAX_SAMPLES} samples per call")
    gate, peak = _loudness_meter(x, sample_rate, return_peak=peak_limit is not None)
    dev = x.device
    x = x.contiguous()
    y = torch.empty_like(x)
    gain = torch.ones((B,), dtype=torch.float64, device=dev) if return_gain else None
    if B > 0:
        target_d = _upload(torch.from_numpy(loudness_power(t)), dev)
        check(lib().mfpa_loudness_apply(ptr(x), _dtype_code(x), B, C, T, ptr(gate.power), ptr(target_d), ptr(peak), limit,
                                        ptr(_apply_mask(apply, B, dev)), ptr(y), ptr(gain), stream()), "mfpa_loudness_apply")
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
