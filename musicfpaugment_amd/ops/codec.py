"""Lossy coding: the MDCT transform codec and mu-law companding (csrc/codec.hip)."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib, ptr, require_gpu, stream
from ._args import (_apply_mask, _check_apply, _dtype_code, _host_f64, _is_number, _out_dtype, _row_limit, _rows, _sample_rate,
                    _upload)
from .delay import DELAY_MAX_SAMPLES    # the row kernels share one sample limit


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
    k = _host_f64(kbps, "kbps")
    rate = _sample_rate(sample_rate)
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
    B, T = _rows(wav, "waveform", DELAY_MAX_SAMPLES)
    out_dtype = _out_dtype(out_dtype, wav.dtype)
    edges = codec_band_edges(band_edges)
    R = codec_bit_budget(kbps, sample_rate, side_bits, edges.size - 1)
    if R.ndim == 1 and R.shape != (B,):
        raise ValueError(f"kbps must be a number or have one entry per row ({B}), got {R.shape}")
    for name, v in (("up_db", up_db), ("down_db", down_db)):
        if not _is_number(v) or not np.isfinite(v) or v < 0:
            raise ValueError(f"{name} must be a finite number that is not negative, got {v!r}")
    _check_apply(apply, B)
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
    apply_d = _apply_mask(apply, dev)
    check(lib().mfpa_transform_codec(ptr(wav), _dtype_code(wav), T, B, T, float(R) if R.ndim == 0 else 0.0, ptr(R_d),
                                     edges.ctypes.data, int(edges.size - 1), float(up_db), float(down_db), ptr(apply_d), ptr(y),
                                     _dtype_code(y), ptr(lam), ptr(coded), stream()), "mfpa_transform_codec")
    return (y, lam, coded) if return_stats else y


def _mulaw(x: torch.Tensor, channels, mode: int, apply, out_dtype) -> torch.Tensor:
    if int(channels) != channels or not 2 <= channels <= 65536:
        raise ValueError(f"channels must be an integer in [2, 65536], got {channels}")
    B, T = x.shape
    _check_apply(apply, B)
    require_gpu(x, "input")
    y = torch.empty((B, T), dtype=out_dtype, device=x.device)
    if B == 0 or T == 0:
        return y
    x = x.contiguous()
    apply_d = _apply_mask(apply, x.device)
    check(lib().mfpa_mulaw(ptr(x), int(x.dtype == torch.float64), B, T, int(channels), mode, ptr(apply_d), ptr(y),
                           int(out_dtype == torch.float64), stream()), "mfpa_mulaw")
    return y


def mu_law(wav: torch.Tensor, channels: int = 256, *, apply=None, return_codes: bool = False, out_dtype=None):
    """Mu-law companding of (B, T) float32 or float64 samples on the GPU and back, in one pass (include/mfpa.h, mfpa_mulaw;
    torchaudio's mu_law_encoding / mu_law_decoding formulas in float64, parity with torchaudio's float32 unpinned): the samples are
    clamped to [-1, 1], quantised to `channels` levels on the logarithmic scale and expanded again; 256 is G.711's 8 bits.
    `apply` (B,) of booleans: a row with a false entry is copied through.  With return_codes also the codes (B, T) int32 of every
    row (a second launch)."""
    B, T = _rows(wav, "waveform", DELAY_MAX_SAMPLES)
    out_dtype = _out_dtype(out_dtype, wav.dtype)
    y = _mulaw(wav, channels, MULAW_ROUNDTRIP, apply, out_dtype)
    return (y, mu_law_encode(wav, channels)) if return_codes else y


def mu_law_encode(wav: torch.Tensor, channels: int = 256) -> torch.Tensor:
    """(B, T) float32 or float64 samples -> int32 codes in [0, channels - 1] on the GPU."""
    _rows(wav, "waveform", DELAY_MAX_SAMPLES)
    return _mulaw(wav, channels, MULAW_ENCODE, None, torch.int32)


def mu_law_decode(codes: torch.Tensor, channels: int = 256, *, out_dtype=torch.float32) -> torch.Tensor:
    """(B, T) int32 codes -> samples in [-1, 1] on the GPU, float32 (the float64 value rounded once) or float64."""
    if not isinstance(codes, torch.Tensor) or codes.dim() != 2 or codes.dtype != torch.int32:
        raise ValueError("codes must be a (B, T) int32 tensor")
    _row_limit(codes.shape[0], codes.shape[1], DELAY_MAX_SAMPLES)
    return _mulaw(codes, channels, MULAW_DECODE, None, _out_dtype(out_dtype))
