"""SpectralDenoiser: the model-free entry of the denoising side -- a minimum-statistics noise tracker, the decision-directed
a-priori SNR and a Wiener gain on the STFT magnitudes the pipeline already has (ops.spectral_suppress, csrc/denoise.hip).  It has
no weights and takes the place the UNet takes: `Audfprint_peaks(denoising=True, denoising_model="unet", unet=SpectralDenoiser())`,
`fingerprint_peaks_batch(..., denoising=True, denoising_model="unet", unet=SpectralDenoiser(domain="power"))`,
`set_denoisers(unet=SpectralDenoiser(domain="power"))`; as a waveform denoiser its forward has Demucs's call shape."""
from __future__ import annotations

import torch
from torch import nn

from . import ops

_KEYS = ("alpha", "back", "ahead", "bias", "dd", "xi_min_db", "floor_db")


class SpectralDenoiser(nn.Module):
    """Keywords: ops.spectral_suppress's (alpha, back, ahead, bias, dd, xi_min_db, floor_db) and domain = "magnitude" | "power".
    "power" is for a caller that hands over a PSD and squares what comes back (Dejavu's): the square roots of the PSD and of the
    maxima are taken with torch.sqrt on the device -- torch's, not fused into the kernel -- and the same kernel runs on them."""

    def __init__(self, domain: str = "magnitude", **suppress_kw) -> None:
        super().__init__()
        if domain not in ("magnitude", "power"):
            raise ValueError(f"domain must be 'magnitude' or 'power', got {domain!r}")
        unknown = sorted(set(suppress_kw) - set(_KEYS))
        if unknown:
            raise ValueError(f"unknown keywords {unknown}: SpectralDenoiser takes {list(_KEYS)}")
        self.domain = domain
        self.suppress_kw = dict(suppress_kw)
        ops.suppress_thresholds(self.suppress_kw.get("xi_min_db", -25.0), self.suppress_kw.get("floor_db", -20.0))

    def extra_repr(self) -> str:
        return ", ".join([f"domain={self.domain!r}"] + [f"{k}={v!r}" for k, v in self.suppress_kw.items()])

    def denoise_spectrogram(self, spec64: torch.Tensor, clip_max: torch.Tensor, per_clip: bool) -> torch.Tensor:
        """UNet.denoise_spectrogram's signature and return: raw (B, F, nF) |STFT| (or PSD with domain="power") and the (B,) float64
        maxima -> the suppressed spectrogram divided by the maxima, float32.  per_clip=False divides by the batch maximum."""
        B = spec64.shape[0]
        if not per_clip:
            clip_max = clip_max.max().expand(B)
        if self.domain == "power":
            spec64, clip_max = torch.sqrt(spec64), torch.sqrt(clip_max)
        return ops.spectral_suppress(spec64, denom=clip_max.contiguous(), out_dtype=torch.float32, **self.suppress_kw)

    def denoise_waveform(self, wav: torch.Tensor) -> torch.Tensor:
        """(B, T) float32 mixture -> (B, T) float32: one complex STFT, the suppressor on its magnitudes, the inverse STFT of the
        suppressed magnitudes on the mixture's phase (the chain of UNet.denoise_waveform)."""
        spec, mag, _ = ops.stft_complex(wav, want_mag=True)
        return ops.istft(spec, wav.shape[1], mag=ops.spectral_suppress(mag, **self.suppress_kw))

    def forward(self, wav: torch.Tensor) -> torch.Tensor:
        """(B, T) or (B, 1, T) float32 -> (B, 1, T), like Demucs."""
        if wav.dim() == 3 and wav.shape[1] == 1:
            wav = wav[:, 0]
        if wav.dim() != 2:
            raise ValueError("waveform must be (B, T) or (B, 1, T)")
        return self.denoise_waveform(wav.contiguous())[:, None, :]
