"""Audfprint peak extraction on MI355X -- mirror of afp/audfprint/peak_extractor.py:76-311.

``Audfprint_peaks(params, denoising, denoising_model)`` keeps the reference's constructor and
``find_peaks(d) -> (pklist, peaks_mask, spec)`` contract (empty input -> ``([], np.array([]))``,
peak_extractor.py:253-254).  Unlike the reference, importing this module loads no checkpoint and
needs no NVIDIA GPU: the denoiser is passed in (``unet=``).  ``find_peaks_batch`` is the batched,
sync-free form the benchmark uses; ``find_peaks`` wraps it for one clip.
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Tuple

import numpy as np
import torch

from ... import ops
from ...constants import afp_settings


def landmarks2hashes(landmarks_list) -> np.ndarray:
    """[(time, bin1, bin2, dtime)] -> (n, 2) int32 (time, hash).  afp/audfprint/peak_extractor.py:40-58.
    Pure bit packing of a host list (no device work needed); the batched device path packs hashes inside
    mfpa_audfprint_landmarks."""
    lm = np.array(landmarks_list, dtype=np.int64).reshape(-1, 4)
    if lm.shape[0] == 0:
        return np.zeros((0, 2), dtype=np.int32)
    out = np.zeros((lm.shape[0], 2), dtype=np.int32)
    out[:, 0] = lm[:, 0]
    out[:, 1] = ((lm[:, 1] & 255) << 12) | (((lm[:, 2] - lm[:, 1]) & 63) << 6) | (lm[:, 3] & 63)
    return out


class Audfprint_peaks(object):
    def __init__(self, params: Optional[Dict[str, Any]] = None, denoising: bool = False, denoising_model=None,
                 unet=None, device="cuda", demucs=None, float32_log: str = "rounded", whole_tracks: bool = False) -> None:
        """`whole_tracks` (default off: every call behaves and fails as without it): inputs of more than 1500 STFT frames, up to
        16384 (the 14 time bits of the hash table), are picked and hashed by the track kernels (ops.audfprint_pick_track,
        ops.audfprint_landmarks_track) with the results the reference gives for a file of that length; shorter inputs take the same
        kernels as ever (un-denoised inputs of 1435 to 1500 frames, whose launch those kernels cannot hold, take the track kernels
        too).  Not together with a denoiser.
        `float32_log` ("rounded" | "numpy"): the logarithm find_peaks takes of the UNet's float32 output (:265-276) -- "numpy" is
        numpy's own float32 log bit for bit, the reference's arithmetic; "rounded" (the default) the float64 log rounded once to
        float32.  The un-denoised branch is float64 in the reference and is not affected."""
        ops._float32_log_code(float32_log)
        self.float32_log = float32_log
        self.whole_tracks = bool(whole_tracks)
        params = afp_settings["audfprint"] if params is None else params
        self.density = params["density"]
        self.target_sr = params["samplerate"]
        self.n_fft = params["n_fft"]
        self.n_hop = params["n_hop"]
        self.shifts = params["shifts"]
        self.f_sd = params["freq-sd"]
        self.maxpksperframe = params["pks-per-frame"]
        self.maxpairsperpeak = 3
        self.mindt = 2
        self.targetdt = 63
        self.targetdf = 31
        self.denoising = denoising
        self.denoising_model = denoising_model
        self.device = torch.device(device)
        if self.n_fft != 512 or self.n_hop != 256:
            raise NotImplementedError("the HIP STFT is built for n_fft 512 / hop 256 (testing/parameters.py:24-25)")
        if self.denoising:
            assert self.denoising_model in ["demucs", "unet"]
            if self.denoising_model == "demucs":
                if demucs is None:
                    raise ValueError("denoising_model='demucs' needs the Demucs instance (demucs=...): this module loads no checkpoint")
                self.unet, self.demucs = None, demucs.to(self.device).eval()
            else:
                if unet is None:
                    raise ValueError("denoising=True needs the UNet instance (unet=...): this module loads no checkpoint")
                self.unet, self.demucs = unet.to(self.device).eval(), None
        else:
            self.unet, self.demucs = None, None

    CLIP_MAX_FRAMES = 1500           # ops.audfprint_prune: the event list of a clip in LDS
    PREPARE_MAX_FRAMES = 45 * 8192 // 257      # 1434: the float64 frame-major mfpa_audfprint_prepare keeps 2 KB of LDS per 8192-element chunk of
                                               # np.mean's reduction beside its 66 KB of tiles; 46 chunks no longer fit a CU's 160 KB (the launch fails)

    def _track_path(self, n_samples: int) -> bool:
        """Whether an input of n_samples takes the track kernels: `whole_tracks` and more than 1500 frames -- or, without a denoiser,
        more than the 1434 the clip kernels' launch can hold."""
        frames = ops.stft_frames(int(n_samples))
        if not self.whole_tracks:
            return False
        if frames <= self.CLIP_MAX_FRAMES:
            return not self.denoising and frames > self.PREPARE_MAX_FRAMES
        if frames > ops.TRACK_MAX_FRAMES:
            raise ValueError(f"{n_samples} samples = {frames} STFT frames: whole tracks take at most {ops.TRACK_MAX_FRAMES} frames "
                             f"({ops.TRACK_MAX_FRAMES * self.n_hop / self.target_sr:.0f} s), what the 14 time bits of the hash table "
                             "store without wrapping")
        if self.denoising:
            raise NotImplementedError(f"{frames} STFT frames with a denoiser: whole tracks are fingerprinted without one (the database "
                                      f"side of the experiment never denoises); denoised inputs take at most {self.CLIP_MAX_FRAMES} frames")
        return True

    # ------------------------------------------------------------------ batched device path
    def find_peaks_batch(self, wav: torch.Tensor, want_spec: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(B, T) float32 on the GPU -> (mask (B,256,nF) uint8, npeaks (B,) int32, spec (B,257,nF)).

        STFT -> per-clip /max -> [UNet] -> log/mean/high-pass -> forward + backward pruning; no host sync.
        spec is float64 without denoising and float32 with it, like the reference's third return value.  `want_spec=False`
        (peak masks only, no denoiser): the normalised spectrogram is not materialised -- the division by the clip maximum
        happens inside the log / high-pass kernel, same float64 quotient -- and None is returned in its place.
        """
        if self._track_path(wav.shape[-1]):
            mag, cmax = ops.stft_mag(wav, torch.float64)
            mask, npeaks = ops.audfprint_pick_track(mag, cmax, ops.audfprint_a_dec(self.density, self.n_hop), self.maxpksperframe,
                                                    float(self.f_sd))
            return mask, npeaks, (ops.normalize_(mag, cmax, per_clip=True) if want_spec else None)   # the same float64 quotient
        mag, cmax = ops.stft_mag(wav, torch.float64)
        a_dec = ops.audfprint_a_dec(self.density, self.n_hop)
        if self.unet is not None:
            spec = self.unet.denoise_spectrogram(mag, cmax, per_clip=True)        # float32 (B,257,nF)
            filtered = ops.audfprint_prepare(spec, None, mean_order=0,            # C-contiguous in the reference
                                             float32_log=self.float32_log)
        elif want_spec:
            spec = ops.normalize_(mag, cmax, per_clip=True)
            filtered = ops.audfprint_prepare(spec, None, mean_order=1)            # |stft| is a transposed view there
        else:
            if mag.shape[2] <= 512 and (256 * mag.shape[2]) % 16 == 0:               # stages 1 + 2 fused: no filtered spectrogram in memory
                mask, npeaks = ops.audfprint_pick(mag, cmax, a_dec, self.maxpksperframe, float(self.f_sd))
                return mask, npeaks, None
            spec = None
            filtered = ops.audfprint_prepare(mag, cmax, mean_order=1, denom_is_clip_max=True)
        mask, npeaks = ops.audfprint_prune(filtered, a_dec, self.maxpksperframe, float(self.f_sd))
        return mask, npeaks, spec

    def wav2peaks_batch(self, wav: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """wavfile2peaks (peak_extractor.py:347-430) for waveforms already in memory: with denoising_model == "demucs" the
        WAVEFORM goes through the Demucs denoiser first (:369-376), then find_peaks; the UNet acts inside find_peaks."""
        if self.demucs is not None:
            self._track_path(wav.shape[-1])                  # (raises for a track: Demucs is not run over minutes of audio)
            wav = self.demucs(wav)[:, 0].contiguous()
        return self.find_peaks_batch(wav)

    # ------------------------------------------------------------------ reference call surface
    def find_peaks(self, d) -> Tuple[List[Tuple[int, int]], np.ndarray, np.ndarray]:
        if len(d) == 0:
            return [], np.array([])
        x = torch.as_tensor(np.asarray(d) if not isinstance(d, torch.Tensor) else d).to(self.device, torch.float32)
        mask, _, spec = self.find_peaks_batch(x.reshape(1, -1))
        m = mask[0]
        cols, bins = torch.nonzero(m.t(), as_tuple=True)                          # column-major ascending (:305-309)
        pklist = list(zip(cols.tolist(), bins.tolist()))
        return pklist, m.to(torch.float32).cpu().numpy(), spec[0].cpu().numpy()

    # ------------------------------------------------------------------ file-level entry points of the reference
    @staticmethod
    def _read_waveform(filename: str, target_sr: int) -> torch.Tensor:
        """.pkl: the pickled 8 kHz waveform of the reference's query sets (peak_extractor.py:361-368); .wav: PCM / float at any
        rate, resampled to `target_sr` on the device like the reference's torchaudio Resample (:378-388; transforms.Resample).
        mp3 decoding is file I/O outside the hot path."""
        ext = filename.rsplit(".", 1)[-1].lower()
        if ext == "pkl":
            import pickle
            with open(filename, "rb") as fh:
                return torch.as_tensor(np.asarray(pickle.load(fh)), dtype=torch.float32).reshape(-1)
        if ext == "wav":
            from scipy.io import wavfile
            sr, data = wavfile.read(filename)
            x = np.asarray(data)
            x = x.astype(np.float32) / float(2 ** (8 * x.dtype.itemsize - 1)) if x.dtype.kind == "i" else x.astype(np.float32)
            d = torch.from_numpy(np.ascontiguousarray(x.mean(axis=1) if x.ndim == 2 else x, dtype=np.float32))
            if int(sr) != int(target_sr):
                from ...transforms import Resample
                d = Resample(int(sr), int(target_sr))(d)
            return d
        raise NotImplementedError(f"{filename}: only .pkl and .wav inputs (decode other formats offline)")

    def wavfile2peaks(self, filename: str, shifts: Optional[int] = None, get_masks_waveforms: bool = False):
        """peak_extractor.py:347-424: [(time, bin)] of one file, or the list of `shifts` such lists, or
        (peaks_mask, waveform, sgram) with get_masks_waveforms."""
        d = self._read_waveform(filename, self.target_sr)
        if self.demucs is not None:
            self._track_path(len(d))                         # (raises for a track)
            d = self.demucs(d.reshape(1, -1).to(self.device))[0, 0].cpu()           # :369-376
        self.soundfiledur = len(d) / self.target_sr
        if shifts is None or shifts < 2:
            peaks, peaks_mask, sgram = self.find_peaks(d)
        else:
            peaks = [self.find_peaks(d[int(s / self.shifts * self.n_hop):])[0] for s in range(shifts)]
            peaks_mask = sgram = None
        if get_masks_waveforms:
            return peaks_mask, d, sgram
        return peaks

    def wavfile2hashes(self, filename: str) -> np.ndarray:
        """peak_extractor.py:426-460: unique sorted (time, hash) rows of one file (the instance's `shifts`)."""
        d = self._read_waveform(filename, self.target_sr).reshape(1, -1).to(self.device)
        if self.demucs is not None:
            self._track_path(d.shape[1])                     # (raises for a track)
            d = self.demucs(d)[:, 0].contiguous()
        self.soundfiledur = d.shape[1] / self.target_sr
        uq, n = self.hashes_batch(d)
        n0 = int(n[0])
        if n0 < 0:                                           # never a slice bound: hashes_batch raises on overflow, this guards the contract
            raise ValueError("landmark capacity exceeded")
        return uq[0, :n0].cpu().numpy().astype(np.int32)

    def ingest(self, hashtable, filename: str) -> Tuple[float, int]:
        """peak_extractor.py:462-481: add one file's hashes to `hashtable` (hash_table.HashTable); (duration, n hashes)."""
        hashes = self.wavfile2hashes(filename)
        hashtable.store(filename, hashes)
        return self.soundfiledur, len(hashes)

    # ------------------------------------------------------------------ landmarks / hashes (next-tier row §8f-1)
    def hashes_batch(self, wav: torch.Tensor, cap: int = 4096, shifts: Optional[int] = None):
        """(B, T) float32 on the GPU -> (unique sorted (time, hash) rows (B, cap', 2) int32, counts (B,) int32):
        wavfile2hashes (peak_extractor.py:426-460) for a whole batch, peaks never leaving the device.  `shifts` (default:
        the instance's, 1 in testing/parameters.py): hashes of the waveform advanced by s / shifts frames, s = 0..shifts-1,
        are merged before the duplicate removal (:406-424, :437-444); cap' = cap * shifts."""
        shifts = self.shifts if shifts is None else shifts
        if shifts is None or shifts < 2:
            if self._track_path(wav.shape[-1]):
                return self._track_hashes(wav)
            mask, _, _ = self.find_peaks_batch(wav)
            while True:
                _, _, uniq, counts = ops.audfprint_landmarks(mask, cap, self.mindt, self.targetdt, self.targetdf,
                                                             self.maxpairsperpeak)
                if not bool((counts < 0).any()):            # the kernel flags an overflowing clip with counts [-1, -1]
                    return uniq, counts[:, 1].contiguous()
                if cap >= 8192:
                    raise ValueError("more than 8 peaks in one frame or more than 8192 landmarks in one clip: outside the device "
                                     "kernel's limits")
                cap = 8192                                   # retry once with the kernel's largest capacity
        B = wav.shape[0]
        keys = []
        for s in range(shifts):
            shiftsamps = int(s / self.shifts * self.n_hop) if self.shifts and self.shifts > 1 else int(s / shifts * self.n_hop)
            shifted = wav[:, shiftsamps:].contiguous()
            if self._track_path(shifted.shape[-1]):          # a track: its unique rows (the union below removes what the shifts share)
                hs, n = self._track_hashes(shifted)
                n = n[:, None]
            else:
                mask, _, _ = self.find_peaks_batch(shifted)
                _, hs, _, counts = ops.audfprint_landmarks(mask, cap, self.mindt, self.targetdt, self.targetdf, self.maxpairsperpeak)
                if bool((counts < 0).any()):
                    raise ValueError("landmark capacity exceeded: raise `cap` (the kernel's limit is 8192 landmarks per clip)")
                n = counts[:, :1]
            k = (hs[:, :, 0].to(torch.int64) << 32) + (hs[:, :, 1].to(torch.int64) & 0xFFFFFFFF)     # :447-449
            valid = torch.arange(hs.shape[1], device=wav.device)[None, :] < n
            keys.append(torch.where(valid, k, torch.full_like(k, torch.iinfo(torch.int64).max)))
        k = torch.sort(torch.cat(keys, dim=1), dim=1).values                                           # np.sort(np.unique(.))
        first = torch.ones_like(k, dtype=torch.bool)
        first[:, 1:] = k[:, 1:] != k[:, :-1]
        first &= k != torch.iinfo(torch.int64).max
        n = first.sum(dim=1).to(torch.int32)
        pos = torch.cumsum(first.to(torch.int64), dim=1) - 1
        out = torch.zeros((B, k.shape[1], 2), dtype=torch.int32, device=wav.device)           # cap * shifts for clips
        b_idx = torch.arange(B, device=wav.device)[:, None].expand_as(k)
        out[b_idx[first], pos[first], 0] = (k[first] >> 32).to(torch.int32)
        out[b_idx[first], pos[first], 1] = (k[first] & 0xFFFFFFFF).to(torch.int32)
        return out, n

    def _track_hashes(self, wav: torch.Tensor):
        """hashes_batch (one shift) through the track kernels.  The capacity is maxpairsperpeak * the most peaks of a clip, an exact
        upper bound at the cost of one sync: no retry."""
        mask, npeaks, _ = self.find_peaks_batch(wav, want_spec=False)
        cap = max(16, self.maxpairsperpeak * int(npeaks.max())) if wav.shape[0] else 16
        _, _, uniq, counts = ops.audfprint_landmarks_track(mask, cap, self.mindt, self.targetdt, self.targetdf, self.maxpairsperpeak)
        if bool((counts < 0).any()):
            raise ValueError("more than 8 peaks in one frame: outside the device kernel's limits")
        return uniq, counts[:, 1].contiguous()

    def peaks2landmarks(self, pklist: List[Tuple[int, int]]) -> List[Tuple[int, int, int, int]]:
        """[(col, bin)] -> [(col, bin1, bin2, dcol)], peak_extractor.py:313-346, through the device kernel."""
        if len(pklist) == 0:
            return []
        pk = np.asarray(pklist, dtype=np.int64).reshape(-1, 2)
        T, R = int(pk[:, 0].max()) + 1, 256
        if pk[:, 1].max() >= R:
            raise ValueError("bins must be < 256 (they are packed into 8 bits, peak_extractor.py:54)")
        mask = torch.zeros((1, R, T), dtype=torch.uint8)
        mask[0, pk[:, 1], pk[:, 0]] = 1
        cap = min(8192, max(16, 3 * len(pk)))
        lm, _, _, counts = ops.audfprint_landmarks(mask.to(self.device), cap, self.mindt, self.targetdt, self.targetdf,
                                                   self.maxpairsperpeak)
        n = int(counts[0, 0])
        if n < 0:
            raise ValueError("more than 8 peaks in one frame or more than 8192 landmarks: outside the device kernel's limits")
        return [tuple(r) for r in lm[0, :n].cpu().tolist()]
