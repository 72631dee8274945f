"""Thin, typed wrappers over the C ABI (include/mfpa.h): torch tensors in, torch tensors out.

Each function allocates its outputs with torch on the input's device, checks shapes on the
host (a kernel must never see a shape its grid does not assume) and enqueues on torch's
current HIP stream.  Nothing here computes on the CPU.

One module per kernel file of csrc/; what the wrappers do to their arguments before a launch is written once, in _args.
"""
from .._lib import F32, F64
from ._args import _upload
from .stft import (ISTFT_CLAMP, ISTFT_ENVELOPE_MIN, N_BINS, N_FFT, N_HOP, audfprint_window, default_tables, dejavu_window, f64_to_f32,
                   istft, istft_envelope_min, normalize_, nplog_f32, specgram_psd, stft_complex, stft_frames, stft_mag, stft_tables)
from .resampler import (RESAMPLE_ANY_RATIO_HINT, RESAMPLE_LOWPASS_FILTER_WIDTH, RESAMPLE_ROLLOFF, RESAMPLE_TAP_ALIGN, resample,
                        resample_geometry, resample_kernel_for, resample_sparse_geometry, resample_sparse_taps, resample_sparse_tile,
                        resample_tap_pitch, resample_taps, resample_tile)
from .segments import (SEGMENT_DBS_THRESHOLD, SEGMENT_MAX_PER_TRACK, segment_gather, segment_geometry, segment_select, segment_stats,
                       segment_threshold)
from .peaks import (AUDFPRINT_DENSITY, AUDFPRINT_F_SD, AUDFPRINT_MAX_PKS, AUDFPRINT_POLE, DEJAVU_AMP_MIN, DEJAVU_RADIUS, FLOAT32_LOGS,
                    TRACK_MAX_FRAMES, _float32_log_code, audfprint_a_dec, audfprint_pick, audfprint_pick_track, audfprint_prepare,
                    audfprint_prune, dejavu_pick, dejavu_prepare, dejavu_prepare_f32, gauss_table, localmax2d, peak_metrics_counts,
                    psnr_stats)
from .hashes import audfprint_landmarks, audfprint_landmarks_track, dejavu_hashes
from .audfprint_match import (MAINTAIN_FULL_ROWS, audfprint_match, audfprint_remove, audfprint_retrieve, audfprint_store,
                              match_scratch_bytes, pow2_roundup_mask)
from .dejavu_match import (DEJAVU_DIRBITS, DEJAVU_MAX_SID, dejavu_lookup, dejavu_match, dejavu_match_scratch_bytes, dejavu_store,
                           dejavu_table_digests)
from .transforms import FILTER_ZEROS, RFFT_MAX_N, RFFT_MAX_RADICES, bandpass_taps, colored_noise, rfft_plan, rfft_twiddles
from .vocoder import VOCODER_MAX_FRAMES, phase_vocoder, pitch_shift, time_stretch, vocoder_frames
from .iir import SOS_MAX_SAMPLES, SOS_MAX_SECTIONS, sos_normalized, sosfilt
from .rir import RIR_MAX_FILTER, RIR_MAX_LENGTH, RIR_MAX_ORDER, RIR_MAX_ROOMS, rir_geometry, rir_image_count, simulate_rir
from .dynamics import DYNAMICS_MAX_SAMPLES, DYNAMICS_PARAMS, compressor, dynamics_params, envelope_follow, time_coef
from .delay import (COMB_MAX_DELAY, DELAY_MAX_SAMPLES, DELAY_MAX_VOICES, VARIDELAY_TILE, VARIDELAY_WINDOW, comb, comb_params, lfo_delay,
                    speed_drift_delay, variable_delay)
from .codec import (CODEC_BAND_EDGES, CODEC_FRAMES, CODEC_MAX_BANDS, MULAW_DECODE, MULAW_ENCODE, MULAW_ROUNDTRIP, codec_band_edges,
                    codec_bit_budget, codec_frames, mu_law, mu_law_decode, mu_law_encode, transform_codec)
from .denoise import DENOISE_MAX_FRAMES, DENOISE_MAX_WINDOW, spectral_suppress, suppress_thresholds
from .loudness_meter import (LOUDNESS_MAX_CHANNELS, LOUDNESS_MAX_HOP, LOUDNESS_MAX_RANGE_BLOCKS, LOUDNESS_MAX_SAMPLES, LOUDNESS_MAX_WINDOW,
                             LOUDNESS_OFFSET, LOUDNESS_WINDOWS, LoudnessGate, loudness, loudness_curve, loudness_gate, loudness_hop,
                             loudness_lufs, loudness_normalize, loudness_power, loudness_range, loudness_segments, true_peak)
