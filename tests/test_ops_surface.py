"""The surface of musicfpaugment_amd.ops, frozen, and the refusals its wrappers share, on a machine without a GPU.

SIGNATURES and CONSTANTS were printed from the single-file ops module this package replaced (str(inspect.signature(f)) of every public
callable, the value of every public constant), not from the package they now check."""
import inspect
import math
import types

import numpy as np
import pytest
import torch

from musicfpaugment_amd import ops

# fmt: off
SIGNATURES = {'LoudnessGate': '(*values)',
 'audfprint_a_dec': "(density: 'float' = 20, n_hop: 'int' = 256) -> 'float'",
 'audfprint_landmarks': "(mask: 'torch.Tensor', cap: 'int' = 4096, mindt: 'int' = 2, targetdt: 'int' = 63, targetdf: 'int' = 31, maxpairs: 'int' = "
                        '3)',
 'audfprint_landmarks_track': "(mask: 'torch.Tensor', cap: 'int', mindt: 'int' = 2, targetdt: 'int' = 63, targetdf: 'int' = 31, maxpairs: 'int' = 3, "
                              "want_lists: 'bool' = False)",
 'audfprint_match': "(table: 'torch.Tensor', counts: 'torch.Tensor', hashesperid: 'torch.Tensor', hashes: 'torch.Tensor', nq: 'torch.Tensor', k: "
                    "'int' = 1, threshcount: 'int' = 5, search_depth: 'int' = 100, window: 'int' = 2, max_alignments_per_id: 'int' = 100, hcap: "
                    "'int' = 32768, timebits: 'int' = 14, scratch_budget: 'int' = 1073741824, exact_count: 'bool' = False, find_time_range: 'bool' = "
                    "False, time_quantile: 'float' = 0.05, hashesfor: 'Optional[int]' = None, hashes_cap: 'int' = 2048, extended: 'Optional[bool]' = "
                    'None)',
 'audfprint_pick': "(mag: 'torch.Tensor', clip_max: 'torch.Tensor', a_dec: 'Optional[float]' = None, maxpks: 'int' = 5, f_sd: 'float' = 30.0, pole: "
                   "'float' = 0.98)",
 'audfprint_pick_track': "(mag: 'torch.Tensor', clip_max: 'torch.Tensor', a_dec: 'Optional[float]' = None, maxpks: 'int' = 5, f_sd: 'float' = 30.0, "
                         "pole: 'float' = 0.98)",
 'audfprint_prepare': "(spec: 'torch.Tensor', denom: 'Optional[torch.Tensor]' = None, mean_order: 'int' = 0, log_input: 'bool' = False, pole: "
                      "'float' = 0.98, denom_is_clip_max: 'bool' = False, float32_log: 'str' = 'rounded') -> 'torch.Tensor'",
 'audfprint_prune': "(filtered: 'torch.Tensor', a_dec: 'Optional[float]' = None, maxpks: 'int' = 5, f_sd: 'float' = 30.0)",
 'audfprint_remove': "(table: 'torch.Tensor', counts: 'torch.Tensor', ids, n_ids: 'int', timebits: 'int' = 14, full_rows: 'bool' = False) -> "
                     "'torch.Tensor'",
 'audfprint_retrieve': "(table: 'torch.Tensor', counts: 'torch.Tensor', ids, timebits: 'int' = 14, full_rows: 'bool' = False)",
 'audfprint_store': "(table: 'torch.Tensor', counts: 'torch.Tensor', rows: 'torch.Tensor', ids: 'torch.Tensor', seed: 'int' = 0, timebits: 'int' = "
                    "14) -> 'None'",
 'audfprint_window': "() -> 'np.ndarray'",
 'bandpass_taps': '(cut_lo, cut_hi, device=None)',
 'codec_band_edges': "(band_edges=None) -> 'np.ndarray'",
 'codec_bit_budget': "(kbps, sample_rate=8000, side_bits=6, n_bands: 'int' = 19) -> 'np.ndarray'",
 'codec_frames': "(T: 'int') -> 'int'",
 'colored_noise': "(white: 'torch.Tensor', f_decay: 'torch.Tensor', num_samples: 'int') -> 'torch.Tensor'",
 'comb': "(wav: 'torch.Tensor', delay, b0=1.0, bD=0.0, aD=0.0, *, apply=None, out_dtype=None) -> 'torch.Tensor'",
 'comb_params': "(delay, b0=1.0, bD=0.0, aD=0.0) -> 'np.ndarray'",
 'compressor': "(wav: 'torch.Tensor', params, *, apply=None, zi=None, return_gain_reduction: 'bool' = False, return_state: 'bool' = False)",
 'default_tables': "(device, kind: 'str' = 'audfprint') -> 'torch.Tensor'",
 'dejavu_hashes': "(mask: 'torch.Tensor', cap: 'int' = 4096, peak_cap: 'int' = 4096, fan_value: 'int' = 3, min_dt: 'int' = 0, max_dt: 'int' = 200)",
 'dejavu_lookup': "(table: 'torch.Tensor', directory: 'torch.Tensor', digests: 'torch.Tensor') -> 'torch.Tensor'",
 'dejavu_match': "(table: 'torch.Tensor', directory: 'torch.Tensor', digests: 'torch.Tensor', t1: 'torch.Tensor', nq: 'torch.Tensor', k: 'int' = 1, "
                 "hcap: 'int' = 32768, scratch_budget: 'int' = 1073741824) -> 'Tuple[torch.Tensor, torch.Tensor, int]'",
 'dejavu_match_scratch_bytes': "(cap: 'int', hcap: 'int') -> 'int'",
 'dejavu_pick': "(psd: 'torch.Tensor', clip_max: 'torch.Tensor', scale: 'float' = 10.0, mean_order: 'int' = 1, radius: 'int' = 10, amp_min: 'float' "
                '= 50)',
 'dejavu_prepare': "(psd: 'torch.Tensor', denom: 'Optional[torch.Tensor]', scale: 'float' = 10.0, mean_order: 'int' = 1) -> 'torch.Tensor'",
 'dejavu_prepare_f32': "(x: 'torch.Tensor', square: 'bool' = True, scale: 'float' = 10.0, mean_order: 'int' = 0, float32_log: 'str' = 'rounded') -> "
                       "'torch.Tensor'",
 'dejavu_store': "(digests: 'torch.Tensor', sids: 'torch.Tensor', offsets: 'torch.Tensor', dirbits: 'int' = 20)",
 'dejavu_table_digests': "(table: 'torch.Tensor') -> 'torch.Tensor'",
 'dejavu_window': "() -> 'np.ndarray'",
 'dynamics_params': "(params, B: 'Optional[int]' = None) -> 'np.ndarray'",
 'envelope_follow': "(level: 'torch.Tensor', attack_coef, release_coef, *, zi=None, return_state: 'bool' = False)",
 'f64_to_f32': "(x: 'torch.Tensor') -> 'torch.Tensor'",
 'gauss_table': "(npoints: 'int', width: 'float', device) -> 'torch.Tensor'",
 'istft': "(spec: 'torch.Tensor', length: 'Optional[int]' = None, mag: 'Optional[torch.Tensor]' = None, denom: 'Optional[torch.Tensor]' = None, "
          "clamp: 'bool' = False, out_dtype=torch.float32, tables: 'Optional[torch.Tensor]' = None) -> 'torch.Tensor'",
 'istft_envelope_min': "(window: 'np.ndarray', n_frames: 'int', length: 'int') -> 'float'",
 'lfo_delay': "(B: 'int', T: 'int', sample_rate, *, base_ms, depth_ms, rate_hz, phase=0.0, device='cuda') -> 'torch.Tensor'",
 'localmax2d': "(arr: 'torch.Tensor', radius: 'int' = 10, amp_min: 'float' = 50)",
 'loudness': "(wav: 'torch.Tensor', sample_rate, *, design: 'str' = 'bs1770', weights=None) -> 'torch.Tensor'",
 'loudness_curve': "(wav: 'torch.Tensor', sample_rate, window: 'str' = 'momentary') -> 'torch.Tensor'",
 'loudness_gate': "(seg: 'torch.Tensor', hop: 'int', *, win: 'int' = 4, rel: 'float' = 0.1, weights=None, abs_lufs: 'float' = -70.0, return_blocks: "
                  "'bool' = False, want_range: 'bool' = False) -> 'LoudnessGate'",
 'loudness_hop': "(sample_rate) -> 'int'",
 'loudness_lufs': "(power: 'torch.Tensor') -> 'torch.Tensor'",
 'loudness_normalize': "(wav: 'torch.Tensor', sample_rate, target_lufs, *, peak_limit: 'Optional[float]' = None, apply=None, return_gain: 'bool' = "
                       'False)',
 'loudness_power': '(lufs)',
 'loudness_range': "(wav: 'torch.Tensor', sample_rate) -> 'torch.Tensor'",
 'loudness_segments': "(wav: 'torch.Tensor', sos, hop: 'int', *, return_peak: 'bool' = False)",
 'match_scratch_bytes': "(hcap: 'int', extended: 'bool' = False) -> 'int'",
 'mu_law': "(wav: 'torch.Tensor', channels: 'int' = 256, *, apply=None, return_codes: 'bool' = False, out_dtype=None)",
 'mu_law_decode': "(codes: 'torch.Tensor', channels: 'int' = 256, *, out_dtype=torch.float32) -> 'torch.Tensor'",
 'mu_law_encode': "(wav: 'torch.Tensor', channels: 'int' = 256) -> 'torch.Tensor'",
 'normalize_': "(data: 'torch.Tensor', clip_max: 'torch.Tensor', per_clip: 'bool') -> 'torch.Tensor'",
 'nplog_f32': "(x: 'torch.Tensor') -> 'torch.Tensor'",
 'peak_metrics_counts': "(predicted: 'torch.Tensor', gt: 'torch.Tensor') -> 'torch.Tensor'",
 'phase_vocoder': "(spec: 'torch.Tensor', rates, ld_out: 'Optional[int]' = None) -> 'Tuple[torch.Tensor, torch.Tensor]'",
 'pitch_shift': "(wav: 'torch.Tensor', ratios, rates: 'Optional[float]' = None, *, any_ratio: 'bool' = False) -> 'torch.Tensor'",
 'pow2_roundup_mask': "() -> 'int'",
 'psnr_stats': "(pred: 'torch.Tensor', target: 'torch.Tensor') -> 'torch.Tensor'",
 'resample': "(wav: 'torch.Tensor', orig_freq: 'int', new_freq: 'int', *, any_ratio: 'bool' = False, kernel: 'Optional[str]' = None) -> "
             "'torch.Tensor'",
 'resample_geometry': "(orig_freq: 'int', new_freq: 'int', T: 'int' = 0) -> 'Tuple[int, int, int, int, int]'",
 'resample_kernel_for': "(orig_freq: 'int', new_freq: 'int', any_ratio: 'bool' = False, kernel: 'Optional[str]' = None) -> 'str'",
 'resample_sparse_geometry': "(orig_freq: 'int', new_freq: 'int', T: 'int' = 0) -> 'Tuple[int, int, int, int, int]'",
 'resample_sparse_taps': "(orig_freq: 'int', new_freq: 'int', device) -> 'Tuple[torch.Tensor, torch.Tensor]'",
 'resample_sparse_tile': "(orig_freq: 'int', new_freq: 'int') -> 'int'",
 'resample_tap_pitch': "(ntaps: 'int') -> 'int'",
 'resample_taps': "(orig_freq: 'int', new_freq: 'int', device) -> 'torch.Tensor'",
 'resample_tile': "(orig_freq: 'int', new_freq: 'int') -> 'int'",
 'rfft_plan': "(N: 'int') -> 'Tuple[Tuple[int, ...], int]'",
 'rfft_twiddles': "(N: 'int', device) -> 'torch.Tensor'",
 'rir_geometry': "(room, source, mic, absorption) -> 'np.ndarray'",
 'rir_image_count': "(max_order: 'int') -> 'int'",
 'segment_gather': "(bank: 'torch.Tensor', src: 'torch.Tensor', div: 'Optional[torch.Tensor]', L: 'int', out: 'Optional[torch.Tensor]' = None) -> "
                   "'torch.Tensor'",
 'segment_geometry': "(lengths, L: 'int', S: 'int') -> 'np.ndarray'",
 'segment_select': "(seg_sumsq: 'torch.Tensor', trk_sumsq: 'torch.Tensor', trk_peak: 'torch.Tensor', off: 'torch.Tensor', lens: 'torch.Tensor', "
                   "seg_off: 'torch.Tensor', L: 'int', S: 'int', keys: 'torch.Tensor', dbs_threshold: 'float' = -7.5, n_keep: 'int' = 1, do_norm: "
                   "'bool' = True, with_mask: 'bool' = False)",
 'segment_stats': "(bank: 'torch.Tensor', off: 'torch.Tensor', lens: 'torch.Tensor', seg_off: 'torch.Tensor', n_seg: 'int', L: 'int', S: 'int') -> "
                  "'Tuple[torch.Tensor, torch.Tensor, torch.Tensor]'",
 'segment_threshold': "(dbs_threshold: 'float' = -7.5) -> 'float'",
 'simulate_rir': "(room, source, mic, absorption, max_order: 'int', length: 'int', sample_rate: 'float', *, sound_speed: 'float' = 343.0, "
                 "filter_len: 'int' = 81, reversed: 'bool' = False, out_dtype=torch.float32, device='cuda') -> 'torch.Tensor'",
 'sos_normalized': "(sos) -> 'np.ndarray'",
 'sosfilt': "(wav: 'torch.Tensor', sos, *, apply=None, zi=None, clamp: 'bool' = False)",
 'specgram_psd': "(wav: 'torch.Tensor', scale_in: 'float' = 1.0, tables: 'Optional[torch.Tensor]' = None)",
 'spectral_suppress': "(mag: 'torch.Tensor', *, alpha: 'float' = 0.7, back: 'int' = 48, ahead: 'int' = 48, bias: 'float' = 3.0, dd: 'float' = 0.9, "
                      "xi_min_db: 'float' = -25.0, floor_db: 'float' = -20.0, noise_psd=None, denom=None, apply=None, out_dtype=None, return_gain: "
                      "'bool' = False, return_noise: 'bool' = False)",
 'speed_drift_delay': "(B: 'int', T: 'int', sample_rate, components, *, device='cuda') -> 'torch.Tensor'",
 'stft_complex': "(wav: 'torch.Tensor', tables: 'Optional[torch.Tensor]' = None, want_mag: 'bool' = False, mag_dtype=torch.float64)",
 'stft_frames': "(n_samples: 'int') -> 'int'",
 'stft_mag': "(wav: 'torch.Tensor', out_dtype=torch.float64, tables: 'Optional[torch.Tensor]' = None, want_max: 'bool' = True) -> "
             "'Tuple[torch.Tensor, Optional[torch.Tensor]]'",
 'stft_tables': "(window: 'np.ndarray', device) -> 'torch.Tensor'",
 'suppress_thresholds': "(xi_min_db: 'float' = -25.0, floor_db: 'float' = -20.0) -> 'Tuple[float, float]'",
 'time_coef': '(seconds, sample_rate)',
 'time_stretch': "(wav: 'torch.Tensor', rates, out_dtype=torch.float32) -> 'Tuple[torch.Tensor, torch.Tensor]'",
 'transform_codec': "(wav: 'torch.Tensor', kbps, *, sample_rate=8000, side_bits=6, band_edges=None, up_db: 'float' = 10.0, down_db: 'float' = 25.0, "
                    "apply=None, return_stats: 'bool' = False, out_dtype=None)",
 'true_peak': "(wav: 'torch.Tensor', oversample: 'int' = 4) -> 'torch.Tensor'",
 'variable_delay': "(wav: 'torch.Tensor', delay, gains=1.0, *, dry=0.0, filter_len: 'int' = 81, apply=None, out_dtype=None) -> 'torch.Tensor'",
 'vocoder_frames': "(n_frames: 'int', rate: 'float') -> 'int'"}

CONSTANTS = {'AUDFPRINT_DENSITY': 20,
 'AUDFPRINT_F_SD': 30.0,
 'AUDFPRINT_MAX_PKS': 5,
 'AUDFPRINT_POLE': 0.98,
 'CODEC_BAND_EDGES': (0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 88, 104, 124, 148, 176, 208, 256),
 'CODEC_FRAMES': 31,
 'CODEC_MAX_BANDS': 32,
 'COMB_MAX_DELAY': 16777216,
 'DEJAVU_AMP_MIN': 50,
 'DEJAVU_DIRBITS': 20,
 'DEJAVU_MAX_SID': 16777215,
 'DEJAVU_RADIUS': 10,
 'DELAY_MAX_SAMPLES': 1073741824,
 'DELAY_MAX_VOICES': 8,
 'DENOISE_MAX_FRAMES': 16384,
 'DENOISE_MAX_WINDOW': 128,
 'DYNAMICS_MAX_SAMPLES': 1073741824,
 'DYNAMICS_PARAMS': ('threshold_db', 'slope', 'knee_db', 'attack_coef', 'release_coef', 'makeup_db'),
 'F32': 0,
 'F64': 1,
 'FILTER_ZEROS': 8,
 'FLOAT32_LOGS': ('rounded', 'numpy'),
 'ISTFT_CLAMP': 1,
 'ISTFT_ENVELOPE_MIN': 1e-11,
 'LOUDNESS_MAX_CHANNELS': 8,
 'LOUDNESS_MAX_HOP': 16777216,
 'LOUDNESS_MAX_RANGE_BLOCKS': 16384,
 'LOUDNESS_MAX_SAMPLES': 1073741824,
 'LOUDNESS_MAX_WINDOW': 64,
 'LOUDNESS_OFFSET': -0.691,
 'LOUDNESS_WINDOWS': {'momentary': 4, 'short': 30},
 'MAINTAIN_FULL_ROWS': 1,
 'MULAW_DECODE': 1,
 'MULAW_ENCODE': 0,
 'MULAW_ROUNDTRIP': 2,
 'N_BINS': 257,
 'N_FFT': 512,
 'N_HOP': 256,
 'RESAMPLE_ANY_RATIO_HINT': 'the dense resampling kernel does not take this pair of rates (at most 1024 phases and 8192 taps per phase after '
                            'reduction by the gcd); pass any_ratio=True for the sparse-tap kernel, which takes every pair below 65536 Hz',
 'RESAMPLE_LOWPASS_FILTER_WIDTH': 6,
 'RESAMPLE_ROLLOFF': 0.99,
 'RESAMPLE_TAP_ALIGN': 16,
 'RFFT_MAX_N': 16384,
 'RFFT_MAX_RADICES': 16,
 'RIR_MAX_FILTER': 255,
 'RIR_MAX_LENGTH': 262144,
 'RIR_MAX_ORDER': 128,
 'RIR_MAX_ROOMS': 65535,
 'SEGMENT_DBS_THRESHOLD': -7.5,
 'SEGMENT_MAX_PER_TRACK': 8192,
 'SOS_MAX_SAMPLES': 1073741824,
 'SOS_MAX_SECTIONS': 8,
 'TRACK_MAX_FRAMES': 16384,
 'VARIDELAY_TILE': 256,
 'VARIDELAY_WINDOW': 1024,
 'VOCODER_MAX_FRAMES': 16384}

# fmt: on


def _public():
    return {n: getattr(ops, n) for n in vars(ops) if not n.startswith("_") and not isinstance(getattr(ops, n), types.ModuleType)}


def test_surface_is_frozen():
    public = _public()
    callables = {n: o for n, o in public.items() if callable(o)}
    constants = {n: o for n, o in public.items() if not callable(o)}
    assert sorted(callables) == sorted(SIGNATURES)
    assert sorted(constants) == sorted(CONSTANTS)
    for n, o in callables.items():
        assert str(inspect.signature(o)) == SIGNATURES[n], n
        assert (o.__module__ + ".").startswith("musicfpaugment_amd.ops."), (n, o.__module__)
    for n, v in constants.items():
        assert type(v) is type(CONSTANTS[n]) and v == CONSTANTS[n], n
    assert callable(ops._float32_log_code) and callable(ops._upload)


# ------------------------------------------------------------------ the shared refusals, once per caller, on CPU tensors
# tests/test_capi_{iir,dynamics,delay,codec,denoise,loudness,rir}.py::test_python_refusals_need_no_gpu assert most of these as a bare
# ValueError among each wrapper's own refusals; here every caller of one shared check is held to the one wording, and MfpaError ("no
# GPU") is a RuntimeError, so it does not pass for a ValueError.  time_stretch and istft ask for the GPU before they look at
# out_dtype, as they always did: their out_dtype refusal cannot be seen without one.
X = torch.zeros(2, 8)
X3 = torch.zeros(2, 1, 8)
MAG = torch.zeros(2, 3, 4, dtype=torch.float64)
DELAY = torch.zeros(2, 8, dtype=torch.float64)
SOS = [[1.0, 0.0, 0.0, 1.0, 0.0, 0.0]]
COMP = [-20.0, 0.75, 6.0, 0.9, 0.99, 0.0]
ROOM, SRC, MIC = [5.2, 4.1, 2.7], [1.3, 2.9, 1.1], [3.7, 0.8, 1.6]

APPLY_CALLERS = {
    "sosfilt": ("row", lambda a: ops.sosfilt(X, SOS, apply=a)),
    "compressor": ("row", lambda a: ops.compressor(X, COMP, apply=a)),
    "variable_delay": ("row", lambda a: ops.variable_delay(X, DELAY, apply=a)),
    "comb": ("row", lambda a: ops.comb(X, 3, apply=a)),
    "transform_codec": ("row", lambda a: ops.transform_codec(X, 16.0, apply=a)),
    "mu_law": ("row", lambda a: ops.mu_law(X, apply=a)),
    "spectral_suppress": ("clip", lambda a: ops.spectral_suppress(MAG, apply=a)),
    "loudness_normalize": ("example", lambda a: ops.loudness_normalize(X3, 8000, -23.0, apply=a)),
}


@pytest.mark.parametrize("name", sorted(APPLY_CALLERS))
def test_wrong_length_apply_is_a_value_error(name):
    noun, call = APPLY_CALLERS[name]
    for bad in ([True], torch.ones(3, dtype=torch.bool), np.ones((2, 1), dtype=bool), True):
        with pytest.raises(ValueError, match=rf"apply must have one entry per {noun} \(2\)"):
            call(bad)


OUT_DTYPE_CALLERS = {
    "variable_delay": lambda dt: ops.variable_delay(X, DELAY, out_dtype=dt),
    "comb": lambda dt: ops.comb(X, 3, out_dtype=dt),
    "transform_codec": lambda dt: ops.transform_codec(X, 16.0, out_dtype=dt),
    "mu_law": lambda dt: ops.mu_law(X, out_dtype=dt),
    "mu_law_decode": lambda dt: ops.mu_law_decode(torch.zeros(2, 8, dtype=torch.int32), out_dtype=dt),
    "spectral_suppress": lambda dt: ops.spectral_suppress(MAG, out_dtype=dt),
    "simulate_rir": lambda dt: ops.simulate_rir(ROOM, SRC, MIC, 0.3, 3, 100, 8000, out_dtype=dt),
}


@pytest.mark.parametrize("name", sorted(OUT_DTYPE_CALLERS))
def test_wrong_out_dtype_is_a_value_error(name):
    for bad in (torch.float16, torch.int32, "float32"):
        with pytest.raises(ValueError, match=r"out_dtype must be torch\.float32 or torch\.float64, got "):
            OUT_DTYPE_CALLERS[name](bad)


SAMPLE_RATE_CALLERS = {
    "time_coef": lambda r: ops.time_coef(0.1, r),
    "lfo_delay": lambda r: ops.lfo_delay(2, 8, r, base_ms=1.0, depth_ms=1.0, rate_hz=1.0),
    "speed_drift_delay": lambda r: ops.speed_drift_delay(2, 8, r, [(0.001, 1.0, 0.0)]),
    "codec_bit_budget": lambda r: ops.codec_bit_budget(16.0, r),
    "transform_codec": lambda r: ops.transform_codec(X, 16.0, sample_rate=r),
    "loudness_hop": lambda r: ops.loudness_hop(r),
    "loudness": lambda r: ops.loudness(X3, r),
    "loudness_normalize": lambda r: ops.loudness_normalize(X3, r, -23.0),
    "simulate_rir": lambda r: ops.simulate_rir(ROOM, SRC, MIC, 0.3, 3, 100, r),
}


@pytest.mark.parametrize("name", sorted(SAMPLE_RATE_CALLERS))
def test_bad_sample_rate_is_a_value_error(name):
    for bad in (0, -8000, math.nan, math.inf):
        with pytest.raises(ValueError, match="sample_rate must be positive, got "):
            SAMPLE_RATE_CALLERS[name](bad)


ROW_CALLERS = {
    "sosfilt": lambda w: ops.sosfilt(w, SOS),
    "compressor": lambda w: ops.compressor(w, COMP),
    "envelope_follow": lambda w: ops.envelope_follow(w, 0.9, 0.99),
    "variable_delay": lambda w: ops.variable_delay(w, DELAY),
    "comb": lambda w: ops.comb(w, 3),
    "transform_codec": lambda w: ops.transform_codec(w, 16.0),
    "mu_law": lambda w: ops.mu_law(w),
    "mu_law_encode": lambda w: ops.mu_law_encode(w),
}


@pytest.mark.parametrize("name", sorted(ROW_CALLERS))
def test_a_waveform_that_is_not_rows_is_a_value_error(name):
    for bad in (X3, torch.zeros(8), X.to(torch.float16), np.zeros((2, 8), dtype=np.float32)):
        with pytest.raises(ValueError, match=r"(waveform|level) must be a \(B, T\) float32 or float64 tensor"):
            ROW_CALLERS[name](bad)
