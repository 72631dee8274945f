/*
 * mfpa.h -- C ABI of libmfpa.so, the MI355X (gfx950) implementation of the
 * musicFPaugment hot path:
 *
 *   waveform -> STFT magnitude -> [UNet denoiser] -> spectral-peak picking -> peak-mask metrics
 *
 * The reference (deezer/musicFPaugment) is pure Python and has no FFI of its own;
 * each entry point below names the reference function (file:line under the
 * reference tree) whose arithmetic it replaces.  INTEGRATION.md shows the ctypes
 * binding a maintainer of the reference would add at those call sites.
 *
 * Conventions
 *  - every function returns 0 on success, MFPA_EINVAL for a shape/argument error,
 *    or MFPA_EHIP - hipError_t for a HIP runtime failure; nothing aborts or throws;
 *  - all pointers are DEVICE pointers owned by the caller (e.g. torch allocations),
 *    all arrays dense row-major; the library allocates nothing;
 *  - work is enqueued on `stream` (a hipStream_t passed as void*; NULL = default
 *    stream) with no host synchronisation, so calls can be captured in a hipGraph;
 *  - functions are re-entrant; one process drives one GPU (multi-GPU = one process
 *    per GPU, sharding clips across ranks).
 */
#ifndef MFPA_H
#define MFPA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFPA_OK 0
#define MFPA_EINVAL (-22)
#define MFPA_EHIP (-1000) /* result is MFPA_EHIP - hipError_t */

#define MFPA_F32 0
#define MFPA_F64 1

/* The logarithm of the pickers' FLOAT32 (denoised) branch.  The reference takes np.log of a float32 array there
 * (afp/audfprint/peak_extractor.py:265-276, afp/dejavu/fingerprint.py:70-79), and numpy's float32 log is a SIMD kernel that is
 * not correctly rounded: it differs from the float64 log rounded once to float32 on 22 % of the float32 arguments in (1e-6, 1].
 *   ROUNDED (the default): the float64 log rounded once to float32;
 *   NUMPY: numpy's own float32 log restated (csrc/mfpa_nplog.h), equal to np.log on every non-negative float32 where numpy
 *          dispatches that kernel (AVX512F or AVX2 + FMA3) -- the reference's log values bit for bit.
 * MFPA_LOG_NUMPY_F32 is the bit of mfpa_audfprint_prepare's log_input that selects NUMPY. */
#define MFPA_F32LOG_ROUNDED 0
#define MFPA_F32LOG_NUMPY 1
#define MFPA_LOG_NUMPY_F32 4

#define MFPA_N_FFT 512
#define MFPA_N_HOP 256
#define MFPA_N_BINS 257

/* ABI version: bumps when a signature changes or an entry point is added. */
int mfpa_version(void);

/* ---------------------------------------------------------------------------------------
 * STFT tables (HOST function, no GPU work): fills out[MFPA_STFT_TABLE_LEN] doubles on the host
 * from a 512-point window -- [0,512) the window, then the FFT twiddles.  The caller uploads the
 * array once and passes the device pointer as `tables` below (the window is an argument of the
 * reference's stft too, afp/audfprint/stft.py:15-19; the library itself keeps no state).
 */
#define MFPA_STFT_TABLE_LEN 1288
int mfpa_stft_tables(const double* window512, double* out);

/* STFT magnitude.  Replaces torch.stft + abs in training/visualisation.py:20-28 and
 * np.abs(stft.stft(...)) in afp/audfprint/peak_extractor.py:259-261 (afp/audfprint/stft.py:15-62).
 *   wav      (B, T_w) float32, T_w > 256
 *   tables   device copy of mfpa_stft_tables(np.hanning(514)[1:-1]) for both reference call sites
 *   mag      (B, 257, n_frames) float32 or float64 (out_dtype), n_frames = 1 + T_w / 256;
 *            centre / reflect padding, one-sided, unnormalised, computed in float64
 *   clip_max (B) float64, may be NULL: max float64 magnitude of each clip
 */
int mfpa_stft_mag(const float* wav, int B, int T_w, const double* tables,
                  void* mag, int out_dtype, double* clip_max, void* stream);

/* Number of STFT frames for T_w samples (1 + T_w / 256). */
int mfpa_stft_frames(int T_w);

/* mlab.specgram power spectrogram, afp/dejavu/fingerprint.py:60-66: no padding, frames at
 * multiples of 256 while a full frame fits ((T_w - 256) / 256 frames), one-sided PSD with bins
 * 1..255 doubled; samples are multiplied by scale_in first (dejavu.py:109 feeds x * 32767).
 * The common factor 1/(Fs*sum(w^2)) is NOT applied: the reference divides by the maximum
 * immediately (fingerprint.py:68).
 *   tables   device copy of mfpa_stft_tables(np.hanning(512))
 *   psd (B, 257, n_frames) float64, clip_max (B) float64 may be NULL. */
int mfpa_specgram_psd(const float* wav, int B, int T_w, double scale_in, const double* tables,
                      double* psd, double* clip_max, void* stream);
int mfpa_specgram_frames(int T_w);

/* In-place division by a maximum.  per_clip = 0: one max over the whole batch
 * (torch.max(specgram), training/visualisation.py:29); per_clip = 1: each clip by its own
 * (sgram /= np.max(sgram), peak_extractor.py:263; arr2D /= arr2D.max(), fingerprint.py:68).
 *   data (B, n) dtype, clip_max (B) float64 as produced by mfpa_stft_mag. */
int mfpa_normalize(void* data, int dtype, int B, long long n, const double* clip_max,
                   int per_clip, void* stream);

/* data (B, n) float64 -> out (B, n) float32 (the `.float()` of training/train.py:272). */
/* out[b][i] = (float)(in[b][i] / denom[b]), in (B, n) float64: the reference's `spectrogram / max` + `.float()` (training/train.py:264-272)
 * as one pass -- the same float64 quotient rounded to float32 that mfpa_conv3x3_c1_bn_relu / mfpa_wgrad_c1 form per tap from (spec64, denom). */
int mfpa_normalize_f32(const double* in, int B, long long n, const double* denom, float* out, void* stream);
int mfpa_f64_to_f32(const double* in, float* out, long long n, void* stream);

/* ---------------------------------------------------------------------------------------
 * Audfprint peak picker = everything of Audfprint_peaks.find_peaks after the optional UNet,
 * afp/audfprint/peak_extractor.py:271-311.
 *
 * Stage 1, mfpa_audfprint_prepare: log(max(s, max/1e6)) - mean, per-bin 1-pole high-pass
 * (scipy lfilter([1,-1],[1,-0.98])), Nyquist bin dropped  (peak_extractor.py:272-290).
 *   spec       (B, F, T) float32 or float64 (dtype), F = bins + 1 (257)
 *   denom      (B) float64 or NULL: if given, s = spec / denom[b] first (fuses the
 *              per-clip normalisation of peak_extractor.py:263)
 *   mean_order 0: numpy sums the spectrogram bin-major (C order: the UNet output),
 *              1: frame-major (the un-denoised |stft| array, which is a transposed view)
 *              -- the pairwise summation tree of np.mean is reproduced in that order
 *   log_input  bit 0: `spec` already holds log(max(s, max/1e6)) computed by the caller
 *              (strict mode: everything downstream is IEEE add/mul/compare -> bit-exact);
 *              bit 1 (value 2): denom[b] is the maximum of the float64 spec[b] itself, as
 *              mfpa_stft_mag returned it with this spectrogram: max(spec / denom) is then 1
 *              exactly (NaN for an all-zero clip, like numpy) and the max pass is skipped;
 *              bit 2 (value 4, MFPA_LOG_NUMPY_F32): the log of a float32 spectrogram is numpy's own float32 log, np.log of the
 *              UNet output at peak_extractor.py:265-276 bit for bit, instead of the float64 log rounded once to float32;
 *              MFPA_EINVAL with dtype MFPA_F64 or together with bit 0 (there is no float32 log to take)
 *   filtered   (B, T, F-1) float64, FRAME-major workspace consumed by mfpa_audfprint_prune
 *   scratch    (B, F*T) float64 workspace
 */
int mfpa_audfprint_prepare(const void* spec, int dtype, int B, int F, int T, const double* denom,
                           int mean_order, int log_input, double pole,
                           double* filtered, double* scratch, void* stream);

/* Stage 2, mfpa_audfprint_prune: forward decaying-threshold pass then backward pruning
 * (_decaying_threshold_fwd_prune / _bwd_prune_peaks, peak_extractor.py:173-234).
 *   filtered (B, T, R) float64 frame-major, R = 256 bins (R % 4 == 0, R <= 256)
 *   gauss    (2R+1) float64: exp(-0.5*((j-R)/f_sd)^2), the table of peak_extractor.py:163-165
 *   a_dec    threshold decay per frame (peak_extractor.py:295)
 *   maxpks   peaks kept per frame (<= 8; reference 5)
 *   mask     (B, R, T) uint8 in {0,1} -- peaks_mask of find_peaks, bin-major like the reference
 *   npeaks   (B) int32
 */
int mfpa_audfprint_prune(const double* filtered, int B, int R, int T, const double* gauss,
                         double a_dec, int maxpks, uint8_t* mask, int32_t* npeaks, void* stream);

/* Stages 1 + 2 in one call for the un-denoised path, Audfprint_peaks.find_peaks(d) without a denoiser
 * (afp/audfprint/peak_extractor.py:253-311): raw |STFT| + its per-clip maxima as mfpa_stft_mag returned them -> peak mask.
 * Same arithmetic as mfpa_audfprint_prepare(denom = clip_max, mean_order = 1, log_input = 2) followed by
 * mfpa_audfprint_prune, as two launches: the log values (frame-major) + the pairwise-tree node sums of np.mean, then a pruner
 * that applies "- mean, lfilter" to the frames as it walks them -- the filtered spectrogram is never written.
 *   spec (B, F, T) float64, 141 <= F = R + 1 <= 257, R % 4 == 0, T <= 512, R * T % 16 == 0 (the pruner zeroes the 16-byte aligned mask itself);  clip_max (B) float64
 *   work (B * F * T + B * 128) float64 workspace;  gauss / a_dec / maxpks / mask / npeaks as for mfpa_audfprint_prune */
/* out[i] = v[i] / den[i] by the sequence the pick kernels use per spectrogram cell (one reciprocal per clip there): q0 = v * RN(1 / den), two
 * residual / correction multiply-adds -- correctly rounded for normal operands with normal residuals (Markstein), i.e. bit-identical to the IEEE
 * division; exported so that the tests can compare it with the division on arbitrary pairs. */
int mfpa_div_by_reciprocal(const double* v, const double* den, long long n, double* out, void* stream);
int mfpa_audfprint_pick(const double* spec, const double* clip_max, int B, int F, int T, double pole,
                        const double* gauss, double a_dec, int maxpks, double* work, uint8_t* mask,
                        int32_t* npeaks, void* stream);

/* The same for a whole track: Audfprint_peaks.find_peaks(d) without a denoiser on a file of any length
 * (afp/audfprint/peak_extractor.py:236-311), up to 16384 frames -- what the 14 time bits of the hash table store without
 * wrapping (afp/audfprint/hash_table.py:55).  The arithmetic of mfpa_audfprint_pick, value for value; the pruner keeps its event
 * list in the caller's workspace instead of LDS, and the node sums of np.mean's tree are read at the stride their number asks for.
 *   spec (B, F, T) float64, 141 <= F = R + 1 <= 257, R % 4 == 0, 1 <= T <= 16384;  clip_max (B) float64, the maxima of spec
 *   logs   (B, T, F) float64 workspace (the log values, frame-major)
 *   sums   (B, 2 * nchunks) float64 workspace, nchunks = ceil(F * T / 8192)
 *   events B * (T * maxpks * (8 + 4) + 4 * (T + 2)) bytes of workspace, 8-byte aligned
 *   gauss / a_dec / maxpks / mask / npeaks as for mfpa_audfprint_prune */
int mfpa_audfprint_pick_track(const double* spec, const double* clip_max, int B, int F, int T, double pole,
                              const double* gauss, double a_dec, int maxpks, double* logs, double* sums, void* events,
                              uint8_t* mask, int32_t* npeaks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Dejavu picker.  mfpa_dejavu_prepare: arr = scale*ln(max(a, max/1e6)) - mean with
 * a = psd / denom (fingerprint.py:68,78-79; scale = 10; mean_order as for mfpa_audfprint_prepare:
 * mlab.specgram hands back a frame-major array, so the reference sums with mean_order = 1).  mfpa_localmax2d: get_2D_peaks,
 * afp/dejavu/fingerprint.py:94-171: (2r+1)^2 maximum filter with scipy 'reflect' borders,
 * equality test, XOR with the eroded exact-zero background (border_value 1), amp > amp_min.
 *   arr  (B, F, T) float64;  mask (B, F, T) uint8;  npeaks (B) int32;  2 <= radius <= 16 (the reference uses 10)
 */
int mfpa_dejavu_prepare(const double* psd, int B, int F, int T, const double* denom, double scale,
                        int mean_order, double* arr, void* stream);
/* The denoised branch (fingerprint.py:70-79): x is the UNet's float32 output (B, F, T) for the normalised spectrogram,
 * a = x*x when square != 0, and max / floor / log / mean / subtraction are float32 operations as numpy performs them on a
 * float32 array (the network output is C-contiguous: mean_order = 0); arr is that float32 result widened to float64. */
int mfpa_dejavu_prepare_f32(const float* x, int B, int F, int T, int square, double scale, int mean_order, double* arr,
                            void* stream);
/* The same with the float32 logarithm chosen: float32_log = MFPA_F32LOG_ROUNDED (what mfpa_dejavu_prepare_f32 computes) or
 * MFPA_F32LOG_NUMPY (numpy's own float32 log: 10 * np.log(...) of fingerprint.py:78 on the float32 array of :70-75, bit for bit);
 * any other value: MFPA_EINVAL. */
int mfpa_dejavu_prepare_f32_ex(const float* x, int B, int F, int T, int square, double scale, int mean_order, int float32_log,
                               double* arr, void* stream);
/* y[i] = np.log(x[i]) as numpy's float32 SIMD kernel returns it (csrc/mfpa_nplog.h; the log the reference takes at
 * afp/audfprint/peak_extractor.py:276 and afp/dejavu/fingerprint.py:78 after the UNet), x and y (n) float32, distinct arrays: MFPA_EINVAL when the two ranges overlap.
 * x < 0 and NaN give NaN, 0 gives -inf, +inf gives +inf; denormals are handled whatever the denormal mode. */
int mfpa_nplog_f32(const float* x, float* y, long long n, void* stream);
int mfpa_localmax2d(const double* arr, int B, int F, int T, int radius, double amp_min,
                    uint8_t* mask, int32_t* npeaks, void* stream);

/* The un-denoised Dejavu chain after the spectrogram in one call -- fingerprint.py:68,78-79 + get_2D_peaks (:94-171): the PSD and
 * its per-clip maxima as mfpa_specgram_psd returned them -> peak mask.  Same arithmetic as mfpa_dejavu_prepare(denom = clip_max)
 * followed by mfpa_localmax2d, as two launches: scale * ln(max(a, 1e-6)) + the node sums of np.mean's pairwise tree (many
 * workgroups per clip), then the local-maximum kernel, which forms the mean from the node sums and subtracts it while it loads
 * its tiles -- the mean-subtracted array is never written.  clip_max[b] MUST be the maximum of psd[b] (max(a) = 1 is assumed).
 *   psd (B, F, T) float64, 141 <= F <= 257, T <= 512;  work: B * mfpa_dejavu_pick_work_doubles(F, T) float64;  mask / npeaks as for mfpa_localmax2d */
int mfpa_dejavu_pick_work_doubles(int F, int T, long long* per_clip);
int mfpa_dejavu_pick(const double* psd, const double* clip_max, int B, int F, int T, double scale, int mean_order, int radius,
                     double amp_min, double* work, uint8_t* mask, int32_t* npeaks, void* stream);

/* ---------------------------------------------------------------------------------------
 * Peak-mask metrics, testing/metrics.py:10-192.  For 0/1 masks (B, N1, N2), N1,N2 >= 2:
 *   counts (B, 4) int64 = [hits_precision, n_predicted, hits_recall, n_ground_truth] per clip,
 * where a peak (i, j) of one mask is looked up in the other at (i + [i==0], j + [j==0])
 * (the reference's low-border quirk).  Precision = sum hits_p / sum n_p, etc.
 */
int mfpa_peak_metrics(const uint8_t* predicted, const uint8_t* gt, int B, int N1, int N2,
                      int64_t* counts, void* stream);

/* Per-clip PSNR statistics (testing/metrics.py:7, torchmetrics PeakSignalNoiseRatio; used by
 * testing/audfprint_exps.py:136-137): pred (B,n) float32|float64, target (B,n) float64,
 * out (B,3) float64 = [sum (pred-target)^2, min(target), max(target)]. */
int mfpa_psnr_stats(const void* pred, int pred_dtype, const double* target, int B, long long n, double* out,
                    void* stream);

/* ---------------------------------------------------------------------------------------
 * Landmark pairing + hashing, the step after the pickers (next-tier row SURVEY.md §8f-1).  Integer only.
 *
 * mfpa_audfprint_landmarks: peaks2landmarks + landmarks2hashes + the duplicate removal of wavfile2hashes
 * (afp/audfprint/peak_extractor.py:313-346, :40-58, :443-460) from the peak mask of mfpa_audfprint_prune.
 *   mask (B,R,T) uint8 (<= 8 peaks per frame); cap = row capacity per clip (<= 8192)
 *   landmarks (B,cap,4) int32 (col, bin1, bin2, dcol) in the reference's list order
 *   hashes    (B,cap,2) int32 (time, hash) in the same order
 *   uniq      (B,cap,2) int32 unique rows sorted by (time << 32) + hash
 *   counts    (B,2) int32 = [n_landmarks, n_unique], or [-1,-1] when a clip overflows cap / 8 peaks per frame
 *   reference constants: mindt 2, targetdt 63, targetdf 31, maxpairs 3 (peak_extractor.py:99-107)
 *
 * mfpa_dejavu_hashes: generate_hashes (afp/dejavu/fingerprint.py:174-213) from the mask of mfpa_localmax2d:
 * peaks in (time, freq) order, each with its next fan-1 peaks, min_dt <= dt <= max_dt,
 * SHA-1("f1|f2|dt") truncated to 10 bytes (= 20 hex digits).
 *   digests (B,cap,10) uint8, t1 (B,cap) int32, counts (B) int32 (-1: more than peak_cap peaks or cap hashes)
 */
int mfpa_audfprint_landmarks(const uint8_t* mask, int B, int R, int T, int cap, int mindt, int targetdt,
                             int targetdf, int maxpairs, int32_t* landmarks, int32_t* hashes, int32_t* uniq,
                             int32_t* counts, void* stream);
int mfpa_dejavu_hashes(const uint8_t* mask, int B, int F, int T, int cap, int peak_cap, int fan, int min_dt,
                       int max_dt, uint8_t* digests, int32_t* t1, int32_t* counts, void* stream);

/* mfpa_audfprint_landmarks for a whole track (peaks2landmarks takes a list of any length, afp/audfprint/peak_extractor.py:313-346;
 * landmarks2hashes :40-58; the duplicate removal of wavfile2hashes :443-460): the frames are cut into tiles of 256, each sorted on its
 * own -- the key is time << 32 | hash, so the tiles in order are the sorted list.  Same outputs and the same [-1, -1] for a clip with
 * more than 8 peaks in a frame or more than `cap` landmarks; what differs:
 *   mask (B,R,T) uint8, R <= 256, R % 4 == 0, 1 <= T <= 16384;  cap >= 1, any size
 *   tiles (B, ceil(T / 256), 2) int32 workspace
 *   landmarks, hashes: both may be NULL and are then not written
 *   mindt >= 0, 1 <= targetdt <= 256, targetdf >= 0, 1 <= maxpairs <= 4 */
int mfpa_audfprint_landmarks_track(const uint8_t* mask, int B, int R, int T, int cap, int mindt, int targetdt,
                                   int targetdf, int maxpairs, int32_t* tiles, int32_t* landmarks, int32_t* hashes,
                                   int32_t* uniq, int32_t* counts, void* stream);

/* ---------------------------------------------------------------------------------------
 * Audfprint hash table and matcher (identification-rate experiment, testing/audfprint_exps.py:17-84).  Integer only, except
 * the weighted count rawcount / hashesperid (one float64 division).  The table is (2^hashbits, depth) uint32 of
 * ((id + 1) << timebits) | (time & (2^timebits - 1)); counts (2^hashbits) int32; hashesperid (n_ids) int32.
 *
 * mfpa_audfprint_store: HashTable.store (afp/audfprint/hash_table.py:72-113) for a batch of entries.  rows (N,2) int32
 * (time, hash) and ids (N) int32 in arrival order; order (N) int64 = the arrival indices stably sorted by hash & mask;
 * seg_start (n_seg + 1) int32 = offsets into `order` of each bucket's run.  Slots are arrival ranks; a full bucket draws
 * slot uniform over 0..count from a counter-based generator keyed by (seed, bucket, count) -- the reference draws from
 * Python's global `random` (:99-103) -- and stores only when slot < depth; counts keep growing.  (id + 1) << timebits
 * must fit 32 bits (the caller checks).
 *
 * mfpa_audfprint_match: Matcher.match_hashes without exact_count / find_time_range (afp/audfprint/audfprint_match.py:322-346:
 * get_hits, _best_count_ids :105-137, _approx_match_counts :236-320, the sort by filtered count) for B queries.
 *   hashes (B,cap,2) int32 (time, hash), nq (B) int32 rows per query (the layout of mfpa_audfprint_landmarks' uniq);
 *   scratch: B * mfpa_audfprint_match_scratch_bytes(hcap) bytes, hcap a power of two in [64, 2^26] (hits per query);
 *   out (B,K,7) int32 rows [id, filtered_count, time_offset, raw_count, orig_rank, 0, 0], filtered count descending,
 *   ties by (orig_rank, mode order); rows past info[1] are not written;
 *   info (B,3) int32 = [n_hits, rows written, rows in total], or [n_hits, -1, -1] when n_hits > hcap (nothing else is
 *   written: call again with a larger hcap).  search_depth <= 256; ties in the weighted count rank the larger id first.
 */
int mfpa_audfprint_store(const int32_t* rows, const int32_t* ids, const int64_t* order, const int32_t* seg_start, int n_seg,
                         int hashbits, int timebits, int depth, unsigned long long seed, uint32_t* table, int32_t* counts,
                         void* stream);
int mfpa_audfprint_match_scratch_bytes(long long hcap, long long* bytes);
int mfpa_audfprint_match(const uint32_t* table, const int32_t* counts, const int32_t* hashesperid, int n_ids, int hashbits,
                         int timebits, int depth, const int32_t* hashes, const int32_t* nq, int B, int cap, int threshcount,
                         int search_depth, int window, int max_alignments, long long hcap, void* scratch, int K, int32_t* out,
                         int32_t* info, void* stream);

/* mfpa_audfprint_match_ex: the same matcher with exact_count, find_time_range and hashesfor (audfprint_match.py:131-233,
 * :293-296, :343-349).  Arguments as mfpa_audfprint_match, and:
 *   flags: 1 = exact_count (every local maximum of an id's dt histogram with count >= threshcount is a mode, dt ascending,
 *          no max_alignments cap; filtered_count = distinct query_time + (hash << timebits) inside the window, computed in
 *          64 bits with timebits = max(1, encpowerof2(largest query time that has a hit)); rows with count < threshcount
 *          are dropped; needs threshcount >= 1), 2 = find_time_range (columns 5-6 = min_time, max_time: the sorted query
 *          times mt of the window's hits, one per hit, at mt[int(n * q)] and mt[int(n * (1 - q)) - 1], -1 = the last);
 *   time_quantile q in [0, 1);
 *   pow2_roundup_mask: bit k set when numpy's float64 ceil(log(2^k) / log(2)) gives k + 1 (the caller computes it);
 *   hashesfor >= 0: the sorted distinct packed values of result row `hashesfor` of each query, unpacked to
 *          hf_out (B,hf_cap,2) int32 rows [packed & (2^timebits - 1), packed >> timebits]; hf_count (B) int32 = their
 *          number, -1 when the query has no such row; when it exceeds hf_cap nothing is written (call again with more
 *          room).  -1: no list, hf_out / hf_count are not read;
 *   scratch: B * mfpa_audfprint_match_ex_scratch_bytes(hcap) bytes;  cap <= 32768.  A negative query
 *   time packs as in the reference (int64 arithmetic).
 * Ties of the filtered count: (orig_rank, mode order), mode order being dt ascending under flag 1.  With flags 0 and
 * hashesfor -1 the result is mfpa_audfprint_match's.
 */
int mfpa_audfprint_match_ex_scratch_bytes(long long hcap, long long* bytes);
int mfpa_audfprint_match_ex(const uint32_t* table, const int32_t* counts, const int32_t* hashesperid, int n_ids, int hashbits,
                            int timebits, int depth, const int32_t* hashes, const int32_t* nq, int B, int cap, int threshcount,
                            int search_depth, int window, int max_alignments, int flags, double time_quantile,
                            uint32_t pow2_roundup_mask, int hashesfor, int hf_cap, int32_t* hf_out, int32_t* hf_count,
                            long long hcap, void* scratch, int K, int32_t* out, int32_t* info, void* stream);

/* Maintenance of the Audfprint hash table: HashTable.remove and HashTable.retrieve (afp/audfprint/hash_table.py:277-316).
 * Same table, counts and accepted (hashbits, timebits, depth) as above.  With n = min(counts[b], depth), a MATCH is a slot
 * j < n of bucket b whose (table[b][j] >> timebits) - 1, taken on the unsigned value, is in the requested set.
 * INVARIANT: both are specified on tables in which every slot at or beyond min(counts[b], depth) is zero (what store, reset,
 * load and the reference's save produce); behaviour on other tables is unspecified.
 * flags: 0, or MFPA_MAINTAIN_FULL_ROWS to read all `depth` slots of every bucket instead of counts[b] first and the valid
 * prefix alone (the same results under the invariant).
 *
 * mfpa_audfprint_remove: removes a SET of ids in one pass, in place.  in_set (n_ids) uint8, nonzero = remove the id;
 *   removed (n_ids) int32 receives the matches of each id over the whole table (the call zeroes it first).  A bucket without
 *   a match is left as it is, a counts[b] above depth included; in a bucket with one the other entries of the first n slots
 *   move to the front in order, the rest of the row becomes zero and counts[b] the number kept (the entries the reservoir
 *   dropped are forgotten, :289-290).  The result equals the reference's remove called once per id, in any order.
 *   n_ids == 0 (the empty set): MFPA_OK, no launch.
 *
 * mfpa_audfprint_retrieve_count / mfpa_audfprint_retrieve: the (time, hash) rows of K distinct ids, concatenated in request
 *   order; one id's rows are (table[b][j] & (2^timebits - 1), b) of every match, bucket ascending then slot ascending
 *   (:309-315).  rank (n_ids) int32 = the request rank 0..K-1 of each requested id, -1 elsewhere (ids >= n_ids are not
 *   requested); work: mfpa_audfprint_retrieve_work_ints(hashbits, K) int32, carried from the first call to the second.
 *   _count fills offsets (K + 1) int32: rows of rank k are [offsets[k], offsets[k + 1]); the caller reads offsets[K], sizes
 *   rows (n_rows, 2) int32 and calls mfpa_audfprint_retrieve once (it consumes `work`).  Positions come from counts and
 *   scans, never from the arrival order of atomics: the output is deterministic.  Needs depth * 2^hashbits < 2^31.
 *   K == 0 (and n_rows == 0): MFPA_OK, no launch.
 */
#define MFPA_MAINTAIN_FULL_ROWS 1
int mfpa_audfprint_remove(uint32_t* table, int32_t* counts, int hashbits, int timebits, int depth, const uint8_t* in_set,
                          int n_ids, int flags, int32_t* removed, void* stream);
int mfpa_audfprint_retrieve_work_ints(int hashbits, int K, long long* ints);
int mfpa_audfprint_retrieve_count(const uint32_t* table, const int32_t* counts, int hashbits, int timebits, int depth,
                                  const int32_t* rank, int n_ids, int K, int flags, int32_t* work, int32_t* offsets,
                                  void* stream);
int mfpa_audfprint_retrieve(const uint32_t* table, const int32_t* counts, int hashbits, int timebits, int depth,
                            const int32_t* rank, int n_ids, int K, int flags, int32_t* work, const int32_t* offsets,
                            int32_t* rows, int n_rows, void* stream);

/* Dejavu fingerprint store and matcher.  Integer only; results equal the reference's exactly.
 *
 * Table: (n_rows, 5) int32 rows [w0, w1, w2, song_id, offset], w0..w2 the 10-byte digest (sha1 hex[:20],
 * afp/dejavu/fingerprint.py:174-213) as big-endian words with bytes 8-9 in the high half of w2; sorted by
 * (hash, song_id, offset) and unique -- the fingerprints table of afp/dejavu/postgres_database.py:266-281 under its
 * UNIQUE(song_id, offset, hash) constraint.  directory (2^dirbits + 1) int32: directory[b] = the first row whose leading
 * dirbits hash bits are >= b.  dirbits in [1, 24].  song ids in [1, 2^24 - 1], offsets in [0, 2^31).
 *
 * mfpa_dejavu_store: INSERT ... ON CONFLICT DO NOTHING (postgres_database.py:288-295, :156-178) of a whole set of rows.
 *   digests (n,10) uint8, sids (n) int32, offsets (n) int32; order (n) int64 = the row indices sorted by (hash, song_id,
 *   offset) (any order among equal rows); work: max(1, ceil(n / 256)) int32; table: room for n rows; n_rows (1) int32
 *   receives the number of unique rows written.  The table's bytes depend only on the set of rows.
 *
 * mfpa_dejavu_lookup: row ranges [ranges[2i], ranges[2i+1]) of the n query digests (n,10) uint8
 *   (SELECT_MULTIPLE, postgres_database.py:212-219, one hash per IN list).
 *
 * mfpa_dejavu_match: CommonDatabase.return_matches (postgres_database.py:180-229) + Dejavu.align_matches
 *   (afp/dejavu/dejavu.py:312-378) for B queries, each taken as the SET of its (hash, t1) pairs (file_recognizer.py:20-27).
 *   digests (B,cap,10) uint8, t1 (B,cap) int32, nq (B) int32 pairs per query (the layout of mfpa_dejavu_hashes);
 *   scratch: B * mfpa_dejavu_match_scratch_bytes(cap, hcap) bytes, hcap a power of two in [64, 2^26] (hits per query);
 *   out (B,K,4) int32 rows [song_id, offset, count of that song's best offset, hashes_matched], count descending, ties to
 *   the smaller song id; the best offset of a song is the smallest among its tied maxima; rows past info[2] are not
 *   written.  info (B,4) int32 = [n_hits, n_distinct_pairs, rows written, songs hit], or [n_hits, -1, -1, -1] when
 *   n_hits > hcap (nothing else is written: call again with a larger hcap).
 */
int mfpa_dejavu_store(const uint8_t* digests, const int32_t* sids, const int32_t* offsets, const int64_t* order, long long n,
                      int dirbits, int32_t* work, int32_t* table, int32_t* n_rows, int32_t* directory, void* stream);
int mfpa_dejavu_lookup(const int32_t* table, const int32_t* directory, int dirbits, const uint8_t* digests, int n,
                       int32_t* ranges, void* stream);
int mfpa_dejavu_match_scratch_bytes(int cap, long long hcap, long long* bytes);
int mfpa_dejavu_match(const int32_t* table, const int32_t* directory, int dirbits, const uint8_t* digests, const int32_t* t1,
                      const int32_t* nq, int B, int cap, long long hcap, void* scratch, int K, int32_t* out, int32_t* info,
                      void* stream);

/* ---------------------------------------------------------------------------------------
 * UNet denoiser building blocks, training/unet.py:8-108.  Activations are NHWC float32
 * ("pixels x channels": H = frequency bins, W = frames); with C = 1 at both ends of the
 * network this is byte-identical to the reference's NCHW (B,1,257,T) tensors.
 */

/* 3x3 convolution, padding 1, no bias, fused per-channel affine (folded eval BatchNorm) + ReLU
 * (DoubleConv halves, unet.py:16-21).  The input may be the channel-concatenation of two
 * tensors [x0 | x1] where x1 has its own extent (H1, W1) <= (H, W) and is zero-padded at the
 * bottom/right (Up.forward, unet.py:56-63); pass x1 = NULL, C1 = 0 for a plain conv.
 *   x0 (B,H,W,C0)  x1 (B,H1,W1,C1)  w (9, Cout, C0+C1): [tap = ky*3+kx][Cout][Cin]  scale/shift (Cout)
 *   y  (B,H,W,Cout);  relu: 0/1;  scale/shift may be NULL (identity).
 * C0, C1 multiples of 32; Cout a multiple of 64.  precision: 0 = float32 MFMA (exact fp32 products). */
int mfpa_conv3x3_bn_relu(const float* x0, int C0, const float* x1, int C1, int H1, int W1,
                         int B, int H, int W, const float* w, int Cout,
                         const float* scale, const float* shift, int relu, int precision,
                         float* y, void* stream);

/* General form of the MFMA implicit-GEMM convolution (same kernel as the two entry points above
 * and below), used by the training step: forward with the previous layer's BatchNorm + ReLU applied
 * to source 0 ON LOAD, input gradients (a 3x3 conv of dz with transposed, flipped weights; mode 2 for
 * the transposed conv), cropped outputs.  training/unet.py:8-65, training/train.py:314-316 (backward).
 *   mode 0: 3x3 conv pad 1;  1: ConvTranspose2d(k2,s2) forward (y is (B,2H,2W,Cout));
 *        2: ConvTranspose2d input gradient (x0 is (B,2H,2W,C0), y is (B,H,W,Cout), w (4,Cout,C0))
 *   in_scale0/in_shift0 (C0) or NULL: x0 <- relu(x0*scale+shift) per channel when loaded
 *   x1 (B,H1,W1,C1) zero-padded to (H,W) like mfpa_conv3x3_bn_relu (mode 0 only)
 *   yH,yW: output extent (0 = H,W): pixels beyond are not stored, y is (B,yH,yW,Cout)  (modes 0, 2)
 */
typedef struct mfpa_conv_desc {
  const float* x0; const float* in_scale0; const float* in_shift0;
  const float* x1;
  const float* w; const float* out_scale; const float* out_shift;
  float* y;
  int C0, C1, H1, W1;
  int B, H, W, Cout, relu;
  int yH, yW, mode;
  unsigned drop_seed, drop_thresh; /* training Dropout on source 0 after the affine+ReLU: keep element idx iff */
  float drop_scale;                /* hash(seed, idx) >= thresh (= rate * 2^32), scaled by 1/(1-rate); 0 = off  */
  int precision;                   /* 0 = fp32 MFMA; 1 = bf16x3 (w must then be in the pre-split row format);
                                    * 2 = plain bf16 (mode 0: w_layout 2 only -- the same fragment-ordered image, of which only the hi halves are
                                    *     read; one MFMA per product, relative error ~2^-9: the training step's "bf16 MFMA" arithmetic.  Round 6:
                                    *     also mode 1 with bfloat16 I/O (x0_is_bf16 or y == NULL) and mode 2, on the ROW image of precision 1:
                                    *     the transposed convolution of the training step and its input gradient use the hi halves only) */
  float* y_pool;                   /* mode 0, optional: MaxPool2d(2) of the output fused in the epilogue, (B,H/2,W/2,Cout) */
  const float* w1x1; float b1x1;   /* mode 0, Cout == 64, optional: OutConv 1x1 to one class fused in the epilogue:        */
  float* y1x1;                     /*   y1x1 (B,H,W) = sum_c out[..][c]*w1x1[c] + b1x1; y may then be NULL (not stored)    */
  /* mode 0, C0 == Cout == 64, C1 == 0, optional: source 0 is COMPUTED while it is staged (x0 may be NULL) as the UNet's
   * first layer of mfpa_conv3x3_c1_bn_relu -- relu((conv3x3 of the 1-channel input) * c1_scale + c1_shift), input =
   * c1_x32 (B,H,W) or (float)(c1_spec64 / c1_denom[b]) -- so inc.double_conv's 64-channel intermediate never exists
   * in HBM (unet.py:8-24, 86). */
  const float* c1_x32; const double* c1_spec64; const double* c1_denom;
  const float* c1_w; const float* c1_scale; const float* c1_shift;
  /* precision 1, mode 0: which bf16x3 image `w` holds.  0 = the row image ([tap][Cin / 32][Cout][128 B], staged through LDS);
   * 2 = the FRAGMENT-ORDERED image of the weights-direct kernels (a wave reads the MFMA weight operand of its column tile straight
   * from L1 / L2: no weight tile in LDS, one barrier per 32-channel chunk instead of one per tap): [tap][Cin / 32][Cout / 16]
   * [hi | lo][lane 64][16 B] for v_mfma_f32_16x16x32_bf16 (conv_ws64_kernel, conv_wd16_kernel) -- valid exactly where
   * mfpa_conv_weight_layout() returns 2, MFPA_EINVAL otherwise.  Any other value is MFPA_EINVAL. */
  int w_layout;
  /* w_layout 2, mode 0, optional (training forward): a bf16 copy of source 0 AS THE CONVOLUTION SAW IT (in_scale0 / in_shift0 / ReLU /
   * dropout applied), (B,H,W,C0), written by the halo loader of the first output-channel tile -- the operand mfpa_wgrad_mfma(precision 3)
   * reads in the backward pass, without a cast pass of its own.  Also written by the bf16x3 transposed convolution (mode 1, precision 1).
   * MFPA_EINVAL with any other kernel. */
  void* x0_bf16;
  /* the same for the zero-padded source 1, (B,H1,W1,C1) (plain cast: source 1 carries no on-load transform), and for the OUTPUT,
   * (B,yH,yW,Cout) -- when the output is itself an operand of a later mfpa_wgrad_mfma(precision 3) (the transposed convolution's). */
  void* x1_bf16;
  void* y_bf16;
  /* w_layout 2, mode 0, optional (training forward): per-wave partial BatchNorm statistics of the stored output, [rows][2][Cout] floats
   * with rows = mfpa_conv_stats_rows(B, H, W, C0 + C1, Cout): (sum, sum of squares) per channel over each wave's pixels.
   * mfpa_conv_stats_reduce sums the rows in float64 (fixed order) into the `sums` of mfpa_bn_stats_finish -- the statistics without a
   * pass over the output.  MFPA_EINVAL with any other kernel. */
  float* stats_part;
  /* with stats_part, optional (training backward): the output is the gradient dy w.r.t. relu(bn(bwd_z)) -- bwd_z (B,yH,yW,Cout) the
   * BatchNorm's input, bwd_scale / bwd_shift / bwd_mean / bwd_invstd (Cout) its statistics, no dropout behind it -- and the partials are
   * (sum g, sum g * xhat) with g = dy where bwd_z * scale + shift > 0 else 0: after mfpa_conv_stats_reduce the `local_sums` of
   * mfpa_bn_relu_bwd_finish, without the reduction pass over (dy, z). */
  const float* bwd_z; const float* bwd_scale; const float* bwd_shift; const float* bwd_mean; const float* bwd_invstd;
  /* x0 (and x1, when given) are BFLOAT16 tensors.  precision 2, mode 0, (C0 + C1) % 64 == 0 (conv_wd16_kernel): the bf16 copy of dz
   * written by mfpa_bn_relu_bwd -- staged without any split arithmetic, half the bytes -- or, round 5, the training step's activations
   * kept as bfloat16 in HBM: an on-load affine / ReLU / dropout is applied in float32 to the widened values and rounded to bf16 once
   * (x0_bf16 still receives that copy; x1 is its own copy: x1_bf16 must be null).  mode 1, precision 1: the transposed convolution's
   * source.  Such a launch may also leave its OUTPUT as bfloat16 only: y null, y_bf16 the (B,yH,yW,Cout) [mode 1: (B,2H,2W,Cout)]
   * destination (stats_part still describes the float32 accumulators). */
  int x0_is_bf16;
  /* round 5, inference launches that conv_ws64_kernel serves only (mfpa_conv_scale_folds() == 1; otherwise MFPA_EINVAL): tensors in the
   * SPLIT layout -- same shape and byte count as the float32 NHWC tensor, but every 32-channel chunk of a pixel holds [32 bf16 hi | 32
   * bf16 lo] (x = hi + lo to 2^-17) instead of 32 floats: exactly what a bf16x3 convolution's loader makes of the float32 values, made
   * ONCE by the producer.  x0_split / x1_split: source 0 / 1 arrives in it (the loader waves copy 16-byte pieces, no arithmetic);
   * y_split / y_pool_split: `y` / `y_pool` leave in it.  A split tensor can only feed another such launch. */
  int x0_split, x1_split, y_split, y_pool_split;
  /* bwd_z is a BFLOAT16 tensor (the activations of the line above). */
  int bwd_z_is_bf16;
} mfpa_conv_desc;
int mfpa_conv_mfma(const mfpa_conv_desc* d, void* stream);
/* HOST function, no GPU needed: validation and kernel choice of mfpa_conv_mfma as one routing step (host arithmetic on the descriptor
 * only; no pointer is dereferenced).  Returns MFPA_EINVAL exactly where mfpa_conv_mfma does; otherwise MFPA_OK and, in *out when it is
 * given, the template instantiation that serves `d` -- family MFPA_CONV_NONE for the no-op B == 0.  mfpa_conv_mfma itself launches from
 * this route; mfpa_conv_scale_folds / mfpa_conv_c1_layout / mfpa_conv_stats_rows answer from the shape rules it uses.  The persistent kernels' grids are
 * clamped to the device's CUs at launch: that is not part of the route. */
enum {
  MFPA_CONV_NONE = -1,
  MFPA_CONV_WS64 = 0,          /* conv_ws64_kernel<C1SRC> (csrc/unet_ws.hip): inference, bf16x3, w_layout 2, 8 x 32 patch, 64 channels */
  MFPA_CONV_WD16 = 1,          /* conv_wd16_kernel<PH, PW, ROWS, WMW, SIDE, PLAIN, IN16, AFF16>: w_layout 2, what WS64 does not serve + the training step */
  MFPA_CONV_MFMA = 2,          /* conv_mfma_kernel<BN, PH, PW, PH * PW / 64, BN / 64, MODE, PREC, C1SRC>: the row image, modes 0 and 2 */
  MFPA_CONV_CONVT = 3          /* convT_mfma_kernel<PH, PW, PREC, IO16, PLAIN>: mode 1 */
};
typedef struct mfpa_conv_route {
  int family;                  /* MFPA_CONV_* */
  int ph, pw;                  /* PH x PW: the patch of output pixels [mode 1: input pixels] of one workgroup tile */
  int bn;                      /* output channels per workgroup (conv_mfma_kernel's BN; 64 for WS64 / CONVT; 32 * (8 / WMW) for WD16) */
  int wmw;                     /* WD16: WMW, the wave rows (2: 128-channel tiles, 4: 64-channel tiles); else 0 */
  int mode;                    /* the descriptor's mode (conv_mfma_kernel's MODE: 0 or 2) */
  int prec;                    /* precision family PREC: 0 = fp32 MFMA, 1 = the bf16 matrix cores (bf16x3, or plain bf16 where `plain`) */
  int c1src;                   /* C1SRC (WS64, MFMA): source 0 is the fused first layer */
  int rows, side, plain, in16, aff16;      /* WD16's ROWS / SIDE / PLAIN / IN16 / AFF16 (plain also CONVT's PLAIN) */
  int io16;                    /* CONVT's IO16: bfloat16 source and / or output */
  int stats_rows;              /* rows of stats_part written per tile (WD16 with stats_part: WMW), else 0: mfpa_conv_stats_rows =
                                * ceil(W / pw) * ceil(H / ph) * B * stats_rows */
} mfpa_conv_route;
int mfpa_conv_mfma_route(const mfpa_conv_desc* d, mfpa_conv_route* out);
/* HOST function: the w_layout (0 or 2) the fastest kernel for a (H, W) convolution of this shape reads. */
int mfpa_conv_weight_layout(int H, int W, int Cin, int Cout, int mode, int precision);
/* HOST function (round 5): 1 if the INFERENCE launch of this 3x3 shape (precision 1, w_layout 2, no on-load affine, no training side
 * output) runs on conv_ws64_kernel, whose epilogue is cheapest when the output scale is already IN the weights: pass out_scale = NULL
 * with weights pre-multiplied by the per-output-channel scale (then split / fragment-ordered as usual) and out_shift as before -- the shift
 * becomes the accumulators' start value and the epilogue a bare ReLU.  The same call with out_scale given stays valid everywhere.
 * Answered from the shape rules the route uses, not from a route: where the clip passes conv_ws64_kernel's byte-offset or tile-count limits
 * (or the 16-bit coordinates / 32-bit byte offsets of every kernel) it still says 1 although the launch runs on conv_wd16_kernel or is
 * rejected -- folded weights with out_scale = NULL are valid on every kernel.
 * Reference: the folded eval BatchNorm of DoubleConv, training/unet.py:16-21. */
int mfpa_conv_scale_folds(int H, int W, int Cin, int Cout);
/* HOST function (round 5): the w_layout the FUSED FIRST-LAYER launch of mfpa_conv_mfma (c1_x32 / c1_spec64 given, 64 -> 64 channels,
 * precision 1) reads at this image size: 2 = the fragment image (conv_ws64_kernel computes the first layer in its loader waves on the
 * matrix cores, bf16x3 like every other layer), 0 = the row image (conv_mfma_kernel computes it with exact fp32 FMAs in its loader).
 * Answered from the shape rules the route uses: beyond conv_ws64_kernel's byte-offset limit (H * W * 64 * 4 bytes near 2^32) and for H or W
 * above 32767 it still says 2 although mfpa_conv_mfma rejects that launch.
 * Reference: DoubleConv of `inc`, training/unet.py:16-21, 86. */
int mfpa_conv_c1_layout(int H, int W);
/* Round 6: a decoder level's FIRST convolution with the transposed convolution folded into it -- Up.forward of training/unet.py:58-65,
 *   up = ConvTranspose2d(Cl, Cu, 2, 2)(low); pad to the skip's size; y = relu(bn(conv3x3(cat([skip, up]))))        (eval-mode BatchNorm)
 * as ONE launch that reads `skip` and `low` and never forms `up`: nothing non-linear sits between the two convolutions, so the up half is,
 * per output phase (Y & 1, X & 1), a 2 x 2 convolution of `low` with composite weights (exact algebra; float64 check:
 * tools/exp_phase_composite.py) plus a bias that depends only on the pixel's border class.  Products: bf16x3 or exact fp32 (`precision`).
 *   mfpa_upconv_pack (one-time, device): w3 [9][Cout][Cs + Cu] (tap = 3 ky + kx: mfpa_conv_mfma's fp32 kernel layout), wt [4][Cu][Cl]
 *     (mfpa_convT2x2's layout), bt (Cu), scale (Cout, the folded BatchNorm scale, or NULL) -> wc16 [16][Cout][Cl] float32, index
 *     ((py * 2 + px) * 2 + ty) * 2 + tx = phase (py, px), low-resolution tap (ty - 1 + py, tx - 1 + px), and bias_tab (4, 4, Cout) by
 *     (row class, column class): 0 first row / column of the up-sampled extent, 1 interior, 2 its last, 3 the padding row / column of an
 *     odd size; both with `scale` multiplied in, float64 accumulation.
 *   mfpa_upconv_fused: w_skip = the w_layout-2 fragment image of (w3[:, :, :Cs] * scale) and w_up = that of wc16 (as a 16-tap kernel);
 *     shift (Cout) the folded BatchNorm shift.  skip (B,H,W,Cs), low (B,Hl,Wl,Cl), y (B,H,W,Cout) float32 NHWC; H - 2 Hl and W - 2 Wl in {0, 1}.
 *   mfpa_upconv_serves (HOST): 1 if mfpa_upconv_fused takes this shape, else 0 (the caller then runs mfpa_convT2x2 + mfpa_conv_mfma). */
typedef struct mfpa_upconv_desc {
  const float* skip; const float* low;
  const float* w_skip; const float* w_up;
  const float* shift; const float* bias_tab;
  float* y;
  int B, H, W, Cs, Hl, Wl, Cl, Cout, relu;
  int precision;                   /* 1: bf16x3 (w_skip / w_up = w_layout-2 fragment images); 0: exact fp32 products (v_mfma_f32_16x16x4_f32) on the
                                    * FP32 fragment images [tap][Cin / 32][Cout / 16][piece 2][lane 64][4 floats], lane (g = l >> 4, c = l & 15) =
                                    * output channel 16 t + c, input channels 32 chunk + 8 g + 4 piece .. + 3 */
} mfpa_upconv_desc;
int mfpa_upconv_fused(const mfpa_upconv_desc* d, void* stream);
int mfpa_upconv_pack(const float* w3, const float* wt, const float* bt, const float* scale, int Cout, int Cs, int Cu, int Cl,
                     float* wc16, float* bias_tab, void* stream);
int mfpa_upconv_serves(int H, int W, int Hl, int Wl, int Cs, int Cl, int Cout);

/* HOST function: rows of mfpa_conv_desc.stats_part for this shape (0: its kernel does not write them) = tiles x mfpa_conv_route.stats_rows
 * of the launch.  Answered from the shape rules the route uses: it also gives a row count where mfpa_conv_mfma rejects the launch (Cin % 32 != 0
 * at a multiple-of-128 Cout; H or W above 32767; a clip beyond 32-bit byte offsets), and MFPA_EINVAL above 2^31 - 1 rows. */
int mfpa_conv_stats_rows(int B, int H, int W, int Cin, int Cout);
/* stats_part (rows, 2, C) -> sums[2C] float64 as mfpa_bn_stats_sums produces them; workspace as for mfpa_bn_stats. */
int mfpa_conv_stats_reduce(const float* part, long long rows, int C, double* sums, double* workspace, void* stream);

/* First layer: 3x3 conv from ONE input channel (inc.double_conv.0, unet.py:86) fused with the
 * spectrogram normalisation: x = (float)(spec / denom) when spec64 != NULL, else x32 as is.
 *   w (9, Cout), y (B,H,W,Cout). */
int mfpa_conv3x3_c1_bn_relu(const float* x32, const double* spec64, const double* denom, int per_clip,
                            int B, int H, int W, const float* w, int Cout,
                            const float* scale, const float* shift, int relu, float* y, int y_is_bf16, float* stats_part /* optional: (B * H, 2, Cout) row partials of the output's (sum, sum of squares), see mfpa_conv_desc.stats_part */, void* stream);

/* MaxPool2d(2), floor (unet.py:34).  x (B,H,W,C) -> y (B,H/2,W/2,C). */
int mfpa_maxpool2(const float* x, int B, int H, int W, int C, float* y, void* stream);

/* ConvTranspose2d(k=2, s=2) + bias (unet.py:51-53).  x (B,H,W,Cin), w (4, Cout, Cin): [tap = dy*2+dx][Cout][Cin],
 * y (B,2H,2W,Cout). */
int mfpa_convT2x2(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias,
                  int Cout, int precision, float* y, void* stream);

/* OutConv 1x1 + bias to ONE class (unet.py:68-74).  x (B*H*W, C), w (C), y (B*H*W). */
int mfpa_conv1x1_out(const float* x, long long npix, int C, const float* w, float bias, float* y,
                     void* stream);

/* ---------------------------------------------------------------------------------------
 * UNet training step, training/train.py:257-317 (spec branch): forward in train mode, L1 loss,
 * backward, Adam.  A layer's BatchNorm+ReLU output is never materialised: convolutions write the raw
 * output z, mfpa_bn_stats reduces the batch statistics into per-channel (scale, shift), and consumers
 * apply relu(z*scale+shift) on load (mfpa_conv_mfma's in_scale0/in_shift0).  Reductions are two-stage
 * float64 and deterministic.  `workspace`: at least mfpa_red_blocks() * max(2*C, 65) doubles.
 */
int mfpa_red_blocks(void);

/* nn.BatchNorm2d in train mode (unet.py:17,20): z (npix, C) -> mean, invstd (biased var, eps),
 * scale = gamma*invstd, shift = beta - mean*scale; running_mean/var (momentum, unbiased var) updated
 * in place when non-NULL. */
int mfpa_bn_stats(const float* z, long long npix, int C, const float* gamma, const float* beta, float eps,
                  float momentum, float* mean, float* invstd, float* scale, float* shift,
                  float* running_mean, float* running_var, double* workspace, int z_is_bf16, void* stream);

/* BatchNorm+ReLU backward: dy (gradient w.r.t. relu(bn(z))) is overwritten with the gradient w.r.t. z;
 * dgamma, dbeta (C) are produced; coef is a (3, C) scratch.  dz_bf16 (optional, may be NULL): a bf16 copy of the result, written in
 * the same pass -- the operand mfpa_wgrad_mfma(precision 3) reads. */
int mfpa_bn_relu_bwd(float* dy, const float* z, long long npix, int C, const float* gamma,
                     const float* scale, const float* shift, const float* mean, const float* invstd,
                     float* dgamma, float* dbeta, float* coef, double* workspace,
                     unsigned drop_seed, unsigned drop_thresh, float drop_scale, void* dz_bf16, int write_f32,
                     int z_is_bf16, void* stream);
/* write_f32 = 0 (needs dz_bf16): only the bf16 copy of dz is written -- every consumer reads it (the plain-bf16 train step: the
 * input-gradient convolution takes it through mfpa_conv_desc.x0_is_bf16, the weight gradient as its bf16 operand) and dy is left as it was. */

/* The same two operations split for synchronised BatchNorm under data parallelism (statistics over the GLOBAL batch, as the
 * single-GPU reference computes them): *_sums reduces this rank's per-channel pairs into sums[2C] float64 -- (sum z, sum z^2)
 * forward, (sum g, sum g*xhat) backward, g = the ReLU/dropout-masked incoming gradient -- the caller all-reduces (SUM) them
 * and the pixel count over the ranks, *_finish completes from the global sums.  Backward: dgamma / dbeta come from the LOCAL
 * sums (the gradient all-reduce adds the ranks), the mean terms of the input gradient from the GLOBAL ones. */
int mfpa_bn_stats_sums(const float* z, long long npix, int C, double* sums, double* workspace, int z_is_bf16, void* stream);
/* round 5, single-GPU statistics (no all-reduce between the halves): mfpa_conv_stats_reduce + mfpa_bn_stats_finish as two launches
 * instead of three, and mfpa_conv_stats_reduce + mfpa_bn_relu_bwd_finish as three instead of four -- the finish kernels sum the row
 * blocks' float64 partials themselves, in mfpa_conv_stats_reduce's order: bit-identical results. */
int mfpa_conv_stats_bn_finish(const float* part, long long rows, int C, double count, const float* gamma, const float* beta, float eps,
                              float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                              float* running_var, double* workspace, void* stream);
int mfpa_bn_relu_bwd_from_part(float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                               const float* shift, const float* mean, const float* invstd, const float* part, long long rows,
                               float* dgamma, float* dbeta, float* coef, double* workspace, unsigned drop_seed, unsigned drop_thresh,
                               float drop_scale, void* dz_bf16, int write_f32, int z_is_bf16, int dy_is_bf16, void* stream);
int mfpa_bn_stats_finish(const double* sums, double count, int C, const float* gamma, const float* beta, float eps,
                         float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                         float* running_var, void* stream);
int mfpa_bn_relu_bwd_sums(const float* dy, const float* z, long long npix, int C, const float* scale, const float* shift,
                          const float* mean, const float* invstd, double* sums, double* workspace, unsigned drop_seed,
                          unsigned drop_thresh, float drop_scale, int z_is_bf16, void* stream);
int mfpa_bn_relu_bwd_finish(float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                            const float* shift, const float* mean, const float* invstd, const double* local_sums,
                            const double* global_sums, double global_count, float* dgamma, float* dbeta, float* coef,
                            unsigned drop_seed, unsigned drop_thresh, float drop_scale, void* dz_bf16, int write_f32,
                            int z_is_bf16, int dy_is_bf16, void* stream);

/* out[c] = sum over pixels of x[p][c]  (ConvTranspose2d bias gradient). */
int mfpa_colsum(const float* x, long long npix, int C, float* out, double* workspace, void* stream);

/* p = MaxPool2d(2)(relu(z*scale+shift)) (unet.py:34) and its backward: dy += route(dp) to the window's
 * first maximum.  drop_*: the nn.Dropout (unet.py:83,99-103) that follows this DoubleConv in train mode, applied
 * to relu(bn(z)) with the stateless mask of mfpa_conv_desc (thresh 0 = no dropout); mfpa_bn_relu_bwd applies the
 * same mask to the incoming gradient. */
int mfpa_bn_relu_pool(const float* z, int B, int H, int W, int C, const float* scale, const float* shift,
                      float* p, unsigned drop_seed, unsigned drop_thresh, float drop_scale, int z_is_bf16, int p_is_bf16, void* stream);
int mfpa_maxpool2_bwd_add(const float* z, int B, int H, int W, int C, const float* scale,
                          const float* shift, const float* dp, float* dy,
                          unsigned drop_seed, unsigned drop_thresh, float drop_scale, int z_is_bf16, void* stream);

/* The same pass, which also forms the partial sums of the BatchNorm backward that follows on this layer (training/unet.py:17-20 under
 * autograd: sum g and sum g * xhat per channel, g = dy * [z*scale+shift > 0] (* dropout), xhat = (z - mean) * invstd) over ALL pixels of
 * dy -- the pooled windows, the odd last row / column --, one row of `part` (B * (H / 2), 2, C) float per workgroup, to be finished by
 * mfpa_conv_stats_reduce + mfpa_bn_relu_bwd_finish: the separate reduction pass over dy and z is not needed.  C / 4 must divide 256. */
int mfpa_maxpool2_bwd_add_sums(const float* z, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                               const float* invstd, const float* dp, float* dy, unsigned drop_seed, unsigned drop_thresh,
                               float drop_scale, float* part, int z_is_bf16, void* stream);
/* round 5: an encoder block's last BatchNorm + ReLU backward without its finished input gradient in memory -- dy (the skip path's gradient,
 * (B,H,W,C) float32, or bfloat16 with dy_is_bf16) is only READ: g = dy + route(dp) is reduced to the BatchNorm-backward sums (`part`:
 * (B * (H / 2), 2, C) floats of scratch), dgamma / dbeta / coef ([3][C]) are finished, and g -- formed again -- goes through the backward
 * formula into the bfloat16 dz (B,H,W,C).  Replaces mfpa_maxpool2_bwd_add_sums + mfpa_bn_relu_bwd_from_part (same arithmetic per element;
 * single-GPU statistics; C a power of two <= 1024 with 256 % (C / 4) == 0). */
int mfpa_maxpool2_bwd_bn_relu_bwd(const float* z, int B, int H, int W, int C, const float* gamma, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, const float* dp, const void* dy, int dy_is_bf16, unsigned drop_seed,
                                  unsigned drop_thresh, float drop_scale, float* part, float* dgamma, float* dbeta, float* coef,
                                  double* workspace, void* dz_bf16, int z_is_bf16, void* stream);

/* Weight gradient on MFMA, ACCUMULATED into dw (zero it first):
 *   mode 0: dw[tap][co][ci] += sum_p dz[p][co] * xin[p + tap][ci]          (3x3 conv; dw (9,Cout,C0+C1))
 *   mode 1: dw[tap][co][ci] += sum_p dz[2y+dy,2x+dx][co] * xin[y,x][ci]    (transposed conv; dw (4,Cout,C0))
 * xin = [x0 (affine+ReLU on load if in_scale0) | x1 zero-padded] exactly as the forward saw it.
 * C0, C1, Cout multiples of 64.  precision 0: fp32 MFMA; 1: bf16x3 (both operands split hi + lo, 3 bf16 MFMAs per
 * product, fp32 accumulate) -- like mfpa_conv_desc.precision; 2: plain bf16 products (one MFMA; the sum over every pixel of
 * the batch averages the 2^-9 product rounding: relative L1 ~2e-3 per layer, and only the optimiser consumes the result). */
typedef struct mfpa_wgrad_desc {
  const float* dz; const float* x0; const float* in_scale0; const float* in_shift0; const float* x1;
  float* dw;
  int C0, C1, H1, W1;
  int B, H, W, Cout, mode;
  unsigned drop_seed, drop_thresh;
  float drop_scale;
  int precision;
} mfpa_wgrad_desc;
int mfpa_wgrad_mfma(const mfpa_wgrad_desc* d, void* stream);

/* precision 3 of mfpa_wgrad_mfma: dz / x0 / x1 are bfloat16 tensors of the same shapes holding the ACTIVATED operands (in_scale0 /
 * in_shift0 / dropout must be off), one bf16 MFMA per product like precision 2.  mfpa_act_to_bf16 makes such a copy: out[e] =
 * bf16(z[e]) (scale == NULL), or bf16(dropout_e(relu(z[e] * scale[c] + shift[c]))) -- the on-load transform the fp32 kernels apply
 * (the previous layer's BatchNorm + ReLU + Dropout, training/unet.py:8-25,99-103).  z (n) float32, n a multiple of C, C % 4 == 0. */
int mfpa_act_to_bf16(const float* z, long long n, int C, const float* scale, const float* shift, unsigned drop_seed,
                     unsigned drop_thresh, float drop_scale, void* out_bf16, void* stream);

/* First layer (1 input channel): dw[tap][co] += sum_p dz[p][co] * x[p + tap]; x as in
 * mfpa_conv3x3_c1_bn_relu (per-clip denominators). */
int mfpa_wgrad_c1(const float* dz, const float* x32, const double* spec64, const double* denom, int B, int H,
                  int W, int Cout, float* dw, int dz_is_bf16, void* stream);

/* OutConv in training: pred[p] = sum_c relu(z[p][c]*scale[c]+shift[c]) * w[c] + bias[0];
 * backward: dy[p][c] = dpred[p]*w[c], dwb = [C weight gradients, bias gradient]. */
int mfpa_outconv_fwd(const float* z, long long npix, int C, const float* scale, const float* shift,
                     const float* w, const float* bias, float* pred, int z_is_bf16, void* stream);
int mfpa_outconv_bwd(const float* z, const float* dpred, long long npix, int C, const float* scale,
                     const float* shift, const float* w, float* dy, float* dwb, double* workspace, int z_is_bf16, void* stream);
/* The same backward WITHOUT materialising dy (it is rank 1: dpred[p] * w[c]): the pass forms dwb and, holding z and dy of every element
 * anyway, the partial sums of the BatchNorm backward that follows on z's layer ({sum g, sum g * xhat}, one row of `part`
 * (mfpa_outconv_bwd_rows(npix, C), 2, C) float per workgroup, finished by mfpa_conv_stats_reduce); mfpa_bn_relu_bwd_finish_rank1 then
 * forms dy again from dpred and w while it applies the BatchNorm + ReLU backward: dz to dz_f32 (float32, may be null) and / or
 * dz_bf16.  No dropout on this layer (training/unet.py: the last DoubleConv feeds OutConv directly). */
int mfpa_outconv_bwd_rows(long long npix, int C, int* rows);
int mfpa_outconv_bwd_sums(const float* z, const float* dpred, long long npix, int C, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* w, float* dwb, double* workspace, float* part,
                          int z_is_bf16, void* stream);
int mfpa_bn_relu_bwd_finish_rank1(const float* dpred, const float* w1, const float* z, long long npix, int C, const float* gamma,
                                  const float* scale, const float* shift, const float* mean, const float* invstd,
                                  const double* local_sums, const double* global_sums, double global_count, float* dgamma,
                                  float* dbeta, float* coef, float* dz_f32, void* dz_bf16, int z_is_bf16, void* stream);

/* nn.L1Loss(mean) of float32 pred against the float64 target (train.py:280): loss[0] (float64) and,
 * if dpred != NULL, dpred = sign(pred - target) / n. */
int mfpa_l1_loss(const float* pred, const double* target, long long n, float* dpred, double* loss,
                 double* workspace, void* stream);

/* Operand image of a convolution's weights, rebuilt from the master fp32 parameters after every optimiser step (replaces the
 * host-side flip / transpose / bf16 split of the packing code).  w: [taps][Co][Ci] fp32.  out, precision 0: [taps][nrows][K] float rows;
 * precision 1: the bf16x3 image [taps][K / 32][nrows][128 B], a row = 32 bf16 hi | 32 bf16 lo in eight 16-byte slots stored at slot
 * index (logical ^ ((row >> 1) & 7)) -- a (tap, chunk, 128-row) tile is 16 KB contiguous (csrc/unet_mfma.hip); precision 3: the same split in
 * the FRAGMENT-ORDERED layout of mfpa_conv_desc.w_layout = 2 ([taps][K / 32][nrows / 16][hi | lo][lane][8 bf16]); precision 2 (the
 * image of the retired w_layout 1) is MFPA_EINVAL, and the codes stay numbered 1 + w_layout.  flip_transpose = 0: rows = output
 * channels row0 .. row0+nrows-1, K = Ci (forward operand).  flip_transpose = 1: rows = input channels row0 .. row0+nrows-1,
 * K = Co, and for taps == 9 the kernel is flipped (tap t <- 8 - t): the input-gradient operand (training/unet.py's Conv2d /
 * ConvTranspose2d backward).  Co, Ci, row0, nrows multiples of 32. */
int mfpa_pack_conv_weights(const float* w, int taps, int Co, int Ci, int flip_transpose, int row0, int nrows, int precision,
                           float* out, void* stream);
/* Every operand image a training step needs, in ONE launch (round 5): `jobs_dev` = `njobs` of these in DEVICE memory, each the argument set of
 * one mfpa_pack_conv_weights call (same checks apply, precision 2 included; the caller validates) plus tile0 = the number of 32 x 32 tiles of all jobs before it
 * (a job has (K / 32) * (nrows / 32) * taps tiles, K = flip_transpose ? Co : Ci); total_tiles = their sum.  Pointers and shapes of a
 * training engine never change, so the table is built once and the launch repeated after every optimiser step. */
typedef struct mfpa_pack_job {
  const float* w; float* out;
  int taps, Co, Ci, flip_transpose, row0, nrows, precision, pad_;
  long long tile0;
} mfpa_pack_job;
int mfpa_pack_conv_weights_batch(const mfpa_pack_job* jobs_dev, int njobs, long long total_tiles, void* stream);
/* torch.optim.Adam step (train.py:661: lr 1e-3, betas (0.9, 0.999), eps 1e-8, no weight decay) on flat
 * arrays; g is multiplied by grad_scale first (1/world_size after a SUM all-reduce). step >= 1.
 * The hyper-parameters are taken as float32; the bias corrections 1 - beta^step are formed in double from
 * those float32 betas (tests/test_gpu_adam.py). */
int mfpa_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1,
                   float beta2, float eps, int step, float grad_scale, void* stream);

/* ---------------------------------------------------------------------------------------
 * Demucs causal waveform denoiser, forward (next-tier row SURVEY.md §8f-2), training/model.py:22-110,163-326.
 * Activations are time-major (B, L, C) float32.  Every Conv1d / ConvTranspose1d / LSTM projection is one batched
 * GEMM over (possibly overlapping) row windows on the fp32 matrix cores:
 *     C[b][m][n] = epi( sum_k A[b*strideA + m*lda + k] * W[n*K + k] + bias[n] ),  m < M
 *   W (npad, K) with npad a multiple of 64 (rows beyond N zero), K a multiple of 16
 *   mode 0: + bias, optional ReLU (relu = 1);  mode 2: additionally + addend[b*strideAdd + m*ldadd + n]
 *           (relu = 1: after the addition, relu = 2: before it -- `relu(convT(x)) + skip`, model.py:316)
 *   mode 1: GLU -- each 64-row tile of W holds 32 value rows then their 32 gate rows; N = output columns
 *   mode 3: (acc + bias) * (addend[...] > 0) -- the input gradient of a layer whose input was a ReLU output `addend`
 *   C2 (optional, training): mode 1 also stores the pre-activations (bias included) in the packed tile order, row pitch
 *           ldc2 >= npad; relu = 2 also stores relu(acc + bias) before the addition, mode 3 the unmasked acc + bias
 *           (same indexing as C)
 */
typedef struct mfpa_gemm_desc {
  const float* A; long long lda, strideA;
  const float* W; const float* bias;
  const float* addend; long long ldadd, strideAdd;
  float* C; long long ldc, strideC;
  int batch, M, N, K, npad, mode, relu;
  int precision;   /* 0: fp32 MFMA (K multiple of 16); 1: bf16x3 where K >= 128 is a multiple of 32 or K is 48 / 96 (fp32 MFMA otherwise);
                    * 2: bf16x3 with W ALREADY split -- every 32-element chunk of a row as [32 bf16 hi | 32 bf16 lo], w = hi + lo -- for
                    * weights that do not change between calls (K >= 128 a multiple of 32, npad a multiple of 128, no c1_x) */
  /* optional (K <= 256, fp32 kernel): A is COMPUTED while it is staged as the first encoder layer Conv1d(1 -> K, k8, s4) + ReLU
   * -- A[b][m][c] = relu(c1_b[c] + sum_j c1_w[j][c] * c1_x[b][4m + j]), c1_x (batch, c1_lin), c1_w (8, K) --
   * so its (B, L, K) output never exists in HBM (model.py:231-238); A may then be NULL. */
  const float* c1_x; long long c1_lin; const float* c1_w; const float* c1_b;
  float* C2; long long ldc2, strideC2;
} mfpa_gemm_desc;
int mfpa_gemm_mfma(const mfpa_gemm_desc* d, void* stream);
/* The kernel mfpa_gemm_mfma would launch for `d`, host arithmetic only (no device is touched, nothing is launched): MFPA_EINVAL
 * exactly where mfpa_gemm_mfma returns it, otherwise MFPA_OK with *kernel_id (may be NULL) = one of the ids below;
 * MFPA_GEMM_NONE for the no-ops batch == 0 / M == 0.  mfpa_gemm_mfma itself looks this id up in its
 * launch table (GEMM_KERNELS, csrc/demucs_gemm.hip). */
enum {
  MFPA_GEMM_NONE = -1,
  MFPA_GEMM_PIPE = 0,          /* gemm_bf16x3_pipe_kernel<false>: 256 x 128 tile, K % 64 == 0, K >= 128, npad % 128 == 0, M >= 192 */
  MFPA_GEMM_PIPE_WSPLIT = 1,   /* gemm_bf16x3_pipe_kernel<true>: the same on a pre-split W (precision 2) */
  MFPA_GEMM_WIDE = 2,          /* gemm_bf16x3_wide_kernel<false>: 128 x 128 tile, K % 32 == 0, K >= 128, npad % 128 == 0 */
  MFPA_GEMM_WIDE_WSPLIT = 3,   /* gemm_bf16x3_wide_kernel<true>: the same on a pre-split W (precision 2) */
  MFPA_GEMM_BF16X3 = 4,        /* gemm_bf16x3_kernel: 128 x 64 tile, K % 32 == 0, K >= 128 */
  MFPA_GEMM_SHORTK48_C1 = 5,   /* gemm_shortk_bf16x3_kernel<true, 48, 48>: K == 48, A computed from c1_x */
  MFPA_GEMM_SHORTK48 = 6,      /* gemm_shortk_bf16x3_kernel<false, 48, 48>: K == 48 */
  MFPA_GEMM_SHORTK96 = 7,      /* gemm_shortk_bf16x3_kernel<false, 96, 48>: K == 96 */
  MFPA_GEMM_SMALLK48_C1 = 8,   /* gemm_smallk_kernel<true, 48>: fp32 products, K == 48, A computed from c1_x */
  MFPA_GEMM_SMALLK48 = 9,      /* gemm_smallk_kernel<false, 48>: fp32 products, K == 48 */
  MFPA_GEMM_MFMA_C1 = 10,      /* gemm_mfma_kernel<true>: fp32 products, any K % 16 == 0 up to 256, A computed from c1_x */
  MFPA_GEMM_MFMA = 11          /* gemm_mfma_kernel<false>: fp32 products, any K % 16 == 0 */
};
int mfpa_gemm_mfma_route(const mfpa_gemm_desc* d, int* kernel_id);

/* mix / (floor + std) zero-padded to VL samples, std = unbiased std over time (model.py:293-301). */
int mfpa_demucs_prep(const float* wav, int B, int T, int VL, float floor_, float* out, float* stdv, void* stream);
/* sinc x2 resamplers (model.py:41-88), kernel112 = sinc(t)*hann at the half-sample offsets (model.py:28-38).
 * upsample2: (B,T) -> (B,2T).  downsample2: (B,T) -> first Tkeep (or all ceil(T/2)) samples of the result, row pitch To,
 * each multiplied by scale[b] when scale != NULL (the final `std * x` of model.py:326). */
int mfpa_upsample2(const float* x, int B, int T, const float* kernel112, float* y, void* stream);
int mfpa_downsample2(const float* x, int B, int T, const float* kernel112, float* y, int To, const float* scale,
                     int Tkeep, void* stream);
/* First encoder layer Conv1d(1->C, k8, s4), + ReLU when relu != 0: x (B,Lin) -> y (B,Lout,C), w (8,C) tap-major, bias (C) or
 * NULL.  Without the ReLU and the bias, with x = the gradient of the last ConvTranspose1d's output and w = its (8, C) taps, this
 * is that layer's input gradient. */
int mfpa_conv1d_c1(const float* x, int B, int Lin, int Lout, int C, const float* w, const float* bias, int relu, float* y,
                   void* stream);
/* Last decoder layer ConvTranspose1d(C->1, k8, s4): P (B,L+2,C) with zero first/last rows -> y (B, 4(L+1)), w (8,C). */
int mfpa_convT1d_c1(const float* P, int B, int L, int C, const float* w, float bias, float* y, void* stream);
/* The whole first encoder level in one launch (model.py:66-75,303-307: Conv1d(1, C, 8, 4) + ReLU + Conv1d(C, 2C, 1) + GLU):
 * x (B, Lin) -> y (B, Lout, C), Lout = (Lin - 8) / 4 + 1; the (B, Lout, C) output of the first convolution never exists in
 * memory and, unlike mfpa_gemm_mfma with c1_x set, is evaluated once per row (one workgroup owns all packed GLU columns); the
 * result has the same bits as that form.  w1 (8, C) tap-major, b1 (C) as for mfpa_conv1d_c1; gw (128, C) / gb (128) in the
 * packed GLU tile order.  C must be 48, Lin a multiple of 4 and x 16-byte aligned (a row's 8 samples are read as two float4). */
int mfpa_conv1d_c1_glu(const float* x, int B, int Lin, int Lout, int C, const float* w1, const float* b1, const float* gw,
                       const float* gb, float* y, void* stream);
/* The whole last decoder level in one launch (model.py:80-88,316-318: Conv1d(C, 2C, 1) + GLU + ConvTranspose1d(C, 1, 8, 4)):
 * x (B, L, C) -> y (B, 4 (L + 1)) without the (B, L, C) GLU output in memory.  gw (128, C) / gb (128) = the 1x1 weights and bias
 * in the packed GLU tile order of mfpa_gemm_mfma mode 1, wl (8, C) tap-major as for mfpa_convT1d_c1.  C must be 48 (MFPA_EINVAL
 * otherwise: callers then run mfpa_gemm_mfma mode 1 + mfpa_convT1d_c1). */
int mfpa_glu_convT1d_c1(const float* x, int B, int L, int C, const float* gw, const float* gb, const float* wl, float bias, float* y,
                        void* stream);
/* The same with the bias read from device memory (training: the optimiser updates it there). */
int mfpa_convT1d_c1_dev(const float* P, int B, int L, int C, const float* w, const float* bias_dev, float* y, void* stream);

/* One LSTM time step in ONE launch: gates = hprev W_hh^T + xp (hprev NULL at t = 0: gates = xp), then the cell update (gate
 * order i,f,g,o; model.py:91-110 via nn.LSTM): c (B,H) in/out, hout rows ldh apart; optional hsum = h + addend (the first
 * decoder skip).  whh_grouped = W_hh (4H,H) with rows regrouped to [H/16][i16|f16|g16|o16][H] so a workgroup owns all
 * four gates of its 16 hidden units; xp (B,4H) in the standard gate order, rows ldxp apart, includes both biases.
 * bf16x3 products, fp32 accumulate.  H multiple of 128.  The mfpa_lstm_* entry points, forward and backward, are csrc/lstm.hip. */
int mfpa_lstm_step(const float* hprev, long long ldhp, const float* whh_grouped, const float* xp, long long ldxp, float* c,
                   int B, int H, float* hout, long long ldh, float* hsum, const float* addend, long long ldadd, void* stream);

/* ---------------------------------------------------------------------------------------
 * Demucs training step (training/train.py:275-312, input_type "audio": loss.backward() through training/model.py:290-326).
 * Input gradients are mfpa_gemm_mfma calls on re-laid-out weights (a Conv1d's input gradient is a ConvTranspose1d of the
 * output gradient and vice versa); the entries below are the rest of the backward pass.  csrc/demucs_train.hip (mfpa_lstm_*: csrc/lstm.hip). */
/* mfpa_lstm_step that also keeps what the backward step needs: the gate activations [sig i | sig f | tanh g | sig o] of this
 * step in gsave (B rows ldgs apart; may alias xp) and c_t in cout; the previous cell state is read from cprev (NULL = 0). */
int mfpa_lstm_step_train(const float* hprev, long long ldhp, const float* whh_grouped, const float* xp, long long ldxp,
                         const float* cprev, long long ldcp, float* cout, long long ldco, int B, int H, float* hout, long long ldh,
                         float* hsum, const float* addend, long long ldadd, float* gsave, long long ldgs, void* stream);
/* One LSTM backward time step in one launch: dh = dhout + dgnext W_hh (dgnext = the gate gradients of step t+1, NULL at the
 * last step; whhT = W_hh^T (H, 4H)), then the cell backward: `gates` (the activations mfpa_lstm_step_train saved for step t)
 * is overwritten with the gate pre-activation gradients [di | df | dg | do]; dcstate (B, H) carries dc between steps (zero it
 * before the last step).  ct / cprev: c_t and c_{t-1} (cprev NULL at t = 0).  bf16x3 products.  H multiple of 128. */
int mfpa_lstm_step_bwd(const float* dgnext, long long ldgn, const float* whhT, float* gates, long long ldg, const float* ct,
                       long long ldct, const float* cprev, long long ldcp, const float* dhout, long long lddh, float* dcstate, int B,
                       int H, void* stream);
/* Weight-gradient GEMM: C[m][n] += sum_{b < batch, r < R} A[b*strideA + r*lda + m] * Bm[b*strideB + r*ldb + n]  (C is
 * ACCUMULATED into: zero it first).  Rows are time steps: A = an output gradient (B, L, M), Bm = the layer's input as
 * (possibly overlapping) row windows -- ldb = 4*Cin, N = 8*Cin for the k8/s4 convolutions.  fp32 MFMA
 * (v_mfma_f32_32x32x2_f32: both operands are K-major in HBM, which is that instruction's fragment order), K split over
 * workgroups, float atomics.  M, N, lda, ldb multiples of 4. */
typedef struct mfpa_gemm_tn_desc {
  const float* A; long long lda, strideA;
  const float* Bm; long long ldb, strideB;
  float* C; long long ldc;
  int batch, R, M, N;
  float* colsum;   /* optional (M): colsum[m] += the sum over every row of A[.][m] -- the bias gradient, read off the tiles the
                      workgroups of the first column tile stage anyway */
  int precision;   /* 0: fp32 MFMA; 1: bf16x3 (3 bf16 MFMAs per product); 2: plain bf16 (one MFMA; the sum over every time
                      step of the batch averages the 2^-9 product rounding) -- fragments via ds_read_b64_tr_b16 */
} mfpa_gemm_tn_desc;
int mfpa_gemm_tn(const mfpa_gemm_tn_desc* d, void* stream);
/* GLU backward (nn.GLU(1), model.py:237,246): u (rows, npad) holds the packed pre-activations mfpa_gemm_mfma stored through C2;
 * in place u <- dL/du given dg (rows, N) = dL/d(glu output), row pitch ldg. */
int mfpa_glu_bwd(float* u, long long rows, int npad, int N, const float* dg, long long ldg, void* stream);
/* out[c] += sum_r x[r*ld + c] (bias gradients; out is accumulated into).  C multiple of 4, <= 4096. */
int mfpa_colsum_any(const float* x, long long rows, int C, long long ld, float* out, void* stream);
/* Weight gradient of the two one-channel convolutions (encoder.0.0 and the last ConvTranspose1d), w (8, C) tap-major:
 * dw[j][c] += sum_{b, t < L} x[b*ldx + 4t + j] * g[b*strideG + t*ldg + c].  C <= 256. */
int mfpa_c1_wgrad(const float* x, long long ldx, const float* g, long long ldg, long long strideG, int B, int L, int C, float* dw,
                  void* stream);
/* Adjoint of mfpa_downsample2: dy (B rows ldy apart, nout gradients each, scaled by scale[b] like the forward) -> dx (B, T). */
int mfpa_downsample2_adjoint(const float* dy, int B, int ldy, int nout, const float* kernel112, const float* scale, int T, float* dx,
                             void* stream);

/* Whole-layer forms (one call across the ABI for the launches of time steps [t0, t1); backward: t1-1 down to t0): (B, Tn, .)
 * contiguous buffers.  mfpa_lstm_layer_range: xp (B,Tn,4H) input projections incl. biases; inference (train = 0): cstate (B,H)
 * scratch, cseq unused; train = 1: cseq (B,Tn,H) receives c_t and xp is overwritten with the gate activations; xsum / skip as in
 * mfpa_lstm_step (NULL for the first layer).  mfpa_lstm_layer_bwd_range: gates <- gate pre-activation gradients, dcstate (B,H)
 * scratch.  A sub-range lets the two layers run as a pipeline on two streams: layer 1 works on chunk k while layer 0 is already
 * on chunk k+1.  The state buffers (cstate / dcstate) are zeroed by the call that holds the first step of the recurrence. */
int mfpa_lstm_layer_range(const float* whh_grouped, float* xp, float* hseq, float* cseq, float* cstate, int B, int Tn, int H,
                          float* xsum, const float* skip, int train, int t0, int t1, void* stream);
int mfpa_lstm_layer_bwd_range(const float* whhT, float* gates, const float* cseq, const float* dhout, float* dcstate, int B, int Tn,
                              int H, int t0, int t1, void* stream);

/* mfpa_lstm_layer_range as ONE persistent launch (lstm_seq_kernel, csrc/lstm.hip): a workgroup keeps the W_hh slice of its 16
 * hidden units in registers for all steps, the workgroups of a 64-clip slab exchange h[t] through `work` (already split into
 * bf16 hi / lo) and meet at a device-memory counter after every step.  Same arguments and results as mfpa_lstm_layer_range
 * (model.py:91-110, torch.nn.LSTM's recurrence); `work` = device scratch of the size mfpa_lstm_seq_work_bytes reports, owned by this
 * layer while the call runs, zeroed once before its first use.  Every wait in the kernel is bounded: if one ever gives up the
 * kernel raises the 32-bit word at byte mfpa_lstm_seq_error_offset() of `work` (and finishes with undefined results); callers
 * read that word before the results leave their operator (the Python host does: ops_demucs.lstm_results_ok).  The grid must be
 * co-resident: the call keeps its own workgroups within `wg_budget` (0 = one per CU of the current device; a caller that runs two
 * such launches side by side, like the chunked two-stream pipeline, passes half the CU count), but it cannot see other work --
 * mfpa_lstm_seq_workgroups reports how many workgroups a launch keeps resident so that a host can account for launches in flight on
 * other streams (ops_demucs._ResidentGuard); a second PROCESS occupying the same GPU is the case the bounded waits and the error word
 * exist for; one process per GPU is the intended deployment.  Shapes outside the persistent kernel's range (H / 128 not in
 * {2,4,6,8}, more workgroups than the budget even with 64-clip slabs) take the per-step path inside the same call. */
int mfpa_lstm_seq_work_bytes(int B, int H, long long* bytes);   /* HOST function: *bytes = size of `work` */
int mfpa_lstm_seq_error_offset(void);
int mfpa_lstm_seq_workgroups(int B, int H, int wg_budget, int* workgroups);   /* HOST function: resident workgroups of the launch, 0 = per-step path */
int mfpa_lstm_layer_seq(const float* whh_grouped, float* xp, float* hseq, float* cseq, float* cstate, int B, int Tn, int H, float* xsum,
                        const float* skip, int train, int t0, int t1, int wg_budget, void* work, void* stream);

/* mfpa_lstm_layer_bwd_range as ONE persistent launch (lstm_bwd_seq_kernel, csrc/lstm.hip): the backward recurrence of a layer for
 * steps t1-1 .. t0 (torch.nn.LSTM's backward through time, training/train.py:275-312 via autograd in the reference).  A workgroup keeps
 * the W_hh^T rows of its 16 hidden units in registers (16 x 16 x 32 MFMAs, K = 4H), the workgroups of a 64-clip slab exchange dgates[t]
 * through `work` (already split into bf16 hi / lo) and meet at a device-memory counter after every step.  Same arguments and results as
 * mfpa_lstm_layer_bwd_range; `work`, the bounded waits and the error word as for mfpa_lstm_layer_seq (size: mfpa_lstm_bwd_seq_work_bytes,
 * error word at byte mfpa_lstm_seq_error_offset()).  A workgroup reads its slab's whole dgates[t+1] (K = 4H) every step, so the slab is
 * the smallest of 16 / 32 / 64 clips whose workgroups (slabs x H / 16) fit `wg_budget` (0 = one per CU; a caller that runs two such launches
 * concurrently, like the chunked two-stream pipeline, passes half the CU count: every workgroup of a launch must be resident at once).
 * H / 64 outside {4, 8, 12} or too many workgroups even with 64-clip slabs: the per-step path. */
int mfpa_lstm_bwd_seq_work_bytes(int B, int H, long long* bytes);   /* HOST function */
int mfpa_lstm_bwd_seq_workgroups(int B, int H, int wg_budget, int* workgroups);   /* HOST function, as mfpa_lstm_seq_workgroups */
int mfpa_lstm_layer_bwd_seq(const float* whhT, float* gates, const float* cseq, const float* dhout, float* dcstate, int B, int Tn, int H,
                            int t0, int t1, int wg_budget, void* work, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform-domain spectral losses of the Demucs branch, training/loss.py:10-186 (MultiResolutionSTFTLoss; forward).
 * The STFT of a resolution is mfpa_reflect_pad + mfpa_gemm_mfma (precision 0) with a windowed DFT matrix
 * (rows [re bins | zero rows up to im_off | im bins], K = window length padded to a multiple of 16); then:
 *   mfpa_dft_mag        mag[row][k] = sqrt(clamp(re^2 + im^2, 1e-7))                          (loss.py:10-41, `stft`)
 *   mfpa_stft_loss_sums out3 = [sum (|Y|-|X|)^2, sum |Y|^2, sum |log|Y| - log|X||] (float64)   (loss.py:44-83)
 * workspace: 3 * mfpa_loss_blocks() doubles.  mfpa_reflect_pad: out (B, Lout), out[i] = x[reflect(i + shift - pad)]
 * for i + shift < T + 2 pad, else 0 (torch.stft center=True / pad_mode "reflect"; `shift` makes the 16-byte-aligned copy
 * the odd frames of a hop that is not a multiple of 4 need). */
int mfpa_loss_blocks(void);
int mfpa_reflect_pad(const float* x, int B, int T, int pad, int shift, int Lout, float* out, void* stream);
int mfpa_dft_mag(const float* c, long long rows, int bins, long long ldc, int im_off, float* mag, void* stream);
int mfpa_stft_loss_sums(const float* cx, const float* cy, long long rows, int bins, long long ldc, int im_off, double* out3,
                        double* workspace, void* stream);
/* Gradient of one resolution with respect to the PREDICTED signal (the adjoint chain of the forward above):
 *   mfpa_stft_loss_grad       in place on cx: (re, im) <- dL/d(re, im), L = w_sc * sc + w_mag * mag (w_* carry the factors and the
 *                             1/#resolutions); sums = out3 of mfpa_stft_loss_sums (device); zero below the 1e-7 clamp
 *   (GEMM with the transposed DFT matrix: dframes = d(re, im) x W)
 *   mfpa_frames_adjoint       dxp[b][i] = sum_t dframes[b][t][i - t*hop - off]   (overlap-add of the frame gradients)
 *   mfpa_reflect_pad_adjoint  dx (+)= the reflect padding's adjoint of dxp */
int mfpa_stft_loss_grad(float* cx, const float* cy, long long rows, int bins, long long ldc, int im_off, const double* sums,
                        double w_sc, double w_mag, void* stream);
int mfpa_frames_adjoint(const float* dframes, int B, int frames, long long ldf, int win, int hop, int off, int L, float* dxp,
                        void* stream);
int mfpa_reflect_pad_adjoint(const float* dxp, int B, int T, int pad, int L, int accumulate, float* dx, void* stream);

/* ---------------------------------------------------------------------------------------
 * AugmentFP signal chain (next-tier row SURVEY.md §8f-3), augmentation/__init__.py:46-93 and
 * augmentation/transformations/ (every transform).  Waveforms are (B, T) float32; `apply` (B) uint8 is the transform's Bernoulli
 * gate (0 = copy the example through).  The random draws are made by the host like the reference does.
 */
/* Windowed-sinc low-pass taps, julius 0.2.7 design (zeros 8; pass_filters.py:100 -- julius is NOT in the reference
 * tree: parity unpinned): example b owns the 2*half[b]+1 taps at taps + tap_off[b] (ragged: a 0.5 Hz cut-off at 8 kHz
 * has 128 001 taps, a 3.5 kHz one 19), cutoff = f_c / sample_rate. */
int mfpa_lowpass_taps(const float* cutoff, const int* half, const long long* tap_off, int B, float* taps, void* stream);
/* y[t] = sum_{k < ntaps[b]} taps[tap_off[b] + k] * xpad[t + k - off[b]],  pad_mode 0 replicate / 1 zero;
 * out_mode 0: y (LowPassFilter);  1: x - y (HighPassFilter, pass_filters.py:158-171);
 * out_mode 2: impulse response (impulse_response.py:73-117): taps = time-reversed IR, off = n-1, stores t < T and
 *             writes peak[b] = max |y[t]| over ALL t < Tout = T + n_max - 1 (the reference normalises by the peak of the
 *             full convolution before truncating). */
int mfpa_fir(const float* x, int B, int T, int Tout, const float* taps, const long long* tap_off, const int* ntaps,
             const int* off, const uint8_t* apply, int pad_mode, int out_mode, float* y, float* peak, void* stream);
/* y[b] = x[b] * factor[b] (invert 0: Gain, gain.py:62-70) or x[b] / factor[b] (invert 1) where apply[b] (NULL = all). */
int mfpa_scale_rows(const float* x, int B, int T, const float* factor, const uint8_t* apply, int invert, float* y,
                    void* stream);
/* AddBackgroundNoise.random_background (background_noise.py:64-141, non-mixup branch): out[b] (T samples) = the
 * concatenation of up to P slices bank[src[b*P+p] .. + len[b*P+p]) (len 0 ends the list; the lengths of one example sum
 * to T) of a device-resident noise bank, every slice RMS-normalised (x / (rms + 1e-8), utils.py:190-205) and the whole
 * RMS-normalised again.  The host draws scene / file / offset like the reference (python `random`).
 * A list whose lengths sum to more than T is NOT detected: its last slice is written past the example's T samples.  `out`
 * must hold B * T floats. */
int mfpa_gather_background(const float* bank, const long long* src, const int* len, int B, int P, int T, float* out,
                           void* stream);
/* AddBackgroundNoise (background_noise.py:183-215): y = x + rms(x)/10^(snr/20) * noise, then y /= max|y|.
 * With noise == NULL: PeakNormalization (peak_normalization.py:38-67): y = x / max|x| when the peak is > 0. */
int mfpa_mix_background(const float* x, int B, int T, const float* noise, const float* snr_db, const uint8_t* apply,
                        float* y, void* stream);
/* Clipping (clipping.py:67-100) one example at a time, as AugmentFP.__call__ applies it: clamp to torch.quantile(x, p/2)
 * and torch.quantile(x, 1 - p/2) (linear interpolation), found by an in-LDS radix select. */
int mfpa_clip_quantile(const float* x, int B, int T, const float* pct, const uint8_t* apply, float* y, void* stream);
/* The same transform as the reference's batch_augment applies it to B > 1 examples (clipping.py:77-93: torch.quantile without
 * a dim argument): example b is clamped to the pct[b]/2 and 1 - pct[b]/2 quantiles of ALL selected examples flattened
 * together.  n_apply = number of non-zero entries of apply; n_apply * T <= 16 000 000 (torch.quantile's limit) else EINVAL. */
int mfpa_clip_quantile_flat(const float* x, int B, int T, const float* pct, const uint8_t* apply, int n_apply, float* y,
                            void* stream);

/* ---------------------------------------------------------------------------------------
 * Resampling by any rational ratio: torchaudio.transforms.Resample(orig_freq, new_freq) (sinc_interp_hann, lowpass_filter_width 6,
 * rolloff 0.99) as the reference applies it at afp/audfprint/peak_extractor.py:378-388, afp/dejavu/dejavu.py:91-115,
 * testing/generate_queries.py:39, training/background_noise.py:300 and training/generate_audios.py:51.  torchaudio is NOT in the
 * reference tree: the filter is restated from its public source, parity with torchaudio itself is unpinned.
 *   g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * rolloff, width = ceil(lowpass_filter_width * o / base),
 *   ntaps = 2 * width + o taps for each of the n phases, xpad[m] = x[m - width] inside the clip and 0 outside:
 *   y[j * n + i] = sum_{k < ntaps} tap[i][k] * xpad[j * o + k], of which the first Tout = ceil(n * T / o) samples are kept.
 * Limits (MFPA_EINVAL beyond them): n <= MFPA_RESAMPLE_MAX_PHASES, ntaps <= MFPA_RESAMPLE_MAX_TAPS, T <= MFPA_RESAMPLE_MAX_SAMPLES
 * per clip, B <= 65535, at most MFPA_RESAMPLE_MAX_TILES workgroups per clip.
 */
#define MFPA_RESAMPLE_MAX_PHASES 1024
#define MFPA_RESAMPLE_MAX_TAPS 8192
#define MFPA_RESAMPLE_MAX_SAMPLES (1LL << 40)
#define MFPA_RESAMPLE_MAX_TILES (1LL << 23)
#define MFPA_RESAMPLE_MAX_WINDOW 36864    /* input floats a workgroup stages in LDS, at most */
#define MFPA_RESAMPLE_TAP_ALIGN 16       /* floats: the taps of a phase start at a multiple of this (a 64-byte line) */
#define MFPA_RESAMPLE_TAP_PITCH(ntaps) (((ntaps) + MFPA_RESAMPLE_TAP_ALIGN - 1) / MFPA_RESAMPLE_TAP_ALIGN * MFPA_RESAMPLE_TAP_ALIGN)
/* HOST function, integer and double arithmetic only: the geometry above for T input samples per clip; every output pointer may
 * be NULL.  MFPA_EINVAL: a rate, lowpass_filter_width or rolloff that is not positive, rolloff > 1, T < 0, or beyond the limits. */
int mfpa_resample_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, long long T, int* o, int* n,
                           int* width, int* ntaps, long long* Tout);
/* HOST function: frames j one workgroup of mfpa_resample owns for this geometry (tile * n output samples), > 0, or MFPA_EINVAL:
 * 64 per wave of frames (the 4 or 16 waves of a workgroup split the phases first, then the frames), up to eight such rounds while
 * one batch of staging loads brings the window, and never more than the window limit admits. */
int mfpa_resample_tile(int o, int n, int width);
/* HOST function, float64 math rounded once to float32 (like mfpa_stft_tables): the n * ntaps taps, PHASE-MAJOR with a row pitch of
 * MFPA_RESAMPLE_TAP_PITCH(ntaps) floats: taps[i * pitch + k] is tap k of phase i, the floats between ntaps and the pitch are
 * written as 0 and never read (a wave of the kernel works on a few phases and reads their taps with scalar loads of eight, which
 * want the taps of one phase contiguous and no load across two 64-byte lines).  `taps` holds n * pitch floats.  For phase i, tap k:
 *   t = ((double)((float)(-i) / (float)n) + (double)(k - width) / o) * base, clamped to +-lowpass_filter_width;
 *   tap = sinc(pi t) * cos(t pi / lowpass_filter_width / 2)^2 * (base / o). */
int mfpa_resample_taps(int o, int n, int width, int lowpass_filter_width, double rolloff, float* taps);
/* x (B, T) float32 with row pitch ldx >= T -> y (B, Tout) float32 with row pitch ldy >= Tout, one launch for the batch;
 * taps: device copy of mfpa_resample_taps(o, n, width, ...), n * MFPA_RESAMPLE_TAP_PITCH(ntaps) floats (64-byte aligned for
 * speed; any float alignment is correct).  Every output sample is one fused multiply-add chain over
 * k = 0 .. ntaps-1: its value depends on its clip's T samples and (o, n, width, taps) only -- not on B, the pitches, the
 * workgroup it falls in or the memory behind the clip.  B == 0 or Tout == 0: MFPA_OK, no launch.  MFPA_EINVAL before any launch
 * for null pointers, ldx < T, ldy < Tout, Tout > n * (T / o + 1) and beyond the limits above. */
int mfpa_resample(const float* x, int B, long long T, long long ldx, int o, int n, int width, const float* taps, float* y,
                  long long Tout, long long ldy, void* stream);

/* Sparse-tap form of the same resampler, for the pairs of rates whose dense bank is out of reach (8979 : 8000, two semitones at
 * 8 kHz, would be 8993 taps for each of 8000 phases).  Additive to ABI 47; the mfpa_resample* functions above keep their limits,
 * their results and their routing.
 *
 * The window argument t of a tap is clamped to +-lowpass_filter_width, and at the clamp cos^2(pi / 2) * sinc * scale is about
 * 1e-49 in float64, which rounds to 0.0f: only the taps of the run |t| < lowpass_filter_width, at most 2 * width + 1 consecutive
 * k per phase, are not zero.  The sparse bank keeps support = S = 2 * width + 1 rounded up to a multiple of 4 taps per phase (a
 * row is a multiple of 16 bytes) from k = first[i] on:
 *   y[j * n + i] = chain over u = 0 .. S-1 of acc = fmaf(taps[i * S + u], xpad[j * o + first[i] + u], acc), from acc = 0.f
 * -- ONE ascending chain, the dense chain without its zero taps.  Hence, where mfpa_resample takes the pair, both give the same
 * float32 value for finite input, with two differences: the SIGN of a zero result may differ (the dense chain adds products with
 * zero taps, which can turn -0 into +0), and a NaN or Inf input sample spreads over every output whose DENSE window holds it but
 * here only over the outputs whose support holds it.
 * Limits (MFPA_EINVAL beyond them, nothing written): n <= MFPA_RESAMPLE_SPARSE_MAX_PHASES (every pair of rates below 65 536 Hz),
 * o <= MFPA_RESAMPLE_SPARSE_MAX_ORIG, 2 * width + 1 <= MFPA_RESAMPLE_SPARSE_MAX_SUPPORT (width <= 255: a decimation of about
 * 42 : 1), T <= MFPA_RESAMPLE_MAX_SAMPLES, B <= 65535, at most MFPA_RESAMPLE_MAX_TILES workgroups per clip. */
#define MFPA_RESAMPLE_SPARSE_MAX_PHASES 65536
#define MFPA_RESAMPLE_SPARSE_MAX_ORIG (1 << 20)
#define MFPA_RESAMPLE_SPARSE_MAX_SUPPORT 512
/* HOST function: o, n, width and Tout as mfpa_resample_geometry gives them, support = S; every output pointer may be NULL. */
int mfpa_resample_sparse_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, long long T, int* o, int* n,
                                  int* width, int* support, long long* Tout);
/* HOST function: consecutive OUTPUT samples one workgroup of mfpa_resample_sparse owns, > 0, or MFPA_EINVAL: a multiple of 64,
 * 1024 unless the input span of that many outputs (about tile * o / n + S floats, staged in LDS) would pass 16384 floats.
 * MFPA_EINVAL also for a width so small for o / n that 64 outputs span more than MFPA_RESAMPLE_MAX_WINDOW floats (never the width
 * of mfpa_resample_sparse_geometry); mfpa_resample_sparse refuses the same. */
int mfpa_resample_sparse_tile(int o, int n, int width);
/* HOST function: taps (n * S floats), first (n ints).  Row i holds taps k = first[i] .. first[i] + S - 1 of row i of the dense
 * bank, each bit for bit what mfpa_resample_taps writes for (i, k) -- one expression in the source serves both --; positions
 * with k >= ntaps hold 0.0f (first[i] >= 0).  The builder PROVES that what it leaves out is zero: outside the run
 * |t| < lowpass_filter_width the clamped argument is exactly -lowpass_filter_width or +lowpass_filter_width, so a dropped tap has
 * one of two values; both are evaluated and must be 0.0f, the run of every phase (found with the float64 t itself) must fit in S
 * taps, and first[i] - floor(i * o / n) must lie in [0, 3] (the kernel sizes its LDS window by that; it is 1 or 2 in practice) --
 * else MFPA_EINVAL with nothing written.  n * S tap evaluations, never n * ntaps. */
int mfpa_resample_sparse_taps(int o, int n, int width, int lowpass_filter_width, double rolloff, float* taps, int32_t* first);
/* x (B, T) float32 with row pitch ldx >= T -> y (B, Tout) float32 with row pitch ldy >= Tout, one launch for the batch.
 * taps, first: device copies of mfpa_resample_sparse_taps(o, n, width, ...), taps 16-byte aligned; support = S of the geometry.
 * Every output sample is the one chain above: its value depends on its clip's T samples and the table only -- not on B, the
 * pitches, the workgroup it falls in or the memory behind the clip.  B == 0 or Tout == 0: MFPA_OK, no launch.  MFPA_EINVAL before
 * any launch for null pointers, a misaligned taps, support != S, ldx < T, ldy < Tout, Tout > n * (T / o + 1) and beyond the
 * limits above. */
int mfpa_resample_sparse(const float* x, int B, long long T, long long ldx, int o, int n, int width, int support, const float* taps,
                         const int32_t* first, float* y, long long Tout, long long ldy, void* stream);

/* ---------------------------------------------------------------------------------------
 * Training segments out of whole tracks: the chunk / drop-silence / draw / normalise stage of the reference's AugmentationDataset
 * (training/dataset.py:55-122) and the crops of testing/generate_queries.py:43-49.  Tracks sit back to back in one device float32
 * buffer `bank`: track i owns bank[off[i] .. off[i] + len[i]) (off, len: int64; any 4-byte alignment of a track is fine).
 * With frame length L and step S (tf.signal.frame, no end padding) track i has nf[i] = 1 + (len[i] - L) / S segments, 0 when
 * len[i] < L; segment j of track i starts at off[i] + j * S and has the GLOBAL index seg_off[i] + j, seg_off being the exclusive
 * prefix of nf (n_tracks + 1 ints, NS = seg_off[n_tracks] segments in all).
 * Limits (MFPA_EINVAL beyond them): 1 <= L, S <= MFPA_SEGMENT_MAX_LENGTH, nf[i] <= MFPA_SEGMENT_MAX_PER_TRACK (the sort keys of a
 * track live in LDS), NS <= INT_MAX, n_tracks * n_keep <= INT_MAX, rows <= INT_MAX.
 */
#define MFPA_SEGMENT_MAX_PER_TRACK 8192
#define MFPA_SEGMENT_MAX_LENGTH (1LL << 27)
/* HOST function, integers only: seg_off[0 .. n_tracks] from the HOST array len.  MFPA_EINVAL: a null pointer (len may be NULL when
 * n_tracks == 0), n_tracks < 0, a negative length, or beyond the limits above. */
int mfpa_segment_geometry(const long long* len, int n_tracks, long long L, long long S, int* seg_off);
/* off, len, seg_off: DEVICE copies.  seg_sumsq[NS] (double): sum of x^2 over each segment; trk_sumsq[n_tracks] (double): over each
 * whole track, the tail no segment covers included; trk_peak[n_tracks] (float): max|x| of each whole track (exact).  Every square
 * is taken in float64 (exact for a float32 sample) and added with one rounding, in an order fixed by the sample's position in its
 * segment (or in the tail) alone: no floating-point atomics, and each output is bit for bit the same whatever other tracks are in
 * the call and wherever the track lies in `bank`.  S == L: the audio is read once, a track's sum is its segments' sums plus its
 * tail's in a fixed order; otherwise the track is read a second time for its own sum.  Empty tracks give 0 / 0 / 0.
 * n_tracks == 0: MFPA_OK, no launch.  MFPA_EINVAL before any launch for null pointers and beyond the limits. */
int mfpa_segment_stats(const float* bank, const long long* off, const long long* len, const int* seg_off, int n_tracks, long long L,
                       long long S, double* seg_sumsq, double* trk_sumsq, float* trk_peak, void* stream);
/* One workgroup per track.  Segment j of track i is KEPT iff, in float64,
 *   seg_sumsq[j] * (double)len[i] > (thr * trk_sumsq[i]) * (double)L        (thr = exp(dbs_threshold / 5), thr >= 0)
 * which is the reference's 10 * ln(rms_seg / rms_track) > dbs_threshold (dataset.py:86-99) without the square roots and the
 * logarithm; an all-zero track keeps nothing.  kept[i] = segments kept, before the cut to n_keep; mask[NS] (uint8, may be NULL) =
 * the keep flags.  The winners are the kept segments in ascending (keys[j], j) order, keys being NS uint32 the host drew before it
 * knew the mask: shuffle(kept)[:n_keep] (dataset.py:104-122) with no host round trip.  Row r = i * n_keep + k, k < n_keep:
 *   sel[r] = global index of the k-th winner, src[r] = its first sample in `bank` (int64), both -1 when kept[i] <= k;
 *   div[r] = trk_peak[i] when do_norm and the peak is > 0, else 1 (dataset.py:55-60).
 * n_tracks == 0: MFPA_OK, no launch.  MFPA_EINVAL before any launch for null pointers (mask excepted), n_keep < 1, thr < 0 or NaN
 * and beyond the limits. */
int mfpa_segment_select(const double* seg_sumsq, const double* trk_sumsq, const float* trk_peak, const long long* off, const long long* len,
                        const int* seg_off, int n_tracks, long long L, long long S, const unsigned int* keys, double thr, int n_keep,
                        int do_norm, int* sel, long long* src, float* div, int* kept, unsigned char* mask, void* stream);
/* out[r * ldo + t] = bank[src[r] + t] / div[r] for t < L, an IEEE float32 division (a plain copy when div == NULL); rows with
 * src[r] < 0 are left untouched, and so are the floats between L and ldo.  src[r] may have any alignment; the caller guarantees
 * that src[r] + L stays inside `bank`.  rows == 0: MFPA_OK, no launch.  MFPA_EINVAL before any launch for null pointers (div
 * excepted), ldo < L and beyond the limits. */
int mfpa_segment_gather(const float* bank, const long long* src, const float* div, long long rows, long long L, float* out, long long ldo,
                        void* stream);

/* ---------------------------------------------------------------------------------------
 * Composable waveform transforms (augmentation/transformations/band_filters.py, colored_noise.py): what the AugmentFP kernels
 * above do not already cover.  Gain, Clipping, PeakNormalization, ApplyImpulseResponse, AddBackgroundNoise and the pass filters
 * are the entry points of the AugmentFP section; AddColoredNoise mixes with mfpa_mix_background.
 */
/* Band-pass taps, julius 0.2.7 BandPassFilter restated (julius is NOT in the reference tree: parity unpinned, like
 * mfpa_lowpass_taps): two windowed-sinc low-passes at cut_lo[b] < cut_hi[b] (fractions of the sample rate, 0 < c <= 0.5) on ONE
 * window of 2*half[b]+1 points, half = int(8 / cut_lo / 2), each normalised to its own unit sum in the arithmetic of
 * mfpa_lowpass_taps (but the sine is taken of the phase c * (k - half) reduced to half a turn, exactly, which a window of tens of
 * thousands of points needs to keep the taps within 2e-7 of their float64 values); taps[tap_off[b] + k] = hi[k] - lo[k].  One pass of mfpa_fir (pad_mode 0, off = half) is then the band-pass
 * (out_mode 0) or the band-stop x - bandpass (out_mode 1).  B == 0: MFPA_OK, no launch. */
int mfpa_bandpass_taps(const float* cut_lo, const float* cut_hi, const int* half, const long long* tap_off, int B, float* taps,
                       void* stream);
/* The real FFT of the library: N real samples as N/2 complex points in one LDS buffer of a workgroup, Stockham passes of
 * radix 5, 3, 4 and 2.  The buffer is 64 KiB -- 8 bytes per complex point -- so N/2 <= 8192: MFPA_RFFT_MAX_N.  (The kernel's whole
 * LDS need is that buffer plus 64 bytes of reduction scratch.) */
#define MFPA_RFFT_MAX_N 16384
#define MFPA_RFFT_MAX_RADICES 16
/* HOST function, integers only: which N the device FFT takes and how.  MFPA_OK when N is even, 4 <= N <= MFPA_RFFT_MAX_N and
 * N/2 = 2^a 3^b 5^c: radices[0 .. *n_radices) are the passes in order (their product is N/2; `radices` holds
 * MFPA_RFFT_MAX_RADICES ints, the rest are written as 0), *lds_bytes the LDS bytes of the workgroup.  Every output pointer may
 * be NULL.  MFPA_EINVAL for every other N -- an odd N on purpose: torch's irfft of an rfft of N odd samples returns N-1. */
int mfpa_rfft_plan(int N, int* radices, int* n_radices, int* lds_bytes);
/* HOST function, float64 math rounded once to float32 (like mfpa_stft_tables): out[2q], out[2q+1] = cos, -sin of 2 pi q / N for
 * q < N (2N floats).  MFPA_EINVAL: a null pointer or an N mfpa_rfft_plan refuses. */
int mfpa_rfft_twiddles(int N, float* out);
/* AddColoredNoise._gen_noise (colored_noise.py:12-38) for B examples, one workgroup each:
 *   white (B, N) float32 -> rfft -> * 1 / linspace(1, sqrt(N/2), N/2+1)^f_decay[b] (float32, torch.linspace's two-sided form)
 *   -> irfft (scaled by 1/N) -> x / (sqrt(mean(x^2)) + 1e-8) -> out[b, t] = x[t mod N], t < T    (out (B, T) float32, T >= 1).
 * twiddles: device copy of mfpa_rfft_twiddles(N), 8-byte aligned.  Every value of `out` depends on its example's N samples,
 * f_decay[b] and N only: fixed summation orders, no atomics -- bit for bit independent of B, of the row and of T.
 * MFPA_EINVAL before any launch: a null pointer, B < 0, T < 1, an N mfpa_rfft_plan refuses.  B == 0: MFPA_OK, no launch. */
int mfpa_colored_noise(const float* white, int B, int N, const float* f_decay, int T, const float* twiddles, float* out,
                       void* stream);

/* ---------------------------------------------------------------------------------------
 * Complex STFT and its inverse (csrc/stft.hip, csrc/istft.hip): the library's fixed geometry (n_fft 512, hop 256, one-sided 257
 * bins, centre / reflect framing), float64 arithmetic, the window of `tables` (mfpa_stft_tables).  Additive to ABI 47.
 *
 * mfpa_stft_complex: torch.stft(x.double(), 512, 256, window=w, return_complex=True).
 *   wav      (B, T_w) float32, T_w > 256 (the rules of mfpa_stft_mag; B == 0: MFPA_OK, no launch)
 *   spec     (B, 257, n_frames) complex128 as interleaved (re, im) doubles, 16-byte aligned
 *   mag      may be NULL; otherwise (B, 257, n_frames) of mag_dtype, bit for bit what mfpa_stft_mag writes for the same input
 *   clip_max may be NULL; otherwise (B) float64, bit for bit mfpa_stft_mag's */
int mfpa_stft_complex(const float* wav, int B, int T_w, const double* tables, double* spec, void* mag, int mag_dtype,
                      double* clip_max, void* stream);
/* mfpa_istft: torch.istft(Z, 512, 256, window=w, center=True, length=length) -- per frame the inverse real FFT (the imaginary parts
 * of bins 0 and 256 are ignored, as torch's c2r transform ignores them) times the window, overlap-added, divided by the
 * overlap-added squared window, first 256 samples dropped.
 *   spec   (B, 257, n_frames) complex128 as interleaved doubles, 16-byte aligned
 *   mag    NULL: Z = spec.  Otherwise (B, 257, n_frames) of mag_dtype and Z = m * spec / |spec| with m = mag * denom[b]
 *          (denom (B) float64, may be NULL: m = mag); where |spec| == 0, Z = m (phase 0).  With MFPA_ISTFT_CLAMP in `flags` a
 *          negative m becomes 0; without it a negative m flips the sign.  Z is formed as the spectrum is read and never stored.
 *   out    (B, length) of out_dtype; the float32 output is the float64 value rounded once
 * Every output sample is the sum of at most two frames, added in frame order, by one thread: no atomics, and a row of `out` is
 * bit for bit independent of B, of the row's position and of the memory around its operands.
 * MFPA_EINVAL before any launch: a null spec / tables / out, n_frames < 2, length outside
 * [256 (n_frames - 1), 256 n_frames) -- the lengths an STFT with that many frames can have come from --, an unknown dtype or flag
 * bit, a spec that is not 16-byte aligned, B < 0 or B > 65535.  B == 0: MFPA_OK, no launch. */
#define MFPA_ISTFT_CLAMP 1
int mfpa_istft(const double* spec, const void* mag, int mag_dtype, const double* denom, int flags, int B, int n_frames, int length,
               const double* tables, void* out, int out_dtype, void* stream);
/* HOST function, no GPU work: *out_min = the minimum over the kept samples [256, 256 + length) of the overlap-added squared
 * window, float64, summed in frame order like mfpa_istft's divisor (torch.istft refuses a minimum below 1e-11: "window overlap
 * add min").  MFPA_EINVAL: a null pointer, or n_frames / length outside mfpa_istft's rules. */
int mfpa_istft_envelope_min(const double* window512, int n_frames, int length, double* out_min);

/* ---------------------------------------------------------------------------------------
 * Phase vocoder (csrc/vocoder.hip): torchaudio.functional.phase_vocoder at the library's fixed geometry (257 bins, hop 256) with
 * one rate PER CLIP, float64 throughout.  The arithmetic is restated from torchaudio's public source (torchaudio is not in the
 * reference tree: parity with it is unpinned, as for mfpa_resample).  Additive to ABI 47.
 *
 * Clip b, rate r = rates[b], n_out = ceil(n_frames / r) in double (the length of torch.arange(0, n_frames, r)); output frame
 * i < n_out of bin k:
 *   t = i * r, j = floor(t), alpha = t - j;  Z0 = spec[b, k, j], Z1 = spec[b, k, j + 1] (0 past the last frame)
 *   d = angle(Z1) - angle(Z0) - adv_k, adv_k = pi k (torch.linspace(0, pi * 256, 257)[k]);  d -=2 pi round(d / 2 pi);  inc_i = d + adv_k
 *   phi_i = angle(spec[b, k, 0]) + sum_{m < i} inc_m
 *   out[b, k, i] = (alpha |Z1| + (1 - alpha) |Z0|) * (cos phi_i, sin phi_i)
 * Frames n_out <= i < ld_out are written as zeros.  A clip whose rate is exactly 1.0 is copied through (torchaudio's rule).
 *   spec   (B, 257, n_frames) complex128 as interleaved doubles, 16-byte aligned
 *   rates  (B) float64 on the device
 *   out    (B, 257, ld_out) complex128, 16-byte aligned
 *   n_out  (B) int32 on the device: the clip's frame count, or -1 for a rate the kernel refuses -- not finite, not positive, or
 *          with n_out > ld_out; such a clip's output is all zeros.  The rates live on the device, so the host cannot check them.
 * One wavefront owns one row (b, k) and scans it in 64-frame chunks with a carry: a fixed summation order, no atomics; a row's
 * bits do not depend on B, on the row's position or on its neighbours.
 * MFPA_EINVAL before any launch: B < 0 or B > 65535, n_frames < 1, ld_out < 1, n_frames or ld_out > MFPA_VOCODER_MAX_FRAMES, and
 * with B > 0 a null or misaligned pointer.  B == 0: MFPA_OK, no launch. */
#define MFPA_VOCODER_MAX_FRAMES 16384
int mfpa_phase_vocoder(const double* spec, int B, int n_frames, const double* rates, double* out, int ld_out, int* n_out,
                       void* stream);
/* HOST function, no GPU work: *n_out = ceil(n_frames / rate) by the double arithmetic of the kernel.  MFPA_EINVAL: a null pointer,
 * n_frames < 1 or > MFPA_VOCODER_MAX_FRAMES, a rate that is not finite or not positive, a result above MFPA_VOCODER_MAX_FRAMES. */
int mfpa_vocoder_frames(int n_frames, double rate, int* n_out);

/* ---------------------------------------------------------------------------------------
 * Recursive filters (csrc/iir.hip): scipy.signal.sosfilt -- a cascade of S second-order sections in transposed direct form II, one
 * filter for the batch or one per row.  Additive to ABI 47.
 *
 * Section s has the coefficients b0 b1 b2 a0 a1 a2 with a0 == 1 (the caller normalises; a0 is not read) and the state (z1, z2);
 * sample by sample, the output of section s being the input of section s + 1:
 *   y = b0 x + z1;   z1 = (b1 x - a1 y) + z2;   z2 = b2 x - a2 y
 * State and arithmetic are float64, every product and sum rounded on its own (no fused multiply-add), in this order.  The samples
 * are float32 (x_f64 = 0) or float64 (x_f64 = 1); the float32 output is the float64 result rounded once.
 *   x, y    (B, T) on the device, element aligned (4 or 8 bytes), not overlapping
 *   sos     (S, 6) with sos_per_row = 0, (B, S, 6) with sos_per_row = 1, float64 on the device.  The values are NOT checked (they
 *           live on the device): an unstable or non-finite section gives what float64 gives
 *   apply   NULL, or B bytes on the device: row b with apply[b] == 0 is copied through bit for bit, and its final state is its
 *           initial state
 *   zi, zf  NULL, or (B, S, 2) float64 on the device: scipy's initial state (zeros without zi) and the state after sample T - 1
 *   clamp   1: the output is clamped to [-1, 1] before it is stored (torchaudio.functional.lfilter's default); a NaN stays a NaN
 *   work    work_len >= mfpa_sosfilt_work(B, S, sos_per_row) float64 on the device: per filter and section 64 2x2 matrices, the
 *           powers A^(16 j), j = 1..64, of the section's state matrix A = [[-a1, 1], [-a2, 0]], written by a setup launch that runs
 *           the section's own homogeneous recurrence from the unit states (NOT by squaring A: DESIGN.md section 3.15)
 * One wavefront owns one row and walks it in chunks of 64 lanes x 16 samples: every lane filters its 16 samples from zero state,
 * a shuffle scan over the lanes' end states (with those powers) plus the carry of the chunks before gives each lane its true
 * start state, and the lane filters its samples again from there.  No atomics; a row's bits do not depend on B, on the row's
 * position or on its neighbours.  -0.0 follows the formula: the identity section turns a -0.0 sample into +0.0, like scipy.
 * MFPA_EINVAL before any launch, no pointer dereferenced on the host: B < 0 or B > 65535, T < 1 or T > 2^30, S < 1 or
 * S > MFPA_SOS_MAX_SECTIONS, x_f64 / sos_per_row / clamp other than 0 or 1, work_len too short, and with B > 0 a null x, y, sos or
 * work or a misaligned pointer.  B == 0: MFPA_OK, no launch. */
#define MFPA_SOS_MAX_SECTIONS 8
int mfpa_sosfilt(const void* x, int x_f64, int B, long long T, const double* sos, int S, int sos_per_row, const unsigned char* apply,
                 const double* zi, double* zf, int clamp, double* work, long long work_len, void* y, void* stream);
/* HOST function, no GPU work: *work_len = F * S * 256 doubles, F = B filters with sos_per_row = 1, else 1 (0 for B == 0).
 * MFPA_EINVAL: a null pointer, or B, S or sos_per_row outside mfpa_sosfilt's rules. */
int mfpa_sosfilt_work(int B, int S, int sos_per_row, long long* work_len);

/* ---------------------------------------------------------------------------------------
 * Room impulse responses (csrc/rir.hip): the image-source method for a shoebox room (Allen and Berkley), one room, source and
 * microphone per row.  Additive to ABI 47.  Everything is float64.
 *
 * geom (B, 15) on the device: room Lx Ly Lz in metres, source, microphone, and the six energy absorption coefficients of the walls
 * x0 x1 y0 y1 z0 z1.  The values are NOT checked (they live on the device; the Python layer checks them before the upload).
 * Per axis and signed reflection index i in [-N, N], N = max_order:  p = i mod 2 (1 for odd i),  n = (i + p) / 2,  the image
 * coordinate is s + i L for even i and -s + (i + 1) L for odd i,  X[i] = (image - mic)^2,  G[i] = beta0^|n - p| beta1^|n| with
 * beta = sqrt(1 - alpha) of the axis's two walls.  Per image (ix, iy, iz) with |ix| + |iy| + |iz| <= N:
 *   d = sqrt((X[ix] + Y[iy]) + Z[iz]),   amp = Gx Gy Gz / (4 pi d),   tau = (d fs) / c   (no fused multiply-add)
 *   h[k] += amp w(k - tau) sinc(k - tau)  for 0 <= k < length,  w(x) = 0.5 (1 + cos(pi x / half)) for |x| <= half and 0 outside,
 *   half = (filter_len - 1) / 2,  sinc(0) = 1
 * Taps before sample 0 or from `length` on are dropped; an image at distance 0 or with gain 0 contributes nothing (no inf, no NaN
 * from valid geometry).  out (B, ldo): row b holds h in its first `length` elements, float64 (out_f64 = 1) or float32, the float64
 * value rounded once; reversed = 1 stores h[length - 1 - k] at k, which is what mfpa_fir takes as the taps of an impulse response.
 * One workgroup owns 64 consecutive samples of one room; each of its four wavefronts adds the taps of every fourth image row ix in
 * index order and the four partial sums are added in a fixed order: no atomics, the same bits from run to run, and a row's bits do
 * not depend on B or on the row's position.
 * MFPA_EINVAL before any launch, no pointer dereferenced on the host: B < 0 or B > 65535, max_order outside [0, 128], length outside
 * [1, 262144], ldo < length, filter_len even or outside [3, 255], fs or c not finite or not positive, reversed / out_f64 other than
 * 0 or 1, and with B > 0 a null or misaligned geom or out.  B == 0: MFPA_OK, no launch. */
int mfpa_rir_shoebox(const double* geom, int B, int max_order, int length, double fs, double c, int filter_len, int reversed, int out_f64,
                     void* out, long long ldo, void* stream);
/* HOST function, no GPU work: *out = (2N + 1)(2N^2 + 2N + 3) / 3, the images with |ix| + |iy| + |iz| <= N = max_order.
 * MFPA_EINVAL: a null pointer, max_order outside [0, 128]. */
int mfpa_rir_image_count(int max_order, long long* out);

/* ---------------------------------------------------------------------------------------
 * Dynamic range compression (csrc/dynamics.hip): a feed-forward, log-domain compressor with the smooth decoupled peak detector of
 * Giannoulis, Massberg and Reiss ("Digital Dynamic Range Compressor Design", JAES 2012), along the rows of (B, T) samples, one
 * parameter set for the batch or one per row.  Additive to ABI 47.
 *
 * A parameter set is six float64 values: threshold_db (Th), slope s = 1 - 1/ratio in [0, 1] (a limiter has s = 1), knee_db W >= 0,
 * attack_coef aA in [0, 1), release_coef aR in [0, 1), makeup_db M; a coefficient is exp(-1 / (seconds sample_rate)), formed by the
 * caller, 0 for a time of 0.  A row has the state (y1, yL): (0, 0) or zi at the start, returned after sample T - 1 as zf.  Per
 * sample, state and arithmetic float64, every product and sum rounded on its own (no fused multiply-add), in this order:
 *   xg = 20 log10(max(|x|, 1e-10))
 *   o  = xg - Th
 *   xl = 0                        if 2 o <= -W
 *        s (o + W/2)^2 / (2 W)    if 2 |o| < W
 *        s o                      otherwise            (the gain reduction wanted, dB)
 *   y1 = max(xl, aR y1 + (1 - aR) xl)                  (instant attack, smooth release)
 *   yL = aA yL + (1 - aA) y1                           (attack smoothing)
 *   y  = x 10^((M - yL) / 20)
 * level_in = 0 is this formula; gr, when given, receives yL.  level_in = 1 takes x as xl itself, skips the first and the last
 * line and stores yL in y (the envelope follower; no transcendental function); gr must be NULL.  The samples and both outputs are
 * float32 (x_f64 = 0) or float64 (x_f64 = 1); a float32 output is the float64 value rounded once.
 *   x, y, gr  (B, T) on the device, element aligned (4 or 8 bytes), not overlapping; gr may be NULL
 *   params    (6,) with params_per_row = 0, (B, 6) with params_per_row = 1, float64 on the device.  The values are NOT checked (they
 *             live on the device; the Python layer checks them before the upload)
 *   apply     NULL, or B bytes on the device: row b with apply[b] == 0 is copied through bit for bit, its gr is 0 and its final
 *             state is its initial state
 *   zi, zf    NULL, or (B, 2) float64 on the device: (y1, yL)
 * One workgroup of 8 wavefronts owns one row; a wavefront owns a contiguous part of it in whole super-chunks of 64 lanes x 16
 * samples.  Both recurrences are scans over closed families of maps (y -> max(c, a y + b), and affine): a lane composes the maps of
 * its 16 samples, a shuffle scan composes the lanes' maps, the map of everything before a lane is applied once to the carry, and
 * the lane reruns its samples with the recurrence itself.  The row is walked three times with the parts' carries passed through
 * LDS in wavefront order (csrc/dynamics.hip).  No atomics, no work buffer, no workgroup waits for another; a row's bits do not
 * depend on B, on the row's position or on the run.
 * MFPA_EINVAL before any launch, no pointer dereferenced on the host: B < 0 or B > 65535, T < 1 or T > 2^30, x_f64 /
 * params_per_row / level_in other than 0 or 1, gr given with level_in = 1, and with B > 0 a null x, y or params or a misaligned
 * pointer.  B == 0: MFPA_OK, no launch. */
int mfpa_dynamics(const void* x, int x_f64, int B, long long T, const double* params, int params_per_row, const unsigned char* apply,
                  const double* zi, double* zf, int level_in, void* y, void* gr, void* stream);

/* ---------------------------------------------------------------------------------------
 * Delay lines (csrc/delay.hip): a time-varying fractional delay without feedback (echo, vibrato, chorus, a feed-forward flanger,
 * wow and flutter, Doppler ramps) and a comb with an integer delay and feedback (the regenerating echo, the feed-forward comb, the
 * Schroeder all-pass), along the rows of (B, T) samples.  Additive to ABI 47.
 *
 * mfpa_varidelay.  A row x[0..T) has V voices (1 <= V <= MFPA_DELAY_MAX_VOICES), voice v a gain g[v] and delays d[v][n] in samples
 * (float64, negative = reading ahead), a dry gain g0, and an odd filter_len = 2 half + 1 in [3, 255].  Per output sample n, float64,
 * every product and sum rounded on its own (no fused multiply-add), in this order:
 *   acc = g0 * x[n]
 *   for v in 0 .. V-1 (ascending):
 *     p = (double)n - d[v][n]                                  (one rounding)
 *     s = 0
 *     if p > -(half + 1) and p < T + half:                     (false for a NaN; decided on the double, before any integer is formed)
 *       whole = floor(p);  frac = p - whole                    (frac in [0, 1]; 1 only by rounding, for a tiny negative p)
 *       sf = sinpi(frac);  cw = cospi(frac / half);  sw = sinpi(frac / half)
 *       for j = -half .. half + 1 (ascending):                 (tap x[whole + j], 0 outside [0, T))
 *         t = (double)j - frac
 *         if |t| <= half:
 *           w    = 0.5 * (1 + (cospi(j / half) * cw + sinpi(j / half) * sw))      (the Hann window 0.5 (1 + cos(pi t / half)))
 *           sinc = 1 if t == 0 else (sf if j is odd else -sf) / (pi * t)          (sin(pi t) / (pi t))
 *           s   += x[whole + j] * (w * sinc)
 *     acc += g[v] * s
 *   y[n] = acc, rounded once when y is float32
 * A delay that is not finite, or a position whose window lies wholly outside the row, fails the comparison: that voice adds g[v] * 0
 * at that sample.  Nothing is re-normalised: the windowed sinc's DC ripple (the taps of a fractional position do not sum to exactly 1) is the
 * algorithm's own.  The interpolator does not band-limit: where the read position advances faster than one sample per sample, content above
 * the new Nyquist frequency aliases (negligible for wow and flutter; a large constant ratio is mfpa_resample's job).
 *   x        (B, ldx) on the device, float32 (x_f64 = 0) or float64, ldx >= T; not overlapping y
 *   delay    float64 on the device; d[b][v][n] sits at delay[b * delay_row_stride + v * delay_voice_stride + n * delay_time_stride],
 *            strides in elements, the row and voice strides >= 0, delay_time_stride 1, or 0: one constant delay per voice
 *   gains    (B, V) float64 on the device;  dry (B,) float64 on the device.  The values are NOT checked (the Python layer does)
 *   apply    NULL, or B bytes on the device: row b with apply[b] == 0 is copied through (bit for bit when y has x's type)
 *   y        (B, T) on the device, float32 (y_f64 = 0) or float64
 * A workgroup of four wavefronts produces MFPA_VARIDELAY_TILE consecutive outputs of one row, one per lane.  Per voice the tile
 * reduces the smallest and largest live read position; if the window [floor(min p) - half, floor(max p) + half + 1] holds at most
 * MFPA_VARIDELAY_WINDOW samples it is staged once in LDS as float64, zeros outside the row, and every tap reads LDS; otherwise the
 * taps read global memory.  Both paths run the same arithmetic in the same order and give the same bits.  No atomics, no work
 * buffer; a row's bits do not depend on B, on the row's position or on the path another tile took.
 * MFPA_EINVAL before any launch, no pointer dereferenced on the host: B < 1 or B > 65535, T < 1 or T > 2^30, ldx < T, V outside
 * [1, MFPA_DELAY_MAX_VOICES], filter_len even or outside [3, 255], a negative row or voice stride, delay_time_stride other than 0
 * or 1, x_f64 / y_f64 other than 0 or 1, a null x, delay, gains, dry or y, a misaligned pointer. */
#define MFPA_DELAY_MAX_VOICES 8
#define MFPA_VARIDELAY_TILE 256
#define MFPA_VARIDELAY_WINDOW 1024
int mfpa_varidelay(const void* x, int x_f64, long long ldx, int B, long long T, const double* delay, long long delay_row_stride,
                   long long delay_voice_stride, int delay_time_stride, int V, const double* gains, const double* dry,
                   const unsigned char* apply, int filter_len, void* y, int y_f64, void* stream);
/* mfpa_comb.  y[n] = b0 x[n] + (bD x[n - D] + aD y[n - D]), terms before the row's start 0; three products and two sums, each
 * rounded on its own, the parentheses as written; float64 state (y[n - D] is the unrounded float64 value also when y is float32).
 * b0 = 1, bD = 0: a regenerating echo;  aD = 0: a feed-forward comb;  b0 = -g, bD = 1, aD = g: Schroeder's all-pass.  There is no
 * state across calls.
 *   x        (B, ldx) on the device, float32 (x_f64 = 0) or float64;  y (B, T), float32 (y_f64 = 0) or float64, not overlapping x
 *   params   (4,) with params_per_row = 0, (B, 4) with 1, float64 on the device: D, b0, bD, aD.  The values are NOT checked (the
 *            Python layer does: D an integer in [1, 2^24], |aD| < 1); on the device D is truncated and clamped to [1, max_delay]
 *   max_delay  the largest D of the call, [1, 2^24]: it sizes the grid
 *   apply    as above
 * The residue classes n mod D are independent first-order recurrences: the grid is (ceil(min(max_delay, T) / 256), B), lane r < D
 * walks n = r, r + D, r + 2D, ... with its previous input and output in registers, loads and stores coalesced over consecutive
 * residues; no synchronisation of any kind, and the same bits as the formula evaluated sample by sample.  A small D uses few lanes.
 * MFPA_EINVAL before any launch: B < 1 or B > 65535, T < 1 or T > 2^30, ldx < T, max_delay outside [1, 2^24], x_f64 / y_f64 /
 * params_per_row other than 0 or 1, a null x, params or y, a misaligned pointer. */
int mfpa_comb(const void* x, int x_f64, long long ldx, int B, long long T, const double* params, int params_per_row, long long max_delay,
              const unsigned char* apply, void* y, int y_f64, void* stream);

/* ---------------------------------------------------------------------------------------
 * Lossy coding (csrc/codec.hip): what a transform codec and a telephone channel do to a signal, along the rows of (B, T) samples.
 * Neither is a bit stream: mfpa_transform_codec simulates transform coding (the rate is the high-resolution estimate
 * 1/2 log2(variance / noise power) per coefficient, not an entropy-coded size), mfpa_mulaw is the G.711-style compander.  Additive
 * to ABI 47.
 *
 * mfpa_transform_codec.  M = 256.  The row x[0..T) stands behind M zeros and before zeros; F = ceil(T / M) + 1 frames, frame f the
 * padded samples [f M, f M + 512).  Float64 throughout, every product and sum of the allocation and the quantiser rounded on its own:
 *   w[n]  = sin(pi (n + 1/2) / 512)
 *   X[k]  = sum_{n < 512} w[n] x_f[n] cos(pi / M (n + 1/2 + M / 2) (k + 1/2)),  k < M          (the MDCT)
 *   bands b < n_bands (<= MFPA_CODEC_MAX_BANDS) are [edges[b], edges[b + 1]), edges ascending from 0 to M, widths W_b
 *   var_b = (sum_{k in b} X[k]^2) / W_b, summed in ascending k
 *   m_b   = max over b' of var_b' * 10^(-a(b, b') / 10),  a = up_db (b - b') for b >= b' (a masker spreads upward), down_db (b' - b)
 *           otherwise; the factor of b' = b is exactly 1, so m_b >= var_b; the factors are made on the host as pow(10, -(db * d) / 10)
 *   L_b   = log2 var_b - log2 m_b   (<= 0);  bands with var_b = 0 are out
 *   with R the row's bit budget per frame, for every band j that is in:
 *     S_j = sum W_b,  P_j = sum W_b L_b  over {b in : L_b >= L_j} in ascending b;   lam_j = (P_j - 2 R) / S_j;   admissible if lam_j < L_j
 *   lam   = lam_j of the admissible j with the smallest L_j (equal L_j: the same set, the same value); none admissible (R <= 0, a
 *           silent frame, R NaN on the device): nothing is coded.  Reverse water-filling in closed form: lam is a continuous
 *           function of the band energies, there is no iteration
 *   band b is coded iff L_b > lam:  D_b = m_b * 2^lam,  step_b = sqrt(12 * D_b),  t = |X[k]| / step_b,  q = floor(t + 1/2),
 *           Xq[k] = sign(X[k]) * q * step_b;  where t is not below 2^52 (the step is finer than a double resolves, or underflowed)
 *           Xq[k] = X[k] and q counts as non-zero iff X[k] != 0.  Other bands: Xq[k] = 0 exactly.  q is never an index
 *   y_f[n] = (2 / M) * (w[n] * sum_k Xq[k] cos(...)),  y[h M + i] = y_h[M + i] + y_{h+1}[i]: the earlier frame first
 * R = +inf skips the allocation and the quantiser (Xq = X): y is x up to rounding (the TDAC identity).
 *   x        (B, ldx) on the device, float32 (x_f64 = 0) or float64, ldx >= T; not overlapping y
 *   rate     R of every row when row_rates is NULL;  row_rates: (B,) float64 on the device, R per row (not checked: the Python layer does)
 *   band_edges  n_bands + 1 ints on the HOST, read before the launch
 *   apply    NULL, or B bytes on the device: row b with apply[b] == 0 is copied through (bit for bit when y has x's type), its
 *            lambda_out NaN and coded_out 0
 *   y        (B, T) on the device, float32 (y_f64 = 0, the float64 value rounded once) or float64
 *   lambda_out  NULL or (B, F) float64 on the device: lam per frame, NaN where nothing is coded, -inf with R = +inf
 *   coded_out   NULL or (B, F) int32 on the device: the number of non-zero q of the frame, 0 with R = +inf
 * A workgroup of four wavefronts owns MFPA_CODEC_FRAMES consecutive blocks of M outputs of one row and transforms the
 * MFPA_CODEC_FRAMES + 1 frames that cover them, eight lanes per frame: the fold to 256 reals, a DCT-IV through a 128-point complex
 * transform (the butterflies of csrc/mfpa_fft16.h), the allocation in the frame's lanes, the same DCT-IV back, and the overlap-add
 * from LDS.  The frame two workgroups share is transformed by both.  No atomics, no work buffer; a row's bits do not depend on B,
 * on the row's position or on the grid.
 * MFPA_EINVAL before any launch, no device pointer dereferenced on the host: B < 1 or B > 65535, T < 1 or T > 2^30, ldx < T, x_f64 /
 * y_f64 other than 0 or 1, n_bands outside [1, MFPA_CODEC_MAX_BANDS], a null x, y or band_edges, a misaligned pointer, edges that do
 * not ascend strictly from 0 to 256, up_db or down_db negative or not finite, rate NaN with row_rates NULL. */
#define MFPA_CODEC_FRAMES 31
#define MFPA_CODEC_MAX_BANDS 32
int mfpa_transform_codec(const void* x, int x_f64, long long ldx, int B, long long T, double rate, const double* row_rates,
                         const int* band_edges, int n_bands, double up_db, double down_db, const unsigned char* apply, void* y, int y_f64,
                         double* lambda_out, int* coded_out, void* stream);
/* mfpa_mulaw.  mu = channels - 1, 2 <= channels <= 65536, float64, the formulas of torchaudio's mu_law_encoding / mu_law_decoding:
 *   encode:  v = min(max(x, -1), 1);  c = sign(v) * log1p(mu * |v|) / log1p(mu);  code = floor((c + 1) / 2 * mu + 1/2)
 *   decode:  v = 2 * code / mu - 1;   y = sign(v) * (exp(|v| * log1p(mu)) - 1) / mu
 * log1p(mu) is the host's double.  mode MFPA_MULAW_ENCODE: x float32 / float64 -> y int32 (y_f64 = 0); MFPA_MULAW_DECODE: x int32
 * (x_f64 = 0; any value, the code is a number and never an index) -> y float32 / float64; MFPA_MULAW_ROUNDTRIP: both in one pass, the
 * code kept as a double.  apply (round trip only): NULL, or B bytes on the device, row b with apply[b] == 0 copied through.
 * MFPA_EINVAL before any launch: B < 1 or B > 65535, T < 1 or T > 2^30, channels outside [2, 65536], an unknown mode, x_f64 / y_f64
 * other than 0 or 1 or set on the int32 side, apply outside the round trip, a null or misaligned x or y. */
#define MFPA_MULAW_ENCODE 0
#define MFPA_MULAW_DECODE 1
#define MFPA_MULAW_ROUNDTRIP 2
int mfpa_mulaw(const void* x, int x_f64, int B, long long T, int channels, int mode, const unsigned char* apply, void* y, int y_f64,
               void* stream);

/* ---------------------------------------------------------------------------------------
 * Model-free spectral noise suppression (csrc/denoise.hip): a windowed minimum-statistics noise tracker per frequency bin (Martin
 * 2001, plain form), the decision-directed a-priori SNR (Ephraim and Malah 1984) and a Wiener gain on STFT magnitudes.  No weights.
 * Additive to ABI 47.
 *
 * mfpa_spectral_suppress.  m[b][k][t] >= 0: (B, F, nF) magnitudes, frames contiguous (the layout of mfpa_stft_mag).  Float64
 * throughout; every product, sum and quotient is rounded on its own, in the order written; max and min are fmax and fmin (they
 * select and never round; a NaN operand loses).  Per clip b and bin k, all independent of each other:
 *   p[t]  = m[t] * m[t]
 *   s[0]  = p[0];   s[t] = alpha * s[t-1] + (1 - alpha) * p[t]                 (1 - alpha formed once, on the host)
 *   n[t]  = bias * min{ s[u] : max(0, t - back) <= u <= min(nF - 1, t + ahead) }
 *           or, when noise (B, F) is passed:  n[t] = noise[b][k]  (no bias, no tracker)
 *   d[t]  = max(n[t], DBL_MIN)
 *   q[t]  = p[t] / d[t]                                                        (may be +inf: digital silence inside the window)
 *   i[t]  = max(q[t] - 1, 0)
 *   xi[0] = max(a + (1 - a) * i[0], xi_min)
 *   xi[t] = max(a * ((g[t-1] * g[t-1]) * q[t-1]) + (1 - a) * i[t], xi_min)
 *   g[t]  = max(1 - 1 / (1 + xi[t]), g_floor)                                  (this form gives 1, not NaN, at xi = +inf)
 *   y[t]  = g[t] * m[t]        or  (g[t] * m[t]) / denom[b]  when denom is passed
 *   m        (B, F, nF) on the device, float32 (m_f64 = 0) or float64; not overlapping y
 *   row_floor  NULL, or (B,) float64 on the device: g_floor per clip in place of the argument (not checked: the Python layer does)
 *   noise    NULL, or (B, F) float64 on the device
 *   denom    NULL, or (B,) float64 on the device
 *   apply    NULL, or B bytes on the device: row b with apply[b] == 0 has g = 1 (y = m or m / denom[b]) and n = 0
 *   y        (B, F, nF) on the device, float32 (y_f64 = 0, the float64 value rounded once) or float64
 *   g_out, n_out   NULL, or (B, F, nF) float64 on the device: g and n
 * One launch; a workgroup of one wavefront owns 16 bins of a clip, tiles of 16 bins x 64 frames go through LDS transposed, the gain
 * walk lags the s walk by ceil(ahead / 64) tiles with s in a ring in LDS, the sliding minimum is taken by all lanes by block prefix
 * and suffix minima.  No atomics, no work buffer; a row's bits do not depend on B, on the row's position or on the grid.
 * MFPA_EINVAL before any launch, no device pointer dereferenced on the host: alpha or a outside [0, 1), xi_min <= 0 or not finite,
 * g_floor outside [0, 1], bias <= 0 or not finite, back or ahead negative, back + ahead + 1 > MFPA_DENOISE_MAX_WINDOW, B, F or nF
 * below 1, nF > 16384, B > 65535, F > 2^20, m_f64 / y_f64 other than 0 or 1, a null m or y, a misaligned pointer. */
#define MFPA_DENOISE_MAX_WINDOW 128
int mfpa_spectral_suppress(const void* m, int m_f64, int B, int F, int nF, double alpha, int back, int ahead, double bias, double a,
                           double xi_min, double g_floor, const double* row_floor, const double* noise, const double* denom,
                           const unsigned char* apply, void* y, int y_f64, double* g_out, double* n_out, void* stream);

/* ---------------------------------------------------------------------------------------
 * Programme loudness (csrc/loudness.hip): the meter of ITU-R BS.1770-4 / EBU R 128 with the loudness range of EBU Tech 3342 and a
 * loudness-normalising gain.  Additive to ABI 47.  Rows are the channels of examples: (B, C, T) samples, R = B C rows.
 *
 * Geometry.  hop H samples (100 ms: H = floor(0.1 fs + 0.5), formed by the caller); segment k of a row is its samples
 * [k H, (k + 1) H), nseg = T / H (integer division); a block is win consecutive segments and advances by one: nb = max(0, nseg - win
 * + 1).  win = 4 is the 400 ms block with 75 % overlap of BS.1770, win = 30 the 3 s short-term window.  The trailing T - nseg H
 * samples are filtered and count for the peak but belong to no segment.
 *
 * mfpa_loudness_segments.  y = the row filtered by the S second-order sections sos (S, 6), shared by all rows, float64 on the device,
 * a0 == 1 and not read, zero initial state: mfpa_sosfilt's arithmetic, order and chunking, so y is mfpa_sosfilt's float64 output bit
 * for bit before its rounding to the sample type.  S == 0: y = x (a plain mean-square meter).  y is not stored.
 *   seg[r][k] = sum of y[n]^2 over segment k, float64, in THIS order.  Sample n belongs to lane group n / 16 (16 consecutive samples),
 *   to lane l = (n / 16) mod 64 and to super-chunk n / 1024 (64 lane groups).
 *     t   = the 16 squares of a lane group, those outside the segment replaced by 0, added by the pairwise tree: neighbours first
 *           (s_0 + s_1, s_2 + s_3, ...), then pairs of pairs, four levels
 *     a_l = a_l + t for the lane groups of lane l, one per super-chunk that overlaps the segment, in increasing n; a_l starts at 0
 *     seg = the 64 a_l combined by the binary tree over l: neighbours first (a_0 + a_1, a_2 + a_3, ...), then pairs of pairs, six levels
 *   peak[r] = max |x[n]| over all T samples of the UNFILTERED input, exact, as float64; a NaN sample is skipped (fmax).  NULL: not
 *   wanted.
 *   x (R, T) float32 (x_f64 = 0) or float64 on the device; seg (R, nseg) float64 (may be NULL when nseg == 0); work: work_len >=
 *   mfpa_loudness_work(S) float64 on the device (the powers table of mfpa_sosfilt; may be NULL when S == 0).
 * One wavefront owns a row; no atomics, no work buffer but the powers; a row's bits do not depend on R, on its position or on the grid.
 * MFPA_EINVAL before any launch, no pointer dereferenced on the host: R < 0 or R > 65535, T < 1 or T > 2^30, S < 0 or S >
 * MFPA_SOS_MAX_SECTIONS, hop < 1 or hop > 2^24, x_f64 other than 0 or 1, work_len too short, and with R > 0 a null x, a null seg with
 * nseg > 0, a null sos or work with S > 0, a misaligned pointer.  R == 0: MFPA_OK, no launch.
 *
 * mfpa_loudness_gate, per example b, from seg (B, C, nseg):
 *   p[j] = sum over c of  G[c] * ((seg[c][j] + seg[c][j+1] + ... + seg[c][j+win-1]) / d),   d = (double)win * (double)hop
 *          (k increasing inside the block from seg[c][j], then c increasing from the term of c = 0; G = weights (C,) float64 on the
 *          device, NULL: 1 for every channel; BS.1770 gives the surround pair 1.41)
 *   absolute gate:  A = { j : p[j] > p_abs },  n_abs = |A|,  m_abs = sum(p over A) / n_abs  (0 when n_abs == 0)
 *   relative gate:  G2 = { j in A : p[j] > rel * m_abs },  n_rel = |G2|,  P_gated = sum(p over G2) / n_rel  (0 when n_rel == 0)
 *   A NaN power fails every comparison.  Both sums have this order: t = j mod 256 collects its members in increasing j into a
 *   partial sum that starts at 0; the 256 partial sums a_t are combined by a_t = a_t + a_(t + off) for t < off, off = 128, 64, ..., 1.
 *   The host passes p_abs = 10^((-70 + 0.691) / 10) and rel = 0.1 (integrated loudness) or 0.01 (range); there is no logarithm here.
 *   power (B, 2) float64: P_gated, m_abs.  counts (B, 2) int32: n_abs, n_rel.
 *   blocks  NULL, or (B, nb) float64: p (the momentary curve at win = 4, the short-term curve at win = 30)
 *   range   NULL, or (B, 2) float64: the values at ranks (n + 4) / 10 and (19 n - 9) / 20 (integer divisions, n = n_rel) of the
 *           ascending members of G2: the nearest ranks at 10 % and 95 %; 0 and 0 when n == 0.  nb <= MFPA_LOUDNESS_MAX_RANGE_BLOCKS.
 * LUFS = -0.691 + 10 log10(P) and LRA = 10 log10(P_hi / P_lo) are formed by the caller.
 * MFPA_EINVAL before any launch: B < 0 or B > 65535, C < 1 or C > MFPA_LOUDNESS_MAX_CHANNELS, nseg < 0 or nseg > 2^30, hop < 1 or hop >
 * 2^24, win < 1 or win > MFPA_LOUDNESS_MAX_WINDOW, p_abs or rel negative or not finite, range with nb > MFPA_LOUDNESS_MAX_RANGE_BLOCKS,
 * and with B > 0 a null power or counts, a null seg with nseg > 0, a misaligned pointer.  B == 0: MFPA_OK, no launch.
 *
 * mfpa_loudness_apply.  g[b] = sqrt(target[b] / gated[b]), both correctly rounded; target (B,) float64 holds P_target = 10^((LUFS
 * target + 0.691) / 10) from the host, gated (B,) float64 is P_gated (stride 1: copy it out of `power`).  With peak_limit > 0 and peak
 * (B, C): g = min(g, peak_limit / max_c peak[b][c]).  y = x g in float64, rounded once for float32.  A row is copied bit for bit when
 * gated[b] == 0, when g is not finite, or when apply[b] == 0 (apply NULL or B bytes).  gain: NULL, or (B,) float64: g, 1 for a copied
 * example.  Everything is read on the device: the chain segments -> gate -> apply needs no host synchronisation.
 * MFPA_EINVAL before any launch: B < 0, C < 1 or C > MFPA_LOUDNESS_MAX_CHANNELS, B C > 65535, T < 1 or T > 2^30, x_f64 other than 0 or
 * 1, peak_limit negative or not finite, peak_limit > 0 without peak or peak with peak_limit == 0, and with B > 0 a null x, y, gated
 * or target, a misaligned pointer.  B == 0: MFPA_OK, no launch. */
#define MFPA_LOUDNESS_MAX_CHANNELS 8
#define MFPA_LOUDNESS_MAX_WINDOW 64
#define MFPA_LOUDNESS_MAX_RANGE_BLOCKS 16384
int mfpa_loudness_segments(const void* x, int x_f64, int R, long long T, const double* sos, int S, int hop, double* work, long long work_len,
                           double* seg, double* peak, void* stream);
/* HOST function, no GPU work: *work_len = S * 256 doubles.  MFPA_EINVAL: a null pointer, S < 0 or S > MFPA_SOS_MAX_SECTIONS. */
int mfpa_loudness_work(int S, long long* work_len);
int mfpa_loudness_gate(const double* seg, int B, int C, long long nseg, int hop, int win, const double* weights, double p_abs, double rel,
                       double* power, int* counts, double* blocks, double* range, void* stream);
int mfpa_loudness_apply(const void* x, int x_f64, int B, int C, long long T, const double* gated, const double* target, const double* peak,
                        double peak_limit, const unsigned char* apply, void* y, double* gain, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MFPA_H */
