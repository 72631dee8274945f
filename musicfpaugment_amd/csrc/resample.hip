// Windowed-sinc resampling by any rational ratio for MI355X (gfx950).
// Reference: torchaudio.transforms.Resample(orig_freq, new_freq) (resampling_method "sinc_interp_hann", lowpass_filter_width 6,
// rolloff 0.99), which deezer/musicFPaugment applies at afp/audfprint/peak_extractor.py:378-388, afp/dejavu/dejavu.py:91-115,
// testing/generate_queries.py:39, training/background_noise.py:300 and training/generate_audios.py:51.  torchaudio is NOT in the
// reference tree: the algorithm is restated from its public source and parity with it is unpinned (property- and oracle-tested).
//
// With g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) * rolloff, width = ceil(lowpass_filter_width * o / base) and
// K = 2 * width + o taps per phase, xpad[m] = x[m - width] inside the clip and 0 outside:
//   y[j * n + i] = sum_{k < K} tap[i][k] * xpad[j * o + k],     i < n,    the first ceil(n * T / o) samples are kept.
//
//   resample_kernel   a workgroup owns `tile` consecutive frames j of one clip and stages their input window ((tile - 1) * o + K
//                     floats, zero outside [0, T)) in LDS.  A LANE owns a frame and a WAVE owns P phases at a time: the taps of a
//                     wave are then the same in every lane, so they arrive by scalar loads (phase-major bank, L2-resident, shared
//                     by every workgroup) and enter the multiply-adds as scalar operands -- no vector-memory or LDS traffic for
//                     them; the window sample x[j * o + k] is one LDS read per lane that feeds P multiply-adds.  Lanes read the
//                     window at a stride of o floats: conflict-free for odd o; for even o the window is stored skewed by one
//                     float per 32 (SKEW).  The 4 or 16 waves of a workgroup split into frame groups of 64 and phase groups, and a
//                     lane takes several frames one after the other where the window is small (rs_plan).
//                     Every output is ONE chain acc = fma(tap[i][k], xpad[j * o + k], acc) over k = 0 .. K-1 from acc = 0, so its
//                     value depends on the clip's samples and (o, n, width, taps) alone -- not on the batch, the tile, the row
//                     pitch or the memory behind the clip's T samples.
//
// Nearly all taps of a phase are exact zeros when o is large: the window argument t is clamped to +-lowpass_filter_width, where
// cos^2(pi / 2) * sinc * scale is about 1e-49 and rounds to 0.0f, so only the run |t| < lowpass_filter_width -- at most
// 2 * width + 1 taps, S of them stored per phase (mfpa_resample_sparse_taps, which proves the zeros) -- contributes.
//   resample_sparse_kernel   a workgroup owns `tile` consecutive OUTPUT samples q = j * n + i of one clip and stages the input span
//                     they read (about tile * o / n + S floats, zero outside [0, T)) in LDS.  A LANE owns an output: consecutive
//                     lanes have consecutive phases i (wrapping n-1 -> 0 into the next frame), so their rows of the n x S table are
//                     contiguous in memory and arrive as float4 loads; first[i] is one int per lane.  The window reads of
//                     neighbouring lanes start about o / n floats apart: for ratios near 1 a half-wave spans a little more than
//                     the 32 banks (two-way where it wraps); for an even whole ratio (n == 1) the window is stored skewed by one
//                     float per 32, as above.  Every output is ONE chain acc = fma(tap[i][u], xpad[j * o + first[i] + u], acc)
//                     over u = 0 .. S-1 from acc = 0: the dense chain without its zero taps, so the same float32 value (up to the
//                     sign of a zero), and independent of the batch, the tile, the row pitches and the memory behind the clip.
#include <math.h>
#include <stdint.h>

#include "mfpa_common.h"

namespace {

constexpr int RS_MAX_WAVES = 16;      // of a workgroup (1024 threads)
constexpr int RS_STAGE = 16;          // window loads a thread keeps in flight
constexpr int RS_MAX_ROUNDS = 8;      // frames a lane owns one after the other, at most

struct RsPlan {
  int P;        // phases a wave accumulates at a time (the kernel's template argument): 1, 2 or 5
  int pw;       // phase groups: waves of a workgroup that share the frames and split the phases (a power of two)
  int waves;    // of a workgroup: 4 or 16
  int tile;     // frames per workgroup: 64 * (waves / pw) * rounds, or what the LDS window admits
};

// n = 1 (integer decimation) needs one accumulator; 5 divides the 80 phases of 44.1 -> 8 kHz into the 16 waves of a workgroup.
// Few phases (a short filter on a small o: the memory-bound end) get workgroups of 4 waves, so that eight of them share a CU and
// the staging of one runs under the arithmetic of another; their lanes take up to eight frames one after the other, as many as
// one batch of RS_STAGE loads per thread stages.  Many phases get 16 waves and, for o in the hundreds, the CU's LDS to themselves.
inline RsPlan rs_plan(int o, int n, int K) {
  RsPlan p;
  p.P = n >= 5 ? 5 : (n >= 2 ? 2 : 1);
  const int groups = (n + p.P - 1) / p.P;
  p.pw = 1;
  while (2 * p.pw <= groups && 2 * p.pw <= RS_MAX_WAVES) p.pw *= 2;
  p.waves = p.pw <= 4 ? 4 : RS_MAX_WAVES;
  const int round = 64 * (p.waves / p.pw);                           // frames the workgroup's lanes cover at once
  const int fit = (MFPA_RESAMPLE_MAX_WINDOW - K) / o + 1;            // >= 1: K <= MFPA_RESAMPLE_MAX_TAPS < the window limit
  const int batch = RS_STAGE * 64 * p.waves;                         // floats one batch of staging loads brings
  int rounds = batch >= K ? ((batch - K) / o + 1) / round : 0;
  rounds = rounds > RS_MAX_ROUNDS ? RS_MAX_ROUNDS : rounds;
  p.tile = rounds >= 1 ? round * rounds : (fit < round ? fit : round);
  return p;
}

inline bool rs_shape_ok(int o, int n, int width) {
  if (o < 1 || n < 1 || width < 1 || n > MFPA_RESAMPLE_MAX_PHASES || o > MFPA_RESAMPLE_MAX_TAPS || width > MFPA_RESAMPLE_MAX_TAPS) return false;
  return 2 * width + o <= MFPA_RESAMPLE_MAX_TAPS;
}

// floats between the taps of one phase and the next: a multiple of a 64-byte line, so that the eight-tap scalar loads of the inner
// loop never straddle two lines (the lines a CU's scalar cache has to keep alive are then one per phase in flight, not two)
inline int rs_pitch(int K) { return (K + MFPA_RESAMPLE_TAP_ALIGN - 1) / MFPA_RESAMPLE_TAP_ALIGN * MFPA_RESAMPLE_TAP_ALIGN; }

// The per-tap expression of both bank builders: the float32 phase of torchaudio, the float64 sequence, one rounding.
// rs_tap_value takes the window argument AFTER its clamp to +-lpw, so that the sparse builder can evaluate the two constants every
// tap outside the run |t| < lpw takes.
inline double rs_tap_arg(double phase, int k, int width, int o, double base) { return (phase + (double)(k - width) / (double)o) * base; }

inline float rs_tap_value(double t, double lpw, double scale) {
  const double pi = 3.14159265358979323846;
  const double c = cos(t * pi / lpw / 2.0);
  const double win = c * c;
  t *= pi;
  const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
  return (float)(sinc * win * scale);
}

inline float rs_tap(double phase, int k, int width, int o, double base, double lpw, double scale) {
  double t = rs_tap_arg(phase, k, width, o, base);
  t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
  return rs_tap_value(t, lpw, scale);
}

inline double rs_phase(int i, int n) { return (double)((float)(-i) / (float)n); }      // torchaudio forms the phase offset in float32

// ---- sparse form: only the taps of the run |t| < lpw
constexpr int RSS_THREADS = 256;
constexpr int RSS_MAX_TILE = 1024;     // output samples of a workgroup, at most: four per lane
constexpr int RSS_WINDOW = 16384;      // floats of LDS window a workgroup aims to stay within (two workgroups per CU and more)
constexpr int RSS_STAGE = 8;           // window loads a thread keeps in flight
// first[i] - floor(i * o / n) lies in [RSS_DLO, RSS_DHI] (1 or 2 for every pair tried): mfpa_resample_sparse_taps refuses a table
// for which it does not, and the kernel sizes its window by it.
constexpr int RSS_DLO = 0;
constexpr int RSS_DHI = 3;

inline int rss_support(int width) { return (2 * width + 1 + 3) / 4 * 4; }

inline bool rss_shape_ok(int o, int n, int width) {
  if (o < 1 || n < 1 || width < 1 || n > MFPA_RESAMPLE_SPARSE_MAX_PHASES || o > MFPA_RESAMPLE_SPARSE_MAX_ORIG) return false;
  return 2 * width + 1 <= MFPA_RESAMPLE_SPARSE_MAX_SUPPORT;
}

// floats of input the outputs q0 .. q0 + tile - 1 read, at most: floor(q * o / n) moves by at most ceil((tile - 1) * o / n)
inline long long rss_window(int o, int n, int S, long long tile) { return ((tile - 1) * o + n - 1) / n + (RSS_DHI - RSS_DLO) + S; }

// Output samples per workgroup: a multiple of 64 up to RSS_MAX_TILE whose window stays within RSS_WINDOW floats.  With the width
// that belongs to (o, n), S <= 512 bounds o / n by 43 and 64 outputs span fewer than 3300 floats; a width that does not (a raw
// call) can leave even 64 outputs beyond MFPA_RESAMPLE_MAX_WINDOW, which the entry points refuse.
inline int rss_tile(int o, int n, int width) {
  const int S = rss_support(width);
  int tile = RSS_MAX_TILE;
  while (tile > 64 && rss_window(o, n, S, tile) > RSS_WINDOW) tile -= 64;
  return tile;
}

template <bool SKEW>
__device__ __forceinline__ int rs_slot(int m) {
  return SKEW ? m + (m >> 5) : m;
}

template <int P, bool SKEW>
__global__ MFPA_NO_PK_F32 __launch_bounds__(64 * RS_MAX_WAVES) void resample_kernel(const float* __restrict__ x, long long T, long long ldx, int o, int n,
                                                                            int width, int K, int pitch, int tile, int pw, const float* __restrict__ taps,
                                                                            float* __restrict__ y, long long Tout, long long ldy) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int tid = threadIdx.x, lane = tid & 63, threads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);         // the same in every lane: what follows from it stays scalar
  const long long j0 = (long long)blockIdx.x * tile;                 // first frame of this workgroup
  const float* xb = x + (long long)blockIdx.y * ldx;
  float* yb = y + (long long)blockIdx.y * ldy;
  const int W = (tile - 1) * o + K;
  const long long s0 = j0 * o - width;                               // sample index of the window's first float
  // RS_STAGE loads in flight per thread: every load is unconditional (its index clamped into the clip, the value then selected)
  for (int m0 = tid; m0 < W; m0 += RS_STAGE * threads) {
    float v[RS_STAGE];
#pragma unroll
    for (int u = 0; u < RS_STAGE; ++u) {
      const long long s = s0 + m0 + u * threads;
      v[u] = T > 0 ? xb[s < 0 ? 0 : (s >= T ? T - 1 : s)] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RS_STAGE; ++u) {
      const int m = m0 + u * threads;
      const long long s = s0 + m;
      if (m < W) win[rs_slot<SKEW>(m)] = (s >= 0 && s < T) ? v[u] : 0.f;
    }
  }
  __syncthreads();
  const int fw = (threads >> 6) / pw;
  for (int jt = (wave / pw) * 64 + lane, jw = (wave / pw) * 64; jw < tile; jt += 64 * fw, jw += 64 * fw) {   // jw: the wave's first frame
    const int a0 = (jt < tile ? jt : tile - 1) * o;                  // frames beyond the tile read a valid window and store nothing
    const long long q0 = (j0 + jt) * n;
    for (int i0 = (wave % pw) * P; i0 < n; i0 += pw * P) {
      const float* tp[P];
#pragma unroll
      for (int p = 0; p < P; ++p) tp[p] = taps + (size_t)(i0 + p < n ? i0 + p : n - 1) * pitch;
      float acc[P];
#pragma unroll
      for (int p = 0; p < P; ++p) acc[p] = 0.f;
#pragma unroll 8
      for (int k = 0; k < K; ++k) {
        const float xv = win[rs_slot<SKEW>(a0 + k)];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p] = __builtin_fmaf(tp[p][k], xv, acc[p]);
      }
#pragma unroll
      for (int p = 0; p < P; ++p)
        if (jt < tile && i0 + p < n && q0 + i0 + p < Tout) yb[q0 + i0 + p] = acc[p];
    }
  }
}

template <bool SKEW>
__global__ MFPA_NO_PK_F32 __launch_bounds__(RSS_THREADS) void resample_sparse_kernel(const float* __restrict__ x, long long T, long long ldx, int o, int n,
                                                                              int width, int S, int tile, int W,
                                                                              const float* __restrict__ taps, const int* __restrict__ first,
                                                                              float* __restrict__ y, long long Tout, long long ldy) {
  extern __shared__ __attribute__((aligned(16))) float win[];
  const int tid = threadIdx.x;
  const long long q0 = (long long)blockIdx.x * tile;                 // first output sample of this workgroup
  const long long j0 = q0 / n;
  const int i0 = (int)(q0 - j0 * n);
  const int b0 = (int)((long long)i0 * o / n) + RSS_DLO;             // window slot w holds xpad[j0 * o + b0 + w]
  const float* xb = x + (long long)blockIdx.y * ldx;
  float* yb = y + (long long)blockIdx.y * ldy;
  const long long s0 = j0 * o + b0 - width;                          // sample index of the window's first float
  // every load is unconditional (its index clamped into the clip, the value then selected), as in resample_kernel
  for (int m0 = tid; m0 < W; m0 += RSS_STAGE * RSS_THREADS) {
    float v[RSS_STAGE];
#pragma unroll
    for (int u = 0; u < RSS_STAGE; ++u) {
      const long long s = s0 + m0 + u * RSS_THREADS;
      v[u] = T > 0 ? xb[s < 0 ? 0 : (s >= T ? T - 1 : s)] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < RSS_STAGE; ++u) {
      const int m = m0 + u * RSS_THREADS;
      const long long s = s0 + m;
      if (m < W) win[rs_slot<SKEW>(m)] = (s >= 0 && s < T) ? v[u] : 0.f;
    }
  }
  __syncthreads();
  for (int l = tid; l < tile; l += RSS_THREADS) {
    const int e = i0 + l;                                            // < n + tile
    const int jj = e / n, i = e - jj * n;                            // the phase wraps n-1 -> 0 into the next frame
    int a = jj * o + first[i] - b0;                                  // jj * o <= the window's span + o: no overflow
    a = a < 0 ? 0 : (a > W - S ? W - S : a);                         // a table mfpa_resample_sparse_taps built never needs the clamp
    const float4* tp = reinterpret_cast<const float4*>(taps + (size_t)i * S);
    float acc = 0.f;
#pragma unroll 4
    for (int u = 0; u < S; u += 4) {
      const float4 t = tp[u >> 2];
      acc = __builtin_fmaf(t.x, win[rs_slot<SKEW>(a + u)], acc);
      acc = __builtin_fmaf(t.y, win[rs_slot<SKEW>(a + u + 1)], acc);
      acc = __builtin_fmaf(t.z, win[rs_slot<SKEW>(a + u + 2)], acc);
      acc = __builtin_fmaf(t.w, win[rs_slot<SKEW>(a + u + 3)], acc);
    }
    if (q0 + l < Tout) yb[q0 + l] = acc;
  }
}

template <int P>
void rs_launch(bool skew, dim3 grid, dim3 block, size_t lds, hipStream_t s, const float* x, long long T, long long ldx, int o, int n, int width,
               int K, int pitch, int tile, int pw, const float* taps, float* y, long long Tout, long long ldy) {
  if (skew) hipLaunchKernelGGL((resample_kernel<P, true>), grid, block, lds, s, x, T, ldx, o, n, width, K, pitch, tile, pw, taps, y, Tout, ldy);
  else hipLaunchKernelGGL((resample_kernel<P, false>), grid, block, lds, s, x, T, ldx, o, n, width, K, pitch, tile, pw, taps, y, Tout, ldy);
}

}  // namespace

extern "C" {

int mfpa_resample_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, long long T, int* o, int* n,
                           int* width, int* ntaps, long long* Tout) {
  if (orig_freq < 1 || new_freq < 1 || lowpass_filter_width < 1 || !(rolloff > 0.0) || rolloff > 1.0 || T < 0 || T > MFPA_RESAMPLE_MAX_SAMPLES)
    return MFPA_EINVAL;
  int a = orig_freq, b = new_freq;
  while (b) { const int r = a % b; a = b; b = r; }
  const int oo = orig_freq / a, nn = new_freq / a;
  const double base = (double)(oo < nn ? oo : nn) * rolloff;
  const double wd = ceil((double)lowpass_filter_width * (double)oo / base);
  if (!(wd <= (double)MFPA_RESAMPLE_MAX_TAPS)) return MFPA_EINVAL;
  const int w = (int)wd;
  if (!rs_shape_ok(oo, nn, w)) return MFPA_EINVAL;
  if (o) *o = oo;
  if (n) *n = nn;
  if (width) *width = w;
  if (ntaps) *ntaps = 2 * w + oo;
  if (Tout) *Tout = ((long long)nn * T + oo - 1) / oo;
  return MFPA_OK;
}

int mfpa_resample_tile(int o, int n, int width) {
  if (!rs_shape_ok(o, n, width)) return MFPA_EINVAL;
  return rs_plan(o, n, 2 * width + o).tile;
}

int mfpa_resample_taps(int o, int n, int width, int lowpass_filter_width, double rolloff, float* taps) {
  if (!taps || !rs_shape_ok(o, n, width) || lowpass_filter_width < 1 || !(rolloff > 0.0) || rolloff > 1.0) return MFPA_EINVAL;
  const int K = 2 * width + o, pitch = rs_pitch(K);
  const double base = (double)(o < n ? o : n) * rolloff;
  const double lpw = (double)lowpass_filter_width, scale = base / (double)o;
  for (int i = 0; i < n; ++i) {
    const double phase = rs_phase(i, n);
    for (int k = 0; k < K; ++k) taps[(size_t)i * pitch + k] = rs_tap(phase, k, width, o, base, lpw, scale);
    for (int k = K; k < pitch; ++k) taps[(size_t)i * pitch + k] = 0.f;
  }
  return MFPA_OK;
}

int mfpa_resample(const float* x, int B, long long T, long long ldx, int o, int n, int width, const float* taps, float* y,
                  long long Tout, long long ldy, void* stream) {
  if (B < 0 || T < 0 || Tout < 0 || !rs_shape_ok(o, n, width)) return MFPA_EINVAL;
  if (B == 0 || Tout == 0) return MFPA_OK;
  if (!x || !taps || !y || ldx < T || ldy < Tout || T > MFPA_RESAMPLE_MAX_SAMPLES || B > 65535) return MFPA_EINVAL;
  if (Tout > (long long)n * (T / o + 1)) return MFPA_EINVAL;
  const int K = 2 * width + o;
  const RsPlan p = rs_plan(o, n, K);
  const long long frames = (Tout + n - 1) / n;
  const long long tiles = (frames + p.tile - 1) / p.tile;
  if (tiles > MFPA_RESAMPLE_MAX_TILES) return MFPA_EINVAL;
  const bool skew = (o & 1) == 0;
  const size_t W = (size_t)(p.tile - 1) * o + K;
  const size_t lds = sizeof(float) * (skew ? W + (W >> 5) + 1 : W);
  const dim3 grid((unsigned)tiles, (unsigned)B), block(64u * p.waves);
  hipStream_t s = mfpa_stream(stream);
  if (p.P == 5) rs_launch<5>(skew, grid, block, lds, s, x, T, ldx, o, n, width, K, rs_pitch(K), p.tile, p.pw, taps, y, Tout, ldy);
  else if (p.P == 2) rs_launch<2>(skew, grid, block, lds, s, x, T, ldx, o, n, width, K, rs_pitch(K), p.tile, p.pw, taps, y, Tout, ldy);
  else rs_launch<1>(skew, grid, block, lds, s, x, T, ldx, o, n, width, K, rs_pitch(K), p.tile, p.pw, taps, y, Tout, ldy);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_resample_sparse_geometry(int orig_freq, int new_freq, int lowpass_filter_width, double rolloff, long long T, int* o, int* n,
                                  int* width, int* support, long long* Tout) {
  if (orig_freq < 1 || new_freq < 1 || lowpass_filter_width < 1 || !(rolloff > 0.0) || rolloff > 1.0 || T < 0 || T > MFPA_RESAMPLE_MAX_SAMPLES)
    return MFPA_EINVAL;
  int a = orig_freq, b = new_freq;
  while (b) { const int r = a % b; a = b; b = r; }
  const int oo = orig_freq / a, nn = new_freq / a;
  const double base = (double)(oo < nn ? oo : nn) * rolloff;
  const double wd = ceil((double)lowpass_filter_width * (double)oo / base);
  if (!(wd <= (double)MFPA_RESAMPLE_SPARSE_MAX_SUPPORT)) return MFPA_EINVAL;
  const int w = (int)wd;
  if (!rss_shape_ok(oo, nn, w)) return MFPA_EINVAL;
  if (o) *o = oo;
  if (n) *n = nn;
  if (width) *width = w;
  if (support) *support = rss_support(w);
  if (Tout) *Tout = ((long long)nn * T + oo - 1) / oo;
  return MFPA_OK;
}

int mfpa_resample_sparse_tile(int o, int n, int width) {
  if (!rss_shape_ok(o, n, width)) return MFPA_EINVAL;
  const int tile = rss_tile(o, n, width);
  return rss_window(o, n, rss_support(width), tile) > MFPA_RESAMPLE_MAX_WINDOW ? MFPA_EINVAL : tile;
}

int mfpa_resample_sparse_taps(int o, int n, int width, int lowpass_filter_width, double rolloff, float* taps, int32_t* first) {
  if (!taps || !first || !rss_shape_ok(o, n, width) || lowpass_filter_width < 1 || !(rolloff > 0.0) || rolloff > 1.0) return MFPA_EINVAL;
  const int S = rss_support(width);
  const long long K = 2LL * width + o;
  const double base = (double)(o < n ? o : n) * rolloff;
  const double lpw = (double)lowpass_filter_width, scale = base / (double)o;
  // Outside the run -lpw < t < lpw the clamped argument is exactly -lpw or +lpw: every dropped tap is one of these two values.
  if (rs_tap_value(-lpw, lpw, scale) != 0.f || rs_tap_value(lpw, lpw, scale) != 0.f) return MFPA_EINVAL;
  // First pass, no writes: the run of every phase.  t is monotone in k, so the run is [lo, hi] with t(lo - 1) <= -lpw < t(lo) and
  // t(hi) < lpw <= t(hi + 1); the estimates come from the formula in real numbers and are walked to where the float64 t says.
  for (int pass = 0; pass < 2; ++pass) {
    for (int i = 0; i < n; ++i) {
      const double phase = rs_phase(i, n);
      long long lo = (long long)floor((double)width + (double)o * (-phase - lpw / base));
      while (rs_tap_arg(phase, (int)(lo - 1), width, o, base) > -lpw) --lo;
      while (!(rs_tap_arg(phase, (int)lo, width, o, base) > -lpw)) ++lo;
      long long hi = (long long)floor((double)width + (double)o * (-phase + lpw / base));
      while (rs_tap_arg(phase, (int)(hi + 1), width, o, base) < lpw) ++hi;
      while (!(rs_tap_arg(phase, (int)hi, width, o, base) < lpw)) --hi;
      if (lo < 0) lo = 0;                                            // the dense row starts at k = 0 ...
      if (hi > K - 1) hi = K - 1;                                    // ... and ends at K - 1
      const long long d = lo - (long long)i * o / n;
      if (hi - lo + 1 > S || d < RSS_DLO || d > RSS_DHI) return MFPA_EINVAL;
      if (pass == 0) continue;
      first[i] = (int32_t)lo;
      for (int u = 0; u < S; ++u) {
        const long long k = lo + u;
        taps[(size_t)i * S + u] = k < K ? rs_tap(phase, (int)k, width, o, base, lpw, scale) : 0.f;
      }
    }
  }
  return MFPA_OK;
}

int mfpa_resample_sparse(const float* x, int B, long long T, long long ldx, int o, int n, int width, int support, const float* taps,
                         const int32_t* first, float* y, long long Tout, long long ldy, void* stream) {
  if (B < 0 || T < 0 || Tout < 0 || !rss_shape_ok(o, n, width) || support != rss_support(width)) return MFPA_EINVAL;
  if (B == 0 || Tout == 0) return MFPA_OK;
  if (!x || !taps || !first || !y || ldx < T || ldy < Tout || T > MFPA_RESAMPLE_MAX_SAMPLES || B > 65535) return MFPA_EINVAL;
  if (((uintptr_t)taps & 15) != 0) return MFPA_EINVAL;                // the rows are read as float4
  if (Tout > (long long)n * (T / o + 1)) return MFPA_EINVAL;
  const int tile = rss_tile(o, n, width);
  const long long tiles = (Tout + tile - 1) / tile;
  if (tiles > MFPA_RESAMPLE_MAX_TILES) return MFPA_EINVAL;
  const long long W = rss_window(o, n, support, tile);
  if (W > MFPA_RESAMPLE_MAX_WINDOW) return MFPA_EINVAL;               // a width too small for o / n: see rss_tile
  // lanes start o / n floats apart: an even whole stride (n == 1) puts a half-wave on half the banks or fewer unless the window is
  // skewed.  Counted per half-wave read on the host for the other ratios: a stride near 1 spreads 32 lanes over about 36
  // consecutive floats, two-way on the few banks where the span wraps, and no skew of this kind removes that.
  const bool skew = n == 1 && (o & 1) == 0;
  const size_t lds = sizeof(float) * (size_t)(skew ? W + (W >> 5) + 1 : W);
  const dim3 grid((unsigned)tiles, (unsigned)B), block(RSS_THREADS);
  hipStream_t s = mfpa_stream(stream);
  if (skew) hipLaunchKernelGGL((resample_sparse_kernel<true>), grid, block, lds, s, x, T, ldx, o, n, width, support, tile, (int)W, taps, first, y, Tout, ldy);
  else hipLaunchKernelGGL((resample_sparse_kernel<false>), grid, block, lds, s, x, T, ldx, o, n, width, support, tile, (int)W, taps, first, y, Tout, ldy);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
