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
#include <math.h>

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
  const double pi = 3.14159265358979323846;
  const double base = (double)(o < n ? o : n) * rolloff;
  const double lpw = (double)lowpass_filter_width, scale = base / (double)o;
  for (int i = 0; i < n; ++i) {
    const double phase = (double)((float)(-i) / (float)n);           // torchaudio forms the phase offset in float32
    for (int k = 0; k < K; ++k) {
      double t = (phase + (double)(k - width) / (double)o) * base;
      t = t < -lpw ? -lpw : (t > lpw ? lpw : t);
      const double c = cos(t * pi / lpw / 2.0);
      const double win = c * c;
      t *= pi;
      const double sinc = t == 0.0 ? 1.0 : sin(t) / t;
      taps[(size_t)i * pitch + k] = (float)(sinc * win * scale);
    }
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

}  // extern "C"
