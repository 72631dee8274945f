// Chunking of whole tracks into model-length training segments for MI355X (gfx950): the stage between the resampler and AugmentFP.
// Reference: deezer/musicFPaugment training/dataset.py:55-122 (peak normalisation, tf.signal.frame without end padding, the RMS
// silence rule of select_no_silence_frames, shuffle(kept)[:n_segments]) and testing/generate_queries.py:43-49 (one crop per track).
//
// Tracks sit back to back in one float32 buffer `bank`; track i owns bank[off[i] .. off[i] + len[i]).  With frame length L and
// step S a track of N samples has nf = 1 + (N - L) / S segments (0 when N < L); seg_off is the exclusive prefix of nf.
//
//   seg_sumsq_kernel   a workgroup owns one UNIT at a time: a segment, or a track's remainder (S == L: the tail no segment
//                      covers; otherwise the whole track).  Inside a unit thread t owns the quads q = t, t + 256, ... of four
//                      consecutive samples COUNTED FROM THE UNIT'S FIRST SAMPLE, one float64 accumulator per position in the
//                      quad, acc = fma(x, x, acc) in ascending q (the square of a float32 is exact in float64: one rounding per
//                      sample); then a fixed combine: positions 0..3, the wave's xor tree, the four waves in order.  Nothing
//                      in that order depends on the address of the unit, on the other tracks of the call or on the grid, so
//                      a sum is bit for bit a function of the unit's samples.  The quads are loaded as 16-byte vectors at
//                      4-byte alignment (global_load_dwordx4 needs no more), whatever off[i] is.  The grid is a fixed number of
//                      workgroups that stride over the units: the host never reads seg_off.
//                      max|x| goes to trk_peak by an INTEGER atomic max on the bit pattern (order-free, hence exact).
//   trk_total_kernel   S == L only: a track's sum = its segments' sums (lane l takes j = l, l + 64, ... ascending, xor tree)
//                      + its tail, so the audio is read once.
//   select_kernel      a workgroup owns a track: the keep test in float64, then the kept segments' (key, j) as 64-bit sort
//                      keys in LDS (mfpa_sort.h bitonic passes), silent segments and padding as all-ones behind them.
//   gather_kernel      out[r][t] = bank[src[r] + t] / div[r], 16-byte loads and stores at 4-byte alignment.
#include <limits.h>

#include "mfpa_common.h"
#include "mfpa_sort.h"

namespace {

constexpr int SEG_BLOCK = 256;
constexpr int SEG_WAVES = SEG_BLOCK / 64;
constexpr int SEG_UNROLL = 4;                    // quads a thread keeps in flight
constexpr int SEG_GRID_PER_CU = 8;
constexpr int GATHER_CHUNK = SEG_BLOCK * 4 * 4;  // floats one workgroup of gather_kernel moves

// four floats at any 4-byte alignment: one global_load_dwordx4 / global_store_dwordx4
struct __attribute__((packed, aligned(4))) Quad {
  float v[4];
};
__device__ __forceinline__ Quad ld_quad(const float* p) { return *reinterpret_cast<const Quad*>(p); }
__device__ __forceinline__ void st_quad(float* p, const Quad& q) { *reinterpret_cast<Quad*>(p) = q; }

__device__ __forceinline__ double wave_sum_fixed(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);           // both partners add the same two values: every lane ends equal
  return v;
}

__device__ __forceinline__ float wave_maxf(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

__host__ __device__ __forceinline__ long long seg_count(long long N, long long L, long long S) { return N >= L ? 1 + (N - L) / S : 0; }

// sum of squares (and max|x|) of x[0, n): every thread of the workgroup returns the same values; ends on a barrier
__device__ __forceinline__ double unit_sumsq(const float* __restrict__ x, long long n, double* sh_sum, float* sh_max, float* peak) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  float m = 0.f;
  const long long nq = n >> 2;                                       // whole quads
  long long q = tid;
  for (; q + (long long)(SEG_UNROLL - 1) * SEG_BLOCK < nq; q += (long long)SEG_UNROLL * SEG_BLOCK) {
    Quad v[SEG_UNROLL];
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) v[u] = ld_quad(x + 4 * (q + (long long)u * SEG_BLOCK));
#pragma unroll
    for (int u = 0; u < SEG_UNROLL; ++u) {
      a0 = fma((double)v[u].v[0], (double)v[u].v[0], a0);
      a1 = fma((double)v[u].v[1], (double)v[u].v[1], a1);
      a2 = fma((double)v[u].v[2], (double)v[u].v[2], a2);
      a3 = fma((double)v[u].v[3], (double)v[u].v[3], a3);
      m = fmaxf(m, fmaxf(fmaxf(fabsf(v[u].v[0]), fabsf(v[u].v[1])), fmaxf(fabsf(v[u].v[2]), fabsf(v[u].v[3]))));
    }
  }
  for (; q < nq; q += SEG_BLOCK) {
    const Quad v = ld_quad(x + 4 * q);
    a0 = fma((double)v.v[0], (double)v.v[0], a0);
    a1 = fma((double)v.v[1], (double)v.v[1], a1);
    a2 = fma((double)v.v[2], (double)v.v[2], a2);
    a3 = fma((double)v.v[3], (double)v.v[3], a3);
    m = fmaxf(m, fmaxf(fmaxf(fabsf(v.v[0]), fabsf(v.v[1])), fmaxf(fabsf(v.v[2]), fabsf(v.v[3]))));
  }
  if (q == nq) {                                                     // the thread whose turn the last, partial quad is
    const long long e = 4 * nq;
    if (e < n) { const float f = x[e]; a0 = fma((double)f, (double)f, a0); m = fmaxf(m, fabsf(f)); }
    if (e + 1 < n) { const float f = x[e + 1]; a1 = fma((double)f, (double)f, a1); m = fmaxf(m, fabsf(f)); }
    if (e + 2 < n) { const float f = x[e + 2]; a2 = fma((double)f, (double)f, a2); m = fmaxf(m, fabsf(f)); }
  }
  const double w = wave_sum_fixed((a0 + a1) + (a2 + a3));
  m = wave_maxf(m);
  __syncthreads();                                                   // the previous unit's readers are done with sh_*
  if (lane == 0) { sh_sum[wave] = w; sh_max[wave] = m; }
  __syncthreads();
  double total = sh_sum[0];
  float mm = sh_max[0];
#pragma unroll
  for (int k = 1; k < SEG_WAVES; ++k) { total += sh_sum[k]; mm = fmaxf(mm, sh_max[k]); }
  *peak = mm;
  return total;
}

// binary search: the track whose segments include global segment g (seg_off is non-decreasing, seg_off[n_tracks] > g)
__device__ __forceinline__ int track_of(const int* __restrict__ seg_off, int n_tracks, int g) {
  int lo = 0, hi = n_tracks;                                         // seg_off[lo] <= g < seg_off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (seg_off[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ MFPA_NO_PK_F32 __launch_bounds__(SEG_BLOCK) void seg_sumsq_kernel(const float* __restrict__ bank, const long long* __restrict__ off,
                                                                             const long long* __restrict__ len, const int* __restrict__ seg_off,
                                                                             int n_tracks, long long L, long long S, double* __restrict__ seg_sumsq,
                                                                             double* __restrict__ trk_sumsq, float* __restrict__ trk_peak) {
  __shared__ double sh_sum[SEG_WAVES];
  __shared__ float sh_max[SEG_WAVES];
  const long long NS = seg_off[n_tracks];
  const long long units = NS + n_tracks;
  const bool once = S == L;
  for (long long u = blockIdx.x; u < units; u += gridDim.x) {
    int i;
    const float* x;
    long long n;
    bool is_seg = u < NS;
    if (is_seg) {
      i = track_of(seg_off, n_tracks, (int)u);
      x = bank + off[i] + (u - seg_off[i]) * S;
      n = L;
    } else {
      i = (int)(u - NS);
      const long long N = len[i];
      const long long covered = once ? seg_count(N, L, S) * L : 0;   // S == L: the segments tile [0, nf * L)
      x = bank + off[i] + covered;
      n = N - covered;
    }
    float peak;
    const double sum = unit_sumsq(x, n, sh_sum, sh_max, &peak);
    if (threadIdx.x == 0) {
      if (is_seg) seg_sumsq[u] = sum; else trk_sumsq[i] = sum;       // S == L: the tail for now, trk_total_kernel adds the segments
      if ((once || !is_seg) && peak > 0.f) atomicMax(reinterpret_cast<unsigned int*>(trk_peak + i), __float_as_uint(peak));
    }
  }
}

__global__ MFPA_NO_PK_F32 __launch_bounds__(64) void trk_total_kernel(const int* __restrict__ seg_off, const double* __restrict__ seg_sumsq,
                                                                      double* __restrict__ trk_sumsq) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int j0 = seg_off[i], j1 = seg_off[i + 1];
  double a = 0.0;
  for (int j = j0 + lane; j < j1; j += 64) a += seg_sumsq[j];
  a = wave_sum_fixed(a);
  if (lane == 0) trk_sumsq[i] = a + trk_sumsq[i];
}

__global__ MFPA_NO_PK_F32 __launch_bounds__(SEG_BLOCK) void select_kernel(const double* __restrict__ seg_sumsq, const double* __restrict__ trk_sumsq,
                                                                          const float* __restrict__ trk_peak, const long long* __restrict__ off,
                                                                          const long long* __restrict__ len, const int* __restrict__ seg_off,
                                                                          long long L, long long S, const unsigned int* __restrict__ keys, double thr,
                                                                          int n_keep, int do_norm, int* __restrict__ sel, long long* __restrict__ src,
                                                                          float* __restrict__ div, int* __restrict__ kept, unsigned char* __restrict__ mask) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];   // P sort keys, then one counter
  const int i = blockIdx.x, tid = threadIdx.x;
  const int g0 = seg_off[i], nf = seg_off[i + 1] - g0;
  int P = 1;
  while (P < nf) P <<= 1;                                            // nf <= MFPA_SEGMENT_MAX_PER_TRACK: the caller's seg_off comes from mfpa_segment_geometry
  if (P > MFPA_SEGMENT_MAX_PER_TRACK) P = MFPA_SEGMENT_MAX_PER_TRACK;
  int* count = reinterpret_cast<int*>(sk + MFPA_SEGMENT_MAX_PER_TRACK);
  if (tid == 0) *count = 0;
  __syncthreads();
  const double rhs = thr * trk_sumsq[i] * (double)L;
  const double n = (double)len[i];
  int mine = 0;
  for (int j = tid; j < P; j += SEG_BLOCK) {
    unsigned long long k = ~0ull;
    if (j < nf) {
      const bool keep = seg_sumsq[g0 + j] * n > rhs;                 // false for an all-zero track (0 > 0) and for NaN
      if (mask) mask[g0 + j] = keep ? 1 : 0;
      if (keep) { k = ((unsigned long long)keys[g0 + j] << 32) | (unsigned int)j; ++mine; }
    }
    sk[j] = k;
  }
  if (mine) atomicAdd(count, mine);                                  // an integer count: order-free
  __syncthreads();
  for (long long k = 2; k <= P; k <<= 1) mfpa_sort::lds_bitonic<SEG_BLOCK>(sk, P, 0, k, (int)(k >> 1));
  if (tid == 0) kept[i] = *count;
  const float pk = trk_peak[i];
  const float d = (do_norm && pk > 0.f) ? pk : 1.f;
  for (int k = tid; k < n_keep; k += SEG_BLOCK) {
    const long long r = (long long)i * n_keep + k;
    const unsigned long long key = k < P ? sk[k] : ~0ull;
    if (key != ~0ull) {
      const int j = (int)(key & 0xffffffffull);
      sel[r] = g0 + j;
      src[r] = off[i] + (long long)j * S;
    } else {
      sel[r] = -1;
      src[r] = -1;
    }
    div[r] = d;
  }
}

__global__ MFPA_NO_PK_F32 __launch_bounds__(SEG_BLOCK) void gather_kernel(const float* __restrict__ bank, const long long* __restrict__ src,
                                                                          const float* __restrict__ div, long long L, float* __restrict__ out,
                                                                          long long ldo) {
  const long long r = blockIdx.x;
  const long long s = src[r];
  if (s < 0) return;
  const float d = div ? div[r] : 1.f;
  const float* x = bank + s;
  float* y = out + r * ldo;
  const long long t0 = (long long)blockIdx.y * GATHER_CHUNK;
  const long long t1 = t0 + GATHER_CHUNK < L ? t0 + GATHER_CHUNK : L;
  const long long nq = (t1 - t0) >> 2;
  Quad v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long q = threadIdx.x + (long long)u * SEG_BLOCK;
    if (q < nq) v[u] = ld_quad(x + t0 + 4 * q);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const long long q = threadIdx.x + (long long)u * SEG_BLOCK;
    if (q < nq) {
      if (div) {
#pragma unroll
        for (int c = 0; c < 4; ++c) v[u].v[c] = __fdiv_rn(v[u].v[c], d);
      }
      st_quad(y + t0 + 4 * q, v[u]);
    }
  }
  const long long e = t0 + 4 * nq + threadIdx.x;                     // at most three samples behind the last whole quad
  if (threadIdx.x < 3 && e < t1) y[e] = div ? __fdiv_rn(x[e], d) : x[e];
}

inline bool seg_shape_ok(long long L, long long S) { return L >= 1 && S >= 1 && L <= MFPA_SEGMENT_MAX_LENGTH && S <= MFPA_SEGMENT_MAX_LENGTH; }

}  // namespace

extern "C" {

int mfpa_segment_geometry(const long long* len, int n_tracks, long long L, long long S, int* seg_off) {
  if (!seg_off || n_tracks < 0 || (n_tracks > 0 && !len) || !seg_shape_ok(L, S)) return MFPA_EINVAL;
  long long total = 0;
  for (int i = 0; i < n_tracks; ++i) {
    if (len[i] < 0) return MFPA_EINVAL;
    const long long nf = seg_count(len[i], L, S);
    if (nf > MFPA_SEGMENT_MAX_PER_TRACK) return MFPA_EINVAL;
    if (total + nf > INT_MAX) return MFPA_EINVAL;
    seg_off[i] = (int)total;
    total += nf;
  }
  seg_off[n_tracks] = (int)total;
  return MFPA_OK;
}

int mfpa_segment_stats(const float* bank, const long long* off, const long long* len, const int* seg_off, int n_tracks, long long L,
                       long long S, double* seg_sumsq, double* trk_sumsq, float* trk_peak, void* stream) {
  if (n_tracks < 0 || !seg_shape_ok(L, S)) return MFPA_EINVAL;
  if (n_tracks == 0) return MFPA_OK;
  if (!bank || !off || !len || !seg_off || !seg_sumsq || !trk_sumsq || !trk_peak) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  MFPA_HIP(hipMemsetAsync(trk_peak, 0, sizeof(float) * (size_t)n_tracks, s));
  int cus = mfpa_current_device_cus();
  if (cus < 1) cus = 1;
  hipLaunchKernelGGL(seg_sumsq_kernel, dim3((unsigned)(cus * SEG_GRID_PER_CU)), dim3(SEG_BLOCK), 0, s, bank, off, len, seg_off, n_tracks, L, S,
                     seg_sumsq, trk_sumsq, trk_peak);
  MFPA_CHECK_LAUNCH();
  if (S == L) {
    hipLaunchKernelGGL(trk_total_kernel, dim3((unsigned)n_tracks), dim3(64), 0, s, seg_off, seg_sumsq, trk_sumsq);
    MFPA_CHECK_LAUNCH();
  }
  return MFPA_OK;
}

int mfpa_segment_select(const double* seg_sumsq, const double* trk_sumsq, const float* trk_peak, const long long* off, const long long* len,
                        const int* seg_off, int n_tracks, long long L, long long S, const unsigned int* keys, double thr, int n_keep,
                        int do_norm, int* sel, long long* src, float* div, int* kept, unsigned char* mask, void* stream) {
  if (n_tracks < 0 || n_keep < 1 || !seg_shape_ok(L, S) || !(thr >= 0.0) || (long long)n_tracks * n_keep > INT_MAX) return MFPA_EINVAL;
  if (n_tracks == 0) return MFPA_OK;
  if (!seg_sumsq || !trk_sumsq || !trk_peak || !off || !len || !seg_off || !keys || !sel || !src || !div || !kept) return MFPA_EINVAL;
  const size_t lds = sizeof(unsigned long long) * MFPA_SEGMENT_MAX_PER_TRACK + 16;
  hipLaunchKernelGGL(select_kernel, dim3((unsigned)n_tracks), dim3(SEG_BLOCK), lds, mfpa_stream(stream), seg_sumsq, trk_sumsq, trk_peak, off, len,
                     seg_off, L, S, keys, thr, n_keep, do_norm, sel, src, div, kept, mask);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_segment_gather(const float* bank, const long long* src, const float* div, long long rows, long long L, float* out, long long ldo,
                        void* stream) {
  if (rows < 0 || rows > INT_MAX || L < 1 || L > MFPA_SEGMENT_MAX_LENGTH || ldo < L) return MFPA_EINVAL;
  if (rows == 0) return MFPA_OK;
  if (!bank || !src || !out) return MFPA_EINVAL;
  const dim3 grid((unsigned)rows, (unsigned)((L + GATHER_CHUNK - 1) / GATHER_CHUNK));
  hipLaunchKernelGGL(gather_kernel, grid, dim3(SEG_BLOCK), 0, mfpa_stream(stream), bank, src, div, L, out, ldo);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
