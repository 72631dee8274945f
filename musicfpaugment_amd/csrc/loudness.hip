// Programme loudness for MI355X (gfx950): the meter of ITU-R BS.1770 / EBU R 128 (include/mfpa.h has the definition).
//
// loudness_segments_kernel: K-weighting and segment energies without writing the filtered signal.  The mapping is sosfilt_kernel's
// (iir.hip, mfpa_sos.h): one wavefront = one row, two rows per 128-thread workgroup, super-chunks of 64 lanes x 16 samples, each
// section a zero-state pass, a shuffle scan with the stored powers, the carry and a true pass.  The filtered samples stay in
// registers: each lane squares its 16 and, for every segment that overlaps the super-chunk, adds those of its squares that fall in
// the segment by a pairwise tree (the others replaced by 0, which adds exactly; depth 4, not a chain of 16 dependent additions) to
// its own running sum of the segment, which starts at 0 and stays in a register from one super-chunk to the next.  When the segment
// ends, the 64 running sums are combined by a butterfly over the lanes (offsets 1, 2, ..., 32: a fixed binary tree over the lane
// index): one butterfly per segment, not per super-chunk.  A lane may straddle a boundary, a segment may span many super-chunks, a
// super-chunk may hold many segments: the loop over the segments of a super-chunk is uniform in the wavefront.  No atomics, no work buffer but the powers; a row's bits do not depend on R, on its position or on the grid.
// The peak is fmax over |x| of the unfiltered input (a NaN sample loses).  One wavefront per row: splitting a row over the waves of a
// workgroup was not built.
//
// loudness_gate_kernel: one 256-thread workgroup per example; block powers are recomputed from the segment sums in each of the two
// passes (absolute gate, relative gate) in the same operations, so both passes see the same doubles.  Thread t sums the blocks
// j = t, t + 256, ... that pass, in increasing j; the 256 partial sums are combined by a tree in LDS (offsets 128, 64, ..., 1).  With
// range ranks wanted (a second instantiation, 128 KiB of LDS) the twice-gated powers are sorted in LDS (mfpa_sort.h), the others
// replaced by +inf.  No logarithm anywhere: every decision is taken on powers.
//
// loudness_apply_kernel: the gain from the gated power and the peak on the device (sqrt and division, both correctly rounded), and a
// streaming multiply in float64.
//
// Built with -ffp-contract=off (csrc/build.py): tests/_loudness_oracle.py restates all three kernels operation for operation.
#include "mfpa_sort.h"
#include "mfpa_sos.h"

namespace {

constexpr int ROWS_PER_BLOCK = 2;
constexpr int GATE_BLOCK = 256;
constexpr int APPLY_BLOCK = 256;

template <typename T>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void loudness_segments_kernel(const T* __restrict__ x, int R, long long n, const double* __restrict__ sos,
                                                                                int S, const double* __restrict__ powers, int hop, long long nseg,
                                                                                double* __restrict__ seg, double* __restrict__ peak) {
  __shared__ double tiles[ROWS_PER_BLOCK][MFPA_WAVE * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) double lane_powers[ROWS_PER_BLOCK][MFPA_SOS_MAX_SECTIONS * MFPA_WAVE * 4];
  const int lane = threadIdx.x & (MFPA_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = blockIdx.x * ROWS_PER_BLOCK + wave;
  if (row >= R) return;                                   // whole wavefronts leave: nothing below waits for them
  const T* xr = x + (size_t)row * n;
  double* sr = seg + (size_t)row * nseg;
  double* tile = tiles[wave];
  double* own_powers = lane_powers[wave] + lane * 4;      // M^lane of section s at + s * 256: written and read by this lane only

  double c1 = 0.0, c2 = 0.0;                              // lane s < S keeps section s's carry
  double pk = 0.0;
  // the segment that is open at the start of a super-chunk: its index and its first sample (the same in every lane) and this lane's
  // running sum of it
  long long k = 0, ks = 0;
  double acc = 0.0;

  T raw[L];
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const long long g = (long long)j * MFPA_WAVE + lane;
    raw[j] = xr[g < n ? g : n - 1];
  }
  for (int s = 0; s < S; ++s) {
    const double* q = powers + s * POWER_DOUBLES + 4 * (lane ? lane - 1 : 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) own_powers[s * MFPA_WAVE * 4 + e] = q[e];
  }
#pragma unroll
  for (int j = 0; j < L; ++j) tile[lds_slot(j * MFPA_WAVE + lane)] = (long long)j * MFPA_WAVE + lane < n ? (double)raw[j] : 0.0;
  wave_sync();
  for (long long c0 = 0; c0 < n; c0 += SUPER) {           // c0 and n are the same in every lane: the wavefront stays whole
    double v[L];
#pragma unroll
    for (int i = 0; i < L; ++i) v[i] = tile[lane * LDS_STRIDE + i];
    wave_sync();
#pragma unroll
    for (int j = 0; j < L; ++j) {                          // the next super-chunk
      const long long g = c0 + SUPER + (long long)j * MFPA_WAVE + lane;
      raw[j] = xr[g < n ? g : n - 1];
    }
#pragma unroll
    for (int i = 0; i < L; ++i) pk = fmax(pk, fabs(v[i])); // the padding is zeros

    for (int s = 0; s < S; ++s) {
      const double k1 = __shfl(c1, s), k2 = __shfl(c2, s);
      double f1, f2;
      sos_section(v, sos + s * 6, powers + s * POWER_DOUBLES, own_powers + s * MFPA_WAVE * 4, k1, k2, lane, MFPA_WAVE - 1, L - 1, f1, f2);
      if (lane == s) {
        c1 = f1;
        c2 = f2;
      }
    }

#pragma unroll
    for (int i = 0; i < L; ++i) v[i] = v[i] * v[i];
    const long long base = c0 + (long long)lane * L, c_end = c0 + SUPER;
    while (k < nseg && ks < c_end) {                       // uniform: k, ks, nseg and c_end are
      const long long ke = ks + hop, dlo = ks - base, dhi = ke - base;
      const int lo = dlo < 0 ? 0 : (dlo > L ? L : (int)dlo), hi = dhi < 0 ? 0 : (dhi > L ? L : (int)dhi);
      double m[L];
#pragma unroll
      for (int i = 0; i < L; ++i) m[i] = (i >= lo && i < hi) ? v[i] : 0.0;   // selected, not multiplied: a NaN outside the segment stays out
#pragma unroll
      for (int w = 1; w < L; w <<= 1)
#pragma unroll
        for (int i = 0; i < L; i += 2 * w) m[i] = m[i] + m[i + w];
      acc = acc + m[0];
      if (ke > c_end) break;                               // the segment goes on in the next super-chunk
      double q = acc;
#pragma unroll
      for (int o = 1; o < MFPA_WAVE; o <<= 1) q = q + __shfl_xor(q, o);
      if (lane == (int)(k & (MFPA_WAVE - 1))) sr[k] = q;
      acc = 0.0;
      ++k;
      ks = ke;
    }

#pragma unroll
    for (int j = 0; j < L; ++j) tile[lds_slot(j * MFPA_WAVE + lane)] = c0 + SUPER + (long long)j * MFPA_WAVE + lane < n ? (double)raw[j] : 0.0;
    wave_sync();
  }
  if (peak) {
    pk = mfpa_wave_max(pk);
    if (lane == 0) peak[row] = pk;
  }
}

// p[j]: k increasing inside the block, then c increasing; d = win * hop.
__device__ __forceinline__ double block_power(const double* __restrict__ seg, int C, long long nseg, const double* __restrict__ weights, int win,
                                              double d, long long j) {
  double p = 0.0;
  for (int c = 0; c < C; ++c) {
    const double* s = seg + (size_t)c * nseg + j;
    double a = s[0];
    for (int i = 1; i < win; ++i) a = a + s[i];
    const double t = (weights ? weights[c] : 1.0) * (a / d);
    p = c ? p + t : t;
  }
  return p;
}

// Sum over the workgroup by the tree with offsets 128, 64, ..., 1; every thread gets it.
template <typename V>
__device__ __forceinline__ V gate_tree_sum(V v, V* sh) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = GATE_BLOCK / 2; off > 0; off >>= 1) {
    if (tid < off) sh[tid] = sh[tid] + sh[tid + off];
    __syncthreads();
  }
  const V r = sh[0];
  __syncthreads();
  return r;
}

template <bool RANGE>
__global__ __launch_bounds__(GATE_BLOCK) void loudness_gate_kernel(const double* __restrict__ seg, int C, long long nseg, int nb, int win, double d,
                                                                   const double* __restrict__ weights, double p_abs, double rel,
                                                                   double* __restrict__ power, int* __restrict__ counts, double* __restrict__ blocks,
                                                                   double* __restrict__ range) {
  __shared__ double shd[GATE_BLOCK];
  __shared__ int shi[GATE_BLOCK];
  __shared__ double sk[RANGE ? MFPA_LOUDNESS_MAX_RANGE_BLOCKS : 1];
  const int tid = threadIdx.x, b = blockIdx.x;
  const double* sb = seg + (size_t)b * C * nseg;

  double sum = 0.0;
  int cnt = 0;
  for (int j = tid; j < nb; j += GATE_BLOCK) {
    const double p = block_power(sb, C, nseg, weights, win, d, j);
    if (blocks) blocks[(size_t)b * nb + j] = p;
    if (p > p_abs) {                                       // a NaN fails
      sum = sum + p;
      ++cnt;
    }
  }
  const int n_abs = gate_tree_sum(cnt, shi);
  const double s_abs = gate_tree_sum(sum, shd);
  const double mean_abs = n_abs ? s_abs / (double)n_abs : 0.0;
  const double thr = rel * mean_abs;

  sum = 0.0;
  cnt = 0;
  for (int j = tid; j < nb; j += GATE_BLOCK) {
    const double p = block_power(sb, C, nseg, weights, win, d, j);
    const bool pass = p > p_abs && p > thr;
    if (pass) {
      sum = sum + p;
      ++cnt;
    }
    if (RANGE) sk[j] = pass ? p : __builtin_huge_val();
  }
  const int n_rel = gate_tree_sum(cnt, shi);
  const double s_rel = gate_tree_sum(sum, shd);
  if (tid == 0) {
    power[2 * b] = n_rel ? s_rel / (double)n_rel : 0.0;
    power[2 * b + 1] = mean_abs;
    counts[2 * b] = n_abs;
    counts[2 * b + 1] = n_rel;
  }
  if (RANGE) {
    int P = 2;
    while (P < nb) P <<= 1;                                // <= MFPA_LOUDNESS_MAX_RANGE_BLOCKS, a power of two
    for (int j = nb + tid; j < P; j += GATE_BLOCK) sk[j] = __builtin_huge_val();
    __syncthreads();
    for (long long kk = 2; kk <= P; kk <<= 1) mfpa_sort::lds_bitonic<GATE_BLOCK>(sk, P, 0, kk, (int)(kk >> 1));
    if (tid == 0) {
      range[2 * b] = n_rel ? sk[(n_rel + 4) / 10] : 0.0;
      range[2 * b + 1] = n_rel ? sk[(19 * n_rel - 9) / 20] : 0.0;
    }
  }
}

// blockIdx.y = row (b, c), blockIdx.x strides over the row.
template <typename T>
__global__ __launch_bounds__(APPLY_BLOCK) void loudness_apply_kernel(const T* __restrict__ x, int C, long long n, const double* __restrict__ gated,
                                                                     const double* __restrict__ target, const double* __restrict__ peak,
                                                                     double peak_limit, const unsigned char* __restrict__ apply, T* __restrict__ y,
                                                                     double* __restrict__ gain) {
  const int row = blockIdx.y, b = row / C;
  const double pg = gated[b];
  double g = __dsqrt_rn(target[b] / pg);
  if (peak) {
    double pk = peak[(size_t)b * C];
    for (int c = 1; c < C; ++c) pk = fmax(pk, peak[(size_t)b * C + c]);
    const double lim = peak_limit / pk;
    g = lim < g ? lim : g;
  }
  const bool copy = pg == 0.0 || !(fabs(g) <= 1.79769313486231570815e+308) || (apply && !apply[b]);
  const T* xr = x + (size_t)row * n;
  T* yr = y + (size_t)row * n;
  const long long step = (long long)gridDim.x * APPLY_BLOCK;
  if (copy) {
    for (long long i = (long long)blockIdx.x * APPLY_BLOCK + threadIdx.x; i < n; i += step) yr[i] = xr[i];
  } else {
    for (long long i = (long long)blockIdx.x * APPLY_BLOCK + threadIdx.x; i < n; i += step) yr[i] = (T)((double)xr[i] * g);
  }
  if (gain && blockIdx.x == 0 && threadIdx.x == 0 && row == b * C) gain[b] = copy ? 1.0 : g;
}

bool segments_shape_ok(int R, long long T, int S, int hop, int x_f64) {
  return R >= 0 && R <= 65535 && T >= 1 && T <= (1LL << 30) && S >= 0 && S <= MFPA_SOS_MAX_SECTIONS && hop >= 1 && hop <= (1 << 24) &&
         (x_f64 == 0 || x_f64 == 1);
}

}  // namespace

extern "C" {

int mfpa_loudness_work(int S, long long* work_len) {
  if (!work_len || S < 0 || S > MFPA_SOS_MAX_SECTIONS) return MFPA_EINVAL;
  *work_len = (long long)S * POWER_DOUBLES;
  return MFPA_OK;
}

int mfpa_loudness_segments(const void* x, int x_f64, int R, long long T, const double* sos, int S, int hop, double* work, long long work_len,
                           double* seg, double* peak, void* stream) {
  if (!segments_shape_ok(R, T, S, hop, x_f64) || work_len < (long long)S * POWER_DOUBLES) return MFPA_EINVAL;
  if (R == 0) return MFPA_OK;
  const long long nseg = T / hop;
  if (!x || (nseg > 0 && !seg) || (S > 0 && (!sos || !work))) return MFPA_EINVAL;
  const uintptr_t elem = x_f64 ? 7 : 3;
  if ((reinterpret_cast<uintptr_t>(x) & elem) || (reinterpret_cast<uintptr_t>(sos) & 7) || (reinterpret_cast<uintptr_t>(work) & 7) ||
      (reinterpret_cast<uintptr_t>(seg) & 7) || (reinterpret_cast<uintptr_t>(peak) & 7))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  if (S > 0) {
    hipLaunchKernelGGL(sos_powers_kernel, dim3((2 * S + 63) / 64), dim3(64), 0, st, sos, 2 * S, work);
    MFPA_CHECK_LAUNCH();
  }
  const dim3 grid((R + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(64 * ROWS_PER_BLOCK);
  if (x_f64)
    hipLaunchKernelGGL(loudness_segments_kernel<double>, grid, block, 0, st, static_cast<const double*>(x), R, T, sos, S, work, hop, nseg, seg, peak);
  else
    hipLaunchKernelGGL(loudness_segments_kernel<float>, grid, block, 0, st, static_cast<const float*>(x), R, T, sos, S, work, hop, nseg, seg, peak);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_loudness_gate(const double* seg, int B, int C, long long nseg, int hop, int win, const double* weights, double p_abs, double rel,
                       double* power, int* counts, double* blocks, double* range, void* stream) {
  if (B < 0 || B > 65535 || C < 1 || C > MFPA_LOUDNESS_MAX_CHANNELS || nseg < 0 || nseg > (1LL << 30) || hop < 1 || hop > (1 << 24) || win < 1 ||
      win > MFPA_LOUDNESS_MAX_WINDOW || !(p_abs >= 0.0 && p_abs <= 1.79769313486231570815e+308) || !(rel >= 0.0 && rel <= 1.79769313486231570815e+308))
    return MFPA_EINVAL;
  const long long nb = nseg >= win ? nseg - win + 1 : 0;
  if (range && nb > MFPA_LOUDNESS_MAX_RANGE_BLOCKS) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if ((nseg > 0 && !seg) || !power || !counts) return MFPA_EINVAL;
  if ((reinterpret_cast<uintptr_t>(seg) & 7) || (reinterpret_cast<uintptr_t>(weights) & 7) || (reinterpret_cast<uintptr_t>(power) & 7) ||
      (reinterpret_cast<uintptr_t>(counts) & 3) || (reinterpret_cast<uintptr_t>(blocks) & 7) || (reinterpret_cast<uintptr_t>(range) & 7))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const double d = (double)win * (double)hop;
  if (range)
    hipLaunchKernelGGL(loudness_gate_kernel<true>, dim3(B), dim3(GATE_BLOCK), 0, st, seg, C, nseg, (int)nb, win, d, weights, p_abs, rel, power, counts,
                       blocks, range);
  else
    hipLaunchKernelGGL(loudness_gate_kernel<false>, dim3(B), dim3(GATE_BLOCK), 0, st, seg, C, nseg, (int)nb, win, d, weights, p_abs, rel, power, counts,
                       blocks, range);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_loudness_apply(const void* x, int x_f64, int B, int C, long long T, const double* gated, const double* target, const double* peak,
                        double peak_limit, const unsigned char* apply, void* y, double* gain, void* stream) {
  if (B < 0 || B > 65535 || C < 1 || C > MFPA_LOUDNESS_MAX_CHANNELS || (long long)B * C > 65535 || T < 1 || T > (1LL << 30) ||
      (x_f64 != 0 && x_f64 != 1) || !(peak_limit >= 0.0 && peak_limit <= 1.79769313486231570815e+308) || (peak_limit > 0.0 && !peak) ||
      (peak_limit == 0.0 && peak))
    return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!x || !y || !gated || !target) return MFPA_EINVAL;
  const uintptr_t elem = x_f64 ? 7 : 3;
  if ((reinterpret_cast<uintptr_t>(x) & elem) || (reinterpret_cast<uintptr_t>(y) & elem) || (reinterpret_cast<uintptr_t>(gated) & 7) ||
      (reinterpret_cast<uintptr_t>(target) & 7) || (reinterpret_cast<uintptr_t>(peak) & 7) || (reinterpret_cast<uintptr_t>(gain) & 7))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const long long per_row = (T + APPLY_BLOCK * 4 - 1) / (APPLY_BLOCK * 4);
  const dim3 grid((unsigned)(per_row < 1024 ? per_row : 1024), (unsigned)(B * C));
  if (x_f64)
    hipLaunchKernelGGL(loudness_apply_kernel<double>, grid, dim3(APPLY_BLOCK), 0, st, static_cast<const double*>(x), C, T, gated, target, peak,
                       peak_limit, apply, static_cast<double*>(y), gain);
  else
    hipLaunchKernelGGL(loudness_apply_kernel<float>, grid, dim3(APPLY_BLOCK), 0, st, static_cast<const float*>(x), C, T, gated, target, peak,
                       peak_limit, apply, static_cast<float*>(y), gain);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
