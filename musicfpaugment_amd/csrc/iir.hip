// Recursive (IIR) filtering for MI355X (gfx950): scipy.signal.sosfilt -- a cascade of S <= 8 second-order sections in transposed
// direct form II, float64 state and arithmetic, float32 or float64 samples (include/mfpa.h has the formula).
//
// Mapping: one wavefront = one row, two rows per 128-thread workgroup, no atomics, no workgroup barrier; a row's bits do not depend
// on the batch it sits in.  The wavefront walks its row in super-chunks of 64 lanes x L = 16 samples, lane l owning the 16
// consecutive samples c0 + 16 l ...; they stay in registers (16 doubles) through all S sections.  Per section:
//   1. zero-state pass: the lane runs the recurrence over its 16 samples from state (0, 0) and keeps the end state e_l; samples past
//      T are zeros;
//   2. carry: the lane's true start state obeys s_{l+1} = M s_l + e_l with M = A^16, A = [[-a1, 1], [-a2, 0]], s_0 = the row's carry
//      (zi at the start).  An inclusive shuffle scan v_l += M^(2^k) v_{l - 2^k}, k = 0..5, over the e_l leaves the zero-carry part of
//      s_{l+1} in lane l; one shuffle up, plus the carry propagated in ONE product, s_l = M^l carry + v_{l-1}.  (Folding the carry
//      into lane 0 and letting the scan propagate it through up to six products costs 10-20 times scipy's error for an initial
//      state far from the filter's own trajectories, a random zi for one.);
//   3. true pass: the lane reruns its 16 samples from s_l and leaves the section's output in its registers: the next section's
//      input.  The state after the super-chunk's last real sample (lane 63's end state, or in the last super-chunk the state after
//      sample T - 1, never after the zero padding) is the section's carry into the next super-chunk, and at the end zf.  It comes from
//      the true pass, i.e. from the recurrence itself, not from the scan.
// The powers M^j = A^(16 j), j = 1..64, are NOT formed by squaring A: sos_powers_kernel runs the section's own homogeneous recurrence
// (x = 0) from the unit states (1, 0) and (0, 1) for 64 * 16 steps, one lane per section and unit state, and keeps the states after
// every 16 steps as the columns of M^j.  Squaring loses 13-29 times scipy's own error on low-frequency sections (poles next to z = 1); the
// recurrence's powers carry the rounding the filter itself has and stay at 0.6-1.9 times.
//
// Arithmetic: this file is compiled with -ffp-contract=off (csrc/build.py): every product and sum below is rounded on its own, in the
// order written, which is scipy's own order, y = b0 x + z1; z1 = (b1 x - a1 y) + z2; z2 = b2 x - a2 y.  tests/_iir_oracle.py restates the
// kernel in numpy operation for operation and is compared with it bit for bit, which fused multiply-adds would not allow; the price is
// nine float64 operations per sample and pass instead of five fused ones.
//
// Loads and stores: a lane owns 16 CONSECUTIVE samples, so the super-chunk is loaded coalesced (16 loads of 64 consecutive elements:
// every wavefront access is one contiguous 256 or 512 bytes) and transposed through LDS.  Sample p of the super-chunk lies at double
// (p / 16) * 17 + p % 16: the lane's own 16 doubles are read with ds_read_b64 at a stride of 17 doubles = 34 banks, so the 32 lanes of
// a half-wave hit 32 different bank pairs (34 l mod 64 is 4m for l = 2m and 4m + 34 for l = 2m + 1): conflict free, where a stride of
// 16 doubles would be 16-way.  The loads are element-wide, not 16-byte: rows start at any sample (T is arbitrary), and the kernel is
// bound by one wavefront's serial float64 arithmetic, not by HBM (one read and one write of the row; the time is the same for 64 and
// for 256 rows: DESIGN.md section 3.15).  The next super-chunk's loads are issued before the sections of the current one run and land
// in LDS before the current one's stores are issued.  Each lane's own power M^l of every section sits in LDS too (25 KB per row with
// the tile, hence two rows per workgroup).  One wavefront per row: splitting a row over the waves of a workgroup was not built.
#include "mfpa_sos.h"

// The geometry (L, SUPER, LDS_STRIDE, POWER_DOUBLES), sos_powers_kernel and one section's pass (sos_section) live in mfpa_sos.h, which
// loudness.hip shares.
namespace {

constexpr int ROWS_PER_BLOCK = 2;

template <typename T>
__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void sosfilt_kernel(const T* __restrict__ x, int B, long long n, const double* __restrict__ sos,
                                                                      int S, int sos_per_row, const unsigned char* __restrict__ apply,
                                                                      const double* __restrict__ zi, double* __restrict__ zf, int clamp,
                                                                      const double* __restrict__ powers, T* __restrict__ y) {
  __shared__ double tiles[ROWS_PER_BLOCK][MFPA_WAVE * LDS_STRIDE];
  __shared__ __attribute__((aligned(16))) double lane_powers[ROWS_PER_BLOCK][MFPA_SOS_MAX_SECTIONS * MFPA_WAVE * 4];
  const int lane = threadIdx.x & (MFPA_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = blockIdx.x * ROWS_PER_BLOCK + wave;
  if (row >= B) return;                                   // whole wavefronts leave: nothing below waits for them
  const T* xr = x + (size_t)row * n;
  T* yr = y + (size_t)row * n;
  double* tile = tiles[wave];
  double* own_powers = lane_powers[wave] + lane * 4;      // M^lane of section s at + s * 256: written and read by this lane only

  // lane s < S keeps section s's carry (and, at the end, its final state)
  double c1 = 0.0, c2 = 0.0;
  if (zi && lane < S) {
    c1 = zi[((size_t)row * S + lane) * 2];
    c2 = zi[((size_t)row * S + lane) * 2 + 1];
  }
  if (apply && !apply[row]) {                             // the gate: the row itself, bit for bit, and its state unchanged
    for (long long i = lane; i < n; i += MFPA_WAVE) yr[i] = xr[i];
    if (zf && lane < S) {
      zf[((size_t)row * S + lane) * 2] = c1;
      zf[((size_t)row * S + lane) * 2 + 1] = c2;
    }
    return;
  }
  const double* coef = sos + (sos_per_row ? (size_t)row * S * 6 : 0);
  const double* pw = powers + (sos_per_row ? (size_t)row * S * POWER_DOUBLES : 0);

  // loads past the row's end are made at its last sample instead and zeroed when they go to LDS: every load is unconditional, so
  // the sixteen are in flight together (a guarded load is waited for at once, to be merged with its zero)
  T raw[L];
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const long long g = (long long)j * MFPA_WAVE + lane;
    raw[j] = xr[g < n ? g : n - 1];
  }
  // the lane's own power of every section goes to LDS once: read from global memory inside the section loop, its latency (and a wait
  // for every load and store in flight) would sit in every section of every super-chunk
  for (int s = 0; s < S; ++s) {
    const double* q = pw + s * POWER_DOUBLES + 4 * (lane ? lane - 1 : 0);
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
    // the super-chunk's last real sample: lane 63's sixteenth, or sample n - 1
    const bool last = c0 + SUPER >= n;
    const int tail = last ? (int)(n - 1 - c0) : SUPER - 1;
    const int tail_lane = tail >> 4, tail_i = tail & (L - 1);

    for (int s = 0; s < S; ++s) {
      const double k1 = __shfl(c1, s), k2 = __shfl(c2, s);
      double f1, f2;
      sos_section(v, coef + s * 6, pw + s * POWER_DOUBLES, own_powers + s * MFPA_WAVE * 4, k1, k2, lane, tail_lane, tail_i, f1, f2);
      if (lane == s) {
        c1 = f1;
        c2 = f2;
      }
    }

#pragma unroll
    for (int i = 0; i < L; ++i) tile[lane * LDS_STRIDE + i] = v[i];
    wave_sync();
#pragma unroll
    for (int j = 0; j < L; ++j) v[j] = tile[lds_slot(j * MFPA_WAVE + lane)];
    wave_sync();
    // the next super-chunk goes into LDS BEFORE this one's stores are issued: waiting for its loads then waits for nothing younger,
    // and the stores drain under the next super-chunk's arithmetic (waiting at the top of the loop would wait for them too)
#pragma unroll
    for (int j = 0; j < L; ++j) tile[lds_slot(j * MFPA_WAVE + lane)] = c0 + SUPER + (long long)j * MFPA_WAVE + lane < n ? (double)raw[j] : 0.0;
    wave_sync();
#pragma unroll
    for (int j = 0; j < L; ++j) {
      const long long g = c0 + (long long)j * MFPA_WAVE + lane;
      double o = v[j];
      if (clamp) o = o < -1.0 ? -1.0 : (o > 1.0 ? 1.0 : o);      // a NaN stays a NaN, like torch.clamp
      if (g < n) yr[g] = (T)o;
    }
  }
  if (zf && lane < S) {
    zf[((size_t)row * S + lane) * 2] = c1;
    zf[((size_t)row * S + lane) * 2 + 1] = c2;
  }
}

bool sos_shape_ok(int B, int S, int sos_per_row) {
  return B >= 0 && B <= 65535 && S >= 1 && S <= MFPA_SOS_MAX_SECTIONS && (sos_per_row == 0 || sos_per_row == 1);
}

long long sos_work_len(int B, int S, int sos_per_row) { return (long long)(sos_per_row ? B : (B > 0 ? 1 : 0)) * S * POWER_DOUBLES; }

}  // namespace

extern "C" {

int mfpa_sosfilt_work(int B, int S, int sos_per_row, long long* work_len) {
  if (!work_len || !sos_shape_ok(B, S, sos_per_row)) return MFPA_EINVAL;
  *work_len = sos_work_len(B, S, sos_per_row);
  return MFPA_OK;
}

int mfpa_sosfilt(const void* x, int x_f64, int B, long long T, const double* sos, int S, int sos_per_row, const unsigned char* apply,
                 const double* zi, double* zf, int clamp, double* work, long long work_len, void* y, void* stream) {
  if (!sos_shape_ok(B, S, sos_per_row) || T < 1 || T > (1LL << 30) || (x_f64 != 0 && x_f64 != 1) || (clamp != 0 && clamp != 1) ||
      work_len < sos_work_len(B, S, sos_per_row))
    return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!x || !y || !sos || !work) return MFPA_EINVAL;
  const uintptr_t elem = x_f64 ? 7 : 3;
  if ((reinterpret_cast<uintptr_t>(x) & elem) || (reinterpret_cast<uintptr_t>(y) & elem) || (reinterpret_cast<uintptr_t>(sos) & 7) ||
      (reinterpret_cast<uintptr_t>(work) & 7) || (reinterpret_cast<uintptr_t>(zi) & 7) || (reinterpret_cast<uintptr_t>(zf) & 7))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const int n_pow = (sos_per_row ? B : 1) * S * 2;
  hipLaunchKernelGGL(sos_powers_kernel, dim3((n_pow + 63) / 64), dim3(64), 0, st, sos, n_pow, work);
  MFPA_CHECK_LAUNCH();
  const dim3 grid((B + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK), block(64 * ROWS_PER_BLOCK);
  if (x_f64)
    hipLaunchKernelGGL(sosfilt_kernel<double>, grid, block, 0, st, static_cast<const double*>(x), B, T, sos, S, sos_per_row, apply, zi, zf,
                       clamp, work, static_cast<double*>(y));
  else
    hipLaunchKernelGGL(sosfilt_kernel<float>, grid, block, 0, st, static_cast<const float*>(x), B, T, sos, S, sos_per_row, apply, zi, zf,
                       clamp, work, static_cast<float*>(y));
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
