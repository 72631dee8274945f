// Phase vocoder for MI355X (gfx950): torchaudio.functional.phase_vocoder at the library's fixed geometry (257 bins, hop 256), one
// rate per clip, float64 throughout (include/mfpa.h has the formula).
//
// Mapping: one wavefront = one row (b, k) of the spectrum, which is contiguous in memory; four rows per 256-thread workgroup, no LDS,
// no barrier.  The running sum of the phase increments along the row is the only dependency: the wavefront walks the output row in
// 64-frame chunks, lane l owning output frame c0 + l.
//   1. The lane reads its two input frames j = floor(i r) and j + 1 (neighbouring lanes read neighbouring or equal frames: the
//      row's lines are fetched once), and forms its phase increment and its interpolated magnitude.
//   2. An inclusive shuffle scan over the 64 increments (6 steps), shifted by one lane, plus the carry of the chunks before gives
//      phi_i; the carry moves on by the chunk's total.  The order of the additions is fixed by i alone.
//   3. out = mag (cos phi, sin phi); frames past n_out are zeros.
// HBM traffic of a 64000-sample clip (251 frames) at rate 0.9: 1.03 MB of spectrum in, 1.15 MB out.
#include "mfpa_common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int ROWS_PER_BLOCK = 4;
constexpr int CHUNK = MFPA_WAVE;
constexpr double PI = 3.141592653589793;                 // float64 pi, math.pi
constexpr double TWO_PI = 2.0 * PI;

// ceil(n_frames / rate), the length of torch.arange(0, n_frames, rate), or -1: a rate that is not finite or not positive, or more
// frames than `limit`.  The kernel and mfpa_vocoder_frames share it.
__host__ __device__ inline int vocoder_n_out(int n_frames, double rate, int limit) {
  if (!(rate > 0.0 && rate <= DBL_MAX)) return -1;
  const double n = ceil((double)n_frames / rate);
  return n <= (double)limit ? (int)n : -1;
}

// torch.linspace(0, pi * 256, 257)[k] in float64 = pi k rounded once.  torch counts the upper half from the end, 256 pi - pi (256 - k);
// with the fused multiply-add of its vector kernel that is the same number (256 pi is exact), without it one ulp away at 8 bins.
__device__ __forceinline__ double phase_advance(int k) { return __dmul_rn(PI, (double)k); }

__global__ __launch_bounds__(64 * ROWS_PER_BLOCK) void phase_vocoder_kernel(const double2* __restrict__ spec,
                                                                            const double* __restrict__ rates, int nF, int ld_out,
                                                                            double2* __restrict__ out, int* __restrict__ n_out_p) {
  const int lane = threadIdx.x & (CHUNK - 1);
  const int k = blockIdx.x * ROWS_PER_BLOCK + (threadIdx.x >> 6), b = blockIdx.y;
  if (k >= MFPA_N_BINS) return;                           // whole wavefronts leave: nothing below waits for them
  const double r = rates[b];
  const int n_out = vocoder_n_out(nF, r, ld_out);
  if (k == 0 && lane == 0) n_out_p[b] = n_out;
  const double2* row = spec + ((size_t)b * MFPA_N_BINS + k) * nF;
  double2* orow = out + ((size_t)b * MFPA_N_BINS + k) * ld_out;
  const double2 zero = {0.0, 0.0};

  if (n_out < 0 || r == 1.0) {                            // refused: zeros.  Rate 1: the clip itself (n_out == nF <= ld_out)
    for (int i = lane; i < ld_out; i += CHUNK) orow[i] = (i < n_out) ? row[i] : zero;
    return;
  }

  const double adv = phase_advance(k);
  const double2 z_first = row[0];
  double carry = atan2(z_first.y, z_first.x);             // phi of the chunk's first frame
  for (int c0 = 0; c0 < ld_out; c0 += CHUNK) {            // c0, n_out and ld_out are the same in every lane: the wavefront stays whole
    const int i = c0 + lane;
    if (c0 >= n_out) {
      if (i < ld_out) orow[i] = zero;
      continue;
    }
    double inc = 0.0, mag = 0.0;
    if (i < n_out) {
      const double t = __dmul_rn((double)i, r);
      const double fj = floor(t);
      const int j = (int)fj;                              // t <= nF in exact arithmetic and after rounding; frames >= nF are zeros
      const double alpha = t - fj;
      const double2 z0 = (j < nF) ? row[j] : zero;
      const double2 z1 = (j + 1 < nF) ? row[j + 1] : zero;
      const double a0 = atan2(z0.y, z0.x), a1 = atan2(z1.y, z1.x);
      const double n0 = hypot(z0.x, z0.y), n1 = hypot(z1.x, z1.y);
      double d = a1 - a0 - adv;
      d = d - TWO_PI * rint(d / TWO_PI);
      inc = d + adv;
      mag = alpha * n1 + (1.0 - alpha) * n0;
    }
    double s = inc;                                       // inclusive scan over the chunk
#pragma unroll
    for (int o = 1; o < CHUNK; o <<= 1) {
      const double u = __shfl_up(s, o);
      if (lane >= o) s += u;
    }
    double before = __shfl_up(s, 1);                      // sum of the increments of the chunk's frames before this one
    if (lane == 0) before = 0.0;
    const double phi = carry + before;
    carry += __shfl(s, CHUNK - 1);
    if (i < n_out) {
      double sn, cs;
      sincos(phi, &sn, &cs);
      orow[i] = double2{mag * cs, mag * sn};
    } else if (i < ld_out) {
      orow[i] = zero;
    }
  }
}

}  // namespace

extern "C" {

int mfpa_phase_vocoder(const double* spec, int B, int n_frames, const double* rates, double* out, int ld_out, int* n_out,
                       void* stream) {
  if (B < 0 || B > 65535 || n_frames < 1 || n_frames > MFPA_VOCODER_MAX_FRAMES || ld_out < 1 || ld_out > MFPA_VOCODER_MAX_FRAMES)
    return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!spec || !rates || !out || !n_out) return MFPA_EINVAL;
  if ((reinterpret_cast<uintptr_t>(spec) & 15) || (reinterpret_cast<uintptr_t>(out) & 15) || (reinterpret_cast<uintptr_t>(rates) & 7) ||
      (reinterpret_cast<uintptr_t>(n_out) & 3))
    return MFPA_EINVAL;
  dim3 grid((MFPA_N_BINS + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK, B);
  hipLaunchKernelGGL(phase_vocoder_kernel, grid, dim3(64 * ROWS_PER_BLOCK), 0, mfpa_stream(stream),
                     reinterpret_cast<const double2*>(spec), rates, n_frames, ld_out, reinterpret_cast<double2*>(out), n_out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_vocoder_frames(int n_frames, double rate, int* n_out) {
  if (!n_out || n_frames < 1 || n_frames > MFPA_VOCODER_MAX_FRAMES) return MFPA_EINVAL;
  const int n = vocoder_n_out(n_frames, rate, MFPA_VOCODER_MAX_FRAMES);
  if (n < 0) return MFPA_EINVAL;
  *n_out = n;
  return MFPA_OK;
}

}  // extern "C"
