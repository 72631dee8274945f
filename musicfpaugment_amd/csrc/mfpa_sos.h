// The recurrence scheme of the second-order-section kernels (iir.hip: sosfilt_kernel, loudness.hip: loudness_segments_kernel), written
// once: the geometry of a super-chunk, the setup kernel of the state-matrix powers, and one section's pass over a lane's 16 samples
// (zero-state pass, shuffle scan, carry, true pass).  iir.hip's header comment explains the scheme.  Every file that includes this is
// built with -ffp-contract=off (csrc/build.py): each product and sum is rounded on its own, in the order written.
#pragma once
#include "mfpa_common.h"

namespace {

constexpr int L = 16;                                    // samples per lane
constexpr int SUPER = MFPA_WAVE * L;                     // samples per super-chunk
constexpr int LDS_STRIDE = L + 1;                        // doubles per lane in LDS
constexpr int SCAN_STEPS = 6;                            // offsets 2^k, k < 6: 64 lanes
constexpr int POWER_DOUBLES = MFPA_WAVE * 4;             // per section: m00 m01 m10 m11 of M^j, j = 1..64, at 4 (j - 1)

__device__ __forceinline__ int lds_slot(int p) { return (p >> 4) * LDS_STRIDE + (p & (L - 1)); }

// LDS written by one lane and read by another lane of the SAME wavefront: the hardware keeps a wavefront's LDS operations in order,
// the fences keep the compiler from moving them across.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Thread t = (row r, section s, unit state u): the homogeneous recurrence from e_u; the state after 16 j steps is column u of
// A^(16 j).  z1 <- z2 - a1 y is (b1 0 - a1 y) + z2 of the filter with the zero products left out (the same double).
__global__ void sos_powers_kernel(const double* __restrict__ sos, int n, double* __restrict__ work) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const int u = t & 1;
  const double* c = sos + (size_t)(t >> 1) * 6;
  const double a1 = c[4], a2 = c[5];
  double z1 = u ? 0.0 : 1.0, z2 = u ? 1.0 : 0.0;
  double* out = work + (size_t)(t >> 1) * POWER_DOUBLES + u;
  for (int i = 1; i <= SUPER; ++i) {
    const double y = z1;
    z1 = z2 - a1 * y;
    z2 = -(a2 * y);
    if ((i & (L - 1)) == 0) {
      const int j = i / L - 1;
      out[4 * j] = z1;
      out[4 * j + 2] = z2;
    }
  }
}

// One section over the lane's 16 samples v (in: the section's input, out: its output).  c: the section's six coefficients, m: its 64
// powers, q_own: M^lane (read by this lane only), (k1, k2): the section's carry into this super-chunk.  (f1, f2), the same in every
// lane: the state after sample tail_i of lane tail_lane, from the true pass.
__device__ __forceinline__ void sos_section(double (&v)[L], const double* __restrict__ c, const double* __restrict__ m, const double* q_own,
                                            double k1, double k2, int lane, int tail_lane, int tail_i, double& f1, double& f2) {
  const double b0 = c[0], b1 = c[1], b2 = c[2], a1 = c[4], a2 = c[5];
  double z1 = 0.0, z2 = 0.0;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const double o = b0 * v[i] + z1;
    z1 = (b1 * v[i] - a1 * o) + z2;
    z2 = b2 * v[i] - a2 * o;
  }
#pragma unroll
  for (int k = 0; k < SCAN_STEPS; ++k) {
    const double* q = m + 4 * ((1 << k) - 1);
    const double t1 = __shfl_up(z1, 1 << k), t2 = __shfl_up(z2, 1 << k);
    if (lane >= (1 << k)) {
      z1 = z1 + (q[0] * t1 + q[1] * t2);
      z2 = z2 + (q[2] * t1 + q[3] * t2);
    }
  }
  const double p1 = __shfl_up(z1, 1), p2 = __shfl_up(z2, 1);
  z1 = lane ? (q_own[0] * k1 + q_own[1] * k2) + p1 : k1;
  z2 = lane ? (q_own[2] * k1 + q_own[3] * k2) + p2 : k2;
  f1 = 0.0;
  f2 = 0.0;
#pragma unroll
  for (int i = 0; i < L; ++i) {
    const double o = b0 * v[i] + z1;
    z1 = (b1 * v[i] - a1 * o) + z2;
    z2 = b2 * v[i] - a2 * o;
    v[i] = o;
    if (i == tail_i) {
      f1 = z1;
      f2 = z2;
    }
  }
  f1 = __shfl(f1, tail_lane);
  f2 = __shfl(f2, tail_lane);
}

}  // namespace
