// The 256-point complex float64 FFT that csrc/stft.hip and csrc/istft.hip share: 16 x 16, sixteen lanes per transform, one
// exchange through a padded LDS tile.  The inverse transform runs the same network on conjugated data.
#pragma once
#include "mfpa_common.h"

namespace {

struct cd {
  double re, im;
};
__device__ __forceinline__ cd operator+(cd a, cd b) { return {a.re + b.re, a.im + b.im}; }
__device__ __forceinline__ cd operator-(cd a, cd b) { return {a.re - b.re, a.im - b.im}; }
__device__ __forceinline__ cd cmul(cd a, cd b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

__device__ __forceinline__ void dft4(cd& a, cd& b, cd& c, cd& d) {
  cd s0 = a + c, s1 = a - c, s2 = b + d, s3 = b - d;
  a = s0 + s2;
  c = s0 - s2;
  b = {s1.re + s3.im, s1.im - s3.re};  // s1 - i s3
  d = {s1.re - s3.im, s1.im + s3.re};  // s1 + i s3
}

// In-place 16-point DFT.  On return X[k] sits at v[4*(k&3) + (k>>2)].
__device__ __forceinline__ void dft16(cd (&v)[16]) {
  constexpr double C1 = 0.92387953251128673848, S1 = 0.38268343236508978178, R2 = 0.70710678118654752440;
#pragma unroll
  for (int j2 = 0; j2 < 4; ++j2) dft4(v[j2], v[4 + j2], v[8 + j2], v[12 + j2]);
  // v[4*k1 + j2] *= W16^(j2*k1)
  v[4 * 1 + 1] = cmul(v[4 * 1 + 1], cd{C1, -S1});
  v[4 * 1 + 2] = cmul(v[4 * 1 + 2], cd{R2, -R2});
  v[4 * 1 + 3] = cmul(v[4 * 1 + 3], cd{S1, -C1});
  v[4 * 2 + 1] = cmul(v[4 * 2 + 1], cd{R2, -R2});
  v[4 * 2 + 2] = cd{v[4 * 2 + 2].im, -v[4 * 2 + 2].re};  // * -i
  v[4 * 2 + 3] = cmul(v[4 * 2 + 3], cd{-R2, -R2});
  v[4 * 3 + 1] = cmul(v[4 * 3 + 1], cd{S1, -C1});
  v[4 * 3 + 2] = cmul(v[4 * 3 + 2], cd{-R2, -R2});
  v[4 * 3 + 3] = cmul(v[4 * 3 + 3], cd{-C1, S1});
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1) dft4(v[4 * k1], v[4 * k1 + 1], v[4 * k1 + 2], v[4 * k1 + 3]);
}

constexpr int FFT16_SLOTS = 16 * 17;  // padded 16 x 16 tile of doubles per transform: conflict-free for the row writes and the column reads

// The 16 lanes of a transform sit in ONE wavefront (4 transforms per wave), so the exchanges need no workgroup barrier: a wave's LDS
// operations execute in order, wave_sync() only keeps the compiler from moving them across each other.
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// 256-point forward DFT over the 16 lanes l = 0..15 of one transform.  In: a[j] = z[l + 16 j].  Out: Z[l + 16 k2] at
// c[4*(k2&3) + (k2>>2)].  mybuf: the transform's FFT16_SLOTS doubles of LDS; tw256[2m], tw256[2m+1] = cos, -sin of 2 pi m / 256.
// Real and imaginary parts go through the same 8-byte slots one after the other: 34 KB of LDS per 16 transforms instead of 68 KB.
__device__ __forceinline__ void fft256_lanes(cd (&a)[16], cd (&c)[16], double* mybuf, int l, const double* __restrict__ tw256) {
  dft16(a);  // A[k1] at a[4*(k1&3) + (k1>>2)]
  double tim[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) {
    const int m = (l * k1) & 255;
    const double2 t = *reinterpret_cast<const double2*>(tw256 + 2 * m);
    const cd v = cmul(a[4 * (k1 & 3) + (k1 >> 2)], cd{t.x, t.y});
    mybuf[k1 * 17 + l] = v.re;
    tim[k1] = v.im;
  }
  wave_sync();
#pragma unroll
  for (int q = 0; q < 16; ++q) c[q].re = mybuf[l * 17 + q];
  wave_sync();
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) mybuf[k1 * 17 + l] = tim[k1];
  wave_sync();
#pragma unroll
  for (int q = 0; q < 16; ++q) c[q].im = mybuf[l * 17 + q];
  wave_sync();
  dft16(c);  // Z[l + 16*k2] at c[4*(k2&3) + (k2>>2)]
}

// A (257 bins) x (16 frames) tile of complex128 values in LDS, rows padded to 17 so that the 16 lanes of a frame, which walk the
// bins, do not meet on one bank; both directions move the spectrum between this tile and 256-byte row segments of global memory.
constexpr int SPEC_TILE_PITCH = 17;
constexpr size_t SPEC_TILE_BYTES = sizeof(double2) * MFPA_N_BINS * SPEC_TILE_PITCH;   // 69 904

}  // namespace
