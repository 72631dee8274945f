// Inverse STFT for MI355X (gfx950): torch.istft(Z, 512, 256, window=w, center=True, length=length) at the library's fixed geometry,
// float64 throughout -- the forward transform of csrc/stft.hip run backwards, plus the windowed overlap-add.
//
// Mapping: one 256-thread workgroup = 16 consecutive frames of one clip = the 15 hops between them; 16 lanes per frame (the
// forward's mapping; the grid's neighbour transforms the shared edge frame again: 16 transforms per 15 hops).
//   1. The workgroup reads its (257 bins) x (16 frames) of the spectrum in 256-byte row segments into a padded LDS tile.  With a
//      magnitude tensor the phase is applied here, Z = m * spec / |spec|: no Z tensor ever exists in memory.
//   2. Each lane undoes the real-FFT split for its 16 bins k = l + 16 j (bins k and 256-k give the complex point Z[k] of the
//      256-point transform whose output is x[2n] + i x[2n+1]); the imaginary parts of bins 0 and 256 are never read into it.
//   3. The inverse 256-point DFT is the forward network of mfpa_fft16.h on conjugated data: same butterflies, same twiddles.
//   4. Each frame writes its 512 windowed samples to LDS (the tile's memory, reused); thread i of the workgroup then owns sample i of
//      every hop: frame h-1's second half + frame h's first half, in that order, over the two squared-window terms added in the same
//      order.  One thread forms one sample from at most two addends: no atomics, nothing depends on the batch or on the grid.
// HBM traffic of a 64000-sample clip (251 frames): 1.03 MB of spectrum in (+ 0.26 / 0.52 MB of float32 / float64 magnitudes),
// 0.26 MB of float32 samples out.
#include "mfpa_fft16.h"

#include <cmath>

namespace {

constexpr int FRAMES_PER_BLOCK = 16;
constexpr int HOPS_PER_BLOCK = FRAMES_PER_BLOCK - 1;
static_assert(sizeof(double) * FFT16_SLOTS * FRAMES_PER_BLOCK <= SPEC_TILE_BYTES, "the exchange buffers reuse the tile");
static_assert(sizeof(double) * MFPA_N_FFT * FRAMES_PER_BLOCK <= SPEC_TILE_BYTES, "the overlap-add buffer reuses the tile");

// MAG: 0 = none, 1 = float32, 2 = float64
template <int MAG, typename OutT>
__global__ __launch_bounds__(256, 2) void istft_kernel(const double2* __restrict__ spec, const void* __restrict__ mag,
                                                     const double* __restrict__ denom, int clamp, int nF, int length,
                                                     const double* __restrict__ tables, OutT* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double2* tile = reinterpret_cast<double2*>(smem);   // [257][SPEC_TILE_PITCH]
  const int tid = threadIdx.x, l = tid & 15, fs = tid >> 4;
  const int b = blockIdx.y, f0 = blockIdx.x * HOPS_PER_BLOCK;
  const double* win = tables;
  const double* tw256 = tables + 512;
  const double* tw512 = tables + 1024;

  // 1. spectrum -> tile; frames past the clip's last are zero
  {
    const int nvalid = min(FRAMES_PER_BLOCK, nF - f0);
    const size_t base = (size_t)b * MFPA_N_BINS * nF + f0;
    const double dn = (MAG != 0 && denom != nullptr) ? denom[b] : 1.0;
    for (int idx = tid; idx < MFPA_N_BINS * FRAMES_PER_BLOCK; idx += 256) {
      const int bin = idx >> 4, fr = idx & 15;
      double2 z = {0.0, 0.0};
      if (fr < nvalid) {
        const size_t g = base + (size_t)bin * nF + fr;
        z = spec[g];
        if (MAG != 0) {
          double m = (MAG == 1) ? (double)static_cast<const float*>(mag)[g] : static_cast<const double*>(mag)[g];
          if (denom != nullptr) m *= dn;
          if (clamp && m < 0.0) m = 0.0;
          const double r = hypot(z.x, z.y);
          z = (r == 0.0) ? double2{m, 0.0} : double2{m * (z.x / r), m * (z.y / r)};
        }
      }
      tile[bin * SPEC_TILE_PITCH + fr] = z;
    }
  }
  __syncthreads();

  // 2. Z[k] = E[k] + i O[k], E = (X[k] + conj(X[256-k])) / 2, O = conj(W512^k) (X[k] - conj(X[256-k])) / 2; the 1/256 of the inverse
  //    transform rides along (a power of two: exact).  a[j] = conj(Z[l + 16 j]) for the forward network.
  cd a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = l + 16 * j, kn = 256 - k;
    double2 xk = tile[k * SPEC_TILE_PITCH + fs], xn = tile[kn * SPEC_TILE_PITCH + fs];
    if (k == 0) xk.y = xn.y = 0.0;                        // bins 0 and 256: torch's c2r transform ignores their imaginary parts
    const cd e = {xk.x + xn.x, xk.y - xn.y};
    const cd d = {xk.x - xn.x, xk.y + xn.y};
    const int kt = (k <= 128) ? k : kn;                   // the table holds W512^k for k <= 128; W512^k = -conj(W512^(256-k))
    const double2 t = *reinterpret_cast<const double2*>(tw512 + 2 * kt);
    const cd wc = (k <= 128) ? cd{t.x, -t.y} : cd{-t.x, -t.y};
    const cd o = cmul(wc, d);
    constexpr double S = 1.0 / 512.0;
    a[j] = {(e.re - o.im) * S, -((e.im + o.re) * S)};
  }
  __syncthreads();                                        // the exchange buffers reuse the tile

  // 3. y = conj(DFT256(conj(Z))): y[n] = x[2n] + i x[2n+1] at n = l + 16 k2
  cd c[16];
  double* mybuf = reinterpret_cast<double*>(smem) + fs * FFT16_SLOTS;
  fft256_lanes(a, c, mybuf, l, tw256);
  __syncthreads();                                        // the overlap-add buffer reuses the exchange buffers

  // 4. windowed frames -> LDS, then hop by hop to memory
  double* ola = reinterpret_cast<double*>(smem);          // [16 frames][512]
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) {
    const int n = l + 16 * k2;
    const cd y = c[4 * (k2 & 3) + (k2 >> 2)];
    const double2 w = *reinterpret_cast<const double2*>(win + 2 * n);
    *reinterpret_cast<double2*>(ola + fs * MFPA_N_FFT + 2 * n) = double2{y.re * w.x, -y.im * w.y};
  }
  __syncthreads();
  const double wa = win[256 + tid], wb = win[tid];
  const double ea = __dmul_rn(wa, wa), eb = __dmul_rn(wb, wb);   // rounded products: the divisor is the one mfpa_istft_envelope_min forms
  OutT* ob = out + (size_t)b * length;
  for (int r = 0; r < HOPS_PER_BLOCK; ++r) {
    const int h = f0 + r + 1;                             // hop h of the padded signal = frame h-1's second half + frame h's first
    const long long pos = 256LL * (h - 1) + tid;          // its place behind the 256 dropped samples
    if (h > nF || pos >= length) break;
    double v = ola[r * MFPA_N_FFT + 256 + tid], env = ea;
    if (h < nF) {
      v = __dadd_rn(v, ola[(r + 1) * MFPA_N_FFT + tid]);
      env = __dadd_rn(ea, eb);
    }
    ob[pos] = (OutT)(v / env);
  }
}

template <int MAG>
void launch(int out_dtype, dim3 grid, hipStream_t s, const double* spec, const void* mag, const double* denom, int clamp, int nF,
            int length, const double* tables, void* out) {
  const double2* sp = reinterpret_cast<const double2*>(spec);
  if (out_dtype == MFPA_F64)
    hipLaunchKernelGGL((istft_kernel<MAG, double>), grid, dim3(256), SPEC_TILE_BYTES, s, sp, mag, denom, clamp, nF, length, tables, (double*)out);
  else
    hipLaunchKernelGGL((istft_kernel<MAG, float>), grid, dim3(256), SPEC_TILE_BYTES, s, sp, mag, denom, clamp, nF, length, tables, (float*)out);
}

bool geometry_ok(int n_frames, int length) {
  return n_frames >= 2 && (long long)length >= 256LL * (n_frames - 1) && (long long)length < 256LL * n_frames;
}

}  // namespace

extern "C" {

int mfpa_istft(const double* spec, const void* mag, int mag_dtype, const double* denom, int flags, int B, int n_frames, int length,
               const double* tables, void* out, int out_dtype, void* stream) {
  if (B < 0 || B > 65535 || !geometry_ok(n_frames, length)) return MFPA_EINVAL;
  if (mag_dtype != MFPA_F32 && mag_dtype != MFPA_F64) return MFPA_EINVAL;
  if (out_dtype != MFPA_F32 && out_dtype != MFPA_F64) return MFPA_EINVAL;
  if (flags & ~MFPA_ISTFT_CLAMP) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!spec || !tables || !out || (reinterpret_cast<uintptr_t>(spec) & 15)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int hops = (int)(((long long)length + 255) / 256);                 // hops 1 .. `hops` of the padded signal hold the kept samples
  dim3 grid((hops + HOPS_PER_BLOCK - 1) / HOPS_PER_BLOCK, B);
  const int clamp = flags & MFPA_ISTFT_CLAMP;
  if (!mag)
    launch<0>(out_dtype, grid, s, spec, nullptr, nullptr, 0, n_frames, length, tables, out);
  else if (mag_dtype == MFPA_F32)
    launch<1>(out_dtype, grid, s, spec, mag, denom, clamp, n_frames, length, tables, out);
  else
    launch<2>(out_dtype, grid, s, spec, mag, denom, clamp, n_frames, length, tables, out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_istft_envelope_min(const double* window512, int n_frames, int length, double* out_min) {
  if (!window512 || !out_min || !geometry_ok(n_frames, length)) return MFPA_EINVAL;
  // hops 1 .. n_frames-1 lie under two frames and are kept whole (length >= 256 (n_frames - 1)); what is kept of hop n_frames lies
  // under the last frame's second half alone
  double m = INFINITY;
  for (int i = 0; i < 256; ++i) {
    const volatile double ea = window512[256 + i] * window512[256 + i], eb = window512[i] * window512[i];   // rounded products, then one sum
    m = fmin(m, ea + eb);
  }
  const int tail = length - 256 * (n_frames - 1);
  for (int i = 0; i < tail; ++i) m = fmin(m, window512[256 + i] * window512[256 + i]);
  *out_min = m;
  return MFPA_OK;
}

}  // extern "C"
