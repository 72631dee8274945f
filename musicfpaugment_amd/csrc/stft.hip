// Fused window + 512-point real FFT + magnitude (or one-sided PSD) for MI355X (gfx950).
//
// Replaces torch.stft/abs (training/visualisation.py:20-28), np.abs(stft.stft) (afp/audfprint/
// stft.py:15-62 via peak_extractor.py:259) and mlab.specgram (afp/dejavu/fingerprint.py:60-66).
//
// Mapping: one 256-thread workgroup = 16 consecutive frames of one clip; 16 lanes per frame.
// The 512-point real FFT is a 256-point complex FFT (z[n] = x[2n] + i x[2n+1]) done as
// 16 x 16: each lane runs a 16-point DFT in registers, the 16 lanes of a frame exchange once
// through a padded LDS tile (17-slot rows: conflict-free for both the row writes and the
// column reads), run the second 16-point DFT, and the real-FFT split pairs bins k / 256-k.
// Magnitudes are staged in LDS as [bin][16 frames] so the global store writes 16-frame
// segments of each bin row.  All arithmetic is float64 (the reference's window is float64,
// which promotes the whole STFT): HBM traffic is 514 KB per 8 s clip, the FFT ~4 MFLOP.
// mfpa_stft_complex is the same kernel with SPEC set: the complex bins leave through a second, complex LDS tile before the
// magnitudes do (+1.03 MB per 8 s clip); csrc/istft.hip runs the transform backwards.  The butterflies are in mfpa_fft16.h.
#include "mfpa_fft16.h"

#include <cmath>

namespace {

constexpr int FRAMES_PER_BLOCK = 16;
constexpr int SLOTS = FFT16_SLOTS;  // padded 16x16 tile of doubles per frame (>= 257 + 1 slots of the [bin][16 frames] output tile per frame)

// MODE 0: centre/reflect magnitude (hypot).  MODE 1: no padding, one-sided PSD (|X|^2, interior bins x2).
// SPEC (MODE 0 only): the complex bins go to `spec` as well, through a [bin][16 frames] tile of complex values that takes the whole
// SPEC_TILE_BYTES of LDS (two resident workgroups per CU); `out` and `clip_max` may then be null, and what they receive is what the
// SPEC = false kernel writes: the magnitudes are the same expressions of the same values.
template <int MODE, typename OutT, bool SPEC = false>
__global__ __launch_bounds__(256, SPEC ? 2 : 4) void stft_kernel(const float* __restrict__ wav, int T_w, int nF,
                                                              const double* __restrict__ tables, OutT* __restrict__ out,
                                                              double* __restrict__ clip_max, double scale_in,
                                                              double2* __restrict__ spec) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* buf = reinterpret_cast<double*>(smem);
  const int tid = threadIdx.x, l = tid & 15, fs = tid >> 4;
  const int b = blockIdx.y, f0 = blockIdx.x * FRAMES_PER_BLOCK, f = f0 + fs;
  const bool active = f < nF;
  const float* x = wav + (size_t)b * T_w;
  const double* win = tables;
  const double* tw256 = tables + 512;
  const double* tw512 = tables + 1024;
  double* mybuf = buf + fs * SLOTS;   // this frame's 16 x 17 slots: real parts, then imaginary parts

  cd a[16];
  const int start = (MODE == 0) ? 256 * f - 256 : 256 * f;
  const bool vec_ok = ((T_w & 1) == 0);
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int i0 = 2 * (l + 16 * j);
    int s0 = start + i0, s1 = s0 + 1;
    float v0 = 0.f, v1 = 0.f;
    if (active) {
      if (MODE == 0 && (s0 < 0 || s1 >= T_w)) {
        if (s0 < 0) s0 = -s0;
        if (s1 < 0) s1 = -s1;
        if (s0 >= T_w) s0 = 2 * (T_w - 1) - s0;
        if (s1 >= T_w) s1 = 2 * (T_w - 1) - s1;
        v0 = x[s0];
        v1 = x[s1];
      } else if (vec_ok) {
        const float2 p = *reinterpret_cast<const float2*>(x + s0);
        v0 = p.x;
        v1 = p.y;
      } else {
        v0 = x[s0];
        v1 = x[s1];
      }
    }
    const double2 w = *reinterpret_cast<const double2*>(win + i0);
    if (MODE == 1) {
      a[j] = {(double)v0 * scale_in * w.x, (double)v1 * scale_in * w.y};
    } else {
      a[j] = {(double)v0 * w.x, (double)v1 * w.y};
    }
  }
  dft16(a);  // A[k1] at a[4*(k1&3) + (k1>>2)]
  // The exchange of mfpa_fft16.h's fft256_lanes(), spelled out: called through that function's array references this kernel came out
  // with 8 spilled registers under its 128-VGPR bound.  Real and imaginary parts go through the same 8-byte slots one after the
  // other: 34 KB of LDS per workgroup instead of 68 KB -- four resident workgroups per CU instead of two (the kernel is
  // latency-bound: profiles/r03_prune_sq.md, 1.8 waves per SIMD, 38 % issuing).
  cd c[16];
  {
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
  }
  dft16(c);  // Z[l + 16*k2] at c[4*(k2&3) + (k2>>2)]

  // real-FFT split: bins k and 256-k from Z[k], Z[256-k]; slot(k) = k + (k >> 4)
  double zkr[9], znr[9], zki[9], zni[9];
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) mybuf[l + 17 * k2] = c[4 * (k2 & 3) + (k2 >> 2)].re;
  wave_sync();
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const int k = (m < 8) ? l + 16 * m : 128;
    const int kn = (256 - k) & 255;
    zkr[m] = mybuf[k + (k >> 4)];
    znr[m] = mybuf[kn + (kn >> 4)];
  }
  wave_sync();
#pragma unroll
  for (int k2 = 0; k2 < 16; ++k2) mybuf[l + 17 * k2] = c[4 * (k2 & 3) + (k2 >> 2)].im;
  wave_sync();
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const int k = (m < 8) ? l + 16 * m : 128;
    const int kn = (256 - k) & 255;
    zki[m] = mybuf[k + (k >> 4)];
    zni[m] = mybuf[kn + (kn >> 4)];
  }
  double lo[9], hi[9];
  cd sk[9], sn[9];   // SPEC: bins k and 256-k
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const int k = (m < 8) ? l + 16 * m : 128;
    const cd zk = {zkr[m], zki[m]}, zn = {znr[m], zni[m]};
    const cd e = {0.5 * (zk.re + zn.re), 0.5 * (zk.im - zn.im)};
    const cd o = {0.5 * (zk.im + zn.im), -0.5 * (zk.re - zn.re)};  // -i (zk - conj(zn)) / 2
    const double2 t = *reinterpret_cast<const double2*>(tw512 + 2 * k);
    const cd wo = cmul(cd{t.x, t.y}, o);
    const cd xk = e + wo, xn = e - wo;   // X[k] and conj(X[256-k])
    if (SPEC) {
      sk[m] = xk;
      sn[m] = {xn.re, -xn.im};
    }
    if (MODE == 0) {
      lo[m] = hypot(xk.re, xk.im);          // (sqrt(fma(re, re, im * im)) measured the same time and the same bits on the synthetic clips: kept hypot, numpy's abs)
      hi[m] = hypot(xn.re, xn.im);
    } else {
      lo[m] = (xk.re * xk.re + xk.im * xk.im) * ((k >= 1) ? 2.0 : 1.0);
      hi[m] = (xn.re * xn.re + xn.im * xn.im) * ((k >= 1) ? 2.0 : 1.0);
    }
  }
  __syncthreads();
  if (SPEC) {
    const int nvalid = min(FRAMES_PER_BLOCK, nF - f0);
    double2* ctile = reinterpret_cast<double2*>(smem);  // [257][SPEC_TILE_PITCH]
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int k = l + 16 * m;
      ctile[k * SPEC_TILE_PITCH + fs] = double2{sk[m].re, sk[m].im};
      ctile[(256 - k) * SPEC_TILE_PITCH + fs] = double2{sn[m].re, sn[m].im};   // k == 0: the Nyquist bin
    }
    if (l == 0) ctile[128 * SPEC_TILE_PITCH + fs] = double2{sk[8].re, sk[8].im};
    __syncthreads();
    double2* sbase = spec + (size_t)b * MFPA_N_BINS * nF + f0;
    for (int idx = tid; idx < MFPA_N_BINS * FRAMES_PER_BLOCK; idx += 256) {
      const int bin = idx >> 4, fr = idx & 15;
      if (fr < nvalid) sbase[(size_t)bin * nF + fr] = ctile[bin * SPEC_TILE_PITCH + fr];
    }
    if (out == nullptr && clip_max == nullptr) return;   // the same for every thread of the grid
    __syncthreads();
  }
  double* tile = reinterpret_cast<double*>(smem);  // [257][16]
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int k = l + 16 * m;
    tile[k * 16 + fs] = lo[m];
    if (k > 0) tile[(256 - k) * 16 + fs] = hi[m];
    if (k == 0) tile[256 * 16 + fs] = hi[m];  // Nyquist
  }
  if (l == 0) tile[128 * 16 + fs] = lo[8];
  __syncthreads();

  double vmax = 0.0;
  const int nvalid = min(FRAMES_PER_BLOCK, nF - f0);
  OutT* obase = out + (size_t)b * MFPA_N_BINS * nF + f0;
  for (int idx = tid; idx < MFPA_N_BINS * FRAMES_PER_BLOCK; idx += 256) {
    const int bin = idx >> 4, fr = idx & 15;
    if (fr < nvalid) {
      const double v = tile[idx];
      vmax = fmax(vmax, v);
      if (!SPEC || out != nullptr) obase[(size_t)bin * nF + fr] = (OutT)v;
    }
  }
  if (clip_max != nullptr) {
    vmax = mfpa_wave_max(vmax);
    double* wmax = tile + MFPA_N_BINS * FRAMES_PER_BLOCK;  // past the tile, still inside the FFT buffer
    if ((tid & 63) == 0) wmax[tid >> 6] = vmax;
    __syncthreads();
    if (tid == 0) mfpa_atomic_max_nonneg(clip_max + b, fmax(fmax(wmax[0], wmax[1]), fmax(wmax[2], wmax[3])));
  }
}

template <typename T>
__global__ void normalize_kernel(T* __restrict__ data, long long n, const double* __restrict__ clip_max, int B,
                                 int per_clip) {
  const int b = blockIdx.y;
  double d;
  if (per_clip) {
    d = clip_max[b];
  } else {
    __shared__ double gmax;
    if (threadIdx.x < MFPA_WAVE) {
      double m = 0.0;
      for (int i = threadIdx.x; i < B; i += MFPA_WAVE) m = fmax(m, clip_max[i]);
      m = mfpa_wave_max(m);
      if (threadIdx.x == 0) gmax = m;
    }
    __syncthreads();
    d = gmax;
  }
  T* p = data + (size_t)b * n;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    p[i] = (T)((double)p[i] / d);
}

__global__ void f64_to_f32_kernel(const double* __restrict__ in, float* __restrict__ out, long long n) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    out[i] = (float)in[i];
}

}  // namespace

extern "C" {

int mfpa_version(void) { return 47; }

int mfpa_stft_frames(int T_w) { return 1 + T_w / MFPA_N_HOP; }

int mfpa_stft_tables(const double* window512, double* out) {
  if (!window512 || !out) return MFPA_EINVAL;
  const long double pi = 3.14159265358979323846264338327950288L;
  for (int i = 0; i < 512; ++i) out[i] = window512[i];
  for (int m = 0; m < 256; ++m) {
    out[512 + 2 * m] = (double)cosl(2.0L * pi * m / 256.0L);
    out[512 + 2 * m + 1] = (double)(-sinl(2.0L * pi * m / 256.0L));
  }
  for (int k = 0; k <= 128; ++k) {
    out[1024 + 2 * k] = (double)cosl(2.0L * pi * k / 512.0L);
    out[1024 + 2 * k + 1] = (double)(-sinl(2.0L * pi * k / 512.0L));
  }
  for (int i = 1024 + 258; i < MFPA_STFT_TABLE_LEN; ++i) out[i] = 0.0;
  return MFPA_OK;
}

int mfpa_stft_mag(const float* wav, int B, int T_w, const double* tables, void* mag, int out_dtype,
                  double* clip_max, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!wav || !tables || !mag || B < 0 || T_w <= 256) return MFPA_EINVAL;
  if (out_dtype != MFPA_F32 && out_dtype != MFPA_F64) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nF = mfpa_stft_frames(T_w);
  if (clip_max) MFPA_HIP(hipMemsetAsync(clip_max, 0, sizeof(double) * B, s));
  dim3 grid((nF + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK, B);
  const size_t lds = sizeof(double) * SLOTS * FRAMES_PER_BLOCK;
  if (out_dtype == MFPA_F64)
    hipLaunchKernelGGL((stft_kernel<0, double>), grid, dim3(256), lds, s, wav, T_w, nF, tables, (double*)mag, clip_max, 1.0, nullptr);
  else
    hipLaunchKernelGGL((stft_kernel<0, float>), grid, dim3(256), lds, s, wav, T_w, nF, tables, (float*)mag, clip_max, 1.0, nullptr);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_stft_complex(const float* wav, int B, int T_w, const double* tables, double* spec, void* mag, int mag_dtype,
                      double* clip_max, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!wav || !tables || !spec || B < 0 || T_w <= 256) return MFPA_EINVAL;
  if (mag_dtype != MFPA_F32 && mag_dtype != MFPA_F64) return MFPA_EINVAL;
  if (reinterpret_cast<uintptr_t>(spec) & 15) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nF = mfpa_stft_frames(T_w);
  if (clip_max) MFPA_HIP(hipMemsetAsync(clip_max, 0, sizeof(double) * B, s));
  dim3 grid((nF + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK, B);
  double2* sp = reinterpret_cast<double2*>(spec);
  if (mag_dtype == MFPA_F64)
    hipLaunchKernelGGL((stft_kernel<0, double, true>), grid, dim3(256), SPEC_TILE_BYTES, s, wav, T_w, nF, tables, (double*)mag, clip_max, 1.0, sp);
  else
    hipLaunchKernelGGL((stft_kernel<0, float, true>), grid, dim3(256), SPEC_TILE_BYTES, s, wav, T_w, nF, tables, (float*)mag, clip_max, 1.0, sp);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_specgram_frames(int T_w) { return (T_w - 256) / 256; }

int mfpa_specgram_psd(const float* wav, int B, int T_w, double scale_in, const double* tables, double* psd,
                      double* clip_max, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!wav || !tables || !psd || B < 0 || T_w < 512) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nF = mfpa_specgram_frames(T_w);
  if (clip_max) MFPA_HIP(hipMemsetAsync(clip_max, 0, sizeof(double) * B, s));
  dim3 grid((nF + FRAMES_PER_BLOCK - 1) / FRAMES_PER_BLOCK, B);
  const size_t lds = sizeof(double) * SLOTS * FRAMES_PER_BLOCK;
  hipLaunchKernelGGL((stft_kernel<1, double>), grid, dim3(256), lds, s, wav, T_w, nF, tables, psd, clip_max, scale_in, nullptr);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_normalize(void* data, int dtype, int B, long long n, const double* clip_max, int per_clip, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!data || !clip_max || B < 0 || n < 0) return MFPA_EINVAL;
  if (dtype != MFPA_F32 && dtype != MFPA_F64) return MFPA_EINVAL;
  if (B == 0 || n == 0) return MFPA_OK;
  hipStream_t s = mfpa_stream(stream);
  const int gx = (int)((n + 256 * 8 - 1) / (256 * 8));
  dim3 grid(gx < 1 ? 1 : (gx > 64 ? 64 : gx), B);
  if (dtype == MFPA_F64)
    hipLaunchKernelGGL(normalize_kernel<double>, grid, dim3(256), 0, s, (double*)data, n, clip_max, B, per_clip);
  else
    hipLaunchKernelGGL(normalize_kernel<float>, grid, dim3(256), 0, s, (float*)data, n, clip_max, B, per_clip);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// out[b][i] = (float)(in[b][i] / denom[b]): the reference's `spectrogram / max` followed by `.float()` (training/train.py:264-272) as one pass
__global__ __launch_bounds__(256) void normalize_f32_kernel(const double* __restrict__ in, long long n, const double* __restrict__ denom,
                                                            float* __restrict__ out) {
  const int b = blockIdx.y;
  const double d = denom[b];
  const double* ib = in + (size_t)b * n;
  float* ob = out + (size_t)b * n;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) ob[i] = (float)(ib[i] / d);
}

int mfpa_normalize_f32(const double* in, int B, long long n, const double* denom, float* out, void* stream) {
  if (B == 0 || n == 0) return MFPA_OK;
  if (!in || !denom || !out || B < 0 || B > 65535 || n < 0) return MFPA_EINVAL;
  const long long gx = (n + 255) / 256;
  hipLaunchKernelGGL(normalize_f32_kernel, dim3((unsigned)(gx > 256 ? 256 : gx), (unsigned)B), dim3(256), 0, mfpa_stream(stream), in, n, denom, out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_f64_to_f32(const double* in, float* out, long long n, void* stream) {
  if (!in || !out || n < 0) return MFPA_EINVAL;
  if (n == 0) return MFPA_OK;
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(f64_to_f32_kernel, dim3((int)blocks), dim3(256), 0, mfpa_stream(stream), in, out, n);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
