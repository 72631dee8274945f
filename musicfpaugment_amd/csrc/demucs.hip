// Demucs causal waveform denoiser, forward, for MI355X (gfx950) -- next-tier row SURVEY.md §8f-2.
// Reference: training/model.py:22-110 (sinc resampling, LSTM) and :163-326 (Demucs) of deezer/musicFPaugment.
//
// Activations are time-major "NLC": (B, L, C) float32, channels contiguous.  In that layout every layer is a
// plain GEMM over overlapping row windows, all served by ONE batched strided MFMA GEMM (mfpa_gemm_mfma, csrc/demucs_gemm.hip):
//   Conv1d(k=8, s=4)        : row t = x[4t : 4t+8] flattened (8C contiguous floats), row stride 4C, K = 8C
//   Conv1d(k=1) + GLU       : K = C, weights packed so a wave's 64-column tile is [32 values | their 32 gates]
//   ConvTranspose1d(k8, s4) : row t = [g[t-1] | g[t]] (2C contiguous floats of a buffer with one zero row at each
//                             end), N = 4*Cout: output row t is positions 4t..4t+3 -- the overlap-add of the
//                             transposed convolution becomes part of K; the skip connection of the next decoder
//                             layer is added in the epilogue
//   LSTM                    : input projection of all steps as one GEMM; the recurrence itself is csrc/lstm.hip
// The 1-channel ends (first Conv1d, last ConvTranspose1d), the sinc x2 resamplers and the std normalisation are
// small VALU kernels.
// This file holds the small kernels and their entry points (mfpa_demucs_prep, mfpa_upsample2, mfpa_downsample2, mfpa_conv1d_c1,
// mfpa_convT1d_c1).  The GEMM family behind mfpa_gemm_mfma and the two fused end-level kernels (mfpa_glu_convT1d_c1,
// mfpa_conv1d_c1_glu) are csrc/demucs_gemm.hip.
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"

namespace {

using mfpa_tile::f32x4;

// ---------------------------------------------------------------------------------- small kernels
// mix / (floor + std), zero-padded to VL samples; std = unbiased std over time (model.py:293-301).
__global__ __launch_bounds__(256) void demucs_prep_kernel(const float* __restrict__ wav, int T, int VL, float floor_,
                                                          float* __restrict__ out, float* __restrict__ stdv) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* x = wav + (size_t)b * T;
  double s = 0, ss = 0;
  for (int i = tid; i < T; i += 256) { const double v = x[i]; s += v; ss += v * v; }
  __shared__ double sh[2][256];
  sh[0][tid] = s; sh[1][tid] = ss;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; }
    __syncthreads();
  }
  const double mean = sh[0][0] / T;
  double var = (sh[1][0] - T * mean * mean) / (T - 1);
  if (var < 0) var = 0;
  const float sd = (float)sqrt(var);
  if (tid == 0) stdv[b] = sd;
  const float inv = sd + floor_;
  float* o = out + (size_t)b * VL;
  for (int i = tid; i < VL; i += 256) o[i] = i < T ? x[i] / inv : 0.f;
}

// Sinc x2 resamplers: 112-tap FIRs.  A workgroup produces RS_OUT consecutive filter outputs from a window of the input
// staged once in LDS; a thread owns 4 adjacent outputs and slides a float4 window over the taps (7 LDS float4 reads per
// 4 taps x 4 outputs instead of 16 scalar loads).
constexpr int RS_OUT = 1024, RS_TAPS = 112;

__device__ __forceinline__ void rs_fir4(const float* __restrict__ w, const float* __restrict__ kk, f32x4& acc) {
  f32x4 lo = *reinterpret_cast<const f32x4*>(w);
#pragma unroll 4
  for (int k = 0; k < RS_TAPS; k += 4) {
    const f32x4 hi = *reinterpret_cast<const f32x4*>(w + k + 4);
    const f32x4 c = *reinterpret_cast<const f32x4*>(kk + k);
    acc[0] += c[0] * lo[0] + c[1] * lo[1] + c[2] * lo[2] + c[3] * lo[3];
    acc[1] += c[0] * lo[1] + c[1] * lo[2] + c[2] * lo[3] + c[3] * hi[0];
    acc[2] += c[0] * lo[2] + c[1] * lo[3] + c[2] * hi[0] + c[3] * hi[1];
    acc[3] += c[0] * lo[3] + c[1] * hi[0] + c[2] * hi[1] + c[3] * hi[2];
    lo = hi;
  }
}

// upsample2 (model.py:41-53): y[2i] = x[i], y[2i+1] = sum_k x[i + k - 55] ker[k], k < 112 (zero beyond the ends).
__global__ MFPA_NO_PK_F32 __launch_bounds__(256) void upsample2_kernel(const float* __restrict__ x, int T, const float* __restrict__ ker,
                                                        float* __restrict__ y) {
  __shared__ __attribute__((aligned(16))) float win[RS_OUT + RS_TAPS + 8];
  __shared__ __attribute__((aligned(16))) float kk[RS_TAPS];
  const int b = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * RS_OUT;
  const float* xb = x + (size_t)b * T;
  float* yb = y + (size_t)b * 2 * T;
  if (tid < RS_TAPS) kk[tid] = ker[tid];
  for (int j = tid; j < RS_OUT + RS_TAPS + 4; j += 256) {        // win[j] = x[i0 - 55 + j]
    const int s = i0 - 55 + j;
    win[j] = (s >= 0 && s < T) ? xb[s] : 0.f;
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  rs_fir4(win + 4 * tid, kk, acc);
  const int i = i0 + 4 * tid;
  if (i + 3 < T) {
    const f32x4 xv = {win[4 * tid + 55], win[4 * tid + 56], win[4 * tid + 57], win[4 * tid + 58]};
    *reinterpret_cast<f32x4*>(yb + 2 * (size_t)i) = f32x4{xv[0], acc[0], xv[1], acc[1]};
    *reinterpret_cast<f32x4*>(yb + 2 * (size_t)i + 4) = f32x4{xv[2], acc[2], xv[3], acc[3]};
  } else {
#pragma unroll
    for (int o = 0; o < 4; ++o)
      if (i + o < T) { yb[2 * (size_t)(i + o)] = win[4 * tid + o + 55]; yb[2 * (size_t)(i + o) + 1] = acc[o]; }
  }
}

// downsample2 (model.py:69-88): out[i] = 0.5 * (x[2i] + sum_k xodd[i + k - 56] ker[k]), xodd[j] = x[2j+1] (0 beyond the end).
__global__ MFPA_NO_PK_F32 __launch_bounds__(256) void downsample2_kernel(const float* __restrict__ x, int T, const float* __restrict__ ker,
                                                          float* __restrict__ y, int To, const float* __restrict__ scale,
                                                          int Tkeep) {
  __shared__ __attribute__((aligned(16))) float wodd[RS_OUT + RS_TAPS + 8];
  __shared__ __attribute__((aligned(16))) float kk[RS_TAPS];
  const int b = blockIdx.y, tid = threadIdx.x, i0 = blockIdx.x * RS_OUT;
  const float* xb = x + (size_t)b * T;
  const int Th = (T + 1) / 2;                       // length of xeven / xodd after the odd-length zero pad
  const float sc = scale ? scale[b] : 1.f;
  const int nout = Tkeep > 0 ? Tkeep : Th;
  float* yb = y + (size_t)b * To;
  if (tid < RS_TAPS) kk[tid] = ker[tid];
  for (int j = tid; j < RS_OUT + RS_TAPS + 4; j += 256) {        // wodd[j] = xodd[i0 - 56 + j]
    const int s = i0 - 56 + j;
    wodd[j] = (s >= 0 && s < Th && 2 * s + 1 < T) ? xb[2 * s + 1] : 0.f;
  }
  __syncthreads();
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  rs_fir4(wodd + 4 * tid, kk, acc);
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int i = i0 + 4 * tid + o;
    if (i < nout) yb[i] = sc * (0.5f * (xb[2 * (size_t)i] + acc[o]));
  }
}

// First encoder conv: Conv1d(1 -> C, k=8, s=4) + ReLU on (B, Lin) -> (B, Lout, C).  w [8][C] (tap-major), bias [C].
__global__ __launch_bounds__(256) void conv1d_c1_kernel(const float* __restrict__ x, int Lin, int Lout, int C,
                                                        const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ y, int relu) {
  const int b = blockIdx.y, C4 = C / 4;
  const float* xb = x + (size_t)b * Lin;
  float* yb = y + (size_t)b * Lout * C;
  const long long total = (long long)Lout * C4;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cq = (int)(e % C4);
    const int t = (int)(e / C4);
    const f32x4 bv = bias ? *reinterpret_cast<const f32x4*>(bias + 4 * cq) : f32x4{0.f, 0.f, 0.f, 0.f};
    mfpa_f32x2 a01 = {bv[0], bv[1]}, a23 = {bv[2], bv[3]};       // bias, then taps 0..7: one FMA chain per channel
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const mfpa_f32x2 v = mfpa_bcast2(xb[4 * t + j]);            // packed FMAs without operand selection (mfpa_common.h)
      const f32x4 ww = *reinterpret_cast<const f32x4*>(w + j * C + 4 * cq);
      a01 += v * mfpa_f32x2{ww[0], ww[1]};
      a23 += v * mfpa_f32x2{ww[2], ww[3]};
    }
    f32x4 acc = {a01[0], a01[1], a23[0], a23[1]};
    if (relu) {
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = acc[k] > 0.f ? acc[k] : 0.f;
    }
    *reinterpret_cast<f32x4*>(yb + (size_t)t * C + 4 * cq) = acc;
  }
}

// Last decoder layer: ConvTranspose1d(C -> 1, k=8, s=4) on the zero-padded GLU output P (B, L+2, C):
// out[4t + j] = bias + sum_c P[t+1][c] w[c][j] + P[t][c] w[c][j+4],  t = 0..L, j = 0..3.   w [8][C] (tap-major).
__global__ __launch_bounds__(256) void convT1d_c1_kernel(const float* __restrict__ P, int L, int C,
                                                         const float* __restrict__ w, float bias, const float* __restrict__ biasp,
                                                         float* __restrict__ y) {
  const int b = blockIdx.y;
  if (biasp) bias = biasp[0];
  const float* Pb = P + (size_t)b * (L + 2) * C;
  float* yb = y + (size_t)b * 4 * (L + 1);
  const int total = 4 * (L + 1);
  for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
    const int t = p >> 2, j = p & 3;
    const float* cur = Pb + (size_t)(t + 1) * C;
    const float* prev = Pb + (size_t)t * C;
    float acc = bias;
    for (int c = 0; c < C; c += 4) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(cur + c), a1 = *reinterpret_cast<const f32x4*>(prev + c);
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + j * C + c), w1 = *reinterpret_cast<const f32x4*>(w + (j + 4) * C + c);
      acc += a0[0] * w0[0] + a0[1] * w0[1] + a0[2] * w0[2] + a0[3] * w0[3];
      acc += a1[0] * w1[0] + a1[1] * w1[1] + a1[2] * w1[2] + a1[3] * w1[3];
    }
    yb[p] = acc;
  }
}

}  // namespace

extern "C" {

int mfpa_demucs_prep(const float* wav, int B, int T, int VL, float floor_, float* out, float* stdv, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!wav || !out || !stdv || B < 0 || T < 2 || VL < T) return MFPA_EINVAL;
  hipLaunchKernelGGL(demucs_prep_kernel, dim3(B), dim3(256), 0, mfpa_stream(stream), wav, T, VL, floor_, out, stdv);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_upsample2(const float* x, int B, int T, const float* kernel112, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !kernel112 || !y || B < 0 || B > 65535 || T < 1) return MFPA_EINVAL;
  const int gx = (T + RS_OUT - 1) / RS_OUT;
  hipLaunchKernelGGL(upsample2_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), x, T, kernel112, y);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_downsample2(const float* x, int B, int T, const float* kernel112, float* y, int To, const float* scale, int Tkeep,
                     void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !kernel112 || !y || B < 0 || B > 65535 || T < 2) return MFPA_EINVAL;
  const int nout = Tkeep > 0 ? Tkeep : (T + 1) / 2;
  if (nout > (T + 1) / 2 || To < nout) return MFPA_EINVAL;
  const int gx = (nout + RS_OUT - 1) / RS_OUT;
  hipLaunchKernelGGL(downsample2_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), x, T, kernel112, y, To, scale, Tkeep);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_conv1d_c1(const float* x, int B, int Lin, int Lout, int C, const float* w, const float* bias, int relu, float* y,
                   void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !w || !y || B < 0 || B > 65535 || C < 4 || C % 4 || Lout < 1 || Lin < 4 * (Lout - 1) + 8) return MFPA_EINVAL;
  long long blocks = ((long long)Lout * (C / 4) + 255) / 256; if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(conv1d_c1_kernel, dim3((unsigned)blocks, B), dim3(256), 0, mfpa_stream(stream), x, Lin, Lout, C, w, bias, y, relu);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_convT1d_c1(const float* P, int B, int L, int C, const float* w, float bias, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!P || !w || !y || B < 0 || B > 65535 || L < 1 || C < 4 || C % 4) return MFPA_EINVAL;
  int gx = (4 * (L + 1) + 255) / 256; if (gx > 2048) gx = 2048;
  hipLaunchKernelGGL(convT1d_c1_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), P, L, C, w, bias, (const float*)nullptr, y);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_convT1d_c1_dev(const float* P, int B, int L, int C, const float* w, const float* bias_dev, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!P || !w || !bias_dev || !y || B < 0 || B > 65535 || L < 1 || C < 4 || C % 4) return MFPA_EINVAL;
  int gx = (4 * (L + 1) + 255) / 256; if (gx > 2048) gx = 2048;
  hipLaunchKernelGGL(convT1d_c1_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), P, L, C, w, 0.f, bias_dev, y);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
