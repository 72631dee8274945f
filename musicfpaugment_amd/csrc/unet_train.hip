// Training-step kernels of the UNet denoiser for MI355X (gfx950): the pieces of
// Trainer.train_epoch's spec branch (training/train.py:257-317 of the reference) that are not the
// convolution itself (csrc/unet.hip and the kernels' own files) or its weight gradient (csrc/unet_wgrad.hip):
//
//   BatchNorm batch statistics + running-stat update, BN/ReLU/max-pool forward glue,
//   BN/ReLU backward (reduce + apply), max-pool backward,
//   bias / OutConv gradients, L1 loss forward+backward, fused Adam.
//
// Design: a layer's BatchNorm+ReLU output is never materialised.  The convolution writes its raw
// output z, one bandwidth pass reduces the batch statistics into a per-channel (scale, shift),
// and every consumer (next conv, transposed conv, pool, weight-gradient kernel) applies
// relu(z*scale+shift) while loading.  Reductions are two-stage float64 (per-workgroup partials,
// then one finishing workgroup) so they are deterministic and independent of the grid.
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"

namespace {

using mfpa_tile::bf16x4;
using mfpa_tile::f32x4;

constexpr int RED_BLOCKS = 1024;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }

// ------------------------------------------------------------------ the BatchNorm + ReLU (+ dropout) backward of one element, written once
// Every kernel below that reduces or applies that backward -- on its own or fused into the pool / OutConv backward -- goes through these,
// so the fused and unfused forms of the step stay bit-compatible by construction.
struct BnCh4 {                       // one channel quad's constants of the forward: y = relu(z*scale+shift), xhat = (z-mean)*invstd
  f32x4 scale, shift, mean, invstd;
};
__device__ __forceinline__ BnCh4 bn_ld(const float* scale, const float* shift, const float* mean, const float* invstd, int c) {
  return BnCh4{ld4(scale + c), ld4(shift + c), ld4(mean + c), ld4(invstd + c)};
}
struct BnCoef4 {                     // ... and of the backward: dz = ka*g - kb - kc*xhat (bn_bwd_coef's [3][C])
  f32x4 ka, kb, kc;
};
__device__ __forceinline__ BnCoef4 bn_coef_ld(const float* coef, int C, int c) {
  return BnCoef4{ld4(coef + c), ld4(coef + C + c), ld4(coef + 2 * C + c)};
}
// g = d * [z*scale+shift > 0], then the stateless dropout mask of element idx (drop_thresh 0: no dropout)
__device__ __forceinline__ float bn_gate(float d, float z, const BnCh4& ch, int k, unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                                         unsigned long long idx) {
  float g = (z * ch.scale[k] + ch.shift[k] > 0.f) ? d : 0.f;
  if (drop_thresh) g = mfpa_keep(drop_seed, drop_thresh, idx) ? g * drop_scale : 0.f;
  return g;
}
__device__ __forceinline__ float bn_xhat(float z, const BnCh4& ch, int k) { return (z - ch.mean[k]) * ch.invstd[k]; }
__device__ __forceinline__ float bn_dz(const BnCoef4& co, int k, float g, float xh) { return co.ka[k] * g - co.kb[k] - co.kc[k] * xh; }

// one pixel's channel quad (incoming gradient d, raw activation z, first element idx0) into the backward's pair sums {sum g, sum g*xhat}:
// float64 inside a workgroup (the two sums cancel heavily, and a float32 running sum over a row's ~500 pixels would put its rounding,
// relative to sum |g|, into dgamma / dbeta / dz of every engine precision)
__device__ __forceinline__ void bn_sums4(double (&s0)[4], double (&s1)[4], const f32x4& d, const f32x4& z, const BnCh4& ch, unsigned drop_seed,
                                         unsigned drop_thresh, float drop_scale, unsigned long long idx0) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float g = bn_gate(d[k], z[k], ch, k, drop_seed, drop_thresh, drop_scale, idx0 + k);
    s0[k] += (double)g;
    s1[k] += (double)g * (double)bn_xhat(z[k], ch, k);
  }
}
// ... and through the backward formula: its dz
__device__ __forceinline__ f32x4 bn_dz4(const f32x4& d, const f32x4& z, const BnCh4& ch, const BnCoef4& co, unsigned drop_seed,
                                        unsigned drop_thresh, float drop_scale, unsigned long long idx0) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k)
    o[k] = bn_dz(co, k, bn_gate(d[k], z[k], ch, k, drop_seed, drop_thresh, drop_scale, idx0 + k), bn_xhat(z[k], ch, k));
  return o;
}

__device__ __forceinline__ bf16x4 to_bf16x4(const f32x4& v) {
  bf16x4 h;
#pragma unroll
  for (int k = 0; k < 4; ++k) h[k] = (__bf16)v[k];
  return h;
}
__device__ __forceinline__ void st_bf16x4(__bf16* dst, const f32x4& v) { *reinterpret_cast<bf16x4*>(dst) = to_bf16x4(v); }

// Workgroup combine of per-thread pair sums: thread t holds s0[4], s1[4] of channel quad t % lanes for pixel-row t / lanes (256 % lanes == 0).
// The row-0 thread of each quad (t < lanes: the owner) adds rows 1 .. rows-1 to its own in ascending order -- fixed, so deterministic -- and
// gets true; it then stores with one of the two forms below.  A caller that combines again must __syncthreads() first.
__device__ __forceinline__ bool wg_pair_sums(double (&s0)[4], double (&s1)[4], int lanes, int rows) {
  __shared__ double sh[256 * 8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    sh[threadIdx.x * 8 + k] = s0[k];
    sh[threadIdx.x * 8 + 4 + k] = s1[k];
  }
  __syncthreads();
  if ((int)threadIdx.x >= lanes) return false;
  for (int r = 1; r < rows; ++r)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      s0[k] += sh[(r * lanes + threadIdx.x) * 8 + k];
      s1[k] += sh[(r * lanes + threadIdx.x) * 8 + 4 + k];
    }
  return true;
}
// this workgroup's row of `part` (rows x 2 x C float32, the layout of the convolutions' stats_part, finished in float64 by
// conv_stats_rows_kernel): the float64 sums are rounded to float32 here, once
__device__ __forceinline__ void st_part_row(float* __restrict__ part, int C, int cq, const double (&s0)[4], const double (&s1)[4]) {
  float* row = part + (size_t)blockIdx.x * 2 * C;
  *reinterpret_cast<f32x4*>(row + 4 * cq) = f32x4{(float)s0[0], (float)s0[1], (float)s0[2], (float)s0[3]};
  *reinterpret_cast<f32x4*>(row + C + 4 * cq) = f32x4{(float)s1[0], (float)s1[1], (float)s1[2], (float)s1[3]};
}
// partial[(blk*C + c)*NV + v]: NV float64 sums per channel, as they are
template <int NV>
__device__ __forceinline__ void st_partial(double* __restrict__ partial, int C, int cq, const double (&s0)[4], const double (&s1)[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double* dst = partial + ((size_t)blockIdx.x * C + 4 * cq + k) * NV;
    dst[0] = s0[k];
    if (NV == 2) dst[1] = s1[k];
  }
}

// ------------------------------------------------------------------ per-channel sums over pixels
// partial[(blk*C + c)*NV + v]: NV float64 sums per channel.  MODE 0: {sum z, sum z^2} (BN statistics);
// MODE 1: {sum g, sum g*xhat} with g = dy*[z*scale+shift > 0], xhat = (z-mean)*invstd (BN backward);
// MODE 2: {sum x} (bias gradient).
template <int MODE>
__global__ __launch_bounds__(256) void chan_reduce_kernel(const float* __restrict__ x, const float* __restrict__ z,
                                                          long long npix, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift,
                                                          const float* __restrict__ mean,
                                                          const float* __restrict__ invstd,
                                                          double* __restrict__ partial, unsigned drop_seed,
                                                          unsigned drop_thresh, float drop_scale, int z16) {
  // z16: the activation tensor (x in MODE 0, z in MODE 1) is bfloat16
  constexpr int NV = (MODE == 2) ? 1 : 2;
  const int C4 = C / 4;
  const int lanes = C4 < 256 ? C4 : 256;          // lanes across channel quads
  const int rows = 256 / lanes;                   // pixels in flight per block
  const int cq0 = threadIdx.x % lanes, prow = threadIdx.x / lanes;
  for (int cq = cq0; cq < C4; cq += lanes) {
    double s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
    BnCh4 ch = {};
    if (MODE == 1) ch = bn_ld(scale, shift, mean, invstd, 4 * cq);
    for (long long p = (long long)blockIdx.x * rows + prow; p < npix; p += (long long)gridDim.x * rows) {
      const f32x4 v = (MODE == 0) ? mfpa_ld_act4(x, (size_t)p * C + 4 * cq, z16) : ld4(x + (size_t)p * C + 4 * cq);
      if (MODE == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          s0[k] += (double)v[k];
          s1[k] += (double)v[k] * (double)v[k];
        }
      } else if (MODE == 1) {
        bn_sums4(s0, s1, v, mfpa_ld_act4(z, (size_t)p * C + 4 * cq, z16), ch, drop_seed, drop_thresh, drop_scale,
                 (unsigned long long)p * C + 4 * cq);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) s0[k] += (double)v[k];
      }
    }
    // combine the `rows` pixel-rows of this block for channel quad cq
    if (wg_pair_sums(s0, s1, lanes, rows)) st_partial<NV>(partial, C, cq, s0, s1);
    __syncthreads();
  }
}

// Finish kernels: one 64-lane wavefront per channel sums the per-workgroup float64 partials (lane-strided, then a
// fixed xor-shuffle tree: deterministic), lane 0 finalises.
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// The opening of every finish kernel: c = this wavefront's channel, s[v] = sum over the nblk blocks of partial[(blk*C + c)*NV + v];
// true for the one lane that finalises channel c.
template <int NV>
__device__ __forceinline__ bool wave_channel_sums(const double* __restrict__ partial, int nblk, int C, int& c, double (&s)[NV]) {
  c = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (c >= C) return false;
#pragma unroll
  for (int v = 0; v < NV; ++v) s[v] = 0;
  for (int b = lane; b < nblk; b += 64)
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] += partial[((size_t)b * C + c) * NV + v];
#pragma unroll
  for (int v = 0; v < NV; ++v) s[v] = wave_sum_d(s[v]);
  return lane == 0;
}

// BN statistics finish: mean, biased var -> invstd, fused (scale, shift); running stats with momentum
// (unbiased variance), exactly nn.BatchNorm2d in train mode (training/unet.py:17,20).
__global__ __launch_bounds__(256) void bn_stats_finish_kernel(const double* __restrict__ partial, int nblk, int C,
                                                              double count, float eps, float momentum,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ mean,
                                                              float* __restrict__ invstd, float* __restrict__ scale,
                                                              float* __restrict__ shift, float* __restrict__ running_mean,
                                                              float* __restrict__ running_var) {
  int c;
  double s[2];                                     // {sum z, sum z^2}
  if (!wave_channel_sums<2>(partial, nblk, C, c, s)) return;
  const double m = s[0] / count;
  double var = s[1] / count - m * m;
  if (var < 0) var = 0;
  const double is = 1.0 / sqrt(var + (double)eps);
  mean[c] = (float)m;
  invstd[c] = (float)is;
  const float sc = gamma[c] * (float)is;
  scale[c] = sc;
  shift[c] = beta[c] - (float)m * sc;
  if (running_mean) {
    const double unb = count > 1 ? var * count / (count - 1) : var;
    running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * (float)m;
    running_var[c] = (1.f - momentum) * running_var[c] + momentum * (float)unb;
  }
}

// BN backward finish: dgamma = sum g*xhat, dbeta = sum g; coefficients so that
// dz = ka*g - kb - kc*xhat  with ka = gamma*invstd, kb = ka*dbeta/N, kc = ka*dgamma/N.
// LOCAL sums (lsg, lsgx) are this rank's dgamma / dbeta (the gradient all-reduce adds the ranks); GLOBAL sums (gsg, gsgx) over `count` pixels
// of all ranks give the mean terms of the input gradient.  On one GPU they are the same pair.
__device__ __forceinline__ void bn_bwd_coef(int c, int C, double lsg, double lsgx, double gsg, double gsgx, double count,
                                            const float* __restrict__ gamma, const float* __restrict__ invstd, float* __restrict__ dgamma,
                                            float* __restrict__ dbeta, float* __restrict__ coef /* [3][C] */) {
  dgamma[c] = (float)lsgx;
  dbeta[c] = (float)lsg;
  const double ka = (double)gamma[c] * (double)invstd[c];
  coef[c] = (float)ka;
  coef[C + c] = (float)(ka * gsg / count);
  coef[2 * C + c] = (float)(ka * gsgx / count);
}

__global__ __launch_bounds__(256) void bn_bwd_finish_kernel(const double* __restrict__ partial, int nblk, int C,
                                                            double count, const float* __restrict__ gamma,
                                                            const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, float* __restrict__ coef /* [3][C] */) {
  int c;
  double s[2];                                     // {sum g, sum g*xhat}
  if (wave_channel_sums<2>(partial, nblk, C, c, s)) bn_bwd_coef(c, C, s[0], s[1], s[0], s[1], count, gamma, invstd, dgamma, dbeta, coef);
}

// SyncBN building blocks: per-channel partial pairs -> one [C][2] float64 row (the caller all-reduces it across ranks) ...
__global__ __launch_bounds__(256) void pair_sums_kernel(const double* __restrict__ partial, int nblk, int C,
                                                        double* __restrict__ sums) {
  int c;
  double s[2];
  if (wave_channel_sums<2>(partial, nblk, C, c, s)) { sums[2 * c] = s[0]; sums[2 * c + 1] = s[1]; }
}

// per-wave partial rows of conv_wd16_kernel ([rows][2][C] floats) -> (sum, sum of squares) pairs in float64: a block walks its rows with
// one channel per lane (coalesced), the blocks' results go through the two-stage float64 reduction the other statistics use
__global__ __launch_bounds__(256) void conv_stats_rows_kernel(const float* __restrict__ part, long long rows, int C,
                                                              double* __restrict__ partial) {
  const int lanes = C < 256 ? C : 256, groups = 256 / lanes;
  const int c0 = threadIdx.x % lanes, gq = threadIdx.x / lanes;
  __shared__ double sh[2 * 256];
  for (int c = c0; c < C; c += lanes) {
    double s = 0, q = 0;
    for (long long r = (long long)blockIdx.x * groups + gq; r < rows; r += (long long)gridDim.x * groups) {
      s += (double)part[(size_t)r * 2 * C + c];
      q += (double)part[(size_t)r * 2 * C + C + c];
    }
    sh[threadIdx.x] = s; sh[256 + threadIdx.x] = q;
    __syncthreads();
    if (gq == 0) {
      for (int k = 1; k < groups; ++k) { s += sh[k * lanes + c0]; q += sh[256 + k * lanes + c0]; }
      partial[((size_t)blockIdx.x * C + c) * 2] = s;
      partial[((size_t)blockIdx.x * C + c) * 2 + 1] = q;
    }
    __syncthreads();
  }
}

// ... and the backward finish from the all-reduced [C][2] rows: LOCAL and GLOBAL sums as bn_bwd_coef takes them.
__global__ __launch_bounds__(256) void bn_bwd_finish_sync_kernel(const double* __restrict__ local, const double* __restrict__ global,
                                                                 int C, double count, const float* __restrict__ gamma,
                                                                 const float* __restrict__ invstd, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, float* __restrict__ coef) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  bn_bwd_coef(c, C, local[2 * c], local[2 * c + 1], global[2 * c], global[2 * c + 1], count, gamma, invstd, dgamma, dbeta, coef);
}

__global__ __launch_bounds__(256) void colsum_finish_kernel(const double* __restrict__ partial, int nblk, int C,
                                                            float* __restrict__ out) {
  int c;
  double s[1];
  if (wave_channel_sums<1>(partial, nblk, C, c, s)) out[c] = (float)s[0];
}

// dy <- dz in place (BatchNorm + ReLU backward), all per-channel constants precomputed.
// RANK1: the incoming gradient is the OutConv's, dy[p][c] = dpred[p] * w1[c] (training/unet.py:94-96 backward): it is formed here from the
// (B, H, W) dpred and the 64 weights instead of being written by mfpa_outconv_bwd and read back (2 x 1.06 GB per 64-clip step); dz goes to `dy`.
template <bool RANK1>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(float* __restrict__ dy, const float* __restrict__ z,
                                                           long long npix, int C, const float* __restrict__ scale,
                                                           const float* __restrict__ shift,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ coef, unsigned drop_seed,
                                                           unsigned drop_thresh, float drop_scale, __bf16* __restrict__ dz16,
                                                           int write_f32, const float* __restrict__ dpred, const float* __restrict__ w1, int z16, int dy16) {
  // dy16: the incoming gradient is a bfloat16 tensor (the input-gradient convolution left it so: mfpa_conv_desc.y_bf16 without y); then only dz16 is written
  const int C4 = C / 4;                      // a power of two (checked on the host): no 64-bit division per element
  const int c4_shift = __ffs(C4) - 1;
  const long long total = npix * C4;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int cq = (int)(e & (C4 - 1));
    const BnCh4 ch = bn_ld(scale, shift, mean, invstd, 4 * cq);
    const BnCoef4 co = bn_coef_ld(coef, C, 4 * cq);
    f32x4 g;
    if (RANK1) {
      const float gp = dpred[e >> c4_shift];              // (C4 is a power of two: no 64-bit division per element)
      const f32x4 wv = ld4(w1 + 4 * cq);
#pragma unroll
      for (int k = 0; k < 4; ++k) g[k] = gp * wv[k];
    } else {
      g = mfpa_ld_act4(dy, (size_t)e * 4, dy16);
    }
    const f32x4 o = bn_dz4(g, mfpa_ld_act4(z, (size_t)e * 4, z16), ch, co, drop_seed, drop_thresh, drop_scale, (unsigned long long)e * 4);
    if (write_f32) *reinterpret_cast<f32x4*>(dy + e * 4) = o;   // (0: every consumer of dz reads the bf16 copy -- the plain-bf16 train step)
    if (dz16) st_bf16x4(dz16 + e * 4, o);    // the bf16 copy the weight-gradient kernel reads (wgrad precision 3)
  }
}

// The same pass for bfloat16 z (the plain-bf16 step's activations), EIGHT channels per thread: z arrives as one 16-byte load, dy as two, the
// bf16 dz leaves as one 16-byte store (with four channels per thread the 8-byte z loads / dz stores ran the pass at 4.4 TB/s).
template <bool RANK1>
__global__ __launch_bounds__(256) void bn_bwd_apply8_kernel(float* __restrict__ dy, const unsigned short* __restrict__ z16,
                                                            long long npix, int C, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, const float* __restrict__ mean,
                                                            const float* __restrict__ invstd, const float* __restrict__ coef,
                                                            unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                                                            __bf16* __restrict__ dz16, int write_f32,
                                                            const float* __restrict__ dpred, const float* __restrict__ w1) {
  const int C8 = C / 8;                      // a power of two (checked on the host)
  const int c8_shift = __ffs(C8) - 1;
  const long long total = npix * C8;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c0 = 8 * (int)(e & (C8 - 1));
    f32x4 g[2];
    if (RANK1) {
      const float gp = dpred[e >> c8_shift];                // (C8 is a power of two: no 64-bit division per element)
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const f32x4 wv = ld4(w1 + c0 + 4 * h);
#pragma unroll
        for (int k = 0; k < 4; ++k) g[h][k] = gp * wv[k];
      }
    } else {
      g[0] = ld4(dy + e * 8);
      g[1] = ld4(dy + e * 8 + 4);
    }
    const uint4 zr = *reinterpret_cast<const uint4*>(z16 + e * 8);
    const unsigned zu[4] = {zr.x, zr.y, zr.z, zr.w};
    f32x4 o[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x4 zz = {__uint_as_float(zu[2 * h] << 16), __uint_as_float(zu[2 * h] & 0xffff0000u), __uint_as_float(zu[2 * h + 1] << 16),
                        __uint_as_float(zu[2 * h + 1] & 0xffff0000u)};
      o[h] = bn_dz4(g[h], zz, bn_ld(scale, shift, mean, invstd, c0 + 4 * h), bn_coef_ld(coef, C, c0 + 4 * h), drop_seed, drop_thresh,
                    drop_scale, (unsigned long long)e * 8 + 4 * h);
    }
    if (write_f32) {
      *reinterpret_cast<f32x4*>(dy + e * 8) = o[0];
      *reinterpret_cast<f32x4*>(dy + e * 8 + 4) = o[1];
    }
    if (dz16) {
      const uint2 a = __builtin_bit_cast(uint2, to_bf16x4(o[0])), b = __builtin_bit_cast(uint2, to_bf16x4(o[1]));
      *reinterpret_cast<uint4*>(dz16 + e * 8) = uint4{a.x, a.y, b.x, b.y};
    }
  }
}

// p = maxpool2(relu(z*scale+shift)), floor (unet.py:34 after the BN+ReLU of the DoubleConv).
__global__ __launch_bounds__(256) void bn_relu_pool_kernel(const float* __restrict__ z, int B, int H, int W, int C,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ shift, float* __restrict__ p,
                                                           unsigned drop_seed, unsigned drop_thresh, float drop_scale, int z16, int p16) {
  // z16: z is bfloat16; p16: the pooled activation leaves as bfloat16 (the next convolution's operand as it is: mfpa_conv_desc.x0_is_bf16)
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const int b = blockIdx.x / Ho, yo = blockIdx.x % Ho;     // one workgroup per pooled row: 32-bit index math only
  for (int e32 = threadIdx.x; e32 < Wo * C4; e32 += 256) {
    const int cq = e32 % C4, xo = e32 / C4;
    const size_t e = ((size_t)blockIdx.x * Wo + xo) * C4 + cq;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * cq);
    const f32x4 sf = *reinterpret_cast<const f32x4*>(shift + 4 * cq);
    const size_t base = (((size_t)b * H + 2 * yo) * W + 2 * xo) * C + 4 * cq;
    f32x4 m = {0.f, 0.f, 0.f, 0.f};   // relu output is >= 0
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t off = ((size_t)(t >> 1) * W + (t & 1)) * C;
      const f32x4 v = mfpa_ld_act4(z, base + off, z16);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float y = v[k] * sc[k] + sf[k];
        if (drop_thresh) y = (y > 0.f && mfpa_keep(drop_seed, drop_thresh, (unsigned long long)base + off + k)) ? y * drop_scale : 0.f;
        m[k] = y > m[k] ? y : m[k];
      }
    }
    if (p16) st_bf16x4(reinterpret_cast<__bf16*>(p) + e * 4, m);
    else *reinterpret_cast<f32x4*>(p + e * 4) = m;
  }
}

// dy_full += route(dp): the gradient of a pooled cell goes to the first maximum of its 2x2 window of
// y = relu(z*scale+shift) (scan order (0,0),(0,1),(1,0),(1,1), strict >), as torch's max_pool2d backward.
// SUMS: the pass also holds everything the BatchNorm backward of this very layer reduces next -- the finished dy and z of every pixel --
// so it forms that reduction's per-channel partial sums {sum g, sum g * xhat} (bn_sums4: chan_reduce_kernel<1>'s terms) for its two rows, the
// odd last column and (last workgroup of a clip) the odd last row included, and writes them as one row of `part` (st_part_row, finished in
// float64 by mfpa_conv_stats_reduce): the separate reduction pass over dy and z (2.1 GB at the first level) is not run.
// MODE 0: dy += route(dp); 1: ... and the BatchNorm-backward partial sums (SUMS); 2 (round 5): NOTHING of dy is written -- the pass forms
// g = dy + route(dp) again and applies the BatchNorm + ReLU backward to it on the spot (coef = bn_bwd_finish_kernel's [3][C]), writing only the
// bfloat16 dz: with MODE 1 run as a pure reduction in front (`nowrite`), the finished float32 dy of an encoder block never exists.
// d16: dy (the skip path's gradient) is a bfloat16 tensor (then nothing can be written back into it: nowrite or MODE 2).
template <int MODE>
__global__ __launch_bounds__(256) void maxpool_bwd_add_kernel(const float* __restrict__ z, int B, int H, int W, int C,
                                                              const float* __restrict__ scale,
                                                              const float* __restrict__ shift,
                                                              const float* __restrict__ dp, float* __restrict__ dy,
                                                              unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                                                              const float* __restrict__ mean, const float* __restrict__ invstd,
                                                              float* __restrict__ part, int z16, int d16, int nowrite,
                                                              const float* __restrict__ coef, __bf16* __restrict__ dz16) {
  constexpr bool SUMS = MODE == 1;
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const int b = blockIdx.x / Ho, yo = blockIdx.x % Ho;     // one workgroup per pooled row: 32-bit index math only
  // MODE >= 1: 256 % C4 == 0 (checked by the launcher), so a thread meets ONE channel quad in all its trips: tid % C4
  double s0[4] = {0., 0., 0., 0.}, s1[4] = {0., 0., 0., 0.};
  BnCh4 ch = {};
  BnCoef4 co = {};
  if (MODE >= 1) {
    ch = bn_ld(scale, shift, mean, invstd, 4 * (threadIdx.x % C4));
    if (MODE == 2) co = bn_coef_ld(coef, C, 4 * (threadIdx.x % C4));
  }
  // one pixel's four channels (its finished gradient d, its z, its first element elem0): MODE 1 into the sums, MODE 2 through the
  // BatchNorm + ReLU (+ dropout) backward, bf16 dz out
  auto finish = [&](const f32x4& d, const f32x4& v, size_t elem0) {
    if (SUMS) bn_sums4(s0, s1, d, v, ch, drop_seed, drop_thresh, drop_scale, elem0);
    if (MODE == 2) st_bf16x4(dz16 + elem0, bn_dz4(d, v, ch, co, drop_seed, drop_thresh, drop_scale, elem0));
  };
  for (int e32 = threadIdx.x; e32 < Wo * C4; e32 += 256) {
    const int cq = e32 % C4, xo = e32 / C4;
    const size_t e = ((size_t)blockIdx.x * Wo + xo) * C4 + cq;
    const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * cq);
    const f32x4 sf = *reinterpret_cast<const f32x4*>(shift + 4 * cq);
    const size_t base = (((size_t)b * H + 2 * yo) * W + 2 * xo) * C + 4 * cq;
    const f32x4 g = *reinterpret_cast<const f32x4*>(dp + e * 4);
    float best[4];
    int arg[4];
    f32x4 vz[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const f32x4 v = mfpa_ld_act4(z, base + ((size_t)(t >> 1) * W + (t & 1)) * C, z16);
      vz[t] = v;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float y = v[k] * sc[k] + sf[k];
        y = y > 0.f ? y : 0.f;
        if (drop_thresh) y = mfpa_keep(drop_seed, drop_thresh, (unsigned long long)base + ((size_t)(t >> 1) * W + (t & 1)) * C + k) ? y * drop_scale : 0.f;
        if (t == 0 || y > best[k]) {
          best[k] = y;
          arg[k] = t;
        }
      }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t off = base + ((size_t)(t >> 1) * W + (t & 1)) * C;
      f32x4 cur = mfpa_ld_act4(dy, off, d16);
#pragma unroll
      for (int k = 0; k < 4; ++k) cur[k] += (arg[k] == t) ? g[k] : 0.f;
      if (MODE != 2 && !nowrite) *reinterpret_cast<f32x4*>(dy + off) = cur;
      finish(cur, vz[t], off);
    }
  }
  if (MODE >= 1) {
    if (W & 1) {                                            // the last column lies in no window: its gradient is the skip path's alone
      for (int e32 = threadIdx.x; e32 < 2 * C4; e32 += 256) {
        const int cq = e32 % C4, r = e32 / C4;
        const size_t off = (((size_t)b * H + 2 * yo + r) * W + (W - 1)) * C + 4 * cq;
        finish(mfpa_ld_act4(dy, off, d16), mfpa_ld_act4(z, off, z16), off);
      }
    }
    if ((H & 1) && yo == Ho - 1) {                          // ... and so does the last row: the clip's last workgroup takes it
      for (int e32 = threadIdx.x; e32 < W * C4; e32 += 256) {
        const int cq = e32 % C4, x = e32 / C4;
        const size_t off = (((size_t)b * H + (H - 1)) * W + x) * C + 4 * cq;
        finish(mfpa_ld_act4(dy, off, d16), mfpa_ld_act4(z, off, z16), off);
      }
    }
  }
  if (SUMS && wg_pair_sums(s0, s1, C4, 256 / C4)) st_part_row(part, C, threadIdx.x, s0, s1);
}

// ------------------------------------------------------------------ OutConv (1x1 -> 1 class) in training
// pred[p] = sum_c relu(z[p][c]*scale[c]+shift[c]) * w[c] + bias
__global__ __launch_bounds__(256) void outconv_fwd_kernel(const float* __restrict__ z, long long npix, int C,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ w,
                                                          const float* __restrict__ bias, float* __restrict__ pred, int z16) {
  const int lpp = C / 4, sub = threadIdx.x % lpp, pl = threadIdx.x / lpp, ppb = 256 / lpp;
  const f32x4 wv = *reinterpret_cast<const f32x4*>(w + 4 * sub);
  const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * sub);
  const f32x4 sf = *reinterpret_cast<const f32x4*>(shift + 4 * sub);
  const float b0 = bias[0];
  const long long iters = (npix + (long long)gridDim.x * ppb - 1) / ((long long)gridDim.x * ppb);
  for (long long it = 0; it < iters; ++it) {
    const long long p = (it * gridDim.x + blockIdx.x) * ppb + pl;
    float s = 0.f;
    if (p < npix) {
      const f32x4 v = mfpa_ld_act4(z, (size_t)p * C + 4 * sub, z16);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float y = v[k] * sc[k] + sf[k];
        s += (y > 0.f ? y : 0.f) * wv[k];
      }
    }
    for (int o = lpp >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (sub == 0 && p < npix) pred[p] = s + b0;
  }
}

// dy[p][c] = dpred[p]*w[c];  partial[blk][c] = sum_p dpred[p]*y[p][c] (c < C), partial[blk][C] = sum_p dpred[p]
// SUMS: dy is not written (the BatchNorm backward forms it again from dpred and w: bn_bwd_apply_kernel<RANK1>); instead the pass, which holds
// z and dy of every element anyway, also forms the partial sums of that BatchNorm backward (bn_sums4; the OutConv's input carries no dropout:
// threshold 0) as one row of `part` (blocks x 2 x C float, the convolutions' stats_part layout) per workgroup.
template <bool SUMS>
__global__ __launch_bounds__(256) void outconv_bwd_kernel(const float* __restrict__ z, const float* __restrict__ dpred,
                                                          long long npix, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, const float* __restrict__ w,
                                                          float* __restrict__ dy, double* __restrict__ partial,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          float* __restrict__ part, int z16) {
  const int lpp = C / 4, sub = threadIdx.x % lpp, pl = threadIdx.x / lpp, ppb = 256 / lpp;
  const f32x4 wv = ld4(w + 4 * sub);
  BnCh4 ch = {};
  ch.scale = ld4(scale + 4 * sub);
  ch.shift = ld4(shift + 4 * sub);
  if (SUMS) {
    ch.mean = ld4(mean + 4 * sub);
    ch.invstd = ld4(invstd + 4 * sub);
  }
  double sw[4] = {0, 0, 0, 0}, sb = 0, s0[4] = {0, 0, 0, 0}, s1[4] = {0, 0, 0, 0};
  for (long long p = (long long)blockIdx.x * ppb + pl; p < npix; p += (long long)gridDim.x * ppb) {
    const float g = dpred[p];
    const f32x4 v = mfpa_ld_act4(z, (size_t)p * C + 4 * sub, z16);
    f32x4 o;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float y = v[k] * ch.scale[k] + ch.shift[k];
      sw[k] += (double)g * (double)(y > 0.f ? y : 0.f);
      o[k] = g * wv[k];
    }
    if (SUMS) bn_sums4(s0, s1, o, v, ch, 0u, 0u, 1.f, 0ull);
    else *reinterpret_cast<f32x4*>(dy + (size_t)p * C + 4 * sub) = o;
    if (sub == 0) sb += (double)g;
  }
  if (SUMS && wg_pair_sums(s0, s1, lpp, ppb)) st_part_row(part, C, sub, s0, s1);
  __shared__ double sh[256 * 5];
#pragma unroll
  for (int k = 0; k < 4; ++k) sh[threadIdx.x * 5 + k] = sw[k];
  sh[threadIdx.x * 5 + 4] = sb;
  __syncthreads();
  if (pl == 0) {
    for (int r = 1; r < ppb; ++r) {
#pragma unroll
      for (int k = 0; k < 4; ++k) sw[k] += sh[(r * lpp + sub) * 5 + k];
      if (sub == 0) sb += sh[(r * lpp) * 5 + 4];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) partial[(size_t)blockIdx.x * (C + 1) + 4 * sub + k] = sw[k];
    if (sub == 0) partial[(size_t)blockIdx.x * (C + 1) + C] = sb;
  }
}

// ------------------------------------------------------------------ L1 loss (mean), float32 pred vs float64 target
// sum of one float64 per thread over a 256-thread workgroup (LDS tree, fixed order); the result is thread 0's
__device__ __forceinline__ double block_sum_d(double s) {
  __shared__ double sh[256];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

__global__ __launch_bounds__(256) void l1_kernel(const float* __restrict__ pred, const double* __restrict__ target,
                                                 long long n, float* __restrict__ dpred, double* __restrict__ partial) {
  double s = 0;
  const float inv = (float)(1.0 / (double)n);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double d = (double)pred[i] - target[i];
    s += fabs(d);
    if (dpred) dpred[i] = d > 0 ? inv : (d < 0 ? -inv : 0.f);
  }
  s = block_sum_d(s);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ void l1_finish_kernel(const double* __restrict__ partial, int nblk, long long n, double* __restrict__ loss) {
  double s = 0;
  for (int i = threadIdx.x; i < nblk; i += 256) s += partial[i];
  s = block_sum_d(s);
  if (threadIdx.x == 0) loss[0] = s / (double)n;
}

// ------------------------------------------------------------------ Adam (torch.optim.Adam, no weight decay, no amsgrad)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                   float* __restrict__ m, float* __restrict__ v, long long n, float lr,
                                                   float b1, float b2, float eps, float bc1, float bc2_sqrt,
                                                   float grad_scale) {
  const float step_size = lr / bc1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float gi = g[i] * grad_scale;
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] = p[i] - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
  }
}

inline int grid_for(long long work, int per_block = 256, int cap = 256 * 16) {
  long long b = (work + per_block - 1) / per_block;
  if (b > cap) b = cap;
  return (int)(b < 1 ? 1 : b);
}

// Convolution weights [tap][Co][Ci] (the master fp32 layout) -> the operand image a conv launch reads: precision 0: [tap][row n][K]
// floats; precision 1: the bf16x3 image of csrc/unet_mfma.hip, [tap][chunk of 32 k][row n][128 B = 32 bf16 hi | 32 bf16 lo in 16-byte
// slots XOR-swizzled by the row] (what ops_unet.split_bf16x3 builds on the host).  TR = false: n = co in [row0, row0 + nrows), k = ci (forward).  TR = true: the input-gradient operand --
// tap t reads source tap taps-1-t when taps == 9 (the 3x3 kernel flipped; the 2x2 transposed conv keeps its tap), n = ci in
// [row0, row0 + nrows), k = co.  One workgroup per 32 x 32 (n, k) tile and tap, transposed through LDS so both sides coalesce.
template <bool TR>
__device__ __forceinline__ void pack_conv_weights_tile(float (*tile)[33], const float* __restrict__ w, int taps, int Co, int Ci, int row0,
                                                       int nrows, int precision, float* __restrict__ out, int kx, int ny, int t) {
  const int k0 = kx * 32, n0 = ny * 32;
  const int ts = (TR && taps == 9) ? taps - 1 - t : t;
  const int K = TR ? Co : Ci;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;           // 32 x 8
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    // source element (n = n0 + .., k = k0 + ..): TR: w[ts][co = k][ci = row0 + n], contiguous along n; else w[ts][co = row0 + n][ci = k]
    if (TR) tile[r][tx] = w[((size_t)ts * Co + (k0 + r)) * Ci + row0 + n0 + tx];          // tile[k][n]
    else tile[r][tx] = w[((size_t)ts * Co + (row0 + n0 + r)) * Ci + k0 + tx];             // tile[n][k]
  }
  __syncthreads();
#pragma unroll
  for (int r = ty; r < 32; r += 8) {
    const float v = TR ? tile[tx][r] : tile[r][tx];                  // (n = n0 + r, k = k0 + tx)
    if (precision == 0) {
      out[((size_t)t * nrows + n0 + r) * K + k0 + tx] = v;             // [tap][row][K] floats
    } else if (precision == 3) {
      // the fragment-ordered image of the 16 x 16 x 32 weights-direct kernel (conv_wd16_kernel, ops_unet.split_bf16x3_frag(w, 2)):
      // [tap][chunk][row / 16][hi | lo][lane = (k / 8) * 16 + row % 16][k % 8]
      const int row = n0 + r, k = tx;
      __bf16* ob = reinterpret_cast<__bf16*>(out) + ((((size_t)t * (K / 32) + k0 / 32) * (nrows / 16) + row / 16) << 10);
      const __bf16 hi = (__bf16)v;
      const __bf16 lo = (__bf16)(v - (float)hi);
      const int at = (((k >> 3) * 16 + (row & 15)) << 3) + (k & 7);
      ob[at] = hi;
      ob[at + 512] = lo;
    } else {
      // the bf16x3 image of csrc/unet_mfma.hip: [tap][chunk][row][8 slots of 16 B], logical slot (hi: 0-3, lo: 4-7) at physical slot ^ swz(row)
      const int row = n0 + r, swz = (row >> 1) & 7;
      __bf16* ob = reinterpret_cast<__bf16*>(out + (((size_t)t * (K / 32) + k0 / 32) * nrows + row) * 32);
      const __bf16 hi = (__bf16)v;
      const __bf16 lo = (__bf16)(v - (float)hi);
      ob[(((tx >> 3)) ^ swz) * 8 + (tx & 7)] = hi;
      ob[((4 + (tx >> 3)) ^ swz) * 8 + (tx & 7)] = lo;
    }
  }
}

template <bool TR>
__global__ __launch_bounds__(256) void pack_conv_weights_kernel(const float* __restrict__ w, int taps, int Co, int Ci, int row0,
                                                                int nrows, int precision, float* __restrict__ out) {
  __shared__ float tile[32][33];
  pack_conv_weights_tile<TR>(tile, w, taps, Co, Ci, row0, nrows, precision, out, blockIdx.x, blockIdx.y, blockIdx.z);
}

// Every operand image of a training step in ONE launch (mfpa_pack_conv_weights_batch): workgroup -> (job, tile) through the jobs' tile
// prefix (tile0; a job's tiles are (K / 32) x (nrows / 32) x taps, k fastest), then the single-launch kernel's tile code.
__global__ __launch_bounds__(256) void pack_conv_weights_batch_kernel(const mfpa_pack_job* __restrict__ jobs, int njobs) {
  __shared__ float tile[32][33];
  int lo = 0, hi = njobs - 1;                                // the last job whose tile0 <= blockIdx.x
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].tile0 <= (long long)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const mfpa_pack_job jb = jobs[lo];
  const int K = jb.flip_transpose ? jb.Co : jb.Ci;
  int r = (int)((long long)blockIdx.x - jb.tile0);
  const int kx = r % (K / 32); r /= (K / 32);
  const int ny = r % (jb.nrows / 32);
  const int t = r / (jb.nrows / 32);
  if (t >= jb.taps) return;
  if (jb.flip_transpose) pack_conv_weights_tile<true>(tile, jb.w, jb.taps, jb.Co, jb.Ci, jb.row0, jb.nrows, jb.precision, jb.out, kx, ny, t);
  else pack_conv_weights_tile<false>(tile, jb.w, jb.taps, jb.Co, jb.Ci, jb.row0, jb.nrows, jb.precision, jb.out, kx, ny, t);
}


// Activation -> bf16 copy for the bf16-operand weight-gradient kernel: out[e] = bf16(act(z[e])), act = the consumer's on-load
// transform (relu(z * scale[c] + shift[c]), then the stateless dropout mask of element e) or the identity (scale == NULL).
__global__ __launch_bounds__(256) void act_to_bf16_kernel(const float* __restrict__ z, long long n4, int C, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, unsigned drop_seed, unsigned drop_thresh,
                                                          float drop_scale, __bf16* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    f32x4 v = *reinterpret_cast<const f32x4*>(z + 4 * i);
    if (scale) {
      const int c = (int)((4 * i) % C);
      const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c), sh = *reinterpret_cast<const f32x4*>(shift + c);
      v = v * sc + sh;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
      if (drop_thresh) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(drop_seed, drop_thresh, (unsigned long long)(4 * i + k)) ? v[k] * drop_scale : 0.f;
      }
    }
    st_bf16x4(out + 4 * i, v);
  }
}

// ------------------------------------------------------------------ host side: shape predicates and launch sequences, each written once
// chan_reduce_kernel's shapes: whole channel quads, and a block's 256 threads split evenly over them (or they over the threads)
bool bn_shape_ok(long long npix, int C) {
  return npix >= 0 && C >= 4 && C % 4 == 0 && !(C / 4 < 256 && 256 % (C / 4) != 0) && !(C / 4 > 256 && (C / 4) % 256 != 0);
}
// conv_stats_rows_kernel's: the same split with one channel per lane
bool rows_shape_ok(int C) { return C >= 1 && !(C < 256 && 256 % C) && !(C > 256 && C % 256); }
// the OutConv kernels': one pixel's C / 4 lanes are a power-of-two slice of a wavefront or of the block
bool outconv_shape_ok(long long npix, int C) { return npix >= 0 && C >= 4 && C <= 256 && !(C & (C - 1)); }
// the pool kernels': at least one window, whole channel quads, one workgroup per pooled row in a 32-bit grid
bool pool_shape_ok(int B, int H, int W, int C) {
  return B >= 0 && H >= 2 && W >= 2 && C >= 4 && C % 4 == 0 && (long long)B * (H / 2) <= 0x7fffffffLL;
}

// chan_reduce_kernel<MODE> over npix pixels into `workspace`; returns the number of block partials a finish kernel has to sum
template <int MODE>
int reduce_pixels(hipStream_t s, const float* x, const float* z, long long npix, int C, const float* scale, const float* shift,
                  const float* mean, const float* invstd, double* workspace, unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                  int z16) {
  const int rows = 256 / (C / 4 < 256 ? C / 4 : 256);
  const int nblk = grid_for(npix, rows * 8, RED_BLOCKS);
  hipLaunchKernelGGL(chan_reduce_kernel<MODE>, dim3(nblk), dim3(256), 0, s, x, z, npix, C, scale, shift, mean, invstd, workspace, drop_seed,
                     drop_thresh, drop_scale, z16);
  return nblk;
}
// conv_stats_rows_kernel over the rows of `part`, likewise
int reduce_rows(hipStream_t s, const float* part, long long rows, int C, double* workspace) {
  const int groups = 256 / (C < 256 ? C : 256);
  const int nblk = grid_for(rows, groups * 8, RED_BLOCKS);
  hipLaunchKernelGGL(conv_stats_rows_kernel, dim3(nblk), dim3(256), 0, s, part, rows, C, workspace);
  return nblk;
}

template <bool RANK1>
void launch_bn_bwd_apply(hipStream_t s, float* dy, const float* z, long long npix, int C, const float* scale, const float* shift,
                         const float* mean, const float* invstd, const float* coef, unsigned drop_seed, unsigned drop_thresh,
                         float drop_scale, void* dz_bf16, int write_f32, const float* dpred, const float* w1, int z16, int dy16) {
  __bf16* dz16 = reinterpret_cast<__bf16*>(dz_bf16);
  if (z16 && !dy16 && C % 8 == 0)
    hipLaunchKernelGGL(bn_bwd_apply8_kernel<RANK1>, dim3(grid_for(npix * (C / 8))), dim3(256), 0, s, dy, reinterpret_cast<const unsigned short*>(z),
                       npix, C, scale, shift, mean, invstd, coef, drop_seed, drop_thresh, drop_scale, dz16, write_f32, dpred, w1);
  else
    hipLaunchKernelGGL(bn_bwd_apply_kernel<RANK1>, dim3(grid_for(npix * (C / 4))), dim3(256), 0, s, dy, z, npix, C, scale, shift, mean, invstd,
                       coef, drop_seed, drop_thresh, drop_scale, dz16, write_f32, dpred, w1, z16, dy16);
}

// The single-GPU BatchNorm + ReLU backward from block partials already in `workspace`: dgamma / dbeta / coefficients, then the apply pass
int bn_bwd_finish_apply_local(hipStream_t s, int nblk, float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                              const float* shift, const float* mean, const float* invstd, float* dgamma, float* dbeta, float* coef,
                              double* workspace, unsigned drop_seed, unsigned drop_thresh, float drop_scale, void* dz_bf16, int write_f32,
                              int z16, int dy16) {
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, (double)npix, gamma, invstd, dgamma,
                     dbeta, coef);
  MFPA_CHECK_LAUNCH();
  launch_bn_bwd_apply<false>(s, dy, z, npix, C, scale, shift, mean, invstd, coef, drop_seed, drop_thresh, drop_scale, dz_bf16, write_f32,
                             nullptr, nullptr, z16, dy16);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// mfpa_bn_relu_bwd_finish and ..._finish_rank1 after their argument checks: coefficients from the (all-reduced) sums, then the apply pass
template <bool RANK1>
int bn_bwd_finish_apply(hipStream_t s, float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                        const float* shift, const float* mean, const float* invstd, const double* local_sums, const double* global_sums,
                        double global_count, float* dgamma, float* dbeta, float* coef, unsigned drop_seed, unsigned drop_thresh,
                        float drop_scale, void* dz_bf16, int write_f32, const float* dpred, const float* w1, int z16, int dy16) {
  hipLaunchKernelGGL(bn_bwd_finish_sync_kernel, dim3((C + 255) / 256), dim3(256), 0, s, local_sums, global_sums, C, global_count,
                     gamma, invstd, dgamma, dbeta, coef);
  MFPA_CHECK_LAUNCH();
  if (npix == 0) return MFPA_OK;
  launch_bn_bwd_apply<RANK1>(s, dy, z, npix, C, scale, shift, mean, invstd, coef, drop_seed, drop_thresh, drop_scale, dz_bf16, write_f32,
                             dpred, w1, z16, dy16);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int outconv_bwd_blocks(long long npix, int C) { return grid_for(npix, (256 / (C / 4)) * 16, RED_BLOCKS); }

// mfpa_outconv_bwd (dy written) and ..._sums (the BatchNorm-backward row partials instead) after their argument checks
template <bool SUMS>
int outconv_bwd(hipStream_t s, const float* z, const float* dpred, long long npix, int C, const float* scale, const float* shift,
                const float* mean, const float* invstd, const float* w, float* dy, float* dwb, double* workspace, float* part, int z16) {
  const int nblk = outconv_bwd_blocks(npix, C);
  hipLaunchKernelGGL(outconv_bwd_kernel<SUMS>, dim3(nblk), dim3(256), 0, s, z, dpred, npix, C, scale, shift, w, dy, workspace, mean, invstd,
                     part, z16);
  MFPA_CHECK_LAUNCH();
  // finish: column sums of the (nblk, C+1) partial matrix: C weight gradients then the bias gradient
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 1 + 3) / 4), dim3(256), 0, s, workspace, nblk, C + 1, dwb);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// one maxpool_bwd_add_kernel<MODE> launch: one workgroup per pooled row
template <int MODE>
int pool_bwd(hipStream_t s, const float* z, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
             const float* invstd, const float* dp, float* dy, unsigned drop_seed, unsigned drop_thresh, float drop_scale, float* part, int z16,
             int d16, int nowrite, const float* coef, void* dz_bf16) {
  hipLaunchKernelGGL(maxpool_bwd_add_kernel<MODE>, dim3((unsigned)(B * (H / 2))), dim3(256), 0, s, z, B, H, W, C, scale, shift, dp, dy,
                     drop_seed, drop_thresh, drop_scale, mean, invstd, part, z16, d16, nowrite, coef, reinterpret_cast<__bf16*>(dz_bf16));
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // namespace

extern "C" {

int mfpa_red_blocks(void) { return RED_BLOCKS; }

int mfpa_bn_stats(const float* z, long long npix, int C, const float* gamma, const float* beta, float eps,
                  float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                  float* running_var, double* workspace, int z_is_bf16, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!z || !gamma || !beta || !mean || !invstd || !scale || !shift || !workspace) return MFPA_EINVAL;
  if (!bn_shape_ok(npix, C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_pixels<0>(s, z, nullptr, npix, C, nullptr, nullptr, nullptr, nullptr, workspace, 0u, 0u, 1.f, z_is_bf16);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, (double)npix,
                     eps, momentum, gamma, beta, mean, invstd, scale, shift, running_mean, running_var);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_bn_relu_bwd(float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                     const float* shift, const float* mean, const float* invstd, float* dgamma, float* dbeta,
                     float* coef, double* workspace, unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                     void* dz_bf16, int write_f32, int z_is_bf16, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!write_f32 && !dz_bf16) return MFPA_EINVAL;
  if (!dy || !z || !gamma || !scale || !shift || !mean || !invstd || !dgamma || !dbeta || !coef || !workspace) return MFPA_EINVAL;
  if (C & (C - 1)) return MFPA_EINVAL;   // channel counts of this UNet are powers of two (64 ... 1024)
  if (!bn_shape_ok(npix, C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_pixels<1>(s, dy, z, npix, C, scale, shift, mean, invstd, workspace, drop_seed, drop_thresh, drop_scale, z_is_bf16);
  MFPA_CHECK_LAUNCH();
  return bn_bwd_finish_apply_local(s, nblk, dy, z, npix, C, gamma, scale, shift, mean, invstd, dgamma, dbeta, coef, workspace, drop_seed,
                                   drop_thresh, drop_scale, dz_bf16, write_f32, z_is_bf16, 0);
}

int mfpa_bn_stats_sums(const float* z, long long npix, int C, double* sums, double* workspace, int z_is_bf16, void* stream) {
  if (!sums || !workspace || !bn_shape_ok(npix, C) || (npix > 0 && !z)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  if (npix == 0) { MFPA_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 2 * C, s)); return MFPA_OK; }
  const int nblk = reduce_pixels<0>(s, z, nullptr, npix, C, nullptr, nullptr, nullptr, nullptr, workspace, 0u, 0u, 1.f, z_is_bf16);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(pair_sums_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, sums);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_conv_stats_reduce(const float* part, long long rows, int C, double* sums, double* workspace, void* stream) {
  if (!part || !sums || !workspace || rows < 1 || !rows_shape_ok(C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_rows(s, part, rows, C, workspace);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(pair_sums_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, sums);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// mfpa_conv_stats_reduce + mfpa_bn_stats_finish in two launches instead of three (single-GPU statistics: no all-reduce between them): the
// finish kernel sums the row blocks' partials itself, in the order pair_sums_kernel does -- bit-identical statistics.
int mfpa_conv_stats_bn_finish(const float* part, long long rows, int C, double count, const float* gamma, const float* beta, float eps,
                              float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                              float* running_var, double* workspace, void* stream) {
  if (!part || !workspace || rows < 1 || !rows_shape_ok(C)) return MFPA_EINVAL;
  if (!gamma || !beta || !mean || !invstd || !scale || !shift || !(count >= 1.0)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_rows(s, part, rows, C, workspace);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, count, eps,
                     momentum, gamma, beta, mean, invstd, scale, shift, running_mean, running_var);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// the BatchNorm + ReLU backward from a convolution's (or pool / OutConv backward's) row partials {sum g, sum g * xhat}: rows -> float64
// block sums -> dgamma / dbeta / coefficients -> apply, three launches (mfpa_conv_stats_reduce + mfpa_bn_relu_bwd_finish: four).  Single-GPU
// statistics only (with SyncBN the sums are all-reduced between the two halves: use those two calls).
int mfpa_bn_relu_bwd_from_part(float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                               const float* shift, const float* mean, const float* invstd, const float* part, long long rows,
                               float* dgamma, float* dbeta, float* coef, double* workspace, unsigned drop_seed, unsigned drop_thresh,
                               float drop_scale, void* dz_bf16, int write_f32, int z_is_bf16, int dy_is_bf16, void* stream) {
  if (!gamma || !scale || !shift || !mean || !invstd || !part || !dgamma || !dbeta || !coef || !workspace || rows < 1) return MFPA_EINVAL;
  if (!write_f32 && !dz_bf16) return MFPA_EINVAL;
  if (dy_is_bf16 && write_f32) return MFPA_EINVAL;
  if (npix < 1 || !bn_shape_ok(npix, C) || (C & (C - 1)) || !dy || !z || !rows_shape_ok(C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_rows(s, part, rows, C, workspace);
  MFPA_CHECK_LAUNCH();
  return bn_bwd_finish_apply_local(s, nblk, dy, z, npix, C, gamma, scale, shift, mean, invstd, dgamma, dbeta, coef, workspace, drop_seed,
                                   drop_thresh, drop_scale, dz_bf16, write_f32, z_is_bf16, dy_is_bf16);
}

int mfpa_bn_stats_finish(const double* sums, double count, int C, const float* gamma, const float* beta, float eps,
                         float momentum, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                         float* running_var, void* stream) {
  if (!sums || !gamma || !beta || !mean || !invstd || !scale || !shift || C < 1 || !(count >= 1.0)) return MFPA_EINVAL;
  hipLaunchKernelGGL(bn_stats_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, mfpa_stream(stream), sums, 1, C, count, eps,
                     momentum, gamma, beta, mean, invstd, scale, shift, running_mean, running_var);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_bn_relu_bwd_sums(const float* dy, const float* z, long long npix, int C, const float* scale, const float* shift,
                          const float* mean, const float* invstd, double* sums, double* workspace, unsigned drop_seed,
                          unsigned drop_thresh, float drop_scale, int z_is_bf16, void* stream) {
  if (!sums || !workspace || !scale || !shift || !mean || !invstd || !bn_shape_ok(npix, C) || (C & (C - 1))) return MFPA_EINVAL;
  if (npix > 0 && (!dy || !z)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  if (npix == 0) { MFPA_HIP(hipMemsetAsync(sums, 0, sizeof(double) * 2 * C, s)); return MFPA_OK; }
  const int nblk = reduce_pixels<1>(s, dy, z, npix, C, scale, shift, mean, invstd, workspace, drop_seed, drop_thresh, drop_scale, z_is_bf16);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(pair_sums_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, sums);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_bn_relu_bwd_finish(float* dy, const float* z, long long npix, int C, const float* gamma, const float* scale,
                            const float* shift, const float* mean, const float* invstd, const double* local_sums,
                            const double* global_sums, double global_count, float* dgamma, float* dbeta, float* coef,
                            unsigned drop_seed, unsigned drop_thresh, float drop_scale, void* dz_bf16, int write_f32, int z_is_bf16, int dy_is_bf16, void* stream) {
  if (!gamma || !scale || !shift || !mean || !invstd || !local_sums || !global_sums || !dgamma || !dbeta || !coef) return MFPA_EINVAL;
  if (!write_f32 && !dz_bf16) return MFPA_EINVAL;
  if (dy_is_bf16 && write_f32) return MFPA_EINVAL;                    // a bfloat16 dy cannot take the float32 dz in place
  if (!bn_shape_ok(npix, C) || (C & (C - 1)) || !(global_count >= 1.0) || (npix > 0 && (!dy || !z))) return MFPA_EINVAL;
  return bn_bwd_finish_apply<false>(mfpa_stream(stream), dy, z, npix, C, gamma, scale, shift, mean, invstd, local_sums, global_sums,
                                    global_count, dgamma, dbeta, coef, drop_seed, drop_thresh, drop_scale, dz_bf16, write_f32, nullptr,
                                    nullptr, z_is_bf16, dy_is_bf16);
}

int mfpa_bn_relu_bwd_finish_rank1(const float* dpred, const float* w1, const float* z, long long npix, int C, const float* gamma,
                                  const float* scale, const float* shift, const float* mean, const float* invstd, const double* local_sums,
                                  const double* global_sums, double global_count, float* dgamma, float* dbeta, float* coef,
                                  float* dz_f32, void* dz_bf16, int z_is_bf16, void* stream) {
  if (!dpred || !w1 || !gamma || !scale || !shift || !mean || !invstd || !local_sums || !global_sums || !dgamma || !dbeta || !coef) return MFPA_EINVAL;
  if (!dz_f32 && !dz_bf16) return MFPA_EINVAL;
  if (!bn_shape_ok(npix, C) || (C & (C - 1)) || !(global_count >= 1.0) || (npix > 0 && !z)) return MFPA_EINVAL;
  return bn_bwd_finish_apply<true>(mfpa_stream(stream), dz_f32, z, npix, C, gamma, scale, shift, mean, invstd, local_sums, global_sums,
                                   global_count, dgamma, dbeta, coef, 0u, 0u, 1.f, dz_bf16, dz_f32 != nullptr ? 1 : 0, dpred, w1, z_is_bf16, 0);
}

int mfpa_colsum(const float* x, long long npix, int C, float* out, double* workspace, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!x || !out || !workspace || !bn_shape_ok(npix, C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = reduce_pixels<2>(s, x, nullptr, npix, C, nullptr, nullptr, nullptr, nullptr, workspace, 0u, 0u, 1.f, 0);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(colsum_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_bn_relu_pool(const float* z, int B, int H, int W, int C, const float* scale, const float* shift, float* p,
                      unsigned drop_seed, unsigned drop_thresh, float drop_scale, int z_is_bf16, int p_is_bf16, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!z || !scale || !shift || !p || !pool_shape_ok(B, H, W, C)) return MFPA_EINVAL;
  hipLaunchKernelGGL(bn_relu_pool_kernel, dim3((unsigned)(B * (H / 2))), dim3(256), 0, mfpa_stream(stream), z, B, H, W, C, scale,
                     shift, p, drop_seed, drop_thresh, drop_scale, z_is_bf16, p_is_bf16);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_maxpool2_bwd_add(const float* z, int B, int H, int W, int C, const float* scale, const float* shift,
                          const float* dp, float* dy, unsigned drop_seed, unsigned drop_thresh, float drop_scale,
                          int z_is_bf16, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!z || !scale || !shift || !dp || !dy || !pool_shape_ok(B, H, W, C)) return MFPA_EINVAL;
  return pool_bwd<0>(mfpa_stream(stream), z, B, H, W, C, scale, shift, nullptr, nullptr, dp, dy, drop_seed, drop_thresh, drop_scale, nullptr,
                     z_is_bf16, 0, 0, nullptr, nullptr);
}

int mfpa_maxpool2_bwd_add_sums(const float* z, int B, int H, int W, int C, const float* scale, const float* shift, const float* mean,
                               const float* invstd, const float* dp, float* dy, unsigned drop_seed, unsigned drop_thresh,
                               float drop_scale, float* part, int z_is_bf16, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!z || !scale || !shift || !mean || !invstd || !dp || !dy || !part || !pool_shape_ok(B, H, W, C)) return MFPA_EINVAL;
  if (C / 4 > 256 || 256 % (C / 4)) return MFPA_EINVAL;   // a thread keeps ONE channel quad's sums
  return pool_bwd<1>(mfpa_stream(stream), z, B, H, W, C, scale, shift, mean, invstd, dp, dy, drop_seed, drop_thresh, drop_scale, part,
                     z_is_bf16, 0, 0, nullptr, nullptr);
}

// An encoder block's last BatchNorm + ReLU backward WITHOUT its finished input gradient in memory (round 5): dy = the skip path's gradient
// (float32, or bfloat16 with dy_is_bf16) is only read.  Launch 1: g = dy + route(dp) reduced to the BatchNorm-backward row partials (nothing
// written back); 2 + 3: mfpa_conv_stats_reduce's row kernel and the finish (dgamma, dbeta, coefficients); 4: the same g formed again and pushed
// through the backward formula, bfloat16 dz out.  Against mfpa_maxpool2_bwd_add_sums + mfpa_bn_relu_bwd_from_part: the float32 dy is neither
// written nor read back (2 of 4.75 tensor passes at float32 dy, 1.75 of 4.75 more with a bfloat16 dy).  Single-GPU statistics only.
int mfpa_maxpool2_bwd_bn_relu_bwd(const float* z, int B, int H, int W, int C, const float* gamma, const float* scale, const float* shift,
                                  const float* mean, const float* invstd, const float* dp, const void* dy, int dy_is_bf16, unsigned drop_seed,
                                  unsigned drop_thresh, float drop_scale, float* part, float* dgamma, float* dbeta, float* coef,
                                  double* workspace, void* dz_bf16, int z_is_bf16, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!z || !gamma || !scale || !shift || !mean || !invstd || !dp || !dy || !part || !dgamma || !dbeta || !coef || !workspace || !dz_bf16) return MFPA_EINVAL;
  if (!pool_shape_ok(B, H, W, C) || (C & (C - 1))) return MFPA_EINVAL;
  if (C / 4 > 256 || 256 % (C / 4) || !rows_shape_ok(C)) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  float* dyf = const_cast<float*>(reinterpret_cast<const float*>(dy));
  int rc = pool_bwd<1>(s, z, B, H, W, C, scale, shift, mean, invstd, dp, dyf, drop_seed, drop_thresh, drop_scale, part, z_is_bf16, dy_is_bf16,
                       1, nullptr, nullptr);
  if (rc != MFPA_OK) return rc;
  const int nblk = reduce_rows(s, part, (long long)B * (H / 2), C, workspace);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_bwd_finish_kernel, dim3((C + 3) / 4), dim3(256), 0, s, workspace, nblk, C, (double)((long long)B * H * W), gamma, invstd,
                     dgamma, dbeta, coef);
  MFPA_CHECK_LAUNCH();
  return pool_bwd<2>(s, z, B, H, W, C, scale, shift, mean, invstd, dp, dyf, drop_seed, drop_thresh, drop_scale, nullptr, z_is_bf16, dy_is_bf16,
                     1, coef, dz_bf16);
}

int mfpa_act_to_bf16(const float* z, long long n, int C, const float* scale, const float* shift, unsigned drop_seed,
                     unsigned drop_thresh, float drop_scale, void* out_bf16, void* stream) {
  if (n == 0) return MFPA_OK;
  if (!z || !out_bf16 || n < 0 || C < 4 || C % 4 || n % C) return MFPA_EINVAL;
  if ((scale == nullptr) != (shift == nullptr) || (drop_thresh && !scale)) return MFPA_EINVAL;
  hipLaunchKernelGGL(act_to_bf16_kernel, dim3(grid_for(n / 4, 256, 256 * 32)), dim3(256), 0, mfpa_stream(stream), z, n / 4, C, scale, shift,
                     drop_seed, drop_thresh, drop_scale, reinterpret_cast<__bf16*>(out_bf16));
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_outconv_fwd(const float* z, long long npix, int C, const float* scale, const float* shift, const float* w,
                     const float* bias, float* pred, int z_is_bf16, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!z || !scale || !shift || !w || !bias || !pred || !outconv_shape_ok(npix, C)) return MFPA_EINVAL;
  hipLaunchKernelGGL(outconv_fwd_kernel, dim3(grid_for(npix, 256 / (C / 4), 256 * 32)), dim3(256), 0,
                     mfpa_stream(stream), z, npix, C, scale, shift, w, bias, pred, z_is_bf16);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_outconv_bwd(const float* z, const float* dpred, long long npix, int C, const float* scale, const float* shift,
                     const float* w, float* dy, float* dwb, double* workspace, int z_is_bf16, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!z || !dpred || !scale || !shift || !w || !dy || !dwb || !workspace) return MFPA_EINVAL;
  if (!outconv_shape_ok(npix, C)) return MFPA_EINVAL;
  return outconv_bwd<false>(mfpa_stream(stream), z, dpred, npix, C, scale, shift, nullptr, nullptr, w, dy, dwb, workspace, nullptr, z_is_bf16);
}

int mfpa_outconv_bwd_rows(long long npix, int C, int* rows) {
  if (!rows || !outconv_shape_ok(npix, C)) return MFPA_EINVAL;
  *rows = npix == 0 ? 0 : outconv_bwd_blocks(npix, C);
  return MFPA_OK;
}

int mfpa_outconv_bwd_sums(const float* z, const float* dpred, long long npix, int C, const float* scale, const float* shift,
                          const float* mean, const float* invstd, const float* w, float* dwb, double* workspace, float* part,
                          int z_is_bf16, void* stream) {
  if (npix == 0) return MFPA_OK;
  if (!z || !dpred || !scale || !shift || !mean || !invstd || !w || !dwb || !workspace || !part) return MFPA_EINVAL;
  if (!outconv_shape_ok(npix, C)) return MFPA_EINVAL;
  return outconv_bwd<true>(mfpa_stream(stream), z, dpred, npix, C, scale, shift, mean, invstd, w, nullptr, dwb, workspace, part, z_is_bf16);
}

int mfpa_l1_loss(const float* pred, const double* target, long long n, float* dpred, double* loss, double* workspace,
                 void* stream) {
  if (!pred || !target || !loss || !workspace || n <= 0) return MFPA_EINVAL;
  hipStream_t s = mfpa_stream(stream);
  const int nblk = grid_for(n, 256 * 8, RED_BLOCKS);
  hipLaunchKernelGGL(l1_kernel, dim3(nblk), dim3(256), 0, s, pred, target, n, dpred, workspace);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(256), 0, s, workspace, nblk, n, loss);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_pack_conv_weights(const float* w, int taps, int Co, int Ci, int flip_transpose, int row0, int nrows, int precision,
                            float* out, void* stream) {
  if (!w || !out || taps < 1 || Co < 32 || Ci < 32 || Co % 32 || Ci % 32 || nrows < 32 || nrows % 32 || row0 < 0 || row0 % 32)
    return MFPA_EINVAL;
  if (precision < 0 || precision > 3 || precision == 2) return MFPA_EINVAL;     // 3: the fragment-ordered bf16x3 image (w_layout 2)
  if (row0 + nrows > (flip_transpose ? Ci : Co)) return MFPA_EINVAL;
  const int K = flip_transpose ? Co : Ci;
  dim3 grid(K / 32, nrows / 32, taps);
  if (flip_transpose) hipLaunchKernelGGL(pack_conv_weights_kernel<true>, grid, dim3(256), 0, mfpa_stream(stream), w, taps, Co, Ci, row0, nrows, precision, out);
  else hipLaunchKernelGGL(pack_conv_weights_kernel<false>, grid, dim3(256), 0, mfpa_stream(stream), w, taps, Co, Ci, row0, nrows, precision, out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_pack_conv_weights_batch(const mfpa_pack_job* jobs_dev, int njobs, long long total_tiles, void* stream) {
  if (njobs == 0) return MFPA_OK;
  if (!jobs_dev || njobs < 0 || total_tiles < 1 || total_tiles > 0x7fffffffLL) return MFPA_EINVAL;
  hipLaunchKernelGGL(pack_conv_weights_batch_kernel, dim3((unsigned)total_tiles), dim3(256), 0, mfpa_stream(stream), jobs_dev, njobs);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_adam_step(float* p, const float* g, float* m, float* v, long long n, float lr, float beta1, float beta2,
                   float eps, int step, float grad_scale, void* stream) {
  if (n == 0) return MFPA_OK;
  if (!p || !g || !m || !v || n < 0 || step < 1) return MFPA_EINVAL;
  const double bc1 = 1.0 - pow((double)beta1, step);
  const double bc2 = 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n, 256 * 4, 256 * 16)), dim3(256), 0, mfpa_stream(stream), p, g, m, v, n,
                     lr, beta1, beta2, eps, (float)bc1, (float)sqrt(bc2), grad_scale);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
