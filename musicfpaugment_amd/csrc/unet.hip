// What every launch of the UNet convolution family (training/unet.py:8-108 of the reference; NHWC float32 activations, H = frequency bins,
// W = frames) goes through: conv_route and CONV_KERNELS (validation and kernel choice; every kernel that exists with the route that names
// it, pinned by tests/_conv_route_cases.py), the shape rules the host queries share with the route, the extern "C" entry points of
// include/mfpa.h, and three small VALU kernels (the 1-channel first layer, MaxPool2d(2), the OutConv 1x1).  The MFMA kernels live in their
// own files behind the launchers of csrc/mfpa_unet_args.h: conv_mfma_kernel / convT_mfma_kernel (the row image) in csrc/unet_mfma.hip,
// conv_wd16_kernel in csrc/unet_wd16.hip, conv_ws64_kernel in csrc/unet_ws.hip.
#include <cstring>

#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include "mfpa_unet_args.h"

namespace {

using namespace mfpa_tile;     // vector types, KC

using mfpa_unet::ConvArgs;     // csrc/mfpa_unet_args.h

// First layer: 1 input channel -> Cout (multiple of 4), fused spectrogram normalisation.
// 16 lanes per pixel x 4 channels per lane... generalised: Cout/4 lanes per pixel.
__global__ __launch_bounds__(256) void conv3x3_c1_kernel(const float* __restrict__ x32, const double* __restrict__ spec64,
                                                         const double* __restrict__ denom, int per_clip, int B, int H,
                                                         int W, const float* __restrict__ w, int Cout,
                                                         const float* __restrict__ scale, const float* __restrict__ shift,
                                                         int relu, float* __restrict__ y, int y16, float* __restrict__ stats_part) {
  // stats_part (training forward): one row [2][Cout] per workgroup = (sum, sum of squares) of this image row's outputs per channel, float64
  // inside the workgroup -- mfpa_conv_stats_reduce / mfpa_conv_stats_bn_finish turn the B * H rows into the BatchNorm statistics without
  // the 200 us pass over the output
  const int lanes_per_pix = Cout / 4;
  double st_s[4] = {0., 0., 0., 0.}, st_q[4] = {0., 0., 0., 0.};
  const int pix_per_block = 256 / lanes_per_pix;
  const int sub = threadIdx.x % lanes_per_pix, pl = threadIdx.x / lanes_per_pix;
  float4 wt[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) wt[t] = *reinterpret_cast<const float4*>(w + (size_t)t * Cout + 4 * sub);
  const float4 sc = scale ? *reinterpret_cast<const float4*>(scale + 4 * sub) : make_float4(1.f, 1.f, 1.f, 1.f);
  const float4 sh = shift ? *reinterpret_cast<const float4*>(shift + 4 * sub) : make_float4(0.f, 0.f, 0.f, 0.f);
  double gden = 1.0;
  if (spec64 && denom && !per_clip) {
    gden = 0.0;
    for (int i = 0; i < B; ++i) gden = fmax(gden, denom[i]);
  }
  // one workgroup per (clip, bin row): no 64-bit index divisions in the pixel loop
  const int b = blockIdx.x / H, gy = blockIdx.x % H;
  const double den = (spec64 && denom) ? (per_clip ? denom[b] : gden) : 1.0;
  const int iters = (W + pix_per_block - 1) / pix_per_block;
  for (int itr = 0; itr < iters; ++itr) {              // uniform trip count: every lane takes part in the shuffles
    const int gx_raw = itr * pix_per_block + pl;
    const bool live = gx_raw < W;
    const int gx = live ? gx_raw : W - 1;
    const size_t p = ((size_t)b * H + gy) * W + gx;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lanes_per_pix >= 9) {
      // the lanes of a pixel share its 3x3 input window: lane `sub` < 9 loads (and normalises) tap `sub`, the others
      // receive it by shuffle -- one float64 division per lane instead of nine
      float mine = 0.f;
      if (sub < 9) {
        const int yy = gy + sub / 3 - 1, xx = gx + sub % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const size_t o = ((size_t)b * H + yy) * W + xx;
          mine = spec64 ? (float)(spec64[o] / den) : x32[o];
        }
      }
      const int base = (threadIdx.x & 63) - sub;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float v = __shfl(mine, base + t);
        acc.x += v * wt[t].x;
        acc.y += v * wt[t].y;
        acc.z += v * wt[t].z;
        acc.w += v * wt[t].w;
      }
    } else {
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int yy = gy + t / 3 - 1, xx = gx + t % 3 - 1;
        float v = 0.f;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const size_t o = ((size_t)b * H + yy) * W + xx;
          v = spec64 ? (float)(spec64[o] / den) : x32[o];
        }
        acc.x += v * wt[t].x;
        acc.y += v * wt[t].y;
        acc.z += v * wt[t].z;
        acc.w += v * wt[t].w;
      }
    }
    float4 o4;
    o4.x = acc.x * sc.x + sh.x;
    o4.y = acc.y * sc.y + sh.y;
    o4.z = acc.z * sc.z + sh.z;
    o4.w = acc.w * sc.w + sh.w;
    if (relu) {
      o4.x = fmaxf(o4.x, 0.f);
      o4.y = fmaxf(o4.y, 0.f);
      o4.z = fmaxf(o4.z, 0.f);
      o4.w = fmaxf(o4.w, 0.f);
    }
    if (live && stats_part != nullptr) {
      st_s[0] += (double)o4.x; st_s[1] += (double)o4.y; st_s[2] += (double)o4.z; st_s[3] += (double)o4.w;
      st_q[0] += (double)o4.x * (double)o4.x; st_q[1] += (double)o4.y * (double)o4.y;
      st_q[2] += (double)o4.z * (double)o4.z; st_q[3] += (double)o4.w * (double)o4.w;
    }
    if (live) {
      if (y16) {                                                         // the output kept as bfloat16 (the plain-bf16 training step's activations)
        bf16x4 h;
        h[0] = (__bf16)o4.x; h[1] = (__bf16)o4.y; h[2] = (__bf16)o4.z; h[3] = (__bf16)o4.w;
        *reinterpret_cast<bf16x4*>(reinterpret_cast<__bf16*>(y) + (size_t)p * Cout + 4 * sub) = h;
      } else *reinterpret_cast<float4*>(y + (size_t)p * Cout + 4 * sub) = o4;
    }
  }
  if (stats_part != nullptr) {                                           // (uniform: a kernel argument)
    __shared__ double red[256 * 8];
#pragma unroll
    for (int k = 0; k < 4; ++k) { red[threadIdx.x * 8 + k] = st_s[k]; red[threadIdx.x * 8 + 4 + k] = st_q[k]; }
    __syncthreads();
    if (pl == 0) {                                                       // fixed order over the workgroup's pixel slots: deterministic
      for (int r = 1; r < pix_per_block; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          st_s[k] += red[(r * lanes_per_pix + sub) * 8 + k];
          st_q[k] += red[(r * lanes_per_pix + sub) * 8 + 4 + k];
        }
      float* row = stats_part + (size_t)blockIdx.x * 2 * Cout;
      *reinterpret_cast<float4*>(row + 4 * sub) = make_float4((float)st_s[0], (float)st_s[1], (float)st_s[2], (float)st_s[3]);
      *reinterpret_cast<float4*>(row + Cout + 4 * sub) = make_float4((float)st_q[0], (float)st_q[1], (float)st_q[2], (float)st_q[3]);
    }
  }
}

__global__ __launch_bounds__(256) void maxpool2_kernel(const float* __restrict__ x, int B, int H, int W, int C,
                                                       float* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const long long total = (long long)B * Ho * Wo * C4;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int c4 = (int)(e % C4);
    long long p = e / C4;
    const int xo = (int)(p % Wo); p /= Wo;
    const int yo = (int)(p % Ho);
    const int b = (int)(p / Ho);
    const float* base = x + (((size_t)b * H + 2 * yo) * W + 2 * xo) * C + 4 * c4;
    const float4 v00 = *reinterpret_cast<const float4*>(base);
    const float4 v01 = *reinterpret_cast<const float4*>(base + C);
    const float4 v10 = *reinterpret_cast<const float4*>(base + (size_t)W * C);
    const float4 v11 = *reinterpret_cast<const float4*>(base + (size_t)W * C + C);
    float4 o;
    o.x = fmaxf(fmaxf(v00.x, v01.x), fmaxf(v10.x, v11.x));
    o.y = fmaxf(fmaxf(v00.y, v01.y), fmaxf(v10.y, v11.y));
    o.z = fmaxf(fmaxf(v00.z, v01.z), fmaxf(v10.z, v11.z));
    o.w = fmaxf(fmaxf(v00.w, v01.w), fmaxf(v10.w, v11.w));
    *reinterpret_cast<float4*>(y + (size_t)e * 4) = o;
  }
}

// OutConv 1x1 to one class: C/4 lanes per pixel, float4 per lane, shuffle reduce.
__global__ __launch_bounds__(256) void conv1x1_out_kernel(const float* __restrict__ x, long long npix, int C,
                                                          const float* __restrict__ w, float bias, float* __restrict__ y) {
  const int lpp = C / 4;  // lanes per pixel (power of two <= 64)
  const int sub = threadIdx.x % lpp, pl = threadIdx.x / lpp, ppb = 256 / lpp;
  const float4 wv = *reinterpret_cast<const float4*>(w + 4 * sub);
  const long long iters = (npix + (long long)gridDim.x * ppb - 1) / ((long long)gridDim.x * ppb);
  for (long long it = 0; it < iters; ++it) {
    const long long p = (it * gridDim.x + blockIdx.x) * ppb + pl;
    float s = 0.f;
    if (p < npix) {
      const float4 v = *reinterpret_cast<const float4*>(x + (size_t)p * C + 4 * sub);
      s = v.x * wv.x + v.y * wv.y + v.z * wv.z + v.w * wv.w;
    }
    for (int o = lpp >> 1; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (sub == 0 && p < npix) y[p] = s + bias;
  }
}

// 128-channel tiles of the plain loop: the 8-wave 256-pixel shape from this many input channels on (the bf16x3 3x3 convolution; the
// others keep round 1's measured 256)
constexpr int CONV_BIG_MIN_CIN = 64;
// conv_ws64_kernel also takes outputs of 128 channels and more with at most this many input channels: per layer, 64 clips: 64 -> 128 @
// 128 x 125 431 -> 380 us, 128 -> 128 725 -> 704, 128 -> 256 @ 64 x 62 360 -> 345; from 256 input channels on it loses
constexpr int CONV_WS_ALL = 128;

// Which bf16x3 weight image does the fastest kernel for this shape read?  2 = the fragment-ordered image of the 16 x 16 x 32
// weights-direct kernels (conv_ws64_kernel, conv_wd16_kernel: 3x3 convolution, >= 64 input channels, the 8 x 32 patches of the wide
// levels or the 16 x 16 patches of the 16 x 15 level), 0 = the row image.  The 64-channel outputs take it from 64 input channels on:
// with its persistent tile loop conv_wd16_kernel<.., WMW = 4> beats the plain loop there (64 -> 64 @ 257 x 251, 64 clips, 1366 -> 1008 us).
// The primary rule: the caller packs the weights by it, so it is an INPUT of the routing below.
static int conv_weight_layout(int H, int W, int Cin, int Cout, int mode, int precision) {
  if (mode != 0 || precision != 1 || Cin < CONV_BIG_MIN_CIN) return 0;
  const bool wide = W > 16 && H >= 8;
  if (Cout % 128) return (wide && Cout % 64 == 0 && Cin % 64 == 0) ? 2 : 0;     // 64-channel output tiles
  return (wide || (W <= 16 && H >= 16)) ? 2 : 0;
}

// the shape rules of the weights-direct kernels that the host queries share with conv_route: this one, and conv_wd16_tile (csrc/unet_wd16.hip)
static bool conv_prefers_ws64(int H, int W, int cin, int cout, bool c1) { return W > 16 && H >= 8 && (c1 || cout % 128 || cin <= CONV_WS_ALL); }

// Every kernel of the family that exists, each with the route that names it -- both made from ONE template argument list, so a route cannot
// reach another instantiation than the one it spells.
struct ConvKernel { mfpa_conv_route r; int (*launch)(ConvArgs&, hipStream_t); };
template <bool C1SRC> constexpr ConvKernel k_ws64() { return {{MFPA_CONV_WS64, 8, 32, 64, 0, 0, 1, C1SRC}, mfpa_unet::launch_conv_ws64<C1SRC>}; }
template <int PH, int PW, bool ROWS, int WMW, bool SIDE, bool PLAIN, bool IN16, bool AFF16> constexpr ConvKernel k_wd16() {
  return {{MFPA_CONV_WD16, PH, PW, 32 * (8 / WMW), WMW, 0, 1, 0, ROWS, SIDE, PLAIN, IN16, AFF16}, mfpa_unet::launch_wd16<PH, PW, ROWS, WMW, SIDE, PLAIN, IN16, AFF16>}; }
#define MFPA_K_WD16(...) k_wd16<__VA_ARGS__>(),
template <int BN, int PH, int PW, int MODE, int PREC, bool C1SRC> constexpr ConvKernel k_mfma() {
  return {{MFPA_CONV_MFMA, PH, PW, BN, 0, MODE, PREC, C1SRC}, mfpa_unet::launch_conv<BN, PH, PW, MODE, PREC, C1SRC>}; }
#define MFPA_K_MFMA(...) k_mfma<__VA_ARGS__>(),
template <int PH, int PW, int PREC, bool IO16, bool PLAIN> constexpr ConvKernel k_convT() {
  return {{MFPA_CONV_CONVT, PH, PW, 64, 0, 1, PREC, 0, 0, 0, PLAIN, 0, 0, IO16}, mfpa_unet::launch_convT<PH, PW, PREC, IO16, PLAIN>}; }
#define MFPA_K_CONVT(...) k_convT<__VA_ARGS__>(),
// each group from the list its file's explicit instantiations are made of (csrc/mfpa_unet_args.h): the 29 of csrc/unet_wd16.hip, the 27 + 8
// of csrc/unet_mfma.hip
const ConvKernel CONV_KERNELS[] = {k_ws64<false>(), k_ws64<true>(), MFPA_WD16_FORMS(MFPA_K_WD16) MFPA_MFMA_FORMS(MFPA_K_MFMA) MFPA_CONVT_FORMS(MFPA_K_CONVT)};

// Tile choice.  Waves always own 64 pixels x 64 channels.
//   w_layout 2 (bf16x3 3x3 convolution): conv_ws64_kernel (csrc/unet_ws.hip: 4 compute waves of 128 px x 32 ch + 4 loader waves) for the
//                    fused first layer, the 64-channel outputs and the wider ones up to CONV_WS_ALL input channels; conv_wd16_kernel
//                    for the shapes it does not serve and for the training step's launches.
//   Cout % 128 == 0: 128-channel tiles; 8 waves on 8x32-pixel patches (256 x 128: half the weight traffic and
//                    barriers per MFMA) when K = 9*Cin is long enough to amortise the prologue/epilogue of a
//                    one-workgroup-per-CU kernel, else 4 waves on 4x32 patches (two workgroups per CU overlap).
//   otherwise      : 64-channel tiles, 4 waves stacked along M on 8x32 patches (256 x 64).
//   W <= 16 (the 16x15 bottleneck): 16x16 patches on 8 waves for the bf16x3 3x3 convolution's 128-channel tiles, else 8x16 patches.
// Routing: validation and kernel choice of a launch, host arithmetic only -- MFPA_EINVAL, or MFPA_OK with the kernel arguments in `a` and the
// route in *r (MFPA_CONV_NONE: nothing to do).  Every condition that rejects a launch is here and nowhere else; the launchers size LDS and
// the grid.  (out_offsets = false: mfpa_conv3x3_bn_relu, which has never checked the output's byte offsets.)
static int conv_route(const mfpa_conv_desc* d, ConvArgs& a, mfpa_conv_route* r, const ConvKernel** k, bool out_offsets = true) {
  *r = mfpa_conv_route{}; r->family = MFPA_CONV_NONE; *k = nullptr;
  if (!d) return MFPA_EINVAL;
  if (d->B == 0) return MFPA_OK;
  if ((!d->x0 && !d->c1_x32 && !d->c1_spec64) || !d->w || (!d->y && !d->w1x1 && !d->y_bf16) || d->B < 0 || d->H < 1 || d->W < 1) return MFPA_EINVAL;
  if (d->C0 < KC || d->C0 % KC || d->C1 < 0 || d->C1 % KC || d->Cout < 64 || d->Cout % 64) return MFPA_EINVAL;
  if (d->mode < 0 || d->mode > 2) return MFPA_EINVAL;
  if (d->C1 > 0 && (d->mode != 0 || !d->x1 || d->H1 < 1 || d->W1 < 1 || d->H1 > d->H || d->W1 > d->W)) return MFPA_EINVAL;
  if ((d->in_scale0 == nullptr) != (d->in_shift0 == nullptr)) return MFPA_EINVAL;
  if (out_offsets && 4LL * d->H * d->W * d->Cout * 4 > 0xffffffffLL) return MFPA_EINVAL;   // the epilogue addresses one clip's output with 32-bit byte offsets
  a = ConvArgs{};
  a.x0 = d->x0; a.in_scale0 = d->in_scale0; a.in_shift0 = d->in_shift0;
  a.x1 = d->C1 ? d->x1 : nullptr; a.w = d->w; a.scale = d->out_scale; a.shift = d->out_shift; a.y = d->y;
  a.C0 = d->C0; a.C1 = d->C1; a.H1 = d->C1 ? d->H1 : 0; a.W1 = d->C1 ? d->W1 : 0;
  a.oy1 = d->C1 ? (d->H - d->H1) / 2 : 0;
  a.ox1 = d->C1 ? (d->W - d->W1) / 2 : 0;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Cout = d->Cout; a.relu = d->relu;
  a.yH = (d->mode != 1 && d->yH > 0) ? d->yH : d->H;
  a.yW = (d->mode != 1 && d->yW > 0) ? d->yW : d->W;
  if (a.yH > d->H || a.yW > d->W) return MFPA_EINVAL;
  if (d->drop_thresh && (!d->in_scale0 || d->mode == 2)) return MFPA_EINVAL;
  a.drop_seed = d->drop_seed; a.drop_thresh = d->drop_thresh; a.drop_scale = d->drop_scale;
  if ((d->y_pool || d->w1x1) && d->mode != 0) return MFPA_EINVAL;
  if (d->y_pool && (d->H < 2 || d->W < 2 || a.yH != d->H || a.yW != d->W)) return MFPA_EINVAL;
  if (d->w1x1 && (!d->y1x1 || d->Cout != 64)) return MFPA_EINVAL;      // the 64-channel tile holds every channel
  a.y_pool = d->y_pool; a.w1x1 = d->w1x1; a.b1x1 = d->b1x1; a.y1x1 = d->y1x1;
  if (d->c1_x32 || d->c1_spec64) {
    if (d->mode != 0 || d->C0 != 64 || d->C1 != 0 || d->Cout != 64 || d->W <= 16 || d->H < 8) return MFPA_EINVAL;
    if (!d->c1_w || !d->c1_scale || !d->c1_shift || d->in_scale0 || (d->c1_x32 && d->c1_spec64)) return MFPA_EINVAL;
    a.c1_x32 = d->c1_x32; a.c1_spec64 = d->c1_spec64; a.c1_denom = d->c1_spec64 ? d->c1_denom : nullptr;
    a.c1_w = d->c1_w; a.c1_scale = d->c1_scale; a.c1_shift = d->c1_shift;
  }
  if (d->precision < 0 || d->precision > 2) return MFPA_EINVAL;
  if (d->w_layout != 0 && d->w_layout != 2) return MFPA_EINVAL;         // the row image or the fragment image of the weights-direct kernels
  if (d->w_layout != 0 && (d->mode != 0 || d->precision < 1)) return MFPA_EINVAL;
  // plain bf16: conv_wd16_kernel (mode 0: it reads the hi halves of the fragment image), or -- round 6 -- the transposed convolution of the training
  // step and its input gradient (modes 1 / 2 on the row image: the hi halves of the staged operands)
  if (d->precision == 2 && d->mode == 0 && d->w_layout != 2) return MFPA_EINVAL;
  if (d->precision == 2 && d->mode == 1 && !(d->x0_is_bf16 || !d->y)) return MFPA_EINVAL;      // (its bf16-I/O instantiation carries the plain form)
  a.w_frag = d->w_layout;
  a.plain = d->precision == 2;
  // bfloat16 sources (both of them): the plain-bf16 conv_wd16_kernel (any on-load affine / dropout is applied in float32 and rounded once), or
  // the transposed convolution (mode 1)
  if (d->x0_is_bf16 && !((d->precision == 2 && d->mode == 0 && ((d->C0 + d->C1) % 64) == 0 && !d->x1_bf16) || (d->mode == 1 && d->precision >= 1)))
    return MFPA_EINVAL;
  if (d->x0_is_bf16 && (d->c1_x32 || d->c1_spec64)) return MFPA_EINVAL;
  a.in16 = d->x0_is_bf16 ? 1 : 0;
  // the split layout: only conv_ws64_kernel reads / writes it (a launch it does not serve is rejected below)
  a.x0_split = d->x0_split ? 1 : 0; a.x1_split = d->x1_split ? 1 : 0; a.y_split = d->y_split ? 1 : 0; a.y_pool_split = d->y_pool_split ? 1 : 0;
  const bool any_split = a.x0_split || a.x1_split || a.y_split || a.y_pool_split;
  if (any_split && (d->mode != 0 || d->precision != 1 || d->w_layout != 2 || (a.x1_split && d->C1 < 1) || (a.y_split && !d->y) || (a.y_pool_split && !d->y_pool) ||
                    (a.x0_split && (d->c1_x32 || d->c1_spec64)))) return MFPA_EINVAL;
  if (d->x0_bf16 != nullptr && !((d->w_layout == 2 || (d->mode == 1 && d->precision >= 1)) && d->x0)) return MFPA_EINVAL;   // conv_wd16_kernel's loader, or the bf16x3 transposed convolution's
  if (d->x1_bf16 != nullptr && (d->w_layout != 2 || !d->x1 || d->C1 < 1)) return MFPA_EINVAL;
  // y_bf16 with y: a bf16 copy beside the float32 output; y_bf16 WITHOUT y: the output exists as bfloat16 only (conv_wd16_kernel, or the
  // bf16x3 transposed convolution)
  if (d->y_bf16 != nullptr && !(d->w_layout == 2 || (d->mode == 1 && d->precision >= 1 && !d->y))) return MFPA_EINVAL;
  if (!d->y && d->y_bf16 && (d->y_pool || d->w1x1 || d->precision == 0)) return MFPA_EINVAL;
  a.x0_bf16 = reinterpret_cast<__bf16*>(d->x0_bf16);
  a.x1_bf16 = reinterpret_cast<__bf16*>(d->x1_bf16);
  a.y_bf16 = reinterpret_cast<__bf16*>(d->y_bf16);
  if (d->stats_part != nullptr && (d->w_layout != 2 || (!d->y && !d->y_bf16))) return MFPA_EINVAL;       // only conv_wd16_kernel's epilogue writes them
  a.stats_part = d->stats_part;
  if (d->bwd_z != nullptr && (!d->stats_part || !d->bwd_scale || !d->bwd_shift || !d->bwd_mean || !d->bwd_invstd)) return MFPA_EINVAL;
  if (d->bwd_z != nullptr && d->x0_is_bf16 && (d->in_scale0 || d->x0_bf16)) return MFPA_EINVAL;   // (the training forward's form of the kernel carries no bwd_z code)
  a.bz16 = (d->bwd_z != nullptr && d->bwd_z_is_bf16) ? 1 : 0;
  a.bz = d->bwd_z; a.bz_scale = d->bwd_scale; a.bz_shift = d->bwd_shift; a.bz_mean = d->bwd_mean; a.bz_invstd = d->bwd_invstd;
  const int prec = d->precision ? 1 : 0;                                 // kernel family: fp32 MFMA or the bf16 matrix cores
  // the halo loader packs pixel coordinates into 16 bits each and addresses one clip's input with 32-bit byte offsets
  if (a.H > 32767 || a.W > 32767) return MFPA_EINVAL;
  if ((d->mode == 2 ? 4LL : 1LL) * a.H * a.W * a.C0 * 4 > 0xffffffffLL || 1LL * a.H1 * a.W1 * a.C1 * 4 > 0xffffffffLL) return MFPA_EINVAL;
  const int cin = a.C0 + a.C1;
  const bool bn128 = a.Cout % 128 == 0;
  const bool c1 = a.c1_x32 || a.c1_spec64;
  mfpa_conv_route t{}; t.mode = d->mode; t.prec = prec;
  if (d->mode == 1) {                  // the transposed convolution's forward; bfloat16 I/O (and with it the plain-bf16 form) is a bf16x3 instantiation
    t.family = MFPA_CONV_CONVT; t.bn = 64;
    t.ph = a.W > 16 ? 4 : 8; t.pw = a.W > 16 ? 32 : 16;
    t.io16 = a.in16 || a.y == nullptr;
    t.plain = t.io16 && a.plain;
    if (t.io16 && prec != 1) return MFPA_EINVAL;
  } else if (d->mode == 0 && prec == 1 && a.w_frag) {        // w_layout 2: the 16 x 16 x 32 weights-direct kernels
    if (conv_weight_layout(a.H, a.W, cin, a.Cout, 0, 1) != 2) return MFPA_EINVAL;
    t.ph = 8; t.pw = 32;
    if (conv_prefers_ws64(a.H, a.W, cin, a.Cout, c1) && mfpa_unet::conv_ws64_serves(a)) {
      t.family = MFPA_CONV_WS64; t.bn = 64; t.c1src = c1;
    } else {
      if (c1 || a.x0_split || a.x1_split || a.y_split || a.y_pool_split) return MFPA_EINVAL;   // only conv_ws64_kernel knows these
      t.family = MFPA_CONV_WD16;
      mfpa_unet::conv_wd16_tile(a.W, a.Cout, &t);
      t.plain = a.plain; t.in16 = a.in16;
      // ... in the training forward's form (AFF16), which carries the side outputs' code whether or not one is asked for
      t.aff16 = a.in16 && (a.in_scale0 != nullptr || a.x0_bf16 != nullptr || (a.y == nullptr && a.bz == nullptr));
      t.side = t.aff16 || a.x0_bf16 || a.x1_bf16 || a.y_bf16 || a.stats_part;
      t.rows = t.wmw == 2 && cin % 64 == 0 && (a.plain || cin >= mfpa_unet::CONV_WD16_ROWS);
      t.stats_rows = a.stats_part ? t.wmw : 0;      // [tile * WMW + wm][2][Cout]
    }
  } else {                             // conv_mfma_kernel: the row image
    t.family = MFPA_CONV_MFMA; t.bn = bn128 ? 128 : 64; t.c1src = c1;      // (c1, checked above: Cout == 64, W > 16, H >= 8 -- the 64 x 8 x 32 tile)
    const bool big = cin >= ((prec == 1 && d->mode == 0) ? CONV_BIG_MIN_CIN : 256);
    t.pw = a.W > 16 ? 32 : 16;
    if (a.W > 16) t.ph = (a.H >= 8 && (!bn128 || big)) ? 8 : 4;
    else t.ph = (bn128 && d->mode == 0 && prec == 1 && a.H >= 16) ? 16 : 8;
  }
  a.tiles_x = (a.W + t.pw - 1) / t.pw; a.tiles_y = (a.H + t.ph - 1) / t.ph;
  if ((long long)a.tiles_x * a.tiles_y * a.B > 0x7fffffffLL) return MFPA_EINVAL;      // one tile per workgroup (or per step of a persistent one): a 32-bit grid extent
  *r = t; t.stats_rows = 0;            // (stats_rows names no kernel)
  for (const ConvKernel& e : CONV_KERNELS)
    if (!memcmp(&e.r, &t, sizeof t)) { *k = &e; return MFPA_OK; }
  return MFPA_EHIP - (int)hipErrorInvalidDeviceFunction;     // a route without a kernel (none is made above): an error, never another kernel
}

static int conv_launch(const mfpa_conv_desc* d, void* stream, bool out_offsets = true) {
  ConvArgs a;
  mfpa_conv_route r;
  const ConvKernel* k;
  const int rc = conv_route(d, a, &r, &k, out_offsets);
  return k ? k->launch(a, mfpa_stream(stream)) : rc;
}

}  // namespace

extern "C" {

int mfpa_conv3x3_bn_relu(const float* x0, int C0, const float* x1, int C1, int H1, int W1, int B, int H, int W,
                         const float* w, int Cout, const float* scale, const float* shift, int relu, int precision,
                         float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x0 || !w || !y || B < 0 || H < 1 || W < 1) return MFPA_EINVAL;
  if (C0 < KC || C0 % KC || C1 < 0 || C1 % KC || Cout < 64 || Cout % 64) return MFPA_EINVAL;
  if (C1 > 0 && (!x1 || H1 < 1 || W1 < 1 || H1 > H || W1 > W)) return MFPA_EINVAL;
  if (precision != 0 && precision != 1) return MFPA_EINVAL;
  mfpa_conv_desc d{};                  // (x1 is zero-padded like F.pad(x1, [dx//2, dx-dx//2, dy//2, dy-dy//2]), unet.py:59-62)
  d.x0 = x0; d.x1 = x1; d.w = w; d.out_scale = scale; d.out_shift = shift; d.y = y;
  d.C0 = C0; d.C1 = C1; d.H1 = H1; d.W1 = W1; d.B = B; d.H = H; d.W = W; d.Cout = Cout; d.relu = relu; d.precision = precision;
  return conv_launch(&d, stream, false);
}

int mfpa_convT2x2(const float* x, int B, int H, int W, int Cin, const float* w, const float* bias, int Cout,
                  int precision, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !w || !y || B < 0 || H < 1 || W < 1) return MFPA_EINVAL;
  if (Cin < KC || Cin % KC || Cout < 64 || Cout % 64 || (precision != 0 && precision != 1)) return MFPA_EINVAL;
  if (4LL * H * W * Cout * 4 > 0xffffffffLL || 1LL * H * W * Cin * 4 > 0xffffffffLL) return MFPA_EINVAL;   // 32-bit byte offsets inside one clip
  mfpa_conv_desc d{};
  d.x0 = x; d.w = w; d.out_shift = bias; d.y = y;
  d.C0 = Cin; d.B = B; d.H = H; d.W = W; d.Cout = Cout; d.mode = 1; d.precision = precision;
  return conv_launch(&d, stream);
}

int mfpa_conv_mfma_route(const mfpa_conv_desc* d, mfpa_conv_route* out) {
  ConvArgs a;
  mfpa_conv_route r;
  const ConvKernel* k;
  return conv_route(d, a, out ? out : &r, &k);
}

int mfpa_conv_mfma(const mfpa_conv_desc* d, void* stream) { return conv_launch(d, stream); }

// The three queries below are asked about a SHAPE and answer from the rules conv_route itself calls, not from a route: beyond the limits a
// launch must also meet they keep the answers they always gave (include/mfpa.h at each; NOTES.md, "one routing function").
int mfpa_conv_c1_layout(int H, int W) {
  if (H < 1 || W < 1) return MFPA_EINVAL;
  // the fused first-layer launch (mfpa_conv_desc.c1_*, 64 -> 64) reads the fragment image 2 exactly where conv_ws64_kernel<C1SRC> takes it
  return conv_weight_layout(H, W, 64, 64, 0, 1) == 2 ? 2 : 0;     // (64-channel tiles: the wide levels only)
}

int mfpa_conv_scale_folds(int H, int W, int Cin, int Cout) {
  if (H < 1 || W < 1 || Cin < 1 || Cout < 1) return MFPA_EINVAL;
  return (conv_weight_layout(H, W, Cin, Cout, 0, 1) == 2 && Cin % KC == 0 && conv_prefers_ws64(H, W, Cin, Cout, false)) ? 1 : 0;
}

int mfpa_conv_weight_layout(int H, int W, int Cin, int Cout, int mode, int precision) {
  if (H < 1 || W < 1 || Cin < 1 || Cout < 1) return MFPA_EINVAL;
  return conv_weight_layout(H, W, Cin, Cout, mode, precision);
}

int mfpa_conv_stats_rows(int B, int H, int W, int Cin, int Cout) {
  if (B < 0 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return MFPA_EINVAL;
  if (conv_weight_layout(H, W, Cin, Cout, 0, 1) != 2) return 0;       // no kernel that writes the partials for this shape
  mfpa_conv_route t{};
  mfpa_unet::conv_wd16_tile(W, Cout, &t);                                         // one row per tile and wave row
  const long long rows = (long long)((W + t.pw - 1) / t.pw) * ((H + t.ph - 1) / t.ph) * B * t.wmw;
  return rows > 0x7fffffffLL ? MFPA_EINVAL : (int)rows;
}

int mfpa_conv3x3_c1_bn_relu(const float* x32, const double* spec64, const double* denom, int per_clip, int B, int H,
                            int W, const float* w, int Cout, const float* scale, const float* shift, int relu, float* y,
                            int y_is_bf16, float* stats_part, void* stream) {
  if (B == 0) return MFPA_OK;
  if ((!x32 && !spec64) || !w || !y || B < 0 || H < 1 || W < 1) return MFPA_EINVAL;
  if (Cout % 4 || Cout < 4 || Cout > 1024 || (256 % (Cout / 4)) != 0) return MFPA_EINVAL;
  if ((long long)B * H > 0x7fffffffLL) return MFPA_EINVAL;
  const long long blocks = (long long)B * H;
  hipLaunchKernelGGL(conv3x3_c1_kernel, dim3((unsigned)blocks), dim3(256), 0, mfpa_stream(stream), x32, spec64, denom,
                     per_clip, B, H, W, w, Cout, scale, shift, relu, y, y_is_bf16, stats_part);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_maxpool2(const float* x, int B, int H, int W, int C, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !y || B < 0 || H < 2 || W < 2 || C < 4 || C % 4) return MFPA_EINVAL;
  const long long total = (long long)B * (H / 2) * (W / 2) * (C / 4);
  long long blocks = (total + 255) / 256;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(maxpool2_kernel, dim3((unsigned)blocks), dim3(256), 0, mfpa_stream(stream), x, B, H, W, C, y);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_conv1x1_out(const float* x, long long npix, int C, const float* w, float bias, float* y, void* stream) {
  if (!x || !w || !y || npix < 0 || C < 4 || C > 256 || (C & (C - 1)) != 0) return MFPA_EINVAL;
  if (npix == 0) return MFPA_OK;
  const int ppb = 256 / (C / 4);
  long long blocks = (npix + ppb - 1) / ppb;
  if (blocks > 256 * 32) blocks = 256 * 32;
  hipLaunchKernelGGL(conv1x1_out_kernel, dim3((unsigned)blocks), dim3(256), 0, mfpa_stream(stream), x, npix, C, w, bias, y);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
