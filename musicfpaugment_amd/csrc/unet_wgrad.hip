// Weight gradients of the UNet denoiser's convolutions on MFMA for MI355X (gfx950): mfpa_wgrad_mfma (3x3 and transposed 2x2 layers, four
// precisions) and mfpa_wgrad_c1 (the one-input-channel first layer).  The rest of the training step is csrc/unet_train.hip.
//
// dW[tap][co][ci] += sum over pixels of dz[p][co] * xin[p + tap][ci]   (MODE 0, 3x3 conv, 9 taps)
// dW[tap][co][ci] += sum over pixels of dup[2y+dy, 2x+dx][co] * xin[y,x][ci]   (MODE 1, transposed conv, 4 taps)
// GEMM per tap: M = output channels, N = input channels, K = pixels.  A workgroup owns one (co, ci) tile for ALL taps and walks
// pixel patches (grid-strided over the batch): per patch the dz tile and the haloed xin tile are staged in LDS pixel-major (the
// natural NHWC order); each wave keeps one 32x32 accumulator per tap (9 x 16 VGPRs) and the A fragment of a k-step is reused by all
// taps.  Partial sums are added to dW with one float atomic per element per workgroup (256-B contiguous segments).
//
//   precision 0   wgrad_mfma_kernel<MODE>             fp32 MFMA, 2 x 32 patches, 256 threads
//   precision 1   wgrad_bf16x3_kernel<MODE, PW, false>  fp32 operands split hi + lo while staged, three bf16 MFMAs per product
//   precision 2   wgrad_bf16x3_kernel<MODE, PW, true>   fp32 operands, the hi halves only, one bf16 MFMA per product
//   precision 3   wgrad_bf16_kernel<PW, COT> (MODE 0), wgrad_bf16x3_kernel<1, PW, true, BF16IN, CI128> (MODE 1): bf16 operands, one MFMA per product
// The bf16 kernels run 512 threads on 128-pixel patches, 4 x 32 (PW 32) or 8 x 16 (PW 16, images at most 16 wide).
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"

namespace {

using mfpa_tile::bf16x4;
using mfpa_tile::bf16x8;
using mfpa_tile::f32x4;
using mfpa_tile::floatx16;

struct WgradArgs {
  const float* dz;        // MODE 0: (B,H,W,Cout);  MODE 1: (B,2H,2W,Cout)
  const float* x0;        // (B,H,W,C0)
  const float* in_scale0; // optional affine+ReLU on load for x0
  const float* in_shift0;
  const float* x1;        // (B,H1,W1,C1) zero-padded (MODE 0 only)
  float* dw;              // [taps][Cout][C0+C1]
  int C0, C1, H1, W1, oy1, ox1;
  int B, H, W, Cout;
  int tiles_x, tiles_y;
  unsigned drop_seed, drop_thresh;
  float drop_scale;
  int xcd;                  // bf16 kernels: XCD-aware (patch group, tile) order.  Always 1 (the plain order was an experiment, retired); the field and its
                            // test stay because without them hipcc allocates the wgrad kernels' registers differently
};

constexpr int WG_PH = 2, WG_PW = 32, WG_PIX = 64, WG_T = 64;
constexpr int WGB_THREADS = 512, WGB_PIX = 128;   // the bf16 kernels: one workgroup per CU, two waves per SIMD, 128-pixel patches

// ------------------------------------------------------------------ precision 0: fp32 MFMA
// 64 x 64 (co, ci) tiles, 2x32-pixel patches; MFMA lanes read 32 consecutive channels of one pixel with ds_read_b32 (no transpose).
template <int MODE>
__global__ __launch_bounds__(256, 2) void wgrad_mfma_kernel(WgradArgs a) {
  constexpr int HALO = (MODE == 0) ? 1 : 0;
  constexpr int TAPS = (MODE == 0) ? 9 : 4;
  constexpr int HPW = WG_PW + 2 * HALO, HPH = WG_PH + 2 * HALO, HP = HPW * HPH;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* Ds = reinterpret_cast<float*>(smem);   // [128][64]  dz tile (pixel-major)
  float* Xs = Ds + WG_PIX * WG_T;               // [HP][64]   xin tile with halo (pixel-major)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int cot = wave & 1, cit = wave >> 1;
  const int co0 = blockIdx.x * WG_T, ci0 = blockIdx.y * WG_T;
  const int Cin = a.C0 + a.C1;
  const bool from0 = ci0 < a.C0;
  const long long npatch = (long long)a.B * a.tiles_x * a.tiles_y;

  floatx16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  for (long long patch = blockIdx.z; patch < npatch; patch += gridDim.z) {
    long long q = patch;
    const int tx = (int)(q % a.tiles_x); q /= a.tiles_x;
    const int ty = (int)(q % a.tiles_y);
    const int b = (int)(q / a.tiles_y);
    const int y0 = ty * WG_PH, x0p = tx * WG_PW;
    __syncthreads();   // previous patch's fragment reads are done
    // stage xin (+halo): HP pixels x 64 channels
    for (int idx = tid; idx < HP * (WG_T / 4); idx += 256) {
      const int pix = idx / (WG_T / 4), c4 = idx % (WG_T / 4);
      const int gy = y0 + pix / HPW - HALO, gx = x0p + pix % HPW - HALO;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        if (from0) {
          v = *reinterpret_cast<const f32x4*>(a.x0 + (((size_t)b * a.H + gy) * a.W + gx) * a.C0 + ci0 + 4 * c4);
          if (a.in_scale0) {
            const f32x4 sc = *reinterpret_cast<const f32x4*>(a.in_scale0 + ci0 + 4 * c4);
            const f32x4 sh = *reinterpret_cast<const f32x4*>(a.in_shift0 + ci0 + 4 * c4);
            v = v * sc + sh;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
            if (a.drop_thresh) {
              const unsigned long long e0 = (((unsigned long long)b * a.H + gy) * a.W + gx) * a.C0 + ci0 + 4 * c4;
#pragma unroll
              for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
            }
          }
        } else {
          const int y1 = gy - a.oy1, x1 = gx - a.ox1;
          if (y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1)
            v = *reinterpret_cast<const f32x4*>(a.x1 + (((size_t)b * a.H1 + y1) * a.W1 + x1) * a.C1 + (ci0 - a.C0) + 4 * c4);
        }
      }
      *reinterpret_cast<f32x4*>(Xs + pix * WG_T + 4 * c4) = v;
    }
    for (int tap = 0; tap < (MODE == 0 ? 1 : TAPS); ++tap) {
      if (MODE == 1 && tap > 0) __syncthreads();
      // stage dz: 128 pixels x 64 channels (MODE 1: the tap's strided view of the upsampled gradient)
      for (int idx = tid; idx < WG_PIX * (WG_T / 4); idx += 256) {
        const int pix = idx / (WG_T / 4), c4 = idx % (WG_T / 4);
        const int gy = y0 + pix / WG_PW, gx = x0p + pix % WG_PW;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (gy < a.H && gx < a.W) {
          if (MODE == 0)
            v = *reinterpret_cast<const f32x4*>(a.dz + (((size_t)b * a.H + gy) * a.W + gx) * a.Cout + co0 + 4 * c4);
          else
            v = *reinterpret_cast<const f32x4*>(a.dz + (((size_t)b * (2 * a.H) + 2 * gy + (tap >> 1)) * (2 * a.W) + 2 * gx + (tap & 1)) * a.Cout + co0 + 4 * c4);
        }
        *reinterpret_cast<f32x4*>(Ds + pix * WG_T + 4 * c4) = v;
      }
      __syncthreads();
      const float* Ap = Ds + cot * 32 + li;
      const float* Bp = Xs + cit * 32 + li;
#pragma unroll 4
      for (int k0 = 0; k0 < WG_PIX; k0 += 2) {
        const int m = k0 + lh;
        const float av = Ap[m * WG_T];
        const int hb = ((m / WG_PW) * HPW + (m % WG_PW)) * WG_T;
        if (MODE == 0) {
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const float bv = Bp[hb + ((t / 3) * HPW + (t % 3)) * WG_T];
            acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
          }
        } else {
          const float bv = Bp[hb];
#pragma unroll
          for (int t = 0; t < TAPS; ++t)
            if (t == tap) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[t], 0, 0, 0);
        }
      }
    }
  }
  // D[row = co][col = ci]
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int ci = ci0 + cit * 32 + li;
      atomicAdd(a.dw + ((size_t)t * a.Cout + co) * Cin + ci, acc[t][r]);
    }
}

// ------------------------------------------------------------------ precisions 1 and 2, and precision 3 of the transposed convolution: bf16 MFMA
// bf16x3 products (precision 1): both operands are split x = hi + lo (bf16) while they are
// staged and each tap's product is dz_lo*x_hi + dz_hi*x_lo + dz_hi*x_hi on v_mfma_f32_32x32x16_bf16 -- 3 matrix
// instructions at 16x the fp32-MFMA rate.  K is the PIXEL index, but NHWC tiles are pixel-major: the fragments (8
// consecutive pixels of one channel per lane) come from gfx950's transposing LDS read ds_read_b64_tr_b16, which hands
// lane i of a 16-lane group column i of a 4-row block -- so the tiles stay in their natural order, and a tap shift is a
// whole-row offset folded into the instruction's immediate.  LDS pixel row = [64 ch hi | 64 ch lo | 64 B pad] = 320 B:
// the four rows of a block land on bank offsets 0 / 64 / 128 / 192 (conflict-free).
typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef unsigned int wg_u32x4 __attribute__((ext_vector_type(4)));
constexpr int WGB_ROW = 320;   // bytes per staged pixel

__device__ __forceinline__ bf16x8 wg_tr_frag(const char* p0, const char* p1) {
  typedef wg_s16x4 __attribute__((address_space(3))) * lds_ptr;
  const wg_s16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p0));
  const wg_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p1));
  union { short s[8]; bf16x8 b; } r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.s[j] = u[j]; r.s[4 + j] = v[j]; }
  return r.b;
}

template <bool PLAIN>
__device__ __forceinline__ void wg_store_split(char* row, int c4, f32x4 v) {
  bf16x4 hi, lo;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hi[k] = (__bf16)v[k];
    lo[k] = (__bf16)(v[k] - (float)hi[k]);
  }
  *reinterpret_cast<bf16x4*>(row + 8 * c4) = hi;
  if (!PLAIN) *reinterpret_cast<bf16x4*>(row + 128 + 8 * c4) = lo;
}

// 8 waves: (co half) x (ci half) x (pixel half of a 128-pixel patch, 4x32 or 8x16 for narrow images); one workgroup
// per CU, two waves per SIMD.
// PLAIN: one bf16 MFMA per product (precision 2) -- only the hi halves are staged (192-byte pixel rows: 128 B + 64 B pad keep
// the four rows of a transposing block on bank offsets 0 / 192 / 128 / 64).  A weight gradient sums over every pixel of the
// batch, so the 2^-9 rounding of the products averages out (relative L1 2e-3 vs fp32 on one layer, the level of fp32
// autograd's own noise through the BatchNorm backward) and nothing downstream consumes it except the optimiser.
// BF16IN (with PLAIN): dz / x0 / x1 are bf16 tensors that already hold the ACTIVATED values (mfpa_act_to_bf16: the previous layer's
// BatchNorm + ReLU + dropout applied, or a plain cast) -- every (co, ci) tile re-reads the patches of both operands, so for layers
// with many tiles halving the bytes per re-read pays for one cast pass (the kernel was bound by what it pulls from L2: skipping its
// loads returned 24 %); staging is then a 16-byte copy, no split.  Only instantiated with MODE 1 (MODE 0 with bf16 operands is
// wgrad_bf16_kernel), so ALLTAPS == BF16IN and the MODE 0 arms of the bf16 staging are in no instantiation.  They stay: with the ALLTAPS
// form as a kernel of its own and those arms deleted, hipcc schedules ten of the twelve instantiations differently.
template <int MODE, int PW, bool PLAIN, bool BF16IN = false, bool CI128 = false>
__global__ __launch_bounds__(512, 1) void wgrad_bf16x3_kernel(WgradArgs a) {
  static_assert(!BF16IN || PLAIN, "bf16 operands carry only the hi halves");
  static_assert(!CI128 || (MODE == 1 && BF16IN), "the 128-input-channel tile is a form of ALLTAPS");
  // CI128 (ALLTAPS only): a workgroup owns 64 output x 128 INPUT channels -- waves 2 (co) x 4 (ci), every wave walks all 128 pixels of the patch --
  // so the dz tiles, the larger operand (four taps), are re-read C_in / 128 times instead of C_in / 64: the 64 x 64 form moved 1.25 GB through L2
  // for 64 GFLOP (up1.up) at 5.7 TB/s
  constexpr int CIW = CI128 ? 128 : WG_T;                              // input channels per workgroup
  constexpr int ROWX = CI128 ? 320 : (PLAIN ? 192 : WGB_ROW);          // bytes per staged x pixel (256 B + 64 B pad: rows on bank offsets 0 / 64 / 128 / 192)
  constexpr int ROW = PLAIN ? 192 : WGB_ROW;
  constexpr int WGB_PH = WGB_PIX / PW;
  constexpr int HALO = (MODE == 0) ? 1 : 0;
  constexpr int TAPS = (MODE == 0) ? 9 : 4;
  constexpr int HPW = PW + 2 * HALO, HPH = WGB_PH + 2 * HALO, HP = HPW * HPH;
  constexpr int X_F4 = (HP * (WG_T / 4) + WGB_THREADS - 1) / WGB_THREADS;        // float4 loads per thread for the xin tile
  constexpr int D_F4 = WGB_PIX * (WG_T / 4) / WGB_THREADS;            // ... and for the dz tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // ALLTAPS (the transposed convolution's weight gradient from bf16 operands, round 5): the four taps' strided views of dz are staged TOGETHER
  // -- four dz tiles in LDS, requested with the next patch's x tile under the current patch's MFMAs -- instead of one after the other, each
  // behind its own exposed global round trip and two barriers for 8 MFMAs of work (0.085 MFMA-busy, 1.2 ms per train step)
  constexpr bool ALLTAPS = MODE == 1 && BF16IN;
  constexpr int DT = ALLTAPS ? 4 : 1;
  char* Ds = smem;                          // [DT][128 px][ROW]  dz tile(s)
  char* Xs = smem + DT * WGB_PIX * ROW;  // [HP px][ROWX]  xin tile with halo

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int cot = wave & 1, cit = CI128 ? (wave >> 1) : ((wave >> 1) & 1), ph = CI128 ? 0 : (wave >> 2);   // ph: the patch's upper / lower 64 pixels
  // (co tile, ci tile, patch group) of this workgroup.  Every tile of one patch group reads the same dz / x patches; consecutive
  // workgroup ids are dealt round-robin over the 8 XCDs (one L2 each), so with the plain order every XCD fetched every patch.
  // When the grid size is a multiple of 8, XCD k owns a contiguous range of the (group, tile) order instead, tiles fastest.
  unsigned bxi = blockIdx.x, byi = blockIdx.y, bzi = blockIdx.z;
  {
    const unsigned tiles = gridDim.x * gridDim.y, total = tiles * gridDim.z;
    if (a.xcd && total % 8 == 0) {
      const unsigned hw = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
      const unsigned lin = (hw % 8) * (total / 8) + hw / 8;
      const unsigned tile = lin % tiles;
      bzi = lin / tiles; bxi = tile % gridDim.x; byi = tile / gridDim.x;
    }
  }
  const int co0 = bxi * WG_T, ci0 = byi * CIW;
  const int Cin = a.C0 + a.C1;
  const bool from0 = ci0 < a.C0;
  const bool affine = from0 && a.in_scale0 != nullptr;
  const long long npatch = (long long)a.B * a.tiles_x * a.tiles_y;
  const int c4 = tid % (WG_T / 4);          // this thread's channel quad (the same for every staged pixel: 512 % 16 == 0)
  // transposing read: lane 4q+p of a 16-lane group addresses row q (pixel), columns 4p..4p+3 (channels) of its block
  const int gl = lane & 15, tq = gl >> 2, tp = gl & 3, gsel = (lane >> 4) & 1;
  const char* a_lane = Ds + (64 * ph + 8 * lh + tq) * ROW + (32 * cot + 16 * gsel + 4 * tp) * 2;
  const char* b_lane = Xs + ((64 / PW) * ph * HPW + 8 * lh + tq) * ROWX + (32 * cit + 16 * gsel + 4 * tp) * 2;

  f32x4 a_sc = {1.f, 1.f, 1.f, 1.f}, a_sh = {0.f, 0.f, 0.f, 0.f};
  if (affine) {
    a_sc = *reinterpret_cast<const f32x4*>(a.in_scale0 + ci0 + 4 * c4);
    a_sh = *reinterpret_cast<const f32x4*>(a.in_shift0 + ci0 + 4 * c4);
  }

  floatx16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // Software pipeline over patches: the global loads of patch n+1 are issued (into registers, no dependent use) before
  // the MFMA block of patch n and are split / written to LDS after it.
  f32x4 xr[X_F4], dr[D_F4];
  auto decode = [&](long long patch, int& b, int& y0, int& x0p) __attribute__((always_inline)) {
    long long q = patch;
    const int tx = (int)(q % a.tiles_x); q /= a.tiles_x;
    const int ty = (int)(q % a.tiles_y);
    b = (int)(q / a.tiles_y);
    y0 = ty * WGB_PH; x0p = tx * PW;
  };
  // A thread's staging slots map to fixed pixels of the patch (pixel = tid / 16 + it * THREADS / 16, channel quad c4): a load is a
  // per-patch SCALAR base plus an element offset that depends only on the in-patch (row, column) -- two integer multiply-adds and
  // four compares for the image border, re-derived from compile-time divisors (no register arrays next to the 144 accumulators)
  // -- instead of a division / 64-bit index chain per load (the loads' address work was the largest single cost of this kernel:
  // skipping the next patch's loads returned 24 %).  Loads are unconditional: a pixel outside the image reads the element at offset
  // 0 of its channel quad and is zeroed when it is staged, so there are no exec-mask branches.
  const int t16 = tid / (WG_T / 4);
  constexpr int PIX_STEP = WGB_THREADS / (WG_T / 4);
  auto x_inside = [&](int pix, int y0, int x0p) __attribute__((always_inline)) {            // inside the image (source 0's extent)?
    const int gy = y0 + pix / HPW - HALO, gx = x0p + pix % HPW - HALO;
    return pix < HP && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
  };
  auto x1_inside = [&](int pix, int y0, int x0p) __attribute__((always_inline)) {           // ... and inside the zero-padded second source?
    const int y1 = y0 + pix / HPW - HALO - a.oy1, x1 = x0p + pix % HPW - HALO - a.ox1;
    return pix < HP && y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1;
  };
  auto load_x = [&](int b, int y0, int x0p) __attribute__((always_inline)) {
    // a slot outside the image loads its nearest image pixel (a line its neighbours fetch anyway; one fixed address for all of them
    // would be a hot spot) and is zeroed when it is staged
    if (from0) {
      const float* base = a.x0 + (size_t)b * a.H * a.W * a.C0 + ci0 + 4 * c4;
#pragma unroll
      for (int it = 0; it < X_F4; ++it) {
        const int pix = t16 + it * PIX_STEP;
        const int gy = min(max(y0 + pix / HPW - HALO, 0), a.H - 1), gx = min(max(x0p + pix % HPW - HALO, 0), a.W - 1);
        xr[it] = *reinterpret_cast<const f32x4*>(base + (gy * a.W + gx) * a.C0);
      }
    } else {
      const float* base = a.x1 + (size_t)b * a.H1 * a.W1 * a.C1 + (ci0 - a.C0) + 4 * c4;
#pragma unroll
      for (int it = 0; it < X_F4; ++it) {
        const int pix = t16 + it * PIX_STEP;
        const int y1 = min(max(y0 + pix / HPW - HALO - a.oy1, 0), a.H1 - 1), x1 = min(max(x0p + pix % HPW - HALO - a.ox1, 0), a.W1 - 1);
        xr[it] = *reinterpret_cast<const f32x4*>(base + (y1 * a.W1 + x1) * a.C1);
      }
    }
  };
  auto store_x = [&](int b, int y0, int x0p) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < X_F4; ++it) {
      const int pix = t16 + it * PIX_STEP;
      if (pix < HP) {
        const bool inside = from0 ? x_inside(pix, y0, x0p) : x1_inside(pix, y0, x0p);
        f32x4 v = xr[it];
        if (!inside) v = f32x4{0.f, 0.f, 0.f, 0.f};               // zero padding
        if (affine && inside) {                                    // padding stays exactly zero
          v = v * a_sc + a_sh;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
          if (a.drop_thresh) {
            const int gy = y0 + pix / HPW - HALO, gx = x0p + pix % HPW - HALO;
            const unsigned long long e0 = (((unsigned long long)b * a.H + gy) * a.W + gx) * a.C0 + ci0 + 4 * c4;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
          }
        }
        wg_store_split<PLAIN>(Xs + pix * ROW, c4, v);
      }
    }
  };
  // dz tile: zero past the image border is applied when the tile is staged (store_d keeps the patch position for it)
  int d_y0 = 0, d_x0 = 0;
  auto load_d = [&](int b, int y0, int x0p, int tap) __attribute__((always_inline)) {
    const float* base = (MODE == 0) ? a.dz + (size_t)b * a.H * a.W * a.Cout + co0 + 4 * c4
                                    : a.dz + (size_t)b * (2 * a.H) * (2 * a.W) * a.Cout + co0 + 4 * c4;
#pragma unroll
    for (int it = 0; it < D_F4; ++it) {
      const int pix = t16 + it * PIX_STEP;
      const int gy = min(y0 + pix / PW, a.H - 1), gx = min(x0p + pix % PW, a.W - 1);       // clamped; zeroed in store_d when outside
      const int off = (MODE == 0) ? (gy * a.W + gx) * a.Cout : ((2 * gy + (tap >> 1)) * (2 * a.W) + 2 * gx + (tap & 1)) * a.Cout;
      dr[it] = *reinterpret_cast<const f32x4*>(base + off);
    }
    d_y0 = y0; d_x0 = x0p;
  };
  auto store_d = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < D_F4; ++it) {
      const int pix = t16 + it * PIX_STEP;
      const bool in = d_y0 + pix / PW < a.H && d_x0 + pix % PW < a.W;
      wg_store_split<PLAIN>(Ds + pix * ROW, c4, in ? dr[it] : f32x4{0.f, 0.f, 0.f, 0.f});
    }
  };
  // ---- BF16IN staging: 8 threads per pixel, one 16-byte piece (8 channels) each
  constexpr int X_L = BF16IN ? (HP * 8 + WGB_THREADS - 1) / WGB_THREADS : 1;
  constexpr int D_L = BF16IN ? WGB_PIX * 8 / WGB_THREADS : 1;
  constexpr int PIX_STEP8 = WGB_THREADS / 8;
  const int c8 = tid % 8, t8 = tid / 8;
  wg_u32x4 xr16[X_L], dr16[D_L];
  auto load_x16 = [&](int b, int y0, int x0p) __attribute__((always_inline)) {
    if (from0) {
      const char* base = reinterpret_cast<const char*>(a.x0) + ((size_t)b * a.H * a.W * a.C0 + ci0 + 8 * c8) * 2;
#pragma unroll
      for (int it = 0; it < X_L; ++it) {
        const int pix = t8 + it * PIX_STEP8;
        const int gy = min(max(y0 + pix / HPW - HALO, 0), a.H - 1), gx = min(max(x0p + pix % HPW - HALO, 0), a.W - 1);
        xr16[it] = *reinterpret_cast<const wg_u32x4*>(base + (size_t)((gy * a.W + gx) * a.C0) * 2);
      }
    } else {
      const char* base = reinterpret_cast<const char*>(a.x1) + ((size_t)b * a.H1 * a.W1 * a.C1 + (ci0 - a.C0) + 8 * c8) * 2;
#pragma unroll
      for (int it = 0; it < X_L; ++it) {
        const int pix = t8 + it * PIX_STEP8;
        const int y1 = min(max(y0 + pix / HPW - HALO - a.oy1, 0), a.H1 - 1), x1 = min(max(x0p + pix % HPW - HALO - a.ox1, 0), a.W1 - 1);
        xr16[it] = *reinterpret_cast<const wg_u32x4*>(base + (size_t)((y1 * a.W1 + x1) * a.C1) * 2);
      }
    }
  };
  auto store_x16 = [&](int y0, int x0p) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < X_L; ++it) {
      const int pix = t8 + it * PIX_STEP8;
      if (pix < HP) {
        const bool inside = from0 ? x_inside(pix, y0, x0p) : x1_inside(pix, y0, x0p);
        *reinterpret_cast<wg_u32x4*>(Xs + pix * ROW + 16 * c8) = inside ? xr16[it] : wg_u32x4{0u, 0u, 0u, 0u};
      }
    }
  };
  auto load_d16 = [&](int b, int y0, int x0p, int tap) __attribute__((always_inline)) {
    const char* base = reinterpret_cast<const char*>(a.dz) +
                       ((size_t)b * (MODE == 0 ? 1 : 4) * a.H * a.W * a.Cout + co0 + 8 * c8) * 2;
#pragma unroll
    for (int it = 0; it < D_L; ++it) {
      const int pix = t8 + it * PIX_STEP8;
      const int gy = min(y0 + pix / PW, a.H - 1), gx = min(x0p + pix % PW, a.W - 1);
      const int off = (MODE == 0) ? (gy * a.W + gx) * a.Cout : ((2 * gy + (tap >> 1)) * (2 * a.W) + 2 * gx + (tap & 1)) * a.Cout;
      dr16[it] = *reinterpret_cast<const wg_u32x4*>(base + (size_t)off * 2);
    }
    d_y0 = y0; d_x0 = x0p;
  };
  auto store_d16 = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < D_L; ++it) {
      const int pix = t8 + it * PIX_STEP8;
      const bool in = d_y0 + pix / PW < a.H && d_x0 + pix % PW < a.W;
      *reinterpret_cast<wg_u32x4*>(Ds + pix * ROW + 16 * c8) = in ? dr16[it] : wg_u32x4{0u, 0u, 0u, 0u};
    }
  };
  // CI128: the x tile is 128 pixels x 16 pieces of 16 bytes (no halo in mode 1): four pieces per thread
  constexpr int X_L2 = CI128 ? WGB_PIX * 16 / WGB_THREADS : 1;
  const int c16 = tid % 16, t16b = tid / 16;
  wg_u32x4 xr16w[X_L2];
  auto load_x16w = [&](int b, int y0, int x0p) __attribute__((always_inline)) {
    const char* base = reinterpret_cast<const char*>(a.x0) + ((size_t)b * a.H * a.W * a.C0 + ci0 + 8 * c16) * 2;
#pragma unroll
    for (int it = 0; it < X_L2; ++it) {
      const int pix = t16b + it * (WGB_THREADS / 16);
      const int gy = min(y0 + pix / PW, a.H - 1), gx = min(x0p + pix % PW, a.W - 1);
      xr16w[it] = *reinterpret_cast<const wg_u32x4*>(base + (size_t)((gy * a.W + gx) * a.C0) * 2);
    }
  };
  auto store_x16w = [&](int y0, int x0p) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < X_L2; ++it) {
      const int pix = t16b + it * (WGB_THREADS / 16);
      const bool inside = y0 + pix / PW < a.H && x0p + pix % PW < a.W;
      *reinterpret_cast<wg_u32x4*>(Xs + pix * ROWX + 16 * c16) = inside ? xr16w[it] : wg_u32x4{0u, 0u, 0u, 0u};
    }
  };
  // ALLTAPS: the four taps' tiles at once
  wg_u32x4 dr16q[ALLTAPS ? 4 : 1][D_L];
  auto load_d16_all = [&](int b, int y0, int x0p) __attribute__((always_inline)) {
    const char* base = reinterpret_cast<const char*>(a.dz) + ((size_t)b * 4 * a.H * a.W * a.Cout + co0 + 8 * c8) * 2;
#pragma unroll
    for (int tap = 0; tap < (ALLTAPS ? 4 : 1); ++tap)
#pragma unroll
      for (int it = 0; it < D_L; ++it) {
        const int pix = t8 + it * PIX_STEP8;
        const int gy = min(y0 + pix / PW, a.H - 1), gx = min(x0p + pix % PW, a.W - 1);
        const int off = ((2 * gy + (tap >> 1)) * (2 * a.W) + 2 * gx + (tap & 1)) * a.Cout;
        dr16q[tap][it] = *reinterpret_cast<const wg_u32x4*>(base + (size_t)off * 2);
      }
    d_y0 = y0; d_x0 = x0p;
  };
  auto store_d16_all = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int tap = 0; tap < (ALLTAPS ? 4 : 1); ++tap)
#pragma unroll
      for (int it = 0; it < D_L; ++it) {
        const int pix = t8 + it * PIX_STEP8;
        const bool in = d_y0 + pix / PW < a.H && d_x0 + pix % PW < a.W;
        *reinterpret_cast<wg_u32x4*>(Ds + (tap * WGB_PIX + pix) * ROW + 16 * c8) = in ? dr16q[tap][it] : wg_u32x4{0u, 0u, 0u, 0u};
      }
  };
  // one set of names for the patch loop below
  auto LOAD_X = [&](int b, int y0, int x0p) __attribute__((always_inline)) { if constexpr (BF16IN) load_x16(b, y0, x0p); else load_x(b, y0, x0p); };
  auto STORE_X = [&](int b, int y0, int x0p) __attribute__((always_inline)) { if constexpr (BF16IN) store_x16(y0, x0p); else store_x(b, y0, x0p); };
  auto LOAD_D = [&](int b, int y0, int x0p, int tap) __attribute__((always_inline)) { if constexpr (BF16IN) load_d16(b, y0, x0p, tap); else load_d(b, y0, x0p, tap); };
  auto STORE_D = [&]() __attribute__((always_inline)) { if constexpr (BF16IN) store_d16(); else store_d(); };
  auto mfma3 = [&](floatx16& c, bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl) __attribute__((always_inline)) {
    if (!PLAIN) {
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
      c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    }
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
  };

  int b = 0, y0 = 0, x0p = 0;
  long long patch = bzi;
  if constexpr (ALLTAPS) {
    auto LOAD_XA = [&](int b_, int y_, int x_) __attribute__((always_inline)) { if constexpr (CI128) load_x16w(b_, y_, x_); else LOAD_X(b_, y_, x_); };
    auto STORE_XA = [&](int b_, int y_, int x_) __attribute__((always_inline)) { if constexpr (CI128) store_x16w(y_, x_); else STORE_X(b_, y_, x_); };
    if (patch < npatch) {
      decode(patch, b, y0, x0p);
      LOAD_XA(b, y0, x0p);
      load_d16_all(b, y0, x0p);
    }
    for (; patch < npatch; patch += gridDim.z) {
      __syncthreads();                     // the previous patch's fragment reads are done
      STORE_XA(b, y0, x0p);
      store_d16_all();
      __syncthreads();
      const long long next = patch + gridDim.z;
      int nb = 0, ny0 = 0, nx0 = 0;
      if (next < npatch) {                 // the next patch's five tiles: their loads land during the MFMA block below
        decode(next, nb, ny0, nx0);
        LOAD_XA(nb, ny0, nx0);
        load_d16_all(nb, ny0, nx0);
      }
#pragma unroll 2
      for (int ks = 0; ks < (CI128 ? WGB_PIX : WG_PIX) / 16; ++ks) {
        const char* bp = b_lane + (((16 * ks) / PW) * HPW + (16 * ks) % PW) * ROWX;
        const bf16x8 bh = wg_tr_frag(bp, bp + 4 * ROWX);          // the x fragment serves all four taps
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const char* ap = a_lane + (t * WGB_PIX + 16 * ks) * ROW;
          const bf16x8 ah = wg_tr_frag(ap, ap + 4 * ROW);
          acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t], 0, 0, 0);
        }
      }
      b = nb; y0 = ny0; x0p = nx0;
    }
  } else
  if (patch < npatch) {
    decode(patch, b, y0, x0p);
    LOAD_X(b, y0, x0p);
    LOAD_D(b, y0, x0p, 0);
  }
  for (; !ALLTAPS && patch < npatch; patch += gridDim.z) {
    __syncthreads();                       // the previous patch's fragment reads are done
    STORE_X(b, y0, x0p);
    STORE_D();
    __syncthreads();
    const long long next = patch + gridDim.z;
    int nb = 0, ny0 = 0, nx0 = 0;
    if (MODE == 0 && next < npatch) {      // prefetch the next patch; the loads land during the MFMA block below
      decode(next, nb, ny0, nx0);
      LOAD_X(nb, ny0, nx0);
      LOAD_D(nb, ny0, nx0, 0);
    }
    for (int tap = 0; tap < (MODE == 0 ? 1 : TAPS); ++tap) {
      if (MODE == 1 && tap > 0) {          // transposed conv: the tap's strided view of dz replaces the dz tile
        __syncthreads();
        LOAD_D(b, y0, x0p, tap);
        STORE_D();
        __syncthreads();
      }
#pragma unroll 1   // one k-step's 9 taps in flight at a time: bounds the live fragment registers next to 144 accumulators
      for (int ks = 0; ks < WG_PIX / 16; ++ks) {
        // this lane's 8 pixels: k = 16 ks + 8 lh + (0..7) of the wave's 64: patch row 16 ks / PW, columns 16 ks % PW + 8 lh + (0..7)
        const char* ap = a_lane + (16 * ks) * ROW;
        const bf16x8 ah = wg_tr_frag(ap, ap + 4 * ROW);
        const bf16x8 al = PLAIN ? ah : wg_tr_frag(ap + 128, ap + 4 * ROW + 128);
        if (MODE == 0) {
          const char* bk = b_lane + (((16 * ks) / PW) * HPW + (16 * ks) % PW) * ROW;
#pragma unroll
          for (int t = 0; t < 9; ++t) {
            const char* bp = bk + ((t / 3) * HPW + (t % 3)) * ROW;
            const bf16x8 bh = wg_tr_frag(bp, bp + 4 * ROW);
            mfma3(acc[t], ah, al, bh, PLAIN ? bh : wg_tr_frag(bp + 128, bp + 4 * ROW + 128));
          }
        } else {
          const char* bp = b_lane + (((16 * ks) / PW) * HPW + (16 * ks) % PW) * ROW;
          const bf16x8 bh = wg_tr_frag(bp, bp + 4 * ROW);
          const bf16x8 bl = PLAIN ? bh : wg_tr_frag(bp + 128, bp + 4 * ROW + 128);
#pragma unroll
          for (int t = 0; t < TAPS; ++t)
            if (t == tap) mfma3(acc[t], ah, al, bh, bl);
        }
      }
    }
    if (MODE == 1 && next < npatch) {
      decode(next, nb, ny0, nx0);
      LOAD_X(nb, ny0, nx0);
      LOAD_D(nb, ny0, nx0, 0);
    }
    b = nb; y0 = ny0; x0p = nx0;
  }
  // D[row = co][col = ci]
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int ci = ci0 + cit * 32 + li;
      atomicAdd(a.dw + ((size_t)t * a.Cout + co) * Cin + ci, acc[t][r]);
    }
}

// ------------------------------------------------------------------ precision 3, 3x3: bf16 operands
// One bf16 MFMA per product, from bf16 copies of dz / x0 / x1 ("V2" of the PLAIN + BF16IN form above, which no longer exists for MODE 0).
// What the skip experiments on that form said (tools/exp_wgrad.py, 512 -> 512 @ 32 x 31, 64 clips, 453 us): fragment reads + MFMAs alone
// 220 us, the staging chain alone 176 us, the two together 369 -- the staging sat in front of the MFMA block as a bubble all eight
// waves share (they are in lockstep behind the barriers) -- and the final atomics 130 us of every launch.  Here:
//   * a workgroup owns 32 COT output channels x 64 input channels x 9 taps; with COT = 4 (C_out % 128 == 0) the eight waves are 4 x 2
//     tiles and every wave walks all 128 pixels of a patch -- no two waves hold the same (co, ci) tile, so half the atomics and half the
//     operand bytes per MFMA of the 64 x 64 form (COT = 2: two pixel halves, as before);
//   * two LDS stages, ONE barrier per patch: the staging registers (patch n + 1, requested most of an iteration ago) are written to the
//     other stage between the MFMAs of k-step 0, and take patch n + 2 between the MFMAs of k-step 1 (sched_group_barrier-pinned; the
//     staging code is branch-free so that it can sit inside the MFMA block);
//   * the three dx taps of a halo row share their transposing reads: a lane's pixels P .. P+9 of one x column come from THREE
//     ds_read_b64_tr_b16 (r0..r4 = pixel pairs); tap dx = 0 is r0..r3, dx = 2 is r1..r4 (no instruction), dx = 1 four v_alignbit --
//     11 reads per k-step instead of 20, 22 fragment registers instead of 80, so the next k-step's reads run under this one's MFMAs;
//   * one workgroup per CU and as few patch groups as fill the chip once or twice: the atomics are per workgroup.
template <int PW, int COT>
__global__ __launch_bounds__(512, 1) void wgrad_bf16_kernel(WgradArgs a) {
  constexpr int THREADS = WGB_THREADS, PIX = WGB_PIX, PH_ = PIX / PW, TAPS = 9;
  constexpr int PHS = 4 / COT;                                         // pixel halves (waves that share a (co, ci) tile)
  constexpr int KS = PIX / PHS / 16;                                   // k-steps per wave and patch
  constexpr int COW = 32 * COT;                                        // output channels per workgroup
  constexpr int ROW_D = COW * 2 + 64, ROW_X = 192;                     // staged pixel rows: data + 64 B (the four rows of a transposing block
                                                                       // land on bank offsets 0 / 64 / 128 / 192)
  constexpr int HPW = PW + 2, HPH = PH_ + 2, HP = HPW * HPH;
  constexpr int XROWS = HP + 4;                                        // the third read of a row block runs two pixels past the halo tile
  constexpr int STAGE = PIX * ROW_D + XROWS * ROW_X;
  constexpr int DPP = COW / 8;                                         // 16-byte pieces per dz pixel
  constexpr int D_L = PIX * DPP / THREADS, X_L = (HP * 8 + THREADS - 1) / THREADS;
  static_assert(KS % 2 == 0 && KS >= 4, "fragment sets alternate; k-steps 0 and 1 carry the staging");
  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int cot = wave % COT, cit = (wave / COT) & 1, ph = wave / (2 * COT);
  unsigned bxi = blockIdx.x, byi = blockIdx.y, bzi = blockIdx.z;
  {
    const unsigned tiles = gridDim.x * gridDim.y, total = tiles * gridDim.z;
    if (a.xcd && total % 8 == 0) {
      const unsigned hw = blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
      const unsigned lin = (hw % 8) * (total / 8) + hw / 8;
      const unsigned tile = lin % tiles;
      bzi = lin / tiles; bxi = tile % gridDim.x; byi = tile / gridDim.x;
    }
  }
  const int co0 = bxi * COW, ci0 = byi * WG_T;
  const int Cin = a.C0 + a.C1;
  const bool from0 = ci0 < a.C0;
  const long long npatch = (long long)a.B * a.tiles_x * a.tiles_y;
  const int gl = lane & 15, tq = gl >> 2, tp = gl & 3, gsel = (lane >> 4) & 1;
  const char* a_lane = smem + ((PIX / PHS) * ph + 8 * lh + tq) * ROW_D + (32 * cot + 16 * gsel + 4 * tp) * 2;
  const char* b_lane = smem + PIX * ROW_D + ((PIX / PHS / PW) * ph * HPW + 8 * lh + tq) * ROW_X + (32 * cit + 16 * gsel + 4 * tp) * 2;

  floatx16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  // ---- staging: one code path for both sources of the input (extent, channel count and zero-pad offset of the one this tile reads)
  const int sH = from0 ? a.H : a.H1, sW = from0 ? a.W : a.W1, sC = from0 ? a.C0 : a.C1, soy = from0 ? 0 : a.oy1, sox = from0 ? 0 : a.ox1;
  const int c8 = tid % 8, t8 = tid / 8, cd = tid % DPP, td = tid / DPP;
  const char* xsrc = (from0 ? reinterpret_cast<const char*>(a.x0) + (size_t)(ci0 + 8 * c8) * 2
                            : reinterpret_cast<const char*>(a.x1) + (size_t)(ci0 - a.C0 + 8 * c8) * 2);
  const char* dsrc = reinterpret_cast<const char*>(a.dz) + (size_t)(co0 + 8 * cd) * 2;
  wg_u32x4 xr[X_L], dr[D_L];
  int pb = 0, py = 0, px = 0;                                           // patch in the staging registers
  auto decode = [&](long long patch) __attribute__((always_inline)) {
    long long q = patch;
    const int tx = (int)(q % a.tiles_x); q /= a.tiles_x;
    const int ty = (int)(q % a.tiles_y);
    pb = (int)(q / a.tiles_y); py = ty * PH_; px = tx * PW;
  };
  auto load = [&]() __attribute__((always_inline)) {                    // clamped addresses; what lies outside is zeroed by stage()
    const char* xb = xsrc + (size_t)pb * sH * sW * sC * 2;
#pragma unroll
    for (int it = 0; it < X_L; ++it) {
      const int pix = t8 + it * (THREADS / 8);
      const int gy = min(max(py + pix / HPW - 1 - soy, 0), sH - 1), gx = min(max(px + pix % HPW - 1 - sox, 0), sW - 1);
      xr[it] = *reinterpret_cast<const wg_u32x4*>(xb + (size_t)((gy * sW + gx) * sC) * 2);
    }
    const char* db = dsrc + (size_t)pb * a.H * a.W * a.Cout * 2;
#pragma unroll
    for (int it = 0; it < D_L; ++it) {
      const int pix = td + it * (THREADS / DPP);
      const int gy = min(py + pix / PW, a.H - 1), gx = min(px + pix % PW, a.W - 1);
      dr[it] = *reinterpret_cast<const wg_u32x4*>(db + (size_t)((gy * a.W + gx) * a.Cout) * 2);
    }
  };
  auto stage = [&](int soff) __attribute__((always_inline)) {
#pragma unroll
    for (int it = 0; it < X_L; ++it) {
      const int pix = t8 + it * (THREADS / 8);
      const unsigned sy = (unsigned)(py + pix / HPW - 1 - soy), sx = (unsigned)(px + pix % HPW - 1 - sox);
      const bool inside = (int)(pix < HP) & (int)(sy < (unsigned)sH) & (int)(sx < (unsigned)sW);
      // slots past the tile write zeros into its last slack row
      *reinterpret_cast<wg_u32x4*>(smem + soff + PIX * ROW_D + min(pix, XROWS - 1) * ROW_X + 16 * c8) = inside ? xr[it] : wg_u32x4{0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int it = 0; it < D_L; ++it) {
      const int pix = td + it * (THREADS / DPP);
      const bool in = (int)(py + pix / PW < a.H) & (int)(px + pix % PW < a.W);
      *reinterpret_cast<wg_u32x4*>(smem + soff + pix * ROW_D + 16 * cd) = in ? dr[it] : wg_u32x4{0u, 0u, 0u, 0u};
    }
  };
  // ---- fragments
  typedef wg_s16x4 __attribute__((address_space(3))) * lds_ptr;
  struct Fr { bf16x8 a; unsigned r[3][5]; };
  auto read_fr = [&](Fr& f, int soff, int ks) __attribute__((always_inline)) {
    const char* ap = a_lane + soff + (16 * ks) * ROW_D;
    f.a = wg_tr_frag(ap, ap + 4 * ROW_D);
    const char* bk = b_lane + soff + (((16 * ks) / PW) * HPW + (16 * ks) % PW) * ROW_X;
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      const char* bp = bk + dy * HPW * ROW_X;
      union { wg_s16x4 s; unsigned u[2]; } u0, u1, u2;
      u0.s = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(bp));
      u1.s = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(bp + 4 * ROW_X));
      u2.s = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(bp + 8 * ROW_X));
      f.r[dy][0] = u0.u[0]; f.r[dy][1] = u0.u[1]; f.r[dy][2] = u1.u[0]; f.r[dy][3] = u1.u[1]; f.r[dy][4] = u2.u[0];
    }
  };
  auto mfma9 = [&](const Fr& f) __attribute__((always_inline)) {
#pragma unroll
    for (int dy = 0; dy < 3; ++dy) {
      union { unsigned u[4]; bf16x8 b; } f0, f1, f2;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f0.u[j] = f.r[dy][j];
        f1.u[j] = __builtin_amdgcn_alignbit(f.r[dy][j + 1], f.r[dy][j], 16);
        f2.u[j] = f.r[dy][j + 1];
      }
      acc[3 * dy + 0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a, f0.b, acc[3 * dy + 0], 0, 0, 0);
      acc[3 * dy + 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a, f1.b, acc[3 * dy + 1], 0, 0, 0);
      acc[3 * dy + 2] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a, f2.b, acc[3 * dy + 2], 0, 0, 0);
    }
  };

  long long patch = bzi;
  if (patch < npatch) {
    decode(patch);
    load();
    stage(0);
    decode(patch + gridDim.z < npatch ? patch + gridDim.z : patch);     // past the end: the same patch again, never used
    load();
  }
  __syncthreads();
  int sel = 0;
  Fr fa, fb;
  for (; patch < npatch; patch += gridDim.z) {
    const int soff = sel * STAGE, noff = (sel ^ 1) * STAGE;
    read_fr(fa, soff, 0);
    __builtin_amdgcn_sched_barrier(0);
    // k-step 0: MFMAs || k-step 1's reads, the staging registers -> the other stage
    read_fr(fb, soff, 1);
    stage(noff);
    mfma9(fa);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
      if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    // k-step 1: MFMAs || k-step 2's reads, the staging registers <- patch n + 2
    read_fr(fa, soff, 2);
    {
      const long long n2 = patch + 2 * (long long)gridDim.z;
      decode(n2 < npatch ? n2 : patch);
      load();
    }
    mfma9(fb);
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x002, 10, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 2; ks < KS; ks += 2) {
      read_fr(fb, soff, ks + 1);
      mfma9(fa);
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
        if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      if (ks + 2 < KS) {
        read_fr(fa, soff, ks + 2);
        mfma9(fb);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
          __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
          if (i < 6) __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      } else {
        mfma9(fb);
      }
    }
    __syncthreads();
    sel ^= 1;
  }
  // D[row = co][col = ci]
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = co0 + cot * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int ci = ci0 + cit * 32 + li;
      atomicAdd(a.dw + ((size_t)t * a.Cout + co) * Cin + ci, acc[t][r]);
    }
}

// ------------------------------------------------------------------ first layer (1 input channel)
// dW[tap][co] += sum_p dz[p][co] * x[p + tap].
__global__ __launch_bounds__(256) void wgrad_c1_kernel(const float* __restrict__ dz, const float* __restrict__ x32,
                                                       const double* __restrict__ spec64,
                                                       const double* __restrict__ denom, int B, int H, int W, int Cout,
                                                       float* __restrict__ dw, int dz16) {
  // a workgroup walks image rows (b, gy) and a row's pixels 256 / lanes at a time: 32-bit index arithmetic, one division per ROW (the first
  // form divided a 64-bit pixel index three times per pixel: 441 us for 1.06 GB); dz16: dz is the bfloat16 copy the BatchNorm backward wrote
  const int lanes = Cout / 4, rows = 256 / lanes;
  const int cq = threadIdx.x % lanes, prow = threadIdx.x / lanes;
  float acc[9][4];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[t][k] = 0.f;
  const int nrows = B * H;
  for (int r = blockIdx.x; r < nrows; r += gridDim.x)
  for (int gx = prow; gx < W + rows - 1 - (W + rows - 1) % rows; gx += rows) {      // every lane runs every trip: the shuffles below need whole pixel groups
    const int b = r / H, gy = r % H;
    const bool live = gx < W;
    const size_t p = (size_t)r * W + (live ? gx : 0);
    f32x4 g = mfpa_ld_act4(dz, p * Cout + 4 * cq, dz16);
    if (!live) g = f32x4{0.f, 0.f, 0.f, 0.f};
    const double den = (spec64 && denom) ? denom[b] : 1.0;
    if (lanes >= 9) {
      // the lanes of a pixel share its 3x3 input window: lane cq < 9 loads (and normalises: one float64 division) tap cq,
      // the others receive it by shuffle -- like conv3x3_c1_kernel
      float mine = 0.f;
      if (cq < 9) {
        const int yy = gy + cq / 3 - 1, xx = gx + cq % 3 - 1;
        if (yy >= 0 && yy < H && xx >= 0 && xx < W) {
          const size_t o = ((size_t)b * H + yy) * W + xx;
          mine = spec64 ? (float)(spec64[o] / den) : x32[o];
        }
      }
      const int base = (threadIdx.x & 63) - cq;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float v = __shfl(mine, base + t);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[t][k] += g[k] * v;
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
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[t][k] += g[k] * v;
      }
    }
  }
  __shared__ float sh[256 * 36];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int k = 0; k < 4; ++k) sh[threadIdx.x * 36 + t * 4 + k] = acc[t][k];
  __syncthreads();
  if (prow == 0) {
    for (int r = 1; r < rows; ++r)
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[t][k] += sh[(r * lanes + cq) * 36 + t * 4 + k];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int k = 0; k < 4; ++k) atomicAdd(dw + (size_t)t * Cout + 4 * cq + k, acc[t][k]);
  }
}

typedef void (*wgrad_kernel_t)(WgradArgs);

}  // namespace

// patch groups (grid.z) of a launch: about `target` workgroups over `tiles` (co, ci) tiles, at most one group per patch
static unsigned wg_patch_split(int target, int tiles, long long npatch) {
  long long split = (target + tiles - 1) / tiles;
  if (split > npatch) split = npatch;
  if (split < 1) split = 1;
  if (split > 65535) split = 65535;
  return (unsigned)split;
}

extern "C" {

int mfpa_wgrad_mfma(const mfpa_wgrad_desc* d, void* stream) {
  if (!d) return MFPA_EINVAL;
  if (d->B == 0) return MFPA_OK;
  if (!d->dz || !d->x0 || !d->dw || d->B < 0 || d->H < 1 || d->W < 1) return MFPA_EINVAL;
  if (d->C0 < 64 || d->C0 % 64 || d->C1 < 0 || d->C1 % 64 || d->Cout < 64 || d->Cout % 64) return MFPA_EINVAL;
  if (d->mode != 0 && d->mode != 1) return MFPA_EINVAL;
  if (d->C1 > 0 && (d->mode != 0 || !d->x1 || d->H1 < 1 || d->W1 < 1 || d->H1 > d->H || d->W1 > d->W)) return MFPA_EINVAL;
  if ((d->in_scale0 == nullptr) != (d->in_shift0 == nullptr)) return MFPA_EINVAL;
  if (d->drop_thresh && !d->in_scale0) return MFPA_EINVAL;
  if (d->precision < 0 || d->precision > 3) return MFPA_EINVAL;
  if (d->precision == 3 && (d->in_scale0 || d->drop_thresh)) return MFPA_EINVAL;      // bf16 operands are already activated
  WgradArgs a{};
  a.dz = d->dz; a.x0 = d->x0; a.in_scale0 = d->in_scale0; a.in_shift0 = d->in_shift0;
  a.x1 = d->C1 ? d->x1 : nullptr; a.dw = d->dw;
  a.C0 = d->C0; a.C1 = d->C1; a.H1 = d->C1 ? d->H1 : 0; a.W1 = d->C1 ? d->W1 : 0;
  a.oy1 = d->C1 ? (d->H - d->H1) / 2 : 0;
  a.ox1 = d->C1 ? (d->W - d->W1) / 2 : 0;
  a.B = d->B; a.H = d->H; a.W = d->W; a.Cout = d->Cout;
  a.drop_seed = d->drop_seed; a.drop_thresh = d->drop_thresh; a.drop_scale = d->drop_scale;
  const int mode = d->mode, cin = d->C0 + d->C1;
  const int pw = d->precision == 0 || d->W > 16 ? 32 : 16;            // patch width and height: 2 x 32 (fp32 MFMA), 4 x 32 or 8 x 16
  const int ph = d->precision == 0 ? WG_PH : WGB_PIX / pw;
  a.tiles_x = (d->W + pw - 1) / pw;
  a.tiles_y = (d->H + ph - 1) / ph;
  const long long npatch = (long long)a.B * a.tiles_x * a.tiles_y;
  const int halo_px = (ph + 2) * (pw + 2);                             // a 3x3 layer's x tile
  hipStream_t s = mfpa_stream(stream);
  if (d->precision == 0) {
    static const wgrad_kernel_t kernel[2] = {wgrad_mfma_kernel<0>, wgrad_mfma_kernel<1>};
    const dim3 grid(d->Cout / WG_T, cin / WG_T, wg_patch_split(2048, (d->Cout / WG_T) * (cin / WG_T), npatch));   // ~2048 workgroups in flight in total
    const size_t lds = sizeof(float) * WG_T * (WG_PIX + (mode == 0 ? halo_px : WG_PIX));
    hipLaunchKernelGGL(kernel[mode], grid, dim3(256), lds, s, a);
  } else {
    // transposing LDS reads need every lane live (512-thread workgroups, no early exits) -- guaranteed by the kernel shape
    a.xcd = 1;
    if (d->precision < 3) {
      static const wgrad_kernel_t kernel[2][2][2] = {      // [mode][PW 32][PLAIN]
          {{wgrad_bf16x3_kernel<0, 16, false>, wgrad_bf16x3_kernel<0, 16, true>}, {wgrad_bf16x3_kernel<0, 32, false>, wgrad_bf16x3_kernel<0, 32, true>}},
          {{wgrad_bf16x3_kernel<1, 16, false>, wgrad_bf16x3_kernel<1, 16, true>}, {wgrad_bf16x3_kernel<1, 32, false>, wgrad_bf16x3_kernel<1, 32, true>}}};
      const bool plain = d->precision == 2;
      const dim3 grid(d->Cout / WG_T, cin / WG_T, wg_patch_split(1024, (d->Cout / WG_T) * (cin / WG_T), npatch));   // ~4 workgroup rounds over the launch
      const size_t lds = (size_t)(plain ? 192 : WGB_ROW) * (WGB_PIX + (mode == 0 ? halo_px : WGB_PIX));
      hipLaunchKernelGGL(kernel[mode][pw == 32][plain], grid, dim3(WGB_THREADS), lds, s, a);
    } else if (mode == 0) {
      // wgrad_bf16_kernel: 128-channel output tiles when C_out allows; as few patch groups as give every CU one workgroup (the atomics
      // are per workgroup: 256 / 512 / 1024 workgroups measured 291 / 333 / 385 us on 512 -> 512 @ 32 x 31, 64 clips)
      static const wgrad_kernel_t kernel[2][2] = {         // [PW 32][COT 4]
          {wgrad_bf16_kernel<16, 2>, wgrad_bf16_kernel<16, 4>}, {wgrad_bf16_kernel<32, 2>, wgrad_bf16_kernel<32, 4>}};
      const int cot = d->Cout % 128 == 0 ? 4 : 2;
      const int cus = mfpa_current_device_cus();
      const dim3 grid(d->Cout / (32 * cot), cin / WG_T, wg_patch_split(cus > 0 ? cus : 256, (d->Cout / (32 * cot)) * (cin / WG_T), npatch));
      const size_t lds = 2 * ((size_t)WGB_PIX * (64 * cot + 64) + (size_t)(halo_px + 4) * 192);
      hipLaunchKernelGGL(kernel[pw == 32][cot == 4], grid, dim3(WGB_THREADS), lds, s, a);
    } else {
      // 64 output x 128 input channels per workgroup when C_in allows (halves the re-reads of the four dz tap tiles)
      static const wgrad_kernel_t kernel[2][2] = {         // [PW 32][CI128]
          {wgrad_bf16x3_kernel<1, 16, true, true, false>, wgrad_bf16x3_kernel<1, 16, true, true, true>},
          {wgrad_bf16x3_kernel<1, 32, true, true, false>, wgrad_bf16x3_kernel<1, 32, true, true, true>}};
      const int ciw = d->C0 % 128 == 0 ? 128 : WG_T;
      const dim3 grid(d->Cout / WG_T, cin / ciw, wg_patch_split(1024, (d->Cout / WG_T) * (cin / ciw), npatch));
      const size_t lds = (size_t)192 * 4 * WGB_PIX + (size_t)(ciw == 128 ? 320 : 192) * WGB_PIX;
      hipLaunchKernelGGL(kernel[pw == 32][ciw == 128], grid, dim3(WGB_THREADS), lds, s, a);
    }
  }
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_wgrad_c1(const float* dz, const float* x32, const double* spec64, const double* denom, int B, int H, int W,
                  int Cout, float* dw, int dz_is_bf16, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!dz || (!x32 && !spec64) || !dw || B < 0 || H < 1 || W < 1) return MFPA_EINVAL;
  if (Cout % 4 || Cout < 4 || Cout > 1024 || (256 % (Cout / 4)) != 0) return MFPA_EINVAL;
  if ((long long)B * H > 0x7fffffffLL) return MFPA_EINVAL;
  const int nrows = B * H;
  hipLaunchKernelGGL(wgrad_c1_kernel, dim3(nrows < 2048 ? nrows : 2048), dim3(256), 0, mfpa_stream(stream), dz, x32,
                     spec64, denom, B, H, W, Cout, dw, dz_is_bf16);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
