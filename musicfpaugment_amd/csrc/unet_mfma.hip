// The row-image kernels of the UNet convolution family for MI355X (gfx950), training/unet.py:8-108 of the reference: conv_mfma_kernel (the
// fp32 chain's 3x3 convolution, the C1SRC fallback, the transposed convolution's input gradient) and convT_mfma_kernel (the training step's
// transposed convolution), one LDS geometry each, and their launchers.  conv_route and CONV_KERNELS (csrc/unet.hip) reach the instantiations
// through launch_conv / launch_convT (csrc/mfpa_unet_args.h, MFPA_MFMA_FORMS / MFPA_CONVT_FORMS: each template argument list is written
// there, once).
//
// Activations are NHWC float32 (H = frequency bins, W = frames).  The 3x3 convolutions and the
// 2x2 transposed convolutions are implicit GEMMs on the matrix cores with float32-input MFMA
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate -- the reference is fp32):
//
//   M = output pixels of a PHxPW patch (128 per workgroup), N = output channels (64/128 per
//   workgroup), K = taps x input channels, walked in chunks of 32 channels.
//
// LDS im2col staging: per 32-channel chunk the workgroup stages the patch PLUS its one-pixel
// halo once ((PH+2)x(PW+2) pixels x 32 channels) and all nine taps read their shifted A
// fragments out of that tile, so the input is fetched 1.4-1.6x instead of 9x.  Both operands
// sit in LDS K-contiguous with rows padded to 36 floats: a lane's fragment for four consecutive
// MFMA k-steps is one conflict-free ds_read_b128.  Zero padding of the convolution, ragged
// patch edges and the decoder's pad+concat (Up.forward, unet.py:56-63) are all folded into
// the halo loader; the folded BatchNorm affine + ReLU run in the epilogue on the accumulators.
// Global loads of the next tap's weights (and next chunk's halo) are issued before the MFMA
// block of the current tap and written to LDS after it, so they overlap the matrix work.
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include "mfpa_unet_args.h"

namespace {

using namespace mfpa_tile;     // vector types, KC, dpp_row_add, pin_reads / pin_read_slots, each_index
using mfpa_unet::ConvArgs;

// PREC 1 weight image ("w3", built by ops_unet.split_bf16x3 / mfpa_pack_conv_weights): [tap][chunk][row][128 B], one row =
// the 32 channels of a chunk as 8 slots of 16 B, logical slots 0-3 = 32 bf16 hi, 4-7 = 32 bf16 lo, stored at PHYSICAL slot
// (logical ^ ((row >> 1) & 7)).  A (tap, chunk, 128-row) tile is 16 KB contiguous and is copied verbatim into LDS by LDS-DMA
// in the pipelined kernels (the XOR keeps a wave's ds_read_b128 fragment reads of 128-byte rows bank-conflict-free); the other
// kernels undo the XOR while they stage a tile through registers into their padded rows.
__device__ __forceinline__ int w3_swz(int row) { return (row >> 1) & 7; }

constexpr int LDK = KC + 4;   // padded LDS row (floats): 144 B -> conflict-free b128 fragment reads

// The 32 x 32 MFMA accumulator layout: register r of lane (li = column, lh = lane >> 5) holds row (r & 3) + 8 (r >> 2) + 4 lh of the tile
// that begins at row `base`.  One sum, associated from the left as the kernels always wrote it.
__device__ __forceinline__ constexpr int acc_row(int base, int r, int lh) { return base + (r & 3) + 8 * (r >> 2) + 4 * lh; }

// One staging slot on its way into LDS: the four channels c0 + 4 q .. + 3 of pixel (b, gy, gx) through the on-load affine + ReLU and the dropout
// keep (`affine`), then into row `pix` of the stage `As` -- as floats (PREC 0) or split into bf16 hi | lo (PREC 1; PLAIN: the hi half alone).
// Returns hi.  Values, not references to the caller's arrays, and the addresses formed at the stores (NOTES.md on split_store / put_split).
template <int PREC, bool PLAIN>
__device__ __forceinline__ bf16x4 stage_quad(const ConvArgs& a, f32x4 v, bool affine, f32x4 sc, f32x4 sh, int b, int gy, int gx, int c0, float* As, int pix, int q) {
  if (affine) {
    v = v * sc + sh;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
    if (a.drop_thresh) {
      const unsigned long long e0 = (((unsigned long long)b * a.H + gy) * a.W + gx) * a.C0 + c0 + 4 * q;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
    }
  }
  bf16x4 hi = {};
  if constexpr (PREC == 0) {
    *reinterpret_cast<f32x4*>(As + pix * LDK + 4 * q) = v;
  } else {
    bf16x4 lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hi[k] = (__bf16)v[k];
      lo[k] = (__bf16)(v[k] - (float)hi[k]);
    }
    char* row = reinterpret_cast<char*>(As + pix * LDK);
    *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
    if constexpr (!PLAIN) *reinterpret_cast<bf16x4*>(row + 64 + 8 * q) = lo;
  }
  return hi;
}

// does this instantiation run the software-pipelined main loop (the bf16x3 3x3 convolution on 8 waves: one workgroup per CU, two
// halo stages)?
constexpr bool conv_is_pipe(int WM, int WN, int MODE, int PREC) { return MODE == 0 && PREC == 1 && WM * WN == 8; }

// ---- conv_mfma_kernel's tile and LDS geometry, said once for the kernel and its launcher.  Dynamic LDS of a workgroup, in this order:
//   the halo stages [A_STAGES][HPS][LDK], the weight-tile stages [2][BN][LDK], and with C1SRC the spectrogram patch [SH][SW] and the first
//   layer's weights [9][64]
template <int BN, int PH, int PW, int MODE, int PREC, bool C1SRC>
struct MfmaGeo {
  static constexpr int WM = PH * PW / 64, WN = BN / 64, THREADS = 64 * WM * WN;      // WM x WN waves of 64 pixels x 64 channels
  static constexpr int HALO = (MODE == 0) ? 1 : 0, TAPS = (MODE == 0) ? 9 : 4;
  static constexpr int HPW = PW + 2 * HALO, HPH = PH + 2 * HALO, HP = HPW * HPH, BM = PH * PW;      // HP: halo-tile pixels
  static constexpr int A_F4 = (HP * (KC / 4) + THREADS - 1) / THREADS, B_F4 = (BN * (KC / 4) + THREADS - 1) / THREADS;   // staging slots (16 B) per thread
  static constexpr bool B_EXACT = (BN * (KC / 4)) % THREADS == 0;
  // PIPE (the bf16x3 3x3 convolution on the 8-wave shapes, one workgroup per CU): software-pipelined main loop with the halo
  // tile double-buffered in LDS, see tap_body in the kernel.  The 4-wave shapes keep the plain loop: with 256 threads the staging
  // registers are twice as many per thread and the second fragment set spills (measured: 2x slower).
  static constexpr bool PIPE = conv_is_pipe(WM, WN, MODE, PREC);
  static constexpr int A_STAGES = PIPE ? 2 : 1;
  // PIPE: a halo stage has a row for every staging slot (A_F4 * THREADS / 8 >= HP), so the split / store pass needs no tail
  // predicate: every halo load is consumed on every path and hipcc keeps no "maybe pending" state across iterations
  static constexpr int HPS = PIPE ? A_F4 * (THREADS / (KC / 4)) : HP;
  static constexpr int B_STAGE = BN * LDK;                             // a weight-tile stage: [BN][LDK] padded rows, written through registers
  static constexpr int SW = PW + 4, SH = PH + 4, C1W = 9 * 64;         // C1SRC: spectrogram patch with a 2-pixel halo, then the (9, 64) weights
  static constexpr int lds_bytes = (int)sizeof(float) * (A_STAGES * HPS * LDK + 2 * B_STAGE + (C1SRC ? SH * SW + C1W : 0));
};
// the bytes every launch has always asked for, by (BN, patch, MODE, PIPE, C1SRC); PREC moves them only through PIPE
template <int BN, int PH, int PW, int MODE, int PREC, bool C1SRC = false> constexpr int mfma_lds = MfmaGeo<BN, PH, PW, MODE, PREC, C1SRC>::lds_bytes;
static_assert(mfma_lds<64, 8, 32, 0, 0> == 67392 && mfma_lds<64, 8, 32, 0, 1> == 67392 && mfma_lds<64, 8, 32, 0, 0, true> == 71424 && mfma_lds<64, 8, 32, 0, 1, true> == 71424);
static_assert(mfma_lds<128, 8, 32, 0, 0> == 85824 && mfma_lds<128, 8, 32, 0, 1> == 147456 && mfma_lds<128, 16, 16, 0, 1> == 147456, "the two pipelined forms");
static_assert(mfma_lds<128, 4, 32, 0, 0> == 66240 && mfma_lds<128, 4, 32, 0, 1> == 66240 && mfma_lds<64, 4, 32, 0, 0> == 47808 && mfma_lds<64, 4, 32, 0, 1> == 47808);
static_assert(mfma_lds<128, 8, 16, 0, 0> == 62784 && mfma_lds<128, 8, 16, 0, 1> == 62784 && mfma_lds<64, 8, 16, 0, 0> == 44352 && mfma_lds<64, 8, 16, 0, 1> == 44352);
static_assert(mfma_lds<128, 8, 32, 2, 0> == 73728 && mfma_lds<128, 8, 32, 2, 1> == 73728 && mfma_lds<64, 8, 32, 2, 0> == 55296 && mfma_lds<64, 8, 32, 2, 1> == 55296, "MODE 2: no halo");
static_assert(mfma_lds<128, 4, 32, 2, 0> == 55296 && mfma_lds<128, 4, 32, 2, 1> == 55296 && mfma_lds<128, 8, 16, 2, 0> == 55296 && mfma_lds<128, 8, 16, 2, 1> == 55296);
static_assert(mfma_lds<64, 4, 32, 2, 0> == 36864 && mfma_lds<64, 4, 32, 2, 1> == 36864 && mfma_lds<64, 8, 16, 2, 0> == 36864 && mfma_lds<64, 8, 16, 2, 1> == 36864);

// ---- convT_mfma_kernel's: the staged input chunk [BM][LDK], then the four taps' weight tiles [4][BN][LDK]; 256 threads
template <int PH, int PW>
struct ConvTGeo {
  static constexpr int THREADS = 256, BM = PH * PW, BN = 64;
  static constexpr int A_F4 = BM * (KC / 4) / THREADS;                 // 4
  static constexpr int B_F4 = 4 * BN * (KC / 4) / THREADS;             // 8
  static constexpr int lds_bytes = (int)sizeof(float) * (BM * LDK + 4 * BN * LDK);
};
static_assert(ConvTGeo<4, 32>::lds_bytes == 55296 && ConvTGeo<8, 16>::lds_bytes == 55296, "both patches");

// MODE 0: 3x3 conv, pad 1 (9 taps, halo 1).
// MODE 2: transposed-conv input gradient: 4 taps, A gathered from the (2H,2W) tensor at (2y+dy, 2x+dx).
// (The transposed convolution's forward has its own kernel, convT_mfma_kernel.)
// PREC 0: v_mfma_f32_32x32x2_f32 (exact fp32 products).
// PREC 1: "bf16x3" -- every fp32 operand is split x = hi + lo into two bf16 values and the product is
//         hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_bf16 (fp32 accumulate): 3 matrix instructions at 16x
//         the fp32-MFMA rate, relative error ~2^-17 per product (UNet output: relative L1 ~2e-5, tolerance 1e-4).
//         An LDS row is [32 hi bf16 | 32 lo bf16 | pad] = the same 144 bytes as 32 floats + pad; the weights are
//         pre-split into that row format on the host, activations are split while they are staged.
// WM x WN waves, each 64 pixels x (BN/WN) channels: the workgroup tile is (64*WM pixels) x BN channels.
//
// Pipeline per (chunk, tap) iteration `it`, with the weight tile double-buffered in LDS and two register sets:
//     write B(it+1) registers -> Bs[(it+1)&1]   (loaded from L2/HBM during iteration it-1)
//     issue global loads of B(it+2) -> the other register set; at tap 0 also of the NEXT chunk's halo tile
//     MFMA block of iteration it from As / Bs[it&1]
//     one barrier                                 (+ barrier, halo store, at a chunk's last tap)
// so weight loads have two MFMA blocks to land, and the only exposed cost per iteration is the wave skew.
template <int BN, int PH, int PW, int WM, int WN, int MODE, int PREC, bool C1SRC = false>
__global__ __launch_bounds__(64 * WM * WN, WM * WN == 8 ? 1 : 2) void conv_mfma_kernel(ConvArgs a) {
  static_assert(MODE == 0 || MODE == 2, "3x3 convolution or the transposed convolution's input gradient");
  using G = MfmaGeo<BN, PH, PW, MODE, PREC, C1SRC>;   // the tile and LDS geometry (above)
  static_assert(WM == G::WM && WN == G::WN, "the wave grid is derived from the tile");
  constexpr int THREADS = G::THREADS, HALO = G::HALO, TAPS = G::TAPS, HPW = G::HPW, HP = G::HP, BM = G::BM;
  constexpr int MT = 2;                               // 32-pixel MFMA tiles per wave
  constexpr int WPX = 32 * MT;                        // pixels per wave
  static_assert(BM == WPX * WM, "workgroup tile is 32*MT*WM pixels");
  constexpr int NT = BN / (32 * WN);                  // 32-wide n tiles per wave
  constexpr int A_F4 = G::A_F4, B_F4 = G::B_F4, A_STAGES = G::A_STAGES, HPS = G::HPS, B_STAGE = G::B_STAGE, SW = G::SW, SH = G::SH;
  constexpr bool B_EXACT = G::B_EXACT, PIPE = G::PIPE;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);         // [A_STAGES][HPS][LDK]
  float* Bs0 = As + A_STAGES * HPS * LDK;             // [2][BN][LDK]
  float* Sp = Bs0 + 2 * B_STAGE;                      // C1SRC: [SH][SW]
  float* W1s = Sp + SH * SW;                          // [9][64]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WM, wn = wave / WM;
  const int li = lane & 31, lh = lane >> 5;

  int bx = blockIdx.x;
  const int tx = bx % a.tiles_x; bx /= a.tiles_x;
  const int ty = bx % a.tiles_y; bx /= a.tiles_y;
  const int b = bx;
  const int n0 = blockIdx.y * BN;
  const int y0 = ty * PH, x0p = tx * PW;
  const int Cin = a.C0 + a.C1;
  const int nchunks = Cin / KC;
  const int nit = nchunks * TAPS;

  f32x4 areg[A_F4];
  f32x4 breg[3][B_F4];   // register sets for the weight tile (the pipelined loop uses three), always indexed with compile-time constants

  // The halo pixel of each of a thread's A_F4 staging slots never changes (idx = tid + it * THREADS -> pixel idx / 8, channel quad
  // idx % 8): its image coordinates are computed ONCE, packed (gy << 16 | gx), -1 = outside the image or past the tile.  The
  // per-chunk loader then needs two integer multiply-adds per load instead of the divisions / 64-bit index chains (~40
  // instructions per load, the largest block of vector work in the 64-channel layers).
  static_assert(THREADS % (KC / 4) == 0, "a thread keeps one channel quad for all of its halo pixels");
  const int aq = tid % (KC / 4);
  // packed as: bit 31 = outside the image (or past the tile), bits 30..16 / 15..0 = row / column CLAMPED into the image -- a slot
  // outside still loads (unconditionally, see load_a), from its nearest image pixel: a line its neighbours fetch anyway (every
  // outside slot reading ONE fixed address made that line a hot spot: +4-8 % on the 8-wave fp32 kernel)
  int apix[A_F4];
#pragma unroll
  for (int it = 0; it < A_F4; ++it) {
    const int pix = tid / (KC / 4) + it * (THREADS / (KC / 4));
    const int gy = y0 + pix / HPW - HALO, gx = x0p + pix % HPW - HALO;
    const bool in = pix < HP && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
    const int cy = min(max(gy, 0), a.H - 1), cx = min(max(gx, 0), a.W - 1);
    apix[it] = (in ? 0 : (int)0x80000000) | (cy << 16) | cx;
  }
  // 32-bit byte offsets from per-clip scalar bases (the host checks that one clip's input image fits 2 GB)
  const char* xb0 = reinterpret_cast<const char*>(a.x0) + (size_t)b * (MODE == 2 ? 4 : 1) * a.H * a.W * a.C0 * sizeof(float);
  const char* xb1 = reinterpret_cast<const char*>(a.x1) + (size_t)b * a.H1 * a.W1 * a.C1 * sizeof(float);
  // load_a only ISSUES the global loads of a halo tile (nothing in it reads a loaded value, so no wait lands between the
  // loads); the on-load affine + ReLU + dropout and the bf16 split happen in store_a, a whole chunk later.  Every slot loads
  // UNCONDITIONALLY -- a pixel outside the image reads its nearest image pixel and store_a zeroes it: no exec-mask branches, and
  // a wave issues exactly A_F4 loads per tile, which the pipelined loop's counted vmcnt waits rely on.
  auto src1_inside = [&](int p) __attribute__((always_inline)) {          // inside the (smaller, zero-padded) second source?
    const int y1 = ((p >> 16) & 0x7fff) - a.oy1, x1 = (p & 0xffff) - a.ox1;
    return p >= 0 && y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1;
  };
  auto load_a = [&](int chunk, int tap) __attribute__((always_inline)) {
    if (C1SRC) return;                                 // the tile is computed from the LDS-resident spectrogram patch in store_a
    const int c0 = chunk * KC;
    const bool from0 = c0 < a.C0;
#pragma unroll
    for (int it = 0; it < A_F4; ++it) {
      const int gy = (apix[it] >> 16) & 0x7fff, gx = apix[it] & 0xffff;           // clamped into the image
      // PIPE: every slot loads, so that a wave issues exactly A_F4 loads per tile and hipcc's vmcnt bookkeeping stays exact; the
      // plain loop skips slots outside the image (measured: unconditional loads cost its fp32 8-wave form 4-8 %)
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (from0) {
        unsigned off;
        if (MODE == 2) off = ((unsigned)((2 * gy + (tap >> 1)) * (2 * a.W) + 2 * gx + (tap & 1)) * (unsigned)a.C0 + (unsigned)(c0 + 4 * aq)) * 4u;
        else off = ((unsigned)(gy * a.W + gx) * (unsigned)a.C0 + (unsigned)(c0 + 4 * aq)) * 4u;
        if (PIPE || apix[it] >= 0) v = *reinterpret_cast<const f32x4*>(xb0 + off);
      } else {
        const int y1 = min(max(gy - a.oy1, 0), a.H1 - 1), x1 = min(max(gx - a.ox1, 0), a.W1 - 1);
        const unsigned off = ((unsigned)(y1 * a.W1 + x1) * (unsigned)a.C1 + (unsigned)(c0 - a.C0 + 4 * aq)) * 4u;
        if (PIPE || src1_inside(apix[it])) v = *reinterpret_cast<const f32x4*>(xb1 + off);
      }
      areg[it] = v;
    }
  };
  auto store_a = [&](int chunk, float* As) __attribute__((always_inline)) {      // `As`: the halo stage to fill
    const int c0 = chunk * KC;
    const bool affine = a.in_scale0 != nullptr && c0 < a.C0;
    f32x4 a_sc = {1.f, 1.f, 1.f, 1.f}, a_sh = {0.f, 0.f, 0.f, 0.f};
    if (affine) {
      a_sc = *reinterpret_cast<const f32x4*>(a.in_scale0 + c0 + 4 * aq);
      a_sh = *reinterpret_cast<const f32x4*>(a.in_shift0 + c0 + 4 * aq);
    }
    // C1SRC: a thread keeps ONE channel quad for all of its halo pixels, so the first layer's nine weight quads and its folded
    // BatchNorm are read once per chunk, not once per staging slot (99 -> 9 LDS reads per chunk and thread)
    f32x4 c1w[C1SRC ? 9 : 1], c1s = {1.f, 1.f, 1.f, 1.f}, c1h = {0.f, 0.f, 0.f, 0.f};
    if constexpr (C1SRC) {
#pragma unroll
      for (int t = 0; t < 9; ++t) c1w[t] = *reinterpret_cast<const f32x4*>(W1s + t * 64 + c0 + 4 * aq);
      c1s = *reinterpret_cast<const f32x4*>(a.c1_scale + c0 + 4 * aq);
      c1h = *reinterpret_cast<const f32x4*>(a.c1_shift + c0 + 4 * aq);
    }
#pragma unroll
    for (int it = 0; it < A_F4; ++it) {
      const int pix = tid / (KC / 4) + it * (THREADS / (KC / 4)), q = aq;
      if (PIPE || pix < HP) {
        const bool inside = apix[it] >= 0;
        f32x4 v = areg[it];
        if (!C1SRC && !(c0 < a.C0 ? inside : src1_inside(apix[it]))) v = f32x4{0.f, 0.f, 0.f, 0.f};      // zero padding
        const int gy = (apix[it] >> 16) & 0x7fff, gx = apix[it] & 0xffff;
        if (C1SRC) {
          v = f32x4{0.f, 0.f, 0.f, 0.f};
          if (inside) {                                                    // conv2's zero padding stays exactly zero
            const float* sp = Sp + (pix / HPW) * SW + (pix % HPW);        // 3x3 window of the first layer around (gy, gx)
            // Packed FMAs on a sample broadcast out of the LOW half of a pair (mfpa_bcast2): written as `v += sv * wv` hipcc keeps two
            // samples in one register pair and selects the odd one with v_pk_fma_f32 ... op_sel:[1,0,0], the operand-selection form
            // the library does not ship (mfpa_common.h; tests/test_isa_scan.py).  One v_mov per sample; scalar FMAs in its place made
            // this kernel 18 % slower (7.0 instead of 5.8 vector instructions per MFMA).
            f32x2 v01 = {0.f, 0.f}, v23 = {0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 9; ++t) {
              const float sv = sp[(t / 3) * SW + (t % 3)];
              const f32x2 xx = mfpa_bcast2(sv);
              const f32x4 wv = c1w[t];
              v01 += xx * f32x2{wv.x, wv.y};
              v23 += xx * f32x2{wv.z, wv.w};
            }
            v = f32x4{v01[0], v01[1], v23[0], v23[1]};
            v = v * c1s + c1h;
            v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
          }
        }
        stage_quad<PREC, false>(a, v, !C1SRC && affine && inside, a_sc, a_sh, b, gy, gx, c0, As, pix, q);      // (padding stays exactly zero)
      }
    }
  };
  // a thread's (row, quad) inside a weight tile never changes: 32-bit byte offsets computed once, added to a scalar tile base
  unsigned b_off[B_F4];
#pragma unroll
  for (int it = 0; it < B_F4; ++it) {
    const int idx = tid + it * THREADS;
    const int n = idx / (KC / 4), q = idx % (KC / 4);
    b_off[it] = (PREC == 0) ? (unsigned)(n * Cin + 4 * q) * 4u : (unsigned)(n * KC + 4 * (q ^ w3_swz(n))) * 4u;
  }
  auto load_b_at = [&](int chunk, int tap, auto SET) __attribute__((always_inline)) {     // the weight tile of (chunk, tap) into register set SET
    constexpr int set = decltype(SET)::value;
    // PREC 0: [tap][Cout][Cin] floats; PREC 1: the chunk-major swizzled image (w3_swz above)
    const char* wbase = reinterpret_cast<const char*>((PREC == 0) ? a.w + ((size_t)tap * a.Cout + n0) * Cin + chunk * KC
                                                                 : a.w + (((size_t)tap * nchunks + chunk) * a.Cout + n0) * KC);
#pragma unroll
    for (int it = 0; it < B_F4; ++it)
      if (B_EXACT || tid + it * THREADS < BN * (KC / 4)) breg[set][it] = *reinterpret_cast<const f32x4*>(wbase + b_off[it]);
  };
  auto load_b = [&](int it_flat, auto SET) __attribute__((always_inline)) { load_b_at(it_flat / TAPS, it_flat % TAPS, SET); };
  auto store_b = [&](auto SET, float* Bs) __attribute__((always_inline)) {
    constexpr int set = decltype(SET)::value;
#pragma unroll
    for (int it = 0; it < B_F4; ++it) {
      const int idx = tid + it * THREADS;
      if (B_EXACT || idx < BN * (KC / 4)) {
        const int n = idx / (KC / 4), q = idx % (KC / 4);
        *reinterpret_cast<f32x4*>(Bs + n * LDK + 4 * q) = breg[set][it];
      }
    }
  };

  floatx16 acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.f;

  int a_base[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    const int m = wm * WPX + mt * 32 + li;
    a_base[mt] = ((m / PW) * HPW + (m % PW)) * LDK + 4 * lh;
  }
  int b_base[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) b_base[nt] = (wn * (NT * 32) + nt * 32 + li) * LDK + 4 * lh;

  // round 6: the plain-bf16 training step (mfpa_conv_desc.precision 2) runs the transposed convolution's INPUT GRADIENT (MODE 2) with one
  // bf16 MFMA per product too -- the hi halves of the same staged operands; wave-uniform
  const bool plain_hi = MODE == 2 && PREC == 1 && a.plain != 0;
  // the bf16x3 products of a wave's MT x NT tiles, term-major (lo.hi over all tiles, then hi.lo, then hi.hi): consecutive matrix instructions
  // write different accumulators (dependent distance MT*NT).  The plain loop and the pipelined one both call it.
  auto mfma_terms = [&](const bf16x8 (&ah)[MT], const bf16x8 (&al)[MT], const bf16x8 (&bh)[NT], const bf16x8 (&bl)[NT]) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[mt], bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bl[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
  };
  auto compute = [&](int tap_off, const float* Bs) __attribute__((always_inline)) {       // tap_off: LDS offset (floats) of the tap's shifted A fragments
    if (PREC == 1) {
      if (MODE == 2 && plain_hi) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          bf16x8 ah[MT], bh[NT];
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) ah[mt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(As + a_base[mt] + tap_off) + 32 * s);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) bh[nt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Bs + b_base[nt]) + 32 * s);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[mt], bh[nt], acc[mt][nt], 0, 0, 0);
        }
        return;
      }
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        bf16x8 ah[MT], al[MT], bh[NT], bl[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
          const char* r = reinterpret_cast<const char*>(As + a_base[mt] + tap_off) + 32 * s;
          ah[mt] = *reinterpret_cast<const bf16x8*>(r);
          al[mt] = *reinterpret_cast<const bf16x8*>(r + 64);
        }
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const char* r = reinterpret_cast<const char*>(Bs + b_base[nt]) + 32 * s;
          bh[nt] = *reinterpret_cast<const bf16x8*>(r);
          bl[nt] = *reinterpret_cast<const bf16x8*>(r + 64);
        }
        mfma_terms(ah, al, bh, bl);
      }
    } else {
#pragma unroll
      for (int s = 0; s < KC / 8; ++s) {
        f32x4 af[MT], bf[NT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *reinterpret_cast<const f32x4*>(As + a_base[mt] + tap_off + 8 * s);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bf[nt] = *reinterpret_cast<const f32x4*>(Bs + b_base[nt] + 8 * s);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt].x, bf[nt].x, acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt].y, bf[nt].y, acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt].z, bf[nt].z, acc[mt][nt], 0, 0, 0);
            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt].w, bf[nt].w, acc[mt][nt], 0, 0, 0);
          }
      }
    }
  };

  using Set0 = std::integral_constant<int, 0>;
  using Set1 = std::integral_constant<int, 1>;
  // one pipeline iteration of MODE 2, whose A tile changes with the tap; register set CUR holds B(it+1), the other set receives B(it+2)
  auto step = [&](int it, auto CUR) __attribute__((always_inline)) {
    constexpr int cur = decltype(CUR)::value;
    if (it + 1 < nit) store_b(CUR, Bs0 + ((it + 1) & 1) * B_STAGE);
    if (it + 2 < nit) load_b(it + 2, std::integral_constant<int, 1 - cur>{});
    if (it + 1 < nit) load_a((it + 1) / TAPS, (it + 1) % TAPS);
    compute(0, Bs0 + (it & 1) * B_STAGE);
    if (it + 1 < nit) {
      __syncthreads();            // every wave is done reading As
      store_a((it + 1) / TAPS, As);
    }
    __syncthreads();
  };

  // The same iteration with the tap (and the parity of `it`, i.e. the weight register set and LDS stage) as compile-time constants:
  // the 3x3 convolution's plain loop then runs a chunk as nine straight-line taps -- no it / 9 and it % 9, no runtime tap offset
  // added to every fragment address (PMC on the 64-channel layers: 3.8 scalar and 4.8 vector instructions per MFMA with the
  // runtime form, their K is only 18 .. 36 iterations long)
  auto step_s = [&](auto TAP_, auto PAR_, int chunk) __attribute__((always_inline)) {
    constexpr int tap = decltype(TAP_)::value, par = decltype(PAR_)::value;
    constexpr int tap_off = ((tap / 3) * HPW + (tap % 3)) * LDK;
    const bool more = chunk + 1 < nchunks;                               // a chunk follows this one
    if (tap + 1 < TAPS || more) store_b(std::integral_constant<int, par>{}, Bs0 + (par ^ 1) * B_STAGE);
    if (tap + 2 < TAPS) load_b_at(chunk, tap + 2, std::integral_constant<int, 1 - par>{});
    else if (more) load_b_at(chunk + 1, tap + 2 - TAPS, std::integral_constant<int, 1 - par>{});
    if (tap == 0 && more) load_a(chunk + 1, 0);
    compute(tap_off, Bs0 + par * B_STAGE);
    if (tap == TAPS - 1 && more) {
      __syncthreads();
      store_a(chunk + 1, As);
    }
    __syncthreads();
  };
  auto chunk_s = [&](auto PAR0_, int chunk) __attribute__((always_inline)) {      // nine taps; PAR0 = parity of the chunk's first iteration
    constexpr int p0 = decltype(PAR0_)::value;
    step_s(std::integral_constant<int, 0>{}, std::integral_constant<int, p0>{}, chunk);
    step_s(std::integral_constant<int, 1>{}, std::integral_constant<int, p0 ^ 1>{}, chunk);
    step_s(std::integral_constant<int, 2>{}, std::integral_constant<int, p0>{}, chunk);
    step_s(std::integral_constant<int, 3>{}, std::integral_constant<int, p0 ^ 1>{}, chunk);
    step_s(std::integral_constant<int, 4>{}, std::integral_constant<int, p0>{}, chunk);
    step_s(std::integral_constant<int, 5>{}, std::integral_constant<int, p0 ^ 1>{}, chunk);
    step_s(std::integral_constant<int, 6>{}, std::integral_constant<int, p0>{}, chunk);
    step_s(std::integral_constant<int, 7>{}, std::integral_constant<int, p0 ^ 1>{}, chunk);
    step_s(std::integral_constant<int, 8>{}, std::integral_constant<int, p0>{}, chunk);
  };

  // ---- PIPE: the software-pipelined main loop of the bf16x3 3x3 convolution -------------------------------------------------
  // One (chunk, tap) iteration = two k-substeps of 16 channels, 12 MFMAs each.  The fragments of a substep (8 ds_read_b128 per
  // wave) are read one substep AHEAD into a second register set while the matrix pipe works on the current one, so no MFMA waits
  // on an LDS read it has just issued.  The iteration's one barrier sits BETWEEN its two substeps:
  //     phase A: read frags(it, s=1) -> F1  ||  MFMA(F0); behind the reads: request weight tile it+3, Bs[(it+1) & 1] <- tile it+1
  //     barrier  (tile it+1 visible; every fragment read of tile it has completed: its stage is rewritten in the next phase A)
  //     phase B: (tap 0: issue the loads of the next chunk's halo)  read frags(it+1, s=0) -> F0  ||  MFMA(F1)
  //              (tap 2: split that halo into the OTHER halo stage)
  // Each phase is one basic block whose MFMA : LDS : VMEM interleave is pinned with sched_group_barrier.
  struct Frags { bf16x8 ah[MT], al[MT], bh[NT], bl[NT]; };
  Frags fr0, fr1;
  auto read_frags = [&](Frags& f, const float* Asb, const float* Bsb, int tap_off, int sub) __attribute__((always_inline)) {
    // in the order the MFMAs consume them: (al, bh) terms first, then (ah, bl), then (ah, bh)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      f.al[mt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Asb + a_base[mt] + tap_off) + 32 * sub + 64);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      f.bh[nt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Bsb + b_base[nt]) + 32 * sub);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
      f.ah[mt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Asb + a_base[mt] + tap_off) + 32 * sub);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
      f.bl[nt] = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Bsb + b_base[nt]) + 32 * sub + 64);
  };
  constexpr int N_FR = 2 * (MT + NT), N_MFMA = 3 * MT * NT;     // fragment reads / MFMAs of one phase
  static_assert(N_MFMA >= 3, "a phase needs an MFMA in front of the weight-tile loads and one in front of its LDS stores");
  // the pinned interleave of a phase: the fragment reads spread evenly behind the first MFMAs; (phase A) the loads of the weight
  // tile three iterations ahead behind the next MFMA, the LDS stores of the next tile behind the one after; the remaining MFMAs last
  auto pin_phase = [&](auto WITH_B) __attribute__((always_inline)) {
    constexpr bool with_b = decltype(WITH_B)::value;
    constexpr int slots = with_b ? N_MFMA - 2 : N_MFMA;
    pin_reads<slots, N_FR>();
    constexpr int used = pin_read_slots(slots, N_FR) + (with_b ? 2 : 0);
    if constexpr (with_b) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x020, B_F4, 0);      // the loads of tile it+3 first: they touch no register of the stores
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, B_F4, 0);
    }
    if constexpr (N_MFMA - used > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_MFMA - used, 0);
  };
  // One tap of the pipelined loop; TAP is a compile-time constant (the chunk loop calls it nine times), so every tap-dependent
  // choice -- LDS offsets of the shifted fragments, which of the three weight register sets is stored / refilled, where the halo
  // of the next chunk is loaded and split -- is static, a chunk is straight-line code, and hipcc's own s_waitcnt bookkeeping is
  // EXACT: the LDS stores of tile it+1 wait with vmcnt(B_F4 [+ A_F4]) and leave the loads of tile it+2 in flight.  (With a
  // runtime tap the conditional halo loads made it merge paths and wait vmcnt(0), i.e. also for the tile requested one
  // iteration ago: every iteration stalled on an L2 round trip; skipping just those loads returned 11-13 % on the deep layers.
  // Hiding the loads from hipcc instead -- an inline-asm register ring, and an LDS-DMA ring -- measured 7-15 % SLOWER.)
  static_assert(!PIPE || (B_EXACT && TAPS == 9), "tile it lives in register set it % 3 = tap % 3");
  auto tap_body = [&](auto TAP, int chunk) __attribute__((always_inline)) {
    constexpr int tap = decltype(TAP)::value;
    constexpr int ntap = (tap + 1) % TAPS;
    constexpr int tap_off = ((tap / 3) * HPW + (tap % 3)) * LDK, ntap_off = ((ntap / 3) * HPW + (ntap % 3)) * LDK;
    const int it = chunk * TAPS + tap;
    const int chunk_n = chunk + 1 < nchunks ? chunk + 1 : chunk;             // past the last chunk: the same halo again, into the stage nobody reads
    const float* Asb = As + (chunk & 1) * (HPS * LDK);
    const float* Asn = (tap == TAPS - 1) ? As + ((chunk + 1) & 1) * (HPS * LDK) : Asb;
    const float* Bsb = Bs0 + (it & 1) * B_STAGE;
    float* Bsn = Bs0 + ((it + 1) & 1) * B_STAGE;
    // ---- phase A: read frags(it, s=1) -> F1 || MFMA(F0); Bs[(it+1) & 1] <- tile it+1 (set (tap+1) % 3, requested two iterations
    //      ago; that stage's tile it-1 was last read before the previous barrier); request tile it+3 into set tap % 3
    read_frags(fr1, Asb, Bsb, tap_off, 1);
    mfma_terms(fr0.ah, fr0.al, fr0.bh, fr0.bl);
    store_b(std::integral_constant<int, (tap + 1) % 3>{}, Bsn);
    constexpr int t3 = (tap + 3) % TAPS;
    const int c3 = (tap + 3 >= TAPS) ? chunk_n : chunk;
    load_b_at(c3, t3, std::integral_constant<int, tap % 3>{});
    pin_phase(std::true_type{});
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    // ---- phase B: (tap 0: issue the loads of the next chunk's halo)  read frags(it+1, s=0) -> F0 || MFMA(F1)
    //      (tap 2: split that halo into the OTHER halo stage)
    if (tap == 0) load_a(chunk_n, 0);
    read_frags(fr0, Asn, Bsn, ntap_off, 0);          // past the end: a harmless read of valid LDS
    mfma_terms(fr1.ah, fr1.al, fr1.bh, fr1.bl);
    pin_phase(std::false_type{});
    __builtin_amdgcn_sched_barrier(0);
    if (tap == 2) store_a(chunk_n, As + ((chunk + 1) & 1) * (HPS * LDK));
  };

  if (C1SRC) {
    const double den = a.c1_denom ? a.c1_denom[b] : 1.0;
    for (int i = tid; i < SH * SW; i += THREADS) {
      const int gy = y0 - 2 + i / SW, gx = x0p - 2 + i % SW;
      float v = 0.f;                                   // the first layer's own zero padding
      if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
        const size_t o = ((size_t)b * a.H + gy) * a.W + gx;
        v = a.c1_spec64 ? (float)(a.c1_spec64[o] / den) : a.c1_x32[o];
      }
      Sp[i] = v;
    }
    for (int i = tid; i < G::C1W; i += THREADS) W1s[i] = a.c1_w[i];
    __syncthreads();
  }
  load_a(0, 0);
  if constexpr (PIPE) {
    using Set2 = std::integral_constant<int, 2>;
    load_b_at(0, 0, Set0{});
    store_a(0, As);
    store_b(Set0{}, Bs0);
    load_b_at(0, 1, Set1{});                           // tiles 1 and 2: sets 1 and 2 (tile it lives in set it % 3)
    load_b_at(0, 2, Set2{});
    __syncthreads();
    read_frags(fr0, As, Bs0, 0, 0);
    for (int chunk = 0; chunk < nchunks; ++chunk) {
      each_index<TAPS>(tap_body, chunk);
    }
  } else {
    load_b(0, Set0{});
    store_a(0, As);
    store_b(Set0{}, Bs0);
    if (nit > 1) load_b(1, Set0{});
    __syncthreads();
    if constexpr (MODE == 0) {
      // nine is odd: the parity of a chunk's first iteration alternates from chunk to chunk
      int chunk = 0;
      for (; chunk + 1 < nchunks; chunk += 2) {
        chunk_s(Set0{}, chunk);
        chunk_s(Set1{}, chunk + 1);
      }
      if (chunk < nchunks) chunk_s(Set0{}, chunk);
    } else {
      for (int it = 0; it < nit; it += 2) {
        step(it, Set0{});
        if (it + 1 < nit) step(it + 1, Set1{});
      }
    }
  }

  // epilogue: out = relu(acc * scale[n] + shift[n]); D[row = pixel][col = channel]
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + wn * (NT * 32) + nt * 32 + li;
    const float sc = a.scale ? a.scale[n] : 1.f;
    const float sh = a.shift ? a.shift[n] : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float v = acc[mt][nt][r] * sc + sh;
        if (a.relu) v = v > 0.f ? v : 0.f;
        acc[mt][nt][r] = v;
      }
  }
  if (a.y != nullptr) {
    // 32-bit byte offsets from a scalar per-clip base (the host checks that one clip's output fits 4 GB), the pixel offset
    // computed once for all of a lane's channels, and no bounds checks on interior tiles: the first form of this loop (64-bit
    // index arithmetic and an exec-mask branch per element) was up to 13 % of the 64-channel layers
    const unsigned oW = (unsigned)a.yW, oH = (unsigned)a.yH;
    char* yb = reinterpret_cast<char*>(a.y + (size_t)b * oH * oW * a.Cout);
    const unsigned cout = (unsigned)a.Cout;
    const unsigned nb = (unsigned)(n0 + wn * (NT * 32) + li) * 4u;
    const bool interior = (y0 + PH <= a.yH) && (x0p + PW <= a.yW);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = acc_row(wm * WPX + mt * 32, r, lh);
        const int gy = y0 + m / PW, gx = x0p + m % PW;
        if (interior || (gy < a.yH && gx < a.yW)) {
          const unsigned pix = (unsigned)gy * oW + (unsigned)gx;
          char* yp = yb + (pix * cout * 4u + nb);
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
            *reinterpret_cast<float*>(yp + nt * 128) = acc[mt][nt][r];
        }
      }
    }
  }
  if (MODE == 0 && a.y_pool != nullptr) {
    // MaxPool2d(2) (floor): every 2x2 window lives in ONE lane's accumulators (the two rows of a window are the
    // wave's two 32-pixel MFMA tiles for 32-wide patches, registers r / r+8 for 16-wide ones; the two columns are
    // registers r / r+1), so pooling needs no cross-lane traffic.
    const int Ho = a.H / 2, Wo = a.W / 2;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + wn * (NT * 32) + nt * 32 + li;
      if (PW == 32) {
#pragma unroll
        for (int mp = 0; mp < MT; mp += 2)
#pragma unroll
          for (int r = 0; r < 16; r += 2) {
            const int col = acc_row(0, r, lh);
            const int py = (y0 + wm * MT + mp) / 2, px = (x0p + col) / 2;
            if (py < Ho && px < Wo) {
              const float v = fmaxf(fmaxf(acc[mp][nt][r], acc[mp][nt][r + 1]), fmaxf(acc[mp + 1][nt][r], acc[mp + 1][nt][r + 1]));
              a.y_pool[(((size_t)b * Ho + py) * Wo + px) * a.Cout + n] = v;
            }
          }
      } else {
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
          for (int r = 0; r < 8; r += 2) {
            const int q = acc_row(0, r, lh);       // pixel in the 2x16 tile, row 0
            const int py = (y0 + 2 * (wm * MT + mt)) / 2, px = (x0p + (q % 16)) / 2;
            if (py < Ho && px < Wo) {
              const float v = fmaxf(fmaxf(acc[mt][nt][r], acc[mt][nt][r + 1]), fmaxf(acc[mt][nt][r + 8], acc[mt][nt][r + 9]));
              a.y_pool[(((size_t)b * Ho + py) * Wo + px) * a.Cout + n] = v;
            }
          }
      }
    }
  }
  if (MODE == 0 && WN <= 2 && a.w1x1 != nullptr) {
    // OutConv 1x1 to one class: a wave holds BN / WN channels of its pixels, one channel per lane of a 32-lane half.  The channel
    // sum is a DPP reduction (row_shr 1 / 2 / 4 / 8, then row_bcast:15 into the odd rows: five vector adds, no LDS crossbar -- the
    // ds_bpermute butterfly of __shfl_xor cost 126 waits per workgroup here), the totals of lanes 31 / 63 meet in LDS (the staging
    // buffers are free once every wave has left the main loop; with WN == 2 two waves contribute to a pixel) and are written out
    // one pixel per thread, coalesced along the patch rows.
    float wv[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) wv[nt] = a.w1x1[n0 + wn * (NT * 32) + nt * 32 + li];
    float* red = As;                                     // [WN][BM] channel sums
    __syncthreads();
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float p = 0.f;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) p += acc[mt][nt][r] * wv[nt];
        p = dpp_row_add<0x118>(dpp_row_add<0x114>(dpp_row_add<0x112>(dpp_row_add<0x111>(p))));               // row_shr 1, 2, 4, 8: lane 15 of a row = its total
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x142, 0xa, 0xf, false));      // row_bcast:15 into rows 1 and 3
        const int m = wm * WPX + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;     // acc_row, written out: the call moves all 15 MODE 0 forms (NOTES.md)
        if (li == 31) red[wn * BM + m] = p;
      }
    __syncthreads();
    for (int m = tid; m < BM; m += THREADS) {
      const int gy = y0 + m / PW, gx = x0p + m % PW;
      const float p = red[m] + (WN == 2 ? red[BM + m] : 0.f);
      if (gy < a.H && gx < a.W) a.y1x1[((size_t)b * a.H + gy) * a.W + gx] = p + a.b1x1;
    }
  }
}

// ConvTranspose2d(k = 2, s = 2) forward: out[2y+dy, 2x+dx][co] = sum_ci x[y,x][ci] * w[dy,dx][co][ci] + bias[co].
// K = C_in only, so the generic kernel's one-tap-per-workgroup form re-staged the same input tile four times around a
// 4..32-iteration loop.  Here a workgroup keeps FOUR accumulator sets (one per tap) for 128 input pixels x 64 output
// channels: the input chunk is staged once per 32 channels and its fragments are reused by all four taps; a wave owns
// 32 pixels x 64 channels x 4 taps (128 accumulator VGPRs).  Two workgroups per CU overlap each other's staging.
template <int PH, int PW, int PREC, bool IO16 = false, bool PLAIN = false>
__global__ __launch_bounds__((ConvTGeo<PH, PW>::THREADS), 2) void convT_mfma_kernel(ConvArgs a) {
  static_assert(!PLAIN || (IO16 && PREC == 1), "the plain-bf16 form belongs to the training step's bf16-I/O instantiation");
  // IO16 (the plain-bf16 training step with its activations kept as bfloat16): the source and / or the output are bfloat16 tensors -- its
  // own instantiation, the inference kernels carry none of it
  using G = ConvTGeo<PH, PW>;                          // the tile and LDS geometry (above)
  constexpr int THREADS = G::THREADS, BM = G::BM, BN = G::BN, NT = 2, A_F4 = G::A_F4, B_F4 = G::B_F4;
  static_assert(BM == 128, "four waves of 32 pixels");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);          // [128][LDK]
  float* Bs = As + BM * LDK;                           // [4 taps][64][LDK]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int bx = blockIdx.x;
  const int tx = bx % a.tiles_x; bx /= a.tiles_x;
  const int ty = bx % a.tiles_y; bx /= a.tiles_y;
  const int b = bx;
  const int n0 = blockIdx.y * BN;
  const int y0 = ty * PH, x0p = tx * PW;
  const int nchunks = a.C0 / KC;
  const int q = tid % (KC / 4);
  const bool affine = a.in_scale0 != nullptr;
  const bool in16 = IO16 && a.in16 != 0;                               // source kept as bfloat16 (the training step's activations): widened on load
  const char* xb = reinterpret_cast<const char*>(a.x0) + (size_t)b * a.H * a.W * a.C0 * (in16 ? 2 : 4);   // 32-bit offsets from the clip's base

  f32x4 areg[A_F4], breg[B_F4];
  auto load = [&](int chunk) __attribute__((always_inline)) {
    const int c0 = chunk * KC;
#pragma unroll
    for (int it = 0; it < A_F4; ++it) {
      const int pix = (tid + it * THREADS) / (KC / 4);
      const int gy = y0 + pix / PW, gx = x0p + pix % PW;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (gy < a.H && gx < a.W) {
        const unsigned e = (unsigned)(gy * a.W + gx) * (unsigned)a.C0 + (unsigned)(c0 + 4 * q);
        if (in16) {
          const f32x2 r = *reinterpret_cast<const f32x2*>(xb + e * 2u);
          const unsigned u0 = __float_as_uint(r[0]), u1 = __float_as_uint(r[1]);
          v = f32x4{__uint_as_float(u0 << 16), __uint_as_float(u0 & 0xffff0000u), __uint_as_float(u1 << 16), __uint_as_float(u1 & 0xffff0000u)};
        } else v = *reinterpret_cast<const f32x4*>(xb + e * 4u);
      }
      areg[it] = v;
    }
#pragma unroll
    for (int it = 0; it < B_F4; ++it) {
      const int row = (tid + it * THREADS) / (KC / 4);     // tap * 64 + n
      const int tap = row / BN, n = row % BN;
      if (PREC == 0) breg[it] = *reinterpret_cast<const f32x4*>(a.w + ((size_t)tap * a.Cout + n0 + n) * a.C0 + c0 + 4 * q);
      else breg[it] = *reinterpret_cast<const f32x4*>(a.w + (((size_t)tap * nchunks + chunk) * a.Cout + n0 + n) * KC + 4 * (q ^ w3_swz(n)));
    }
  };
  auto store = [&](int chunk) __attribute__((always_inline)) {
    const int c0 = chunk * KC;
    f32x4 sc = {1.f, 1.f, 1.f, 1.f}, sh = {0.f, 0.f, 0.f, 0.f};
    if (affine) {
      sc = *reinterpret_cast<const f32x4*>(a.in_scale0 + c0 + 4 * q);
      sh = *reinterpret_cast<const f32x4*>(a.in_shift0 + c0 + 4 * q);
    }
#pragma unroll
    for (int it = 0; it < A_F4; ++it) {
      const int pix = (tid + it * THREADS) / (KC / 4);
      const int gy = y0 + pix / PW, gx = x0p + pix % PW;
      const bf16x4 hi = stage_quad<PREC, PLAIN>(a, areg[it], affine, sc, sh, b, gy, gx, c0, As, pix, q);
      if (PREC == 1 && a.x0_bf16 != nullptr && blockIdx.y == 0) {      // training forward: the activated input's bf16 copy (its weight gradient's operand)
        if (gy < a.H && gx < a.W)
          *reinterpret_cast<bf16x4*>(a.x0_bf16 + (((size_t)b * a.H + gy) * a.W + gx) * (size_t)a.C0 + c0 + 4 * q) = hi;
      }
    }
#pragma unroll
    for (int it = 0; it < B_F4; ++it) {
      const int row = (tid + it * THREADS) / (KC / 4);
      *reinterpret_cast<f32x4*>(Bs + row * LDK + 4 * q) = breg[it];      // PREC 1: rows are pre-split [32 hi | 32 lo]
    }
  };

  floatx16 acc[4][NT];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][nt][r] = 0.f;

  const int a_off = (wave * 32 + li) * LDK + 4 * lh;
  const int b_off = li * LDK + 4 * lh;

  load(0);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    __syncthreads();                                   // the previous chunk's fragment reads are done
    store(chunk);
    __syncthreads();
    if (chunk + 1 < nchunks) load(chunk + 1);          // lands during the MFMA block
    if constexpr (PREC == 1) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const char* ar = reinterpret_cast<const char*>(As + a_off) + 32 * s;
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(ar);
        const bf16x8 al = *reinterpret_cast<const bf16x8*>(ar + 64);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const char* br = reinterpret_cast<const char*>(Bs + (t * BN + nt * 32) * LDK + b_off) + 32 * s;
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(br);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(br + 64);
            // PLAIN (round 6, the plain-bf16 training step, mfpa_conv_desc.precision 2): one bf16 MFMA per product on the hi halves, like its
            // 3x3 convolutions; the lo fragments are then never read
            if constexpr (PLAIN) acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t][nt], 0, 0, 0);
            else mfma_bf16x3(acc[t][nt], ah, al, bh, bl);
          }
      }
    } else {
#pragma unroll
      for (int s = 0; s < KC / 8; ++s) {
        const f32x4 af = *reinterpret_cast<const f32x4*>(As + a_off + 8 * s);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const f32x4 bf = *reinterpret_cast<const f32x4*>(Bs + (t * BN + nt * 32) * LDK + b_off + 8 * s);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc[t][nt], 0, 0, 0);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc[t][nt], 0, 0, 0);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc[t][nt], 0, 0, 0);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc[t][nt], 0, 0, 0);
          }
      }
    }
  }
  // epilogue: D[row = pixel][col = channel]; tap t writes output pixel (2 gy + (t >> 1), 2 gx + (t & 1)).  32-bit byte offsets from
  // a scalar per-clip base (the host checks that one clip's output fits 4 GB): one offset per pixel, the four taps and the two
  // channel tiles are wave-uniform displacements of it (the first form computed a 64-bit index per stored element: 128 of them
  // against 48 MFMAs per 32-channel chunk, the largest block of vector work in this kernel)
  float sc[NT], sh[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const int n = n0 + nt * 32 + li;
    sc[nt] = a.scale ? a.scale[n] : 1.f;
    sh[nt] = a.shift ? a.shift[n] : 0.f;
  }
  const bool y16 = IO16 && a.y == nullptr;                             // the output as bfloat16 only (a.y_bf16; checked by mfpa_conv_mfma)
  const unsigned esz = y16 ? 2u : 4u;
  char* yb = (y16 ? reinterpret_cast<char*>(a.y_bf16) : reinterpret_cast<char*>(a.y)) + (size_t)b * (2 * a.H) * (2 * a.W) * a.Cout * esz;
  const unsigned cout4 = (unsigned)a.Cout * esz, row4 = 2u * (unsigned)a.W * cout4;
  const unsigned nb = (unsigned)(n0 + li) * esz;
  if (y16) {
    // bfloat16 output: a lane pair (channels 2k, 2k + 1) swaps one value per two accumulator rows (pixels m, m + 1 -- neighbours in the
    // same patch row), so that the even lane stores both channels of pixel m and the odd lane both channels of pixel m + 1 as one 4-byte
    // piece each (2-byte stores per lane made this write-bound kernel 20 % slower than its float32 form)
    const int odd = li & 1;
    const unsigned nb2 = (unsigned)(n0 + (li & ~1)) * 2u;
#pragma unroll
    for (int rp = 0; rp < 16; rp += 2) {
      const int m = acc_row(wave * 32, rp, lh) + odd;
      const int gy = y0 + m / PW, gx = x0p + m % PW;
      const bool live = gy < a.H && gx < a.W;
      char* yp = yb + ((unsigned)(2 * gy) * row4 + (unsigned)(2 * gx) * cout4 + nb2);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float v0 = acc[t][nt][rp] * sc[nt] + sh[nt], v1 = acc[t][nt][rp + 1] * sc[nt] + sh[nt];
          if (a.relu) { v0 = v0 > 0.f ? v0 : 0.f; v1 = v1 > 0.f ? v1 : 0.f; }
          const float send = odd ? v0 : v1;
          const float recv = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(send), 0xB1, 0xF, 0xF, true));   // quad_perm [1, 0, 3, 2]
          bf16x2 h;
          h[0] = (__bf16)(odd ? recv : v0);
          h[1] = (__bf16)(odd ? v1 : recv);
          if (live) *reinterpret_cast<bf16x2*>(yp + ((t >> 1) * row4 + (t & 1) * cout4 + nt * 64u)) = h;
        }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = acc_row(wave * 32, r, lh);
    const int gy = y0 + m / PW, gx = x0p + m % PW;
    if (gy < a.H && gx < a.W) {
      char* yp = yb + ((unsigned)(2 * gy) * row4 + (unsigned)(2 * gx) * cout4 + nb);
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          float v = acc[t][nt][r] * sc[nt] + sh[nt];
          if (a.relu) v = v > 0.f ? v : 0.f;
          *reinterpret_cast<float*>(yp + ((t >> 1) * row4 + (t & 1) * cout4 + nt * 128u)) = v;
        }
    }
  }
}

}  // namespace

namespace mfpa_unet {

template <int BN, int PH, int PW, int MODE, int PREC, bool C1SRC>
int launch_conv(ConvArgs& a, hipStream_t s) {
  using G = MfmaGeo<BN, PH, PW, MODE, PREC, C1SRC>;
  dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.B), (unsigned)(a.Cout / BN));
  hipLaunchKernelGGL((conv_mfma_kernel<BN, PH, PW, G::WM, G::WN, MODE, PREC, C1SRC>), grid, dim3(G::THREADS), G::lds_bytes, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
#define MFPA_MFMA_INSTANTIATE(...) template int launch_conv<__VA_ARGS__>(ConvArgs&, hipStream_t);
MFPA_MFMA_FORMS(MFPA_MFMA_INSTANTIATE)

template <int PH, int PW, int PREC, bool IO16, bool PLAIN>
int launch_convT(ConvArgs& a, hipStream_t s) {
  using G = ConvTGeo<PH, PW>;
  dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.B), (unsigned)(a.Cout / G::BN));
  hipLaunchKernelGGL((convT_mfma_kernel<PH, PW, PREC, IO16, PLAIN>), grid, dim3(G::THREADS), G::lds_bytes, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
#define MFPA_CONVT_INSTANTIATE(...) template int launch_convT<__VA_ARGS__>(ConvArgs&, hipStream_t);
MFPA_CONVT_FORMS(MFPA_CONVT_INSTANTIATE)

}  // namespace mfpa_unet
