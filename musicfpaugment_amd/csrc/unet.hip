// UNet denoiser kernels for MI355X (gfx950), training/unet.py:8-108 of the reference.
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
#include <cstring>

#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include "mfpa_unet_args.h"

namespace {

using namespace mfpa_tile;     // vector types, pin_reads / pin_read_slots, each_index

// PREC 1 weight image ("w3", built by ops_unet.split_bf16x3 / mfpa_pack_conv_weights): [tap][chunk][row][128 B], one row =
// the 32 channels of a chunk as 8 slots of 16 B, logical slots 0-3 = 32 bf16 hi, 4-7 = 32 bf16 lo, stored at PHYSICAL slot
// (logical ^ ((row >> 1) & 7)).  A (tap, chunk, 128-row) tile is 16 KB contiguous and is copied verbatim into LDS by LDS-DMA
// in the pipelined kernels (the XOR keeps a wave's ds_read_b128 fragment reads of 128-byte rows bank-conflict-free); the other
// kernels undo the XOR while they stage a tile through registers into their padded rows.
__device__ __forceinline__ int w3_swz(int row) { return (row >> 1) & 7; }

constexpr int KC = 32;        // channels per K chunk
constexpr int LDK = KC + 4;   // padded LDS row (floats): 144 B -> conflict-free b128 fragment reads

// does this instantiation run the software-pipelined main loop (the bf16x3 3x3 convolution on 8 waves: one workgroup per CU, two
// halo stages)?
constexpr bool conv_is_pipe(int WM, int WN, int MODE, int PREC) { return MODE == 0 && PREC == 1 && WM * WN == 8; }

using mfpa_unet::ConvArgs;     // csrc/mfpa_unet_args.h (shared with csrc/unet_ws.hip)

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
  constexpr int THREADS = 64 * WM * WN;
  constexpr int HALO = (MODE == 0) ? 1 : 0;
  constexpr int TAPS = (MODE == 0) ? 9 : 4;
  constexpr int HPW = PW + 2 * HALO, HPH = PH + 2 * HALO;
  constexpr int HP = HPW * HPH;                       // halo-tile pixels
  constexpr int BM = PH * PW;
  constexpr int MT = 2;                               // 32-pixel MFMA tiles per wave
  constexpr int WPX = 32 * MT;                        // pixels per wave
  static_assert(BM == WPX * WM, "workgroup tile is 32*MT*WM pixels");
  constexpr int NT = BN / (32 * WN);                  // 32-wide n tiles per wave
  constexpr int A_F4 = (HP * (KC / 4) + THREADS - 1) / THREADS;
  constexpr int B_F4 = (BN * (KC / 4) + THREADS - 1) / THREADS;
  constexpr bool B_EXACT = (BN * (KC / 4)) % THREADS == 0;

  // PIPE (the bf16x3 3x3 convolution on the 8-wave shapes, one workgroup per CU): software-pipelined main loop with the halo
  // tile double-buffered in LDS, see step_pipe below.  The 4-wave shapes keep the plain loop: with 256 threads the staging
  // registers are twice as many per thread and the second fragment set spills (measured: 2x slower).
  constexpr bool PIPE = conv_is_pipe(WM, WN, MODE, PREC);
  constexpr int A_STAGES = PIPE ? 2 : 1;
  // PIPE: a halo stage has a row for every staging slot (A_F4 * THREADS / 8 >= HP), so the split / store pass needs no tail
  // predicate: every halo load is consumed on every path and hipcc keeps no "maybe pending" state across iterations
  constexpr int HPS = PIPE ? ((HP * (KC / 4) + THREADS - 1) / THREADS) * (THREADS / (KC / 4)) : HP;

  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* As = reinterpret_cast<float*>(smem);         // [A_STAGES][HPS][LDK]
  constexpr int B_STAGE = BN * LDK;                   // weight-tile stages: [2][BN][LDK] padded rows, written through registers
  float* Bs0 = As + A_STAGES * HPS * LDK;
  constexpr int SW = PW + 4, SH = PH + 4;             // C1SRC: spectrogram patch with a 2-pixel halo, then the (9, 64) weights
  float* Sp = Bs0 + 2 * B_STAGE;                      // [SH][SW]
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
        if (!C1SRC && affine && inside) {      // padding stays exactly zero
          v = v * a_sc + a_sh;
          v.x = v.x > 0.f ? v.x : 0.f;
          v.y = v.y > 0.f ? v.y : 0.f;
          v.z = v.z > 0.f ? v.z : 0.f;
          v.w = v.w > 0.f ? v.w : 0.f;
          if (a.drop_thresh) {
            const unsigned long long e0 = (((unsigned long long)b * a.H + gy) * a.W + gx) * a.C0 + c0 + 4 * q;
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
          }
        }
        if (PREC == 0) {
          *reinterpret_cast<f32x4*>(As + pix * LDK + 4 * q) = v;
        } else {
          bf16x4 hi, lo;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            hi[k] = (__bf16)v[k];
            lo[k] = (__bf16)(v[k] - (float)hi[k]);
          }
          char* row = reinterpret_cast<char*>(As + pix * LDK);
          *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
          *reinterpret_cast<bf16x4*>(row + 64 + 8 * q) = lo;
        }
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
  auto load_b = [&](int it_flat, auto SET) __attribute__((always_inline)) {
    constexpr int set = decltype(SET)::value;
    const int chunk = it_flat / TAPS, tap = it_flat % TAPS;
    // PREC 0: [tap][Cout][Cin] floats; PREC 1: the chunk-major swizzled image (header of this file)
    const char* wbase = reinterpret_cast<const char*>((PREC == 0) ? a.w + ((size_t)tap * a.Cout + n0) * Cin + chunk * KC
                                                                 : a.w + (((size_t)tap * nchunks + chunk) * a.Cout + n0) * KC);
#pragma unroll
    for (int it = 0; it < B_F4; ++it)
      if (B_EXACT || tid + it * THREADS < BN * (KC / 4)) breg[set][it] = *reinterpret_cast<const f32x4*>(wbase + b_off[it]);
  };
  auto load_b_at = [&](int chunk, int tap, auto SET) __attribute__((always_inline)) {     // load_b with (chunk, tap) given: no division
    constexpr int set = decltype(SET)::value;
    const char* wbase = reinterpret_cast<const char*>((PREC == 0) ? a.w + ((size_t)tap * a.Cout + n0) * Cin + chunk * KC
                                                                 : a.w + (((size_t)tap * nchunks + chunk) * a.Cout + n0) * KC);
#pragma unroll
    for (int it = 0; it < B_F4; ++it)
      if (B_EXACT || tid + it * THREADS < BN * (KC / 4)) breg[set][it] = *reinterpret_cast<const f32x4*>(wbase + b_off[it]);
  };
  auto load_b_ct = [&](int chunk, int tap, auto SET) __attribute__((always_inline)) {     // PREC 1 image, (chunk, tap) given
    constexpr int set = decltype(SET)::value;
    const char* wbase = reinterpret_cast<const char*>(a.w + (((size_t)tap * nchunks + chunk) * a.Cout + n0) * KC);
#pragma unroll
    for (int it = 0; it < B_F4; ++it) breg[set][it] = *reinterpret_cast<const f32x4*>(wbase + b_off[it]);
  };
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
        // term-major order: consecutive matrix instructions write different accumulators (dependent distance MT*NT)
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
    if (it + 1 < nit) store_b(CUR, Bs0 + ((it + 1) & 1) * (BN * LDK));
    if (it + 2 < nit) load_b(it + 2, std::integral_constant<int, 1 - cur>{});
    if (it + 1 < nit) load_a((it + 1) / TAPS, (it + 1) % TAPS);
    compute(0, Bs0 + (it & 1) * (BN * LDK));
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
    if (tap + 1 < TAPS || more) store_b(std::integral_constant<int, par>{}, Bs0 + (par ^ 1) * (BN * LDK));
    if (tap + 2 < TAPS) load_b_at(chunk, tap + 2, std::integral_constant<int, 1 - par>{});
    else if (more) load_b_at(chunk + 1, tap + 2 - TAPS, std::integral_constant<int, 1 - par>{});
    if (tap == 0 && more) load_a(chunk + 1, 0);
    compute(tap_off, Bs0 + par * (BN * LDK));
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
  auto mfma_lo = [&](const Frags& f) __attribute__((always_inline)) {      // the two correction terms: MT*NT*2 MFMAs
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.al[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bl[nt], acc[mt][nt], 0, 0, 0);
  };
  auto mfma_hi = [&](const Frags& f) __attribute__((always_inline)) {      // the main term: MT*NT MFMAs
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.ah[mt], f.bh[nt], acc[mt][nt], 0, 0, 0);
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
    mfma_lo(fr0);
    mfma_hi(fr0);
    store_b(std::integral_constant<int, (tap + 1) % 3>{}, Bsn);
    constexpr int t3 = (tap + 3) % TAPS;
    const int c3 = (tap + 3 >= TAPS) ? chunk_n : chunk;
    load_b_ct(c3, t3, std::integral_constant<int, tap % 3>{});
    pin_phase(std::true_type{});
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    // ---- phase B: (tap 0: issue the loads of the next chunk's halo)  read frags(it+1, s=0) -> F0 || MFMA(F1)
    //      (tap 2: split that halo into the OTHER halo stage)
    if (tap == 0) load_a(chunk_n, 0);
    read_frags(fr0, Asn, Bsn, ntap_off, 0);          // past the end: a harmless read of valid LDS
    mfma_lo(fr1);
    mfma_hi(fr1);
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
    for (int i = tid; i < 9 * 64; i += THREADS) W1s[i] = a.c1_w[i];
    __syncthreads();
  }
  load_a(0, 0);
  if constexpr (PIPE) {
    using Set2 = std::integral_constant<int, 2>;
    load_b_ct(0, 0, Set0{});
    store_a(0, As);
    store_b(Set0{}, Bs0);
    load_b_ct(0, 1, Set1{});                           // tiles 1 and 2: sets 1 and 2 (tile it lives in set it % 3)
    load_b_ct(0, 2, Set2{});
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
        const int m = wm * WPX + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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
            const int col = (r & 3) + 8 * (r >> 2) + 4 * lh;
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
            const int q = (r & 3) + 8 * (r >> 2) + 4 * lh;       // pixel in the 2x16 tile, row 0
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
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x111, 0xf, 0xf, false));      // row_shr:1
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x112, 0xf, 0xf, false));      // row_shr:2
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x114, 0xf, 0xf, false));      // row_shr:4
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x118, 0xf, 0xf, false));      // row_shr:8: lane 15 of a row = its total
        p += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(p), 0x142, 0xa, 0xf, false));      // row_bcast:15 into rows 1 and 3
        const int m = wm * WPX + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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
__global__ __launch_bounds__(256, 2) void convT_mfma_kernel(ConvArgs a) {
  static_assert(!PLAIN || (IO16 && PREC == 1), "the plain-bf16 form belongs to the training step's bf16-I/O instantiation");
  // IO16 (the plain-bf16 training step with its activations kept as bfloat16): the source and / or the output are bfloat16 tensors -- its
  // own instantiation, the inference kernels carry none of it
  constexpr int BM = PH * PW, BN = 64, NT = 2;
  static_assert(BM == 128, "four waves of 32 pixels");
  constexpr int A_F4 = BM * (KC / 4) / 256;            // 4
  constexpr int B_F4 = 4 * BN * (KC / 4) / 256;        // 8
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
      const int pix = (tid + it * 256) / (KC / 4);
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
      const int row = (tid + it * 256) / (KC / 4);     // tap * 64 + n
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
      const int pix = (tid + it * 256) / (KC / 4);
      f32x4 v = areg[it];
      if (affine) {
        v = v * sc + sh;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
        if (a.drop_thresh) {
          const int gy = y0 + pix / PW, gx = x0p + pix % PW;
          const unsigned long long e0 = (((unsigned long long)b * a.H + gy) * a.W + gx) * a.C0 + c0 + 4 * q;
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
        }
      }
      if (PREC == 0) {
        *reinterpret_cast<f32x4*>(As + pix * LDK + 4 * q) = v;
      } else {
        bf16x4 hi, lo;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          hi[k] = (__bf16)v[k];
          lo[k] = (__bf16)(v[k] - (float)hi[k]);
        }
        char* row = reinterpret_cast<char*>(As + pix * LDK);
        *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
        if constexpr (!PLAIN) *reinterpret_cast<bf16x4*>(row + 64 + 8 * q) = lo;
        if (a.x0_bf16 != nullptr && blockIdx.y == 0) {                 // training forward: the activated input's bf16 copy (its weight gradient's operand)
          const int gy = y0 + pix / PW, gx = x0p + pix % PW;
          if (gy < a.H && gx < a.W)
            *reinterpret_cast<bf16x4*>(a.x0_bf16 + (((size_t)b * a.H + gy) * a.W + gx) * (size_t)a.C0 + c0 + 4 * q) = hi;
        }
      }
    }
#pragma unroll
    for (int it = 0; it < B_F4; ++it) {
      const int row = (tid + it * 256) / (KC / 4);
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
    if constexpr (PLAIN) {
      // round 6, the plain-bf16 training step (mfpa_conv_desc.precision 2): one bf16 MFMA per product on the hi halves, like its 3x3 convolutions
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 ah = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(As + a_off) + 32 * s);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(reinterpret_cast<const char*>(Bs + (t * BN + nt * 32) * LDK + b_off) + 32 * s);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t][nt], 0, 0, 0);
          }
      }
    } else if constexpr (PREC == 1) {
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
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc[t][nt], 0, 0, 0);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc[t][nt], 0, 0, 0);
            acc[t][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc[t][nt], 0, 0, 0);
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
      const int m = wave * 32 + (rp & 3) + 8 * (rp >> 2) + 4 * lh + odd;
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
    const int m = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
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

template <int PH, int PW, int PREC, bool IO16 = false, bool PLAIN = false>
int launch_convT(ConvArgs& a, hipStream_t s) {
  const size_t lds = sizeof(float) * ((size_t)PH * PW * LDK + 4 * (size_t)64 * LDK);
  dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.B), (unsigned)(a.Cout / 64));
  hipLaunchKernelGGL((convT_mfma_kernel<PH, PW, PREC, IO16, PLAIN>), grid, dim3(256), lds, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

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

template <int BN, int PH, int PW, int WM, int WN, int MODE, int PREC, bool C1SRC = false>
int launch_conv(ConvArgs& a, hipStream_t s) {
  constexpr int HALO = (MODE == 0) ? 1 : 0;
  constexpr int HP = (PW + 2 * HALO) * (PH + 2 * HALO);
  constexpr bool PIPE = conv_is_pipe(WM, WN, MODE, PREC);           // the kernel's PIPE: two padded halo stages
  constexpr int THREADS = 64 * WM * WN;
  constexpr int HPS = PIPE ? ((HP * (KC / 4) + THREADS - 1) / THREADS) * (THREADS / (KC / 4)) : HP;
  const size_t lds = sizeof(float) * ((size_t)(PIPE ? 2 : 1) * HPS * LDK + 2 * (size_t)BN * LDK + (C1SRC ? (PH + 4) * (PW + 4) + 9 * 64 : 0));
  dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.B), (unsigned)(a.Cout / BN));
  hipLaunchKernelGGL((conv_mfma_kernel<BN, PH, PW, WM, WN, MODE, PREC, C1SRC>), grid, dim3(64 * WM * WN), lds, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
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
template <int BN, int PH, int PW, int MODE, int PREC, bool C1SRC = false> constexpr ConvKernel k_mfma() {
  return {{MFPA_CONV_MFMA, PH, PW, BN, 0, MODE, PREC, C1SRC}, launch_conv<BN, PH, PW, PH * PW / 64, BN / 64, MODE, PREC, C1SRC>}; }
template <int PH, int PW, int PREC, bool IO16 = false, bool PLAIN = false> constexpr ConvKernel k_convT() {
  return {{MFPA_CONV_CONVT, PH, PW, 64, 0, 1, PREC, 0, 0, 0, PLAIN, 0, 0, IO16}, launch_convT<PH, PW, PREC, IO16, PLAIN>}; }
const ConvKernel CONV_KERNELS[] = {
    k_ws64<false>(), k_ws64<true>(),
    MFPA_WD16_FORMS(MFPA_K_WD16)         // the 29 of csrc/unet_wd16.hip, from the list its explicit instantiations are made of (csrc/mfpa_unet_args.h)
    k_mfma<64, 8, 32, 0, 0>(), k_mfma<128, 8, 32, 0, 0>(), k_mfma<128, 4, 32, 0, 0>(), k_mfma<64, 4, 32, 0, 0>(), k_mfma<128, 8, 16, 0, 0>(), k_mfma<64, 8, 16, 0, 0>(),     // <BN, PH, PW, MODE, PREC, C1SRC>
    k_mfma<64, 8, 32, 0, 1>(), k_mfma<128, 8, 32, 0, 1>(), k_mfma<128, 4, 32, 0, 1>(), k_mfma<64, 4, 32, 0, 1>(), k_mfma<128, 8, 16, 0, 1>(), k_mfma<64, 8, 16, 0, 1>(),
    k_mfma<64, 8, 32, 2, 0>(), k_mfma<128, 8, 32, 2, 0>(), k_mfma<128, 4, 32, 2, 0>(), k_mfma<64, 4, 32, 2, 0>(), k_mfma<128, 8, 16, 2, 0>(), k_mfma<64, 8, 16, 2, 0>(),
    k_mfma<64, 8, 32, 2, 1>(), k_mfma<128, 8, 32, 2, 1>(), k_mfma<128, 4, 32, 2, 1>(), k_mfma<64, 4, 32, 2, 1>(), k_mfma<128, 8, 16, 2, 1>(), k_mfma<64, 8, 16, 2, 1>(),
    k_mfma<128, 16, 16, 0, 1>(), k_mfma<64, 8, 32, 0, 0, true>(), k_mfma<64, 8, 32, 0, 1, true>(),
    k_convT<4, 32, 0>(), k_convT<4, 32, 1>(), k_convT<4, 32, 1, true>(), k_convT<4, 32, 1, true, true>(),     // <PH, PW, PREC, IO16, PLAIN>
    k_convT<8, 16, 0>(), k_convT<8, 16, 1>(), k_convT<8, 16, 1, true>(), k_convT<8, 16, 1, true, true>()};

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
