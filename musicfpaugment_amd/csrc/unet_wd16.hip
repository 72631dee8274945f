// conv_wd16_kernel: the weights-direct 3x3 convolution of the UNet family on v_mfma_f32_16x16x32_bf16 (mfpa_conv_desc.w_layout 2), its LDS
// geometry, its launcher and the two shape rules that are its own.  conv_route and CONV_KERNELS (csrc/unet.hip) reach the instantiations
// through launch_wd16 (csrc/mfpa_unet_args.h, MFPA_WD16_FORMS: each template argument list is written there, once).
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include "mfpa_unet_args.h"

namespace {

using namespace mfpa_tile;     // vector types, KC, dpp_row_add, pin_reads / pin_read_slots, each_index
using mfpa_unet::ConvArgs;

// ---- The kernel's LDS layout and its persistence rule, said once for the kernel and its launcher.  Dynamic LDS of a workgroup, in this order:
//   two halo stages (STAGE bytes each: eight planes [hi | lo][k-group 0..3] of HPS pixels x 16 B)
//   the slot-offset table [2 sources][A_F4][THREADS] of 32-bit byte offsets
//   the on-load affine [scale C0 | shift C0]                 (with in_scale0: 8 * C0 bytes, a run-time term)
//   the fused OutConv's partial sums [2][256]                (with w1x1: RED floats, a run-time term)
//   the epilogue's constants [scale BN | shift BN | w1x1 64]
constexpr int wd16_bn(int wmw) { return 32 * (8 / wmw); }            // output channels of a workgroup: 8 / WMW waves of 32
// does a workgroup walk tiles blockIdx.x, blockIdx.x + gridDim.x, ... (and the launcher clamp the grid to one workgroup per CU)?
constexpr bool wd16_persist(bool rows, int wmw, bool side, bool plain) { return wmw == 4 || (!rows && !side) || plain; }
template <int PH, int PW, bool IN16>
struct Wd16Lds {
  static constexpr int THREADS = 512;
  static constexpr int SPP = IN16 ? KC / 8 : KC / 4;                   // staging slots (16 B) per pixel and 32-channel chunk
  static constexpr int HPW = PW + 2, HPH = PH + 2, HP = HPW * HPH;     // the halo patch
  static constexpr int A_F4 = (HP * SPP + THREADS - 1) / THREADS;      // staging slots per thread and chunk
  static constexpr int HPS = A_F4 * (THREADS / SPP);                   // staged pixels (>= HP): every staging slot has a row
  static constexpr int PLANE = ((HPS * 16 + 255) / 256) * 256;         // bytes of one (hi|lo, k-group) plane, a multiple of 256
  static constexpr int HLS = 4 * PLANE + 256;                          // hi -> lo distance (planes 2, 3 sit 128 B further: room for that)
  static constexpr int STAGE = 2 * HLS;
  static constexpr int TBL = 2 * A_F4 * THREADS;                       // entries of the offset table
  // The launcher sizes the table for float32 sources (6 slots per thread) whatever the source: with a bf16 source (3 slots) the kernel's table
  // is half of it and 12 KB stay unused behind the epilogue's constants.  Kept, so that every launch asks for the bytes it always has.
  static constexpr int TBL_BYTES = 2 * ((HP * (KC / 4) + THREADS - 1) / THREADS) * THREADS * (int)sizeof(unsigned);
  static constexpr int RED = 2 * 256;                                  // floats of the fused OutConv's partial sums
  static constexpr int epi_floats(int wmw) { return 2 * wd16_bn(wmw) + 64; }
  static constexpr int fixed_bytes(int wmw) { return 2 * STAGE + TBL_BYTES + epi_floats(wmw) * (int)sizeof(float); }
  __host__ __device__ static constexpr int plane_off(int hl, int kg) { return hl * HLS + kg * PLANE + (kg >> 1) * 128; }
  static_assert(TBL * (int)sizeof(unsigned) <= TBL_BYTES, "the kernel's table fits the launcher's");
};
static_assert(Wd16Lds<8, 32, false>::fixed_bytes(2) == 125184 && Wd16Lds<16, 16, false>::fixed_bytes(2) == 125184 &&
              Wd16Lds<8, 32, true>::fixed_bytes(2) == 125184 && Wd16Lds<16, 16, true>::fixed_bytes(2) == 125184, "LDS of the 128-channel tiles");
static_assert(Wd16Lds<8, 32, false>::fixed_bytes(4) == 124672 && Wd16Lds<8, 32, true>::fixed_bytes(4) == 124672, "LDS of the 64-channel tiles");

// ---------------------------------------------------------------------------------------------------------------------------------
// Weights-direct 3x3 convolution on v_mfma_f32_16x16x32_bf16 ("WD16", mfpa_conv_desc.w_layout 2): 8 waves = 2 pixel halves x 4 column
// tiles, a wave owns 128 pixels x 32 channels, the weight operand comes straight from L1 / L2 out of a fragment-ordered image two taps
// ahead through a ring of three register sets (no weight tile in LDS, no weight barrier), the halo tile is double-buffered in LDS with
// ONE barrier per 32-channel chunk, and the next chunk's halo is split one staging slot per tap inside the MFMA phases.  A whole
// 32-channel chunk is ONE k-step of the 16 x 16 x 32 instruction.  The weights-direct loop is clock (power) limited, and the chip holds
// a higher clock on this instruction than on v_mfma_f32_32x32x16_bf16 under the same loop and operand traffic: 11.07-11.10 ms instead
// of 11.93-12.00 ms for the eleven >= 128-channel layers (64 clips), which is what this kernel is built on.
//   roles: A operand = weights (16 output channels x 32 k), B operand = pixels (32 k x 16 pixels), so D[channel][pixel]: a lane holds FOUR
//          CONSECUTIVE CHANNELS of one pixel -- the epilogue stores 16-byte pieces (16 stores per wave instead of 64 scalar ones) and the
//          2 x 2 max-pool needs one DPP swap of adjacent lanes;
//   LDS:   per halo stage eight planes [hi | lo][k-group 0..3] of (pixel x 16 B): a fragment read is 16 consecutive pixels of one plane per
//          k-group -- conflict-free for ds_read_b128's lane groups exactly when the k-group planes are a multiple of 256 B apart; planes 2, 3
//          sit another 128 B further so that the split's 8-byte stores conflict 2-way instead of 4-way.
//   image: [tap][chunk = Cin / 32][Cout / 16][hi | lo][lane 64][16 B], lane (g = l >> 4, c = l & 15) = channel 16 t + c, k 32 chunk + 8 g .. + 7
//          (ops_unet.split_bf16x3_frag(w, 2), mfpa_pack_conv_weights(precision 3)).
// Not bit-identical to the 32 x 32 x 16 kernels (a k-step sums 32 products inside the instruction); same products, fp32 accumulate.

template <int PH, int PW, bool ROWS, int WMW = 2, bool SIDE = false, bool PLAIN = false, bool IN16 = false, bool AFF16 = false>
__global__ __launch_bounds__(512, 1) void conv_wd16_kernel(ConvArgs a) {
  // AFF16 (with IN16 and SIDE): the bfloat16 source 0 carries an on-load affine + ReLU (+ dropout) and the output may leave as bfloat16 only --
  // the training FORWARD with its activations kept as bfloat16; the input-gradient launches (IN16 without it) carry none of that code
  // PLAIN: plain bf16 products -- one MFMA per product on the hi halves only (the lo planes, their fragment reads, the lo weight
  // fragments and two of the three MFMA terms are gone): the training step's "bf16 MFMA" arithmetic (BASELINE config 4), relative
  // error ~2^-9 per product instead of bf16x3's 2^-17.  Never used by the inference chain (its 1e-4 gate needs bf16x3).
  // IN16 (with PLAIN, one source, no on-load affine): source 0 is a bfloat16 tensor -- the bf16 copy of dz the BatchNorm backward writes --
  // so a staging slot is 8 channels, goes into its (hi, k-group) plane as one 16-byte store without any split arithmetic, and the
  // loader moves half the bytes (the fp32 dz is then never written: mfpa_bn_relu_bwd(write_f32 = 0)).
  static_assert(!IN16 || PLAIN, "a bf16 source feeds the plain-bf16 products");
  using G = Wd16Lds<PH, PW, IN16>;                                     // the LDS layout (above)
  constexpr int SPP = G::SPP, HPW = G::HPW, HP = G::HP, A_F4 = G::A_F4, HLS = G::HLS, STAGE = G::STAGE, TBL = G::TBL;
  constexpr int ESZ = IN16 ? 2 : 4;                                    // bytes per source element
  // (PLAIN halves the MFMA work per fragment read to a third: the tap-by-tap loop's 8 ds_read_b128 per 16 MFMAs saturate the CU's LDS
  //  pipe exactly -- the ROWS form, which reads every halo row once per column offset, is the one that suits it at every depth)
  // SIDE: the training step's side outputs (x0_bf16 / x1_bf16 / y_bf16 / stats_part) -- their own instantiations, so that the inference
  // kernels carry none of their code (it cost the 128-channel form 9 registers and 18 spills)
  // WMW = 2: 2 x 4 waves of 128 px x 32 ch (128-channel output tiles); WMW = 4: 4 x 2 waves of 64 px x 32 ch (the 64-channel layers)
  constexpr int THREADS = G::THREADS, BN = wd16_bn(WMW), WPXW = 256 / WMW, TAPS = 9;
  static_assert((WMW == 2 || WMW == 4) && (!ROWS || WMW == 2), "wave grid");
  constexpr int BM = PH * PW;
  static_assert(BM == 256 && (PW == 32 || PW == 16), "two waves of 128 pixels: eight 16-pixel tiles each");
  constexpr int PT = WPXW / 16;                                        // 16-pixel tiles per wave
  static_assert(A_F4 <= TAPS - 3, "one halo staging slot per tap, taps 2 .. 7");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave % WMW, wn = __builtin_amdgcn_readfirstlane(wave / WMW);
  const int p = lane & 15, g = lane >> 4;

  // PERSIST (WMW = 4): a workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ...; the halo of the next tile's first chunk is
  // requested and split under the last chunk of the current one, so a tile's prologue (a global round trip) and most of its epilogue
  // disappear behind the neighbours' MFMAs -- with 2 .. 4 chunks per tile they were a third of a workgroup's life.
  // The plain-bf16 (training) instantiations persist too: their MFMA time is a third, so prologue / epilogue weigh three times more.
  constexpr bool PERSIST = wd16_persist(ROWS, WMW, SIDE, PLAIN);
  const int n0 = blockIdx.y * BN;
  const int Cin = a.C0 + a.C1;
  const int nchunks = Cin / KC;
  const int ntiles = a.tiles_x * a.tiles_y * a.B;

  // ---- halo loader.  A thread's staging slots map to fixed halo pixels (pix = tid / 8 + 64 it).  Their byte offsets RELATIVE TO THE
  // TILE'S ORIGIN do not depend on the tile: one table [source][slot][thread] in LDS, built once per kernel (as registers the 12
  // offsets were spilled to scratch, and a scratch reload in front of a load drains every outstanding weight load); a tile adds its
  // scalar origin offset.  The loads are raw BUFFER loads through a per-clip descriptor (base = the clip, num_records = its bytes):
  // halo pixels above the first / below the last image row fall outside the clip and return zero without any clamping, pixels left /
  // right of the image read a neighbouring row's valid bytes; either way the slot is zeroed when it is split (`ain`: inside flags,
  // recomputed per tile from the slot's (row, column) and the tile's uniform bounds -- a few compares, no table).  Round 3 rebuilt a
  // clamped absolute table per tile (12 x (two divisions, four clamps, an LDS store) per thread): 3.7 k cycles per tile in front of the
  // first tap of every tile of the persistent form (profiles/r04_c64_timeline.txt).
  const int aq = tid % SPP;
  unsigned* const aoffs0 = reinterpret_cast<unsigned*>(smem + 2 * STAGE);
#pragma unroll
  for (int it = 0; it < A_F4; ++it) {
    const int pix = tid / SPP + it * (THREADS / SPP);
    const int py = pix / HPW - 1, px = pix % HPW - 1;
    aoffs0[it * THREADS + tid] = (unsigned)((py * a.W + px) * a.C0 + (KC / SPP) * aq) * (unsigned)ESZ;    // may be "negative": wraps, see above
    aoffs0[(A_F4 + it) * THREADS + tid] = (unsigned)(((py - a.oy1) * a.W1 + (px - a.ox1)) * a.C1 + (KC / SPP) * aq) * (unsigned)ESZ;
  }
  const unsigned clip0 = (unsigned)a.H * (unsigned)a.W * (unsigned)a.C0 * (unsigned)ESZ, clip1 = (unsigned)a.H1 * (unsigned)a.W1 * (unsigned)a.C1 * (unsigned)ESZ;
  struct Tile { int b, y0, x0p; unsigned ain; unsigned t0, t1; };      // t0 / t1: byte offset of the tile's origin pixel in source 0 / 1
  // decode tile t (workgroup-uniform scalars) and its inside flags (ain bit it: slot inside source 0's image; bit 8 + it: source 1)
  auto make_tile = [&](int t) __attribute__((always_inline)) {
    Tile T;
    int bx = __builtin_amdgcn_readfirstlane(t);
    const int tx = bx % a.tiles_x; bx /= a.tiles_x;
    const int ty = bx % a.tiles_y; bx /= a.tiles_y;
    T.b = bx; T.y0 = ty * PH; T.x0p = tx * PW; T.ain = 0;
    T.t0 = (unsigned)((T.y0 * a.W + T.x0p) * a.C0) * (unsigned)ESZ;
    T.t1 = (unsigned)((T.y0 * a.W1 + T.x0p) * a.C1) * (unsigned)ESZ;
#pragma unroll
    for (int it = 0; it < A_F4; ++it) {
      const int pix = tid / SPP + it * (THREADS / SPP);
      const int gy = T.y0 + pix / HPW - 1, gx = T.x0p + pix % HPW - 1;
      const bool in = pix < HP && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const int y1 = gy - a.oy1, x1 = gx - a.ox1;
      const bool in1 = in && y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1;
      T.ain |= (in ? 1u : 0u) << it | (in1 ? 1u : 0u) << (8 + it);
    }
    return T;
  };
  auto clip_rsrc = [&](const float* base, int b, unsigned clip_bytes) __attribute__((always_inline)) {
    const char* pb = reinterpret_cast<const char*>(base) + (size_t)b * clip_bytes;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pb), 0, base != nullptr ? (int)clip_bytes : 0, 0x00020000);
  };
  int tile = blockIdx.x;
  Tile S = make_tile(tile);                                            // the tile whose halo is being requested / split
  int eb = S.b, ey0 = S.y0, ex0p = S.x0p;                              // the tile being computed (epilogue coordinates)
  // training forward: the producer's per-channel (scale, shift) of source 0, copied to LDS once ([scale C0 | shift C0])
  float* aff = reinterpret_cast<float*>(smem + 2 * STAGE + TBL * sizeof(unsigned));
  if (a.in_scale0 != nullptr) {
    for (int i = tid; i < a.C0; i += THREADS) {
      aff[i] = a.in_scale0[i];
      aff[a.C0 + i] = a.in_shift0[i];
    }
    __syncthreads();
  }
  // the epilogue's per-channel constants (output affine of this workgroup's BN channels, the fused OutConv's weights) into LDS, once per
  // kernel: as global loads inside the epilogue they were followed by s_waitcnt vmcnt(0) -- which also waits for every halo and weight
  // load already in flight for the NEXT tile (persistent form) and for the epilogue's own stores of the previous one
  float* const epi = aff + (a.in_scale0 ? 2 * a.C0 : 0) + (a.w1x1 ? G::RED : 0);      // [scale BN | shift BN | w1x1 64]
  for (int i = tid; i < BN; i += THREADS) {
    epi[i] = a.scale ? a.scale[n0 + i] : 1.f;
    epi[BN + i] = a.shift ? a.shift[n0 + i] : 0.f;
  }
  if (a.w1x1 != nullptr && tid < 64) epi[2 * BN + tid] = a.w1x1[tid];
  // (first read in the first epilogue, behind at least one of the main loop's barriers)
  // ROWS: the staging slots are requested in two halves (slots 0..2 in period 0, 3..5 in period 1) that share three registers
  constexpr int AHALF = (A_F4 + 1) / 2, AREGS = ROWS ? AHALF : A_F4;
  f32x4 areg[AREGS];
  auto load_a_range = [&](int chunk, auto FIRST, auto COUNT) __attribute__((always_inline)) {
    constexpr int first = decltype(FIRST)::value, count = decltype(COUNT)::value;
    const int c0 = chunk * KC;
    const bool from0 = c0 < a.C0;                                      // workgroup-uniform: scalar selects, no branch
    const auto rs = clip_rsrc(from0 ? a.x0 : a.x1, S.b, from0 ? clip0 : clip1);
    const unsigned toff = from0 ? S.t0 + (unsigned)c0 * (unsigned)ESZ : S.t1 + (unsigned)(c0 - a.C0) * (unsigned)ESZ;
    const unsigned* ao = aoffs0 + (from0 ? 0 : A_F4 * THREADS) + tid;
#pragma unroll
    for (int it = first; it < first + count && it < A_F4; ++it)
      areg[it % AREGS] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(ao[it * THREADS] + toff), 0, 0));
  };
  auto load_a = [&](int chunk) __attribute__((always_inline)) {
    load_a_range(chunk, std::integral_constant<int, 0>{}, std::integral_constant<int, AREGS>{});
  };
  // tap-by-tap forms: the slot offsets of the chunk requested at the next tap 0 are read from the LDS table one tap EARLIER (tap 8, when
  // the staging registers are dead) into component 0 of the staging registers themselves, so tap 0 issues its six loads without first
  // waiting for six LDS reads (the wait sat in front of tap 0's MFMAs: tap 0 took twice a steady-state tap, profiles/r04_c64_timeline.txt)
  auto preload_offsets = [&](int chunk) __attribute__((always_inline)) {
    const unsigned* ao = aoffs0 + (chunk * KC < a.C0 ? 0 : A_F4 * THREADS) + tid;
#pragma unroll
    for (int it = 0; it < A_F4; ++it) areg[it % AREGS][0] = __uint_as_float(ao[it * THREADS]);
  };
  auto load_a_pre = [&](int chunk) __attribute__((always_inline)) {
    const int c0 = chunk * KC;
    const bool from0 = c0 < a.C0;
    const auto rs = clip_rsrc(from0 ? a.x0 : a.x1, S.b, from0 ? clip0 : clip1);
    const unsigned toff = from0 ? S.t0 + (unsigned)c0 * (unsigned)ESZ : S.t1 + (unsigned)(c0 - a.C0) * (unsigned)ESZ;
#pragma unroll
    for (int it = 0; it < A_F4; ++it)
      areg[it % AREGS] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)(__float_as_uint(areg[it % AREGS][0]) + toff), 0, 0));
  };
  // one staging slot: zero padding, the training forward's on-load affine + ReLU + dropout, bf16 hi / lo split, two 8-byte stores
  // into the (hi, k-group) and (lo, k-group) planes (a thread's channel quad is half of k-group aq >> 1)
  auto split_slot = [&](auto IT, int chunk, char* stage) __attribute__((always_inline)) {
    constexpr int it = decltype(IT)::value;
    const int pix = tid / SPP + it * (THREADS / SPP);
    const int c0 = chunk * KC;
    const bool inside = (S.ain >> ((c0 < a.C0 ? 0 : 8) + it)) & 1u;
    f32x4 v = areg[it % AREGS];
    if (!inside) v = f32x4{0.f, 0.f, 0.f, 0.f};
    if constexpr (IN16) {                                              // eight bf16 channels = the lane's whole (hi, k-group aq) piece
      if (AFF16 && a.in_scale0 != nullptr && c0 < a.C0 && inside) {
        // bf16 z (the training step's activations kept as bfloat16 in HBM): widen, the producer's BatchNorm affine + ReLU (+ dropout) in
        // float32 exactly as the float32 path applies them, round to bf16 once -- the MFMA operand
        float f[8];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned u = __float_as_uint(v[k]);
          f[2 * k] = __uint_as_float(u << 16);
          f[2 * k + 1] = __uint_as_float(u & 0xffff0000u);
        }
        const float* scp = aff + c0 + 8 * aq;
        const float* shp = aff + a.C0 + c0 + 8 * aq;
        const f32x4 sc0 = *reinterpret_cast<const f32x4*>(scp), sc1 = *reinterpret_cast<const f32x4*>(scp + 4);
        const f32x4 sh0 = *reinterpret_cast<const f32x4*>(shp), sh1 = *reinterpret_cast<const f32x4*>(shp + 4);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          const float y = f[k] * (k < 4 ? sc0[k & 3] : sc1[k & 3]) + (k < 4 ? sh0[k & 3] : sh1[k & 3]);
          f[k] = y > 0.f ? y : 0.f;
        }
        if (a.drop_thresh) {
          const int gy = S.y0 + pix / HPW - 1, gx = S.x0p + pix % HPW - 1;   // inside the image here
          const unsigned long long e0 = (((unsigned long long)S.b * a.H + gy) * a.W + gx) * a.C0 + c0 + 8 * aq;
#pragma unroll
          for (int k = 0; k < 8; ++k) f[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? f[k] * a.drop_scale : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          bf16x2 h2;
          h2[0] = (__bf16)f[2 * k];
          h2[1] = (__bf16)f[2 * k + 1];
          v[k] = __builtin_bit_cast(float, h2);
        }
      }
      *reinterpret_cast<f32x4*>(stage + G::plane_off(0, aq) + pix * 16) = v;
      if constexpr (SIDE && AFF16) {                                   // the activated source 0 as the weight gradient reads it (see below)
        const int py = pix / HPW, px = pix % HPW;
        if (a.x0_bf16 != nullptr && c0 < a.C0 && inside && py >= 1 && py <= PH && px >= 1 && px <= PW && blockIdx.y == 0) {
          const size_t e = (size_t)S.b * a.H * a.W * a.C0 + ((aoffs0[it * THREADS + tid] + S.t0) >> 1) + c0;
          *reinterpret_cast<f32x4*>(a.x0_bf16 + e) = v;
        }
      }
      return;
    }
    if (a.in_scale0 != nullptr && c0 < a.C0 && inside) {
      // from the LDS copy: a global load here is followed by s_waitcnt vmcnt(0), which also waits for every weight load in flight
      const f32x4 sc = *reinterpret_cast<const f32x4*>(aff + c0 + 4 * aq);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(aff + a.C0 + c0 + 4 * aq);
      v = v * sc + sh;
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
      if (a.drop_thresh) {
        const int gy = S.y0 + pix / HPW - 1, gx = S.x0p + pix % HPW - 1;   // inside the image here
        const unsigned long long e0 = (((unsigned long long)S.b * a.H + gy) * a.W + gx) * a.C0 + c0 + 4 * aq;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = mfpa_keep(a.drop_seed, a.drop_thresh, e0 + k) ? v[k] * a.drop_scale : 0.f;
      }
    }
    bf16x4 hi, lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hi[k] = (__bf16)v[k];
      lo[k] = (__bf16)(v[k] - (float)hi[k]);
    }
    char* at = stage + G::plane_off(0, aq >> 1) + pix * 16 + 8 * (aq & 1);
    *reinterpret_cast<bf16x4*>(at) = hi;
    if constexpr (!PLAIN) *reinterpret_cast<bf16x4*>(at + HLS) = lo;
    // training forward: the bf16 copy of the activated source 0 the weight gradient reads -- the hi half is exactly that.  Every pixel
    // is interior (not halo) to one tile; the first output-channel tile writes it.
    if constexpr (SIDE) {
      // (the pixel's element offset inside its clip is the loader's byte offset / 4, read back from the LDS table: as registers the six
      // per-slot offsets would be loop invariants the compiler keeps -- and spills)
      const int py = pix / HPW, px = pix % HPW;
      const bool interior = inside && py >= 1 && py <= PH && px >= 1 && px <= PW && blockIdx.y == 0;
      if (a.x0_bf16 != nullptr && c0 < a.C0 && interior) {
        const size_t e = (size_t)S.b * a.H * a.W * a.C0 + ((aoffs0[it * THREADS + tid] + S.t0) >> 2) + c0;
        *reinterpret_cast<bf16x4*>(a.x0_bf16 + e) = hi;
      }
      if (a.x1_bf16 != nullptr && c0 >= a.C0 && interior) {            // source 1: its own (smaller, offset) geometry
        const size_t e = (size_t)S.b * a.H1 * a.W1 * a.C1 + ((aoffs0[(A_F4 + it) * THREADS + tid] + S.t1) >> 2) + (c0 - a.C0);
        *reinterpret_cast<bf16x4*>(a.x1_bf16 + e) = hi;
      }
    }
  };

  // ---- weight fragments: ring of three sets, [slot][16-channel tile][hi, lo]
  bf16x8 wq[3][2][2];
  // the lane's 16 bytes of the wave's first 16-channel tile (hi; lo 1 KB, the second tile 2 KB further) in the image [tap][chunk][Cout / 16][2 KB]
  auto w_frag = [&](int tap, int chunk) __attribute__((always_inline)) {
    return reinterpret_cast<const char*>(a.w) +
           ((((size_t)tap * nchunks + chunk) * (size_t)(a.Cout / 16) + (size_t)(n0 / 16 + 2 * wn)) << 11) + lane * 16;
  };
  auto load_w = [&](int chunk, int tap, auto SLOT) __attribute__((always_inline)) {
    constexpr int slot = decltype(SLOT)::value;
    const char* wb = w_frag(tap, chunk);
    wq[slot][0][0] = *reinterpret_cast<const bf16x8*>(wb);
    if constexpr (!PLAIN) wq[slot][0][1] = *reinterpret_cast<const bf16x8*>(wb + 1024);
    wq[slot][1][0] = *reinterpret_cast<const bf16x8*>(wb + 2048);
    if constexpr (!PLAIN) wq[slot][1][1] = *reinterpret_cast<const bf16x8*>(wb + 3072);
  };

  // ---- pixel fragments: two sets of four 16-pixel tiles (hi, lo)
  struct XFrags { bf16x8 h[4], l[4]; };
  XFrags fx0, fx1;
  // byte offset of the lane's row of pixel tile 0 in plane (hi, g) at tap (0, 0); the other tiles are compile-time displacements of it
  // (a 16-pixel tile is half a patch row of the 32-wide patches, a whole row of the 16-wide ones)
  const int xbase = (((wm * WPXW + p) / PW) * HPW + ((wm * WPXW + p) % PW)) * 16 + G::plane_off(0, g);
  auto tile_disp = [](int pt) { return (PW == 32) ? ((pt >> 1) * HPW + (pt & 1) * 16) * 16 : pt * HPW * 16; };
  auto read_x = [&](XFrags& f, const char* stage, int tap_off, int half) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const char* r = stage + xbase + tile_disp(4 * half + i) + tap_off;
      if constexpr (!PLAIN) f.l[i] = *reinterpret_cast<const bf16x8*>(r + HLS);
      f.h[i] = *reinterpret_cast<const bf16x8*>(r);
    }
  };
  floatx4 acc[2][PT];
#pragma unroll
  for (int ct = 0; ct < 2; ++ct)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
  auto mfma_half = [&](const XFrags& f, const bf16x8 (&w)[2][2], int half) __attribute__((always_inline)) {
    // term-major: an accumulator is touched every eighth instruction
    if constexpr (!PLAIN) {
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][1], f.h[i], acc[ct][4 * half + i], 0, 0, 0);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][0], f.l[i], acc[ct][4 * half + i], 0, 0, 0);
    }
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][0], f.h[i], acc[ct][4 * half + i], 0, 0, 0);
  };
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  constexpr int N_R = PLAIN ? 4 : 8, N_M = PLAIN ? 8 : 24;             // fragment reads / MFMAs of one phase
  constexpr int N_W = PLAIN ? 2 : 4;                                   // weight-fragment loads of one tap
  // One tap.  Phase A: MFMA(pixel tiles 0..3 of tap t) || read tiles 4..7 of tap t, request the weights of tap t + 2.  Phase B: MFMA(tiles
  // 4..7) || read tiles 0..3 of tap t + 1, (tap 0) request the next chunk's halo, (taps 2..7) split one staging slot of it.  The chunk's
  // one barrier sits between the phases of tap 8: before it every wave has read the last fragments of this chunk's halo stage (rewritten
  // from tap 2 of the next chunk on), behind it the next chunk's stage -- split at taps 2..7 of this chunk by every wave -- is complete.
  auto tap_body = [&](auto TAP, int chunk) __attribute__((always_inline)) {
    constexpr int tap = decltype(TAP)::value;
    constexpr int ntap = (tap + 1) % TAPS;
    constexpr int tap_off = ((tap / 3) * HPW + (tap % 3)) * 16, ntap_off = ((ntap / 3) * HPW + (ntap % 3)) * 16;
    const int chunk_n = chunk + 1 < nchunks ? chunk + 1 : (PERSIST ? 0 : chunk);
    const char* cur = smem + (chunk & 1) * STAGE;
    const char* nxt = (tap == TAPS - 1) ? smem + ((chunk + 1) & 1) * STAGE : cur;
    read_x(fx1, cur, tap_off, 1);
    mfma_half(fx0, wq[tap % 3], 0);
    load_w((tap + 2 >= TAPS) ? chunk_n : chunk, (tap + 2) % TAPS, std::integral_constant<int, (tap + 2) % 3>{});
    pin_reads<N_M - 1, N_R>();
    constexpr int used_a = pin_read_slots(N_M - 1, N_R);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, N_W, 0);
    if constexpr (N_M - used_a - 1 > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - used_a - 1, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (tap == TAPS - 1) {
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
    }
    if (tap == 0) load_a_pre(chunk_n);
    if (tap == TAPS - 1) preload_offsets(PERSIST ? (chunk + 2 < nchunks ? chunk + 2 : chunk + 1 < nchunks ? 0 : 1 < nchunks ? 1 : 0)
                                                 : (chunk + 2 < nchunks ? chunk + 2 : chunk + 1 < nchunks ? chunk + 1 : chunk));   // what the next tap 0 requests
    read_x(fx0, nxt, ntap_off, 0);
    mfma_half(fx1, wq[tap % 3], 1);
    if constexpr (tap >= 2 && tap - 2 < A_F4) {
      split_slot(std::integral_constant<int, tap - 2>{}, chunk_n, smem + ((chunk + 1) & 1) * STAGE);
#pragma unroll
      for (int i = 0; i < N_R; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
      if constexpr (N_M - N_R - 4 > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - N_R - 4, 0);
    } else {
      pin_reads<N_M, N_R>();
      if constexpr (N_M - pin_read_slots(N_M, N_R) > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - pin_read_slots(N_M, N_R), 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // WMW = 4 (a wave owns four pixel tiles): ONE phase per tap -- MFMA(tiles 0..3 of tap t, fragment set t & 1) || read tiles 0..3 of tap
  // t + 1 into the other set, request the weights of tap t + 2, (tap 0) request the next chunk's halo, (taps 2..7) split one staging
  // slot.  Nine taps per chunk: the set parity flips with the chunk, so the loop body is two chunks (PAR = parity of tap 0's set).
  auto tap_body4 = [&](auto TAP, auto PAR, int chunk) __attribute__((always_inline)) {
    constexpr int tap = decltype(TAP)::value, par = (decltype(PAR)::value + tap) & 1;
    constexpr int ntap = (tap + 1) % TAPS;
    constexpr int ntap_off = ((ntap / 3) * HPW + (ntap % 3)) * 16;
    const int chunk_n = chunk + 1 < nchunks ? chunk + 1 : 0;          // past the tile's last chunk: chunk 0 of the next tile (S is that tile by then)
    const char* cur = smem + (chunk & 1) * STAGE;
    const char* nxt = (tap == TAPS - 1) ? smem + ((chunk + 1) & 1) * STAGE : cur;
    if (tap == TAPS - 1) {
      __syncthreads();                                                 // the next stage is complete, this one is read out
      __builtin_amdgcn_sched_barrier(0);
    }
    if (tap == 0) load_a_pre(chunk_n);
    // what the next tap 0 requests: chunk + 2; from the tile's last-but-one chunk on, the next tile's chunk 0, then its chunk 1
    if (tap == TAPS - 1) preload_offsets(chunk + 2 < nchunks ? chunk + 2 : chunk + 1 < nchunks ? 0 : 1 < nchunks ? 1 : 0);
    read_x(par ? fx0 : fx1, nxt, ntap_off, 0);
    mfma_half(par ? fx1 : fx0, wq[tap % 3], 0);
    load_w((tap + 2 >= TAPS) ? chunk_n : chunk, (tap + 2) % TAPS, std::integral_constant<int, (tap + 2) % 3>{});
    if constexpr (tap >= 2 && tap - 2 < A_F4) {
      split_slot(std::integral_constant<int, tap - 2>{}, chunk_n, smem + ((chunk + 1) & 1) * STAGE);
#pragma unroll
      for (int i = 0; i < N_R; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
#pragma unroll
      for (int i = 0; i < N_W; ++i) {
        if constexpr (!PLAIN) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
        __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
      }
      if constexpr (N_M - N_R - 8 > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - N_R - 8, 0);
    } else {
#pragma unroll
      for (int i = 0; i < N_R; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
      }
#pragma unroll
      for (int i = 0; i < N_W; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      if constexpr (N_M - N_R - N_W > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - N_R - N_W, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };

  // ---- ROWS form of the main loop: the three vertical taps of a column offset dx share their pixel fragments.  A wave's 128 pixels are
  // R patch rows (4 of 32 pixels, or 8 of 16); tap (dy, dx) of row r reads halo row r + dy, so for one dx the R + 2 halo rows are read
  // ONCE each (hi and lo) and row h feeds the accumulators of rows h, h - 1, h - 2 with the weights of taps (0, dx), (1, dx), (2, dx):
  // 72 (60) fragment reads per 32-channel chunk instead of 144 -- the half-reads timing experiment on the tap-by-tap loop returned
  // 4-7 % on the >= 128-channel layers (the loop is power limited, LDS traffic is part of the power).  A "period" = one dx: 144 MFMAs,
  // the weights of its three taps in registers, the next period's three taps requested at its start into the other half of a
  // six-set ring (static indices: the loop body is two chunks = six periods), the next chunk's halo requested in period 0 and split
  // in periods 1 and 2, the chunk's one barrier in front of the last row step of period 2 (whose prefetch reads the next stage).
  constexpr int R = BM / 2 / PW, HV = PW / 16;
  bf16x8 wr[2][3][2][2];                                               // [ring half][dy][16-channel tile][hi, lo]
  // pixel fragments: one "unit" = 16 pixels of one halo row (hi and lo); a ring of NB units, read NB - 1 units ahead of their MFMAs (a
  // unit carries only 6 .. 18 MFMAs: one unit of distance is shorter than the LDS latency).  NU units per period, NB divides NU.
  constexpr int NU = (R + 2) * HV, NB = (PW == 32) ? 4 : 5;
  static_assert(NU % NB == 0, "static ring indices");
  auto load_wr1 = [&](int chunk, auto DX, auto PAR, auto DY) __attribute__((always_inline)) {
    constexpr int dx = decltype(DX)::value, par = decltype(PAR)::value, dy = decltype(DY)::value;
    const char* wb = w_frag(dy * 3 + dx, chunk);
    wr[par][dy][0][0] = *reinterpret_cast<const bf16x8*>(wb);
    if constexpr (!PLAIN) wr[par][dy][0][1] = *reinterpret_cast<const bf16x8*>(wb + 1024);
    wr[par][dy][1][0] = *reinterpret_cast<const bf16x8*>(wb + 2048);
    if constexpr (!PLAIN) wr[par][dy][1][1] = *reinterpret_cast<const bf16x8*>(wb + 3072);
  };
  struct XUnit { bf16x8 h, l; };
  XUnit xu[NB];
  auto read_unit = [&](XUnit& f, const char* stage, int u, int dx) __attribute__((always_inline)) {
    const char* r = stage + xbase + ((u / HV) * HPW + (u % HV) * 16 + dx) * 16;
    if constexpr (!PLAIN) f.l = *reinterpret_cast<const bf16x8*>(r + HLS);
    f.h = *reinterpret_cast<const bf16x8*>(r);
  };
  // unit u = (halo row h, half hv): every (dy, r = h - dy) pair it serves, term-major (an accumulator is touched once per term)
  auto mfma_unit = [&](auto U, const XUnit& f, auto PAR) __attribute__((always_inline)) {
    constexpr int h = decltype(U)::value / HV, hv = decltype(U)::value % HV, par = decltype(PAR)::value;
#pragma unroll
    for (int term = PLAIN ? 2 : 0; term < 3; ++term)                    // PLAIN: the hi x hi term only
#pragma unroll
      for (int dy = 0; dy < 3; ++dy) {
        if (h - dy < 0 || h - dy >= R) continue;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          floatx4& c = acc[ct][(h - dy) * HV + hv];
          c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[par][dy][ct][term == 0 ? 1 : 0], term == 1 ? f.l : f.h, c, 0, 0, 0);
        }
      }
  };
  auto unit_mfmas = [](int u) { const int h = u / HV; int n = 0; for (int dy = 0; dy < 3; ++dy) n += (h - dy >= 0 && h - dy < R) ? 1 : 0; return n * (PLAIN ? 2 : 6); };
  constexpr int BARU = NU - NB + 1;                                    // first unit whose prefetch reads the next period
  constexpr int SA = NU / 2, SB = BARU - AHALF;                        // first split units of periods 1 and 2
  static_assert(SA + AHALF < NU && SB >= 0, "staging schedule");
  auto unit_step = [&](auto U, auto DX, auto PAR, int chunk) __attribute__((always_inline)) {
    constexpr int u = decltype(U)::value, dx = decltype(DX)::value, par = decltype(PAR)::value;
    constexpr int n_m = unit_mfmas(u);
    const int chunk_n = chunk + 1 < nchunks ? chunk + 1 : (PERSIST ? 0 : chunk);
    const char* cur = smem + (chunk & 1) * STAGE;
    char* nxs = smem + ((chunk + 1) & 1) * STAGE;
    if constexpr (u == BARU && dx == 2) {
      __syncthreads();                                                 // the next stage is complete, this one is read out
      __builtin_amdgcn_sched_barrier(0);
    }
    constexpr int pu = u + NB - 1;                                     // the unit requested now
    if constexpr (pu < NU) read_unit(xu[pu % NB], cur, pu, dx);
    else read_unit(xu[pu % NB], dx == 2 ? nxs : cur, pu - NU, (dx + 1) % 3);
    mfma_unit(U, xu[u % NB], PAR);
    // the period's other work: the next period's weights (one tap per unit, units 1 .. 3), the next chunk's halo (first half requested
    // in period 0, split in period 1; second half requested in period 1 behind that, split in period 2 in front of the barrier)
    constexpr int split_it = dx == 1 ? u - SA : dx == 2 ? AHALF + u - SB : -1;
    constexpr bool do_split = (dx == 1 && u >= SA && u < SA + AHALF) || (dx == 2 && u >= SB && u < SB + AHALF && split_it < A_F4);
    if constexpr (u == 0 && dx == 0) load_a_range(chunk_n, std::integral_constant<int, 0>{}, std::integral_constant<int, AHALF>{});
    if constexpr (u == SA + AHALF && dx == 1) load_a_range(chunk_n, std::integral_constant<int, AHALF>{}, std::integral_constant<int, AHALF>{});
    if constexpr (u >= 1 && u <= 3) {
      if constexpr (dx < 2) load_wr1(chunk, std::integral_constant<int, (dx + 1) % 3>{}, std::integral_constant<int, par ^ 1>{}, std::integral_constant<int, u - 1>{});
      else load_wr1(chunk_n, std::integral_constant<int, 0>{}, std::integral_constant<int, par ^ 1>{}, std::integral_constant<int, u - 1>{});
    }
    if constexpr (do_split) split_slot(std::integral_constant<int, split_it>{}, chunk_n, nxs);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, PLAIN ? 1 : 2, 0);
    if constexpr (do_split && PLAIN) {
      // a unit carries 2 .. 6 MFMAs here: the split's vector work goes between them in equal parts
#pragma unroll
      for (int i = 1; i < n_m; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x002, (24 + n_m - 2) / (n_m - 1), 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
    } else if constexpr (PLAIN && u >= 1 && u <= 3) {
      __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
      if constexpr (n_m - 1 > 0) __builtin_amdgcn_sched_group_barrier(0x008, n_m - 1, 0);
    } else if constexpr (do_split) {
      __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x002, 6, 0);
      }
      __builtin_amdgcn_sched_group_barrier(0x200, 2, 0);
      if constexpr (n_m - 5 > 0) __builtin_amdgcn_sched_group_barrier(0x008, n_m - 5, 0);
    } else if constexpr (u >= 1 && u <= 3) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
      }
      if constexpr (n_m - 5 > 0) __builtin_amdgcn_sched_group_barrier(0x008, n_m - 5, 0);
    } else {
      if constexpr (n_m - 1 > 0) __builtin_amdgcn_sched_group_barrier(0x008, n_m - 1, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  };
  auto period = [&](auto DX, auto PAR, int chunk) __attribute__((always_inline)) {
    each_index<NU>(unit_step, DX, PAR, chunk);
  };

  if constexpr (ROWS) {
    // chunk 0: all the staging slots in ONE round trip (the second half through temporaries: the fragment ring is not live yet)
    f32x4 keep[AREGS];
    load_a_range(0, std::integral_constant<int, AHALF>{}, std::integral_constant<int, AHALF>{});
#pragma unroll
    for (int i = 0; i < AREGS; ++i) keep[i] = areg[i];
    load_a_range(0, std::integral_constant<int, 0>{}, std::integral_constant<int, AHALF>{});
    // (a lambda, not each_index's argument list: with DY as load_wr1's first parameter 14 of the 22 ROWS forms were scheduled differently)
    each_index<3>([&](auto DY) __attribute__((always_inline)) { load_wr1(0, S0{}, S0{}, DY); });
    // slots [0, AHALF) sit in the staging registers, slots [AHALF, A_F4) in `keep` (AHALF = 3 for float32 sources, 2 for bf16 ones)
    each_index<AHALF>(split_slot, 0, smem);
#pragma unroll
    for (int i = 0; i < AREGS; ++i) areg[i] = keep[i];
    each_index<A_F4 - AHALF, AHALF>(split_slot, 0, smem);
    static_assert(A_F4 <= 2 * AHALF, "two halves of staging slots");
  } else {
    load_a(0);
    load_w(0, 0, S0{});
    load_w(0, 1, S1{});
    each_index<A_F4>(split_slot, 0, smem);
    preload_offsets(1 < nchunks ? 1 : 0);                              // chunk 0's tap 0 requests chunk 1
  }
  auto epilogue = [&]() __attribute__((always_inline)) {
  // ---- epilogue: D[channel 4 g + j of tile ct][pixel p of tile pt]: out = relu(acc * scale + shift), 16-byte stores
  #pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      const int chl = wn * 32 + ct * 16 + 4 * g;                       // channel inside the workgroup's BN
      const f32x4 sc = *reinterpret_cast<const f32x4*>(epi + chl);
      const f32x4 sh = *reinterpret_cast<const f32x4*>(epi + BN + chl);
  #pragma unroll
      for (int pt = 0; pt < PT; ++pt)
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v = acc[ct][pt][j] * sc[j] + sh[j];
          if (a.relu) v = v > 0.f ? v : 0.f;
          acc[ct][pt][j] = v;
        }
    }
    if (SIDE && a.stats_part != nullptr) {
      // training forward: the BatchNorm statistics of this output, one partial row per wave -- (sum, sum of squares) over the wave's
      // stored pixels for each of its 32 channels; rows are summed in float64 by mfpa_conv_stats_reduce (fixed order: deterministic)
      float vm[PT];
  #pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int m = wm * WPXW + pt * 16 + p;
        vm[pt] = (ey0 + m / PW < a.yH && ex0p + m % PW < a.yW) ? 1.f : 0.f;
      }
      float* row = a.stats_part + ((size_t)tile * WMW + wm) * 2 * a.Cout + n0 + wn * 32 + 4 * g;
  #pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        f32x4 sv = {0.f, 0.f, 0.f, 0.f}, qv = {0.f, 0.f, 0.f, 0.f};
        if (!AFF16 && a.bz != nullptr) {                                 // (never in the training forward's AFF16 form)
          // the output is dy of a BatchNorm + ReLU whose input bz has this tensor's shape: (sum g, sum g * xhat) instead (see ConvArgs)
          const int ch = n0 + wn * 32 + ct * 16 + 4 * g;
          const f32x4 bsc = *reinterpret_cast<const f32x4*>(a.bz_scale + ch), bsh = *reinterpret_cast<const f32x4*>(a.bz_shift + ch);
          const f32x4 bmu = *reinterpret_cast<const f32x4*>(a.bz_mean + ch), bis = *reinterpret_cast<const f32x4*>(a.bz_invstd + ch);
          // (the dtype branch sits OUTSIDE the pixel loop: inside it, every iteration was branch -> load -> wait, eight dependent round trips)
          f32x4 zzs[PT];
          auto zoff = [&](int pt) __attribute__((always_inline)) {
            const int m = wm * WPXW + pt * 16 + p;
            const int gy = min(ey0 + m / PW, a.yH - 1), gx = min(ex0p + m % PW, a.yW - 1);      // clamped; masked by vm
            return (((size_t)eb * a.yH + gy) * a.yW + gx) * (size_t)a.Cout + ch;
          };
          if (a.bz16) {                                                  // bz kept as bfloat16 (mfpa_conv_desc.bwd_z_is_bf16)
            f32x2 raw[PT];
  #pragma unroll
            for (int pt = 0; pt < PT; ++pt) raw[pt] = *reinterpret_cast<const f32x2*>(reinterpret_cast<const __bf16*>(a.bz) + zoff(pt));
  #pragma unroll
            for (int pt = 0; pt < PT; ++pt) {
              const unsigned u0 = __float_as_uint(raw[pt][0]), u1 = __float_as_uint(raw[pt][1]);
              zzs[pt] = f32x4{__uint_as_float(u0 << 16), __uint_as_float(u0 & 0xffff0000u), __uint_as_float(u1 << 16), __uint_as_float(u1 & 0xffff0000u)};
            }
          } else {
  #pragma unroll
            for (int pt = 0; pt < PT; ++pt) zzs[pt] = *reinterpret_cast<const f32x4*>(a.bz + zoff(pt));
          }
  #pragma unroll
          for (int pt = 0; pt < PT; ++pt) {
            const f32x4 zz = zzs[pt];
  #pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float gg = (zz[j] * bsc[j] + bsh[j] > 0.f) ? acc[ct][pt][j] * vm[pt] : 0.f;
              sv[j] += gg;
              qv[j] += gg * ((zz[j] - bmu[j]) * bis[j]);
            }
          }
        } else {
  #pragma unroll
        for (int pt = 0; pt < PT; ++pt)
  #pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float v = acc[ct][pt][j] * vm[pt];
            sv[j] += v;
            qv[j] += v * v;
          }
        }
  #pragma unroll
        for (int j = 0; j < 4; ++j) {
          // row_shr 1, 2, 4, 8: lane 15 of a 16-lane row ends with its total
          sv[j] = dpp_row_add<0x118>(dpp_row_add<0x114>(dpp_row_add<0x112>(dpp_row_add<0x111>(sv[j]))));
          qv[j] = dpp_row_add<0x118>(dpp_row_add<0x114>(dpp_row_add<0x112>(dpp_row_add<0x111>(qv[j]))));
        }
        if (p == 15) {
          *reinterpret_cast<f32x4*>(row + ct * 16) = sv;
          *reinterpret_cast<f32x4*>(row + a.Cout + ct * 16) = qv;
        }
      }
    }
    if (a.y != nullptr || (SIDE && IN16 && a.y_bf16 != nullptr)) {      // (y null with y_bf16: the output exists as bfloat16 only)
      char* yb = reinterpret_cast<char*>(a.y + (size_t)eb * a.yH * a.yW * a.Cout);
  #pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int m = wm * WPXW + pt * 16 + p;
        const int gy = ey0 + m / PW, gx = ex0p + m % PW;
        if (gy < a.yH && gx < a.yW) {
          char* yp = yb + (((unsigned)gy * (unsigned)a.yW + (unsigned)gx) * (unsigned)a.Cout + (unsigned)(n0 + wn * 32 + 4 * g)) * 4u;
          if (a.y != nullptr) {
  #pragma unroll
          for (int ct = 0; ct < 2; ++ct) {
            f32x4 o;
  #pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = acc[ct][pt][j];
            *reinterpret_cast<f32x4*>(yp + ct * 64) = o;
          }
          }
          if (SIDE && a.y_bf16 != nullptr) {
            __bf16* hp = a.y_bf16 + (((size_t)eb * a.yH + gy) * a.yW + gx) * (size_t)a.Cout + n0 + wn * 32 + 4 * g;
  #pragma unroll
            for (int ct = 0; ct < 2; ++ct) {
              bf16x4 h;
  #pragma unroll
              for (int j = 0; j < 4; ++j) h[j] = (__bf16)acc[ct][pt][j];
              *reinterpret_cast<bf16x4*>(hp + ct * 16) = h;
            }
          }
        }
      }
    }
    if (a.y_pool != nullptr) {
      // MaxPool2d(2) (floor): the window's two rows are two of the wave's pixel tiles, its two columns adjacent lanes (one DPP swap)
      const int Ho = a.H / 2, Wo = a.W / 2;
      constexpr int ROWSTEP = (PW == 32) ? 2 : 1;                        // pixel tiles per patch row
  #pragma unroll
      for (int ct = 0; ct < 2; ++ct)
  #pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          const int row = pt / ROWSTEP;                                  // patch row inside the wave's block
          if (row & 1) continue;
          f32x4 v;
  #pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float t = fmaxf(acc[ct][pt][j], acc[ct][pt + ROWSTEP][j]);
            const float o = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(t), 0xB1, 0xf, 0xf, true));      // quad_perm [1,0,3,2]
            v[j] = fmaxf(t, o);
          }
          const int m = wm * WPXW + pt * 16 + p;
          const int py = (ey0 + m / PW) / 2, px = (ex0p + m % PW) / 2;
          if (!(p & 1) && py < Ho && px < Wo)
            *reinterpret_cast<f32x4*>(a.y_pool + (((size_t)eb * Ho + py) * Wo + px) * a.Cout + n0 + wn * 32 + ct * 16 + 4 * g) = v;
        }
    }
  
    if constexpr (WMW == 4) {
      if (a.w1x1 != nullptr) {
        // fused OutConv 1x1 to one class (the whole C_out = 64 is in this workgroup): a lane's eight channels times their weights,
        // the four channel groups of a wave through two ds_bpermute butterflies, the two channel-tile waves through LDS; then one
        // pixel per thread, stored coalesced
        float* red = reinterpret_cast<float*>(smem + 2 * STAGE + TBL * sizeof(unsigned)) + (a.in_scale0 ? 2 * a.C0 : 0);   // [2][256]
        const f32x4 w0 = *reinterpret_cast<const f32x4*>(epi + 2 * BN + wn * 32 + 4 * g);
        const f32x4 w1 = *reinterpret_cast<const f32x4*>(epi + 2 * BN + wn * 32 + 16 + 4 * g);
  #pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          float v = 0.f;
  #pragma unroll
          for (int j = 0; j < 4; ++j) v += acc[0][pt][j] * w0[j] + acc[1][pt][j] * w1[j];
          v += __shfl_xor(v, 16);
          v += __shfl_xor(v, 32);
          if (g == 0) red[wn * 256 + wm * WPXW + pt * 16 + p] = v;
        }
        __syncthreads();
        if (tid < 256) {
          const int gy = ey0 + tid / PW, gx = ex0p + tid % PW;
          if (gy < a.H && gx < a.W) a.y1x1[((size_t)eb * a.H + gy) * a.W + gx] = red[tid] + red[256 + tid] + a.b1x1;
        }
        __syncthreads();                                               // red is reused by the next tile
      }
    }
  };

  __syncthreads();
  if constexpr (ROWS) {
#pragma unroll
    for (int u = 0; u < NB - 1; ++u) read_unit(xu[u], smem, u, 0);
  } else {
    read_x(fx0, smem, 0, 0);
  }
  // ---- the tile walk, once for the three loop forms.  PERSIST: N is the workgroup's next tile (past its last one: this tile again -- its first
  // chunk is requested once more and never used); it becomes the staged tile S in front of the tile's last chunk, whose loader steps then
  // request and split the next tile's first chunk.  Not PERSIST: one tile.
  for (;;) {
    const int tile_n = tile + (int)gridDim.x;
    const bool has_next = PERSIST && tile_n < ntiles;
    const Tile N = PERSIST ? make_tile(has_next ? tile_n : tile) : S;
    if constexpr (ROWS) {
      using D0 = std::integral_constant<int, 0>;
      using D1 = std::integral_constant<int, 1>;
      using D2 = std::integral_constant<int, 2>;
      for (int chunk = 0; chunk < nchunks; chunk += 2) {                 // nchunks is even (C_in % 64 == 0, checked by the dispatcher)
        period(D0{}, S0{}, chunk);
        period(D1{}, S1{}, chunk);
        period(D2{}, S0{}, chunk);
        if (PERSIST && chunk + 2 >= nchunks) S = N;
        period(D0{}, S1{}, chunk + 1);
        period(D1{}, S0{}, chunk + 1);
        period(D2{}, S1{}, chunk + 1);
      }
    } else if constexpr (WMW == 4) {
      for (int chunk = 0; chunk < nchunks; chunk += 2) {                 // nchunks is even (C_in % 64 == 0, checked by the dispatcher)
        each_index<TAPS>(tap_body4, S0{}, chunk);
        if (chunk + 2 >= nchunks) S = N;
        each_index<TAPS>(tap_body4, S1{}, chunk + 1);
      }
    } else {                                                           // WMW = 2, tap-by-tap
      for (int chunk = 0; chunk < nchunks; ++chunk) {
        if (PERSIST && chunk + 1 >= nchunks) S = N;
        each_index<TAPS>(tap_body, chunk);
      }
    }
    epilogue();
    if (!has_next) break;
    tile = tile_n; eb = S.b; ey0 = S.y0; ex0p = S.x0p;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
  }
}

}  // namespace

namespace mfpa_unet {

// conv_wd16_kernel's ROWS loop form from this many input channels up: same-call pairs on the UNet's layers, 64 clips: +2 .. +4 % at 512 /
// 1024 input channels, -1 .. -4 % at 64 .. 256 (its longer pipeline fill costs more than the halved fragment reads return when a tile has
// only 2 .. 8 chunks)
const int CONV_WD16_ROWS = 512;
void conv_wd16_tile(int W, int Cout, mfpa_conv_route* t) {     // 64-channel output tiles: 4 x 2 waves of 64 px x 32 ch
  t->wmw = Cout % 128 ? 4 : 2; t->bn = 32 * (8 / t->wmw);
  t->pw = (t->wmw == 2 && W <= 16) ? 16 : 32; t->ph = 256 / t->pw;
}

template <int PH, int PW, bool ROWS, int WMW, bool SIDE, bool PLAIN, bool IN16, bool AFF16>
int launch_wd16(ConvArgs& a, hipStream_t s) {
  using G = Wd16Lds<PH, PW, IN16>;
  const size_t lds = (size_t)G::fixed_bytes(WMW) +                                         // two halo stages + the slot offsets + the epilogue's constants
                     (a.in_scale0 ? (size_t)2 * a.C0 * sizeof(float) : 0) +                // + the on-load affine
                     (a.w1x1 ? G::RED * sizeof(float) : 0);                                // + the fused OutConv's partial sums
  dim3 grid((unsigned)((long long)a.tiles_x * a.tiles_y * a.B), (unsigned)(a.Cout / wd16_bn(WMW)));
  if constexpr (wd16_persist(ROWS, WMW, SIDE, PLAIN)) {                // one workgroup per CU (and output-channel tile) walks the tiles
    // ... where the chunk count is even: the halo stage of a chunk is (chunk & 1), so the next tile's chunk 0, split behind this tile's last
    // chunk, lands in stage 0 only then.  An odd count (C_in % 64 == 32: the tap-by-tap WMW = 2 forms alone take it) keeps one tile per workgroup.
    const int cus = mfpa_current_device_cus();
    const unsigned per = (unsigned)((cus > 0 ? cus : 256) / (int)grid.y);
    if (per >= 1 && grid.x > per && ((a.C0 + a.C1) / KC) % 2 == 0) grid.x = per;
  }
  hipLaunchKernelGGL((conv_wd16_kernel<PH, PW, ROWS, WMW, SIDE, PLAIN, IN16, AFF16>), grid, dim3(G::THREADS), lds, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
#define MFPA_WD16_INSTANTIATE(...) template int launch_wd16<__VA_ARGS__>(ConvArgs&, hipStream_t);
MFPA_WD16_FORMS(MFPA_WD16_INSTANTIATE)

}  // namespace mfpa_unet
