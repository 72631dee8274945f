// Wave-specialised 3x3 convolution for the UNet's 64-channel full-resolution layers (training/unet.py:8-25 DoubleConv of `inc` and
// `up4`; inference, bf16x3 products on v_mfma_f32_16x16x32_bf16).  Round 5.
//
// Why another kernel.  conv_wd16_kernel<.., WMW = 4> (csrc/unet_wd16.hip) gives these layers 8 waves that ALL do everything -- request the halo
// from HBM, split it into bf16 hi / lo planes in LDS, pull their weight fragments through the L1 and issue the MFMAs -- with the two
// waves of a SIMD in barrier lock-step.  Vector-memory returns are in order, so a wave's wait for a weight fragment requested behind the
// chunk's six HBM halo loads is a wait for HBM, and while it waits it issues no MFMA either; its SIMD-mate waits for the same thing.
// Measured on the shipped code (profiles/r04_c64_skip_variants_product_code.txt): MFMA stream alone 480 us, everything else alone
// 379 us, together 901 us -- they add.  And four pixel-waves fetch the same 8 KB of weights per tap (texture addresser 59 % busy).
//
// Here the 8 waves of a workgroup have two ROLES, one wave of each role per SIMD:
//   * waves 0..3, COMPUTE: 2 pixel halves x 2 channel halves, a wave owns 128 px x 32 ch (the wave tile of the 128-channel form: half
//     the weight bytes per MFMA of the 64 px x 32 ch tile).  Their instruction stream is MFMAs, LDS fragment reads and the weight
//     fragments (L1 / L2 hits, two taps ahead through a ring of three register sets) -- nothing in it ever waits for HBM.
//   * waves 4..7, LOADERS: request the NEXT chunk's halo (256 threads x 11 staging slots of 16 B), split fp32 -> bf16 hi | lo, write the
//     planes of the other LDS stage, and request the chunk after that into the freed registers -- a whole chunk period (~3.5 us) ahead
//     of its use.  Their vector work issues in the gaps a v_mfma_f32_16x16x32_bf16 leaves on the SIMD's issue port.
// The loaders also take the EPILOGUE's memory work: a compute wave applies the output affine + ReLU and writes its accumulators to a 64 KB
// LDS tile (XOR-swizzled 16-byte pieces: conflict-free both ways) and goes straight on to the next tile's MFMAs; one barrier later the
// loaders read the tile and issue the global stores (a CU's store path takes ~10 B/clk: the 64 KB of a tile held the compute waves for
// ~6 k cycles, a quarter of a two-chunk tile) and, for up4's second layer, the fused OutConv's 64-channel dot product per pixel.
// One s_barrier per 32-channel chunk hands a finished stage to the compute waves and a read-out stage back to the loaders.  The tile loop
// is persistent (one workgroup per CU walks tiles b, b + G, ...): the loaders simply run on into the next tile's first chunk.
// LDS: two stages of eight planes [hi | lo][k-group] of (halo pixel x 16 B) (conflict-free ds_read_b128), a halo row's columns de-interleaved
// (even, then odd: mfpa_conv_tile.h) because a compute wave's 16-pixel groups are pixels two columns apart -- the column-odd groups at one
// tap and the column-even groups at the next tap of the row then want the same fragments, and a chunk costs 12 sets of reads, not 18.
// Same products and the same summation inside an instruction as conv_wd16_kernel: bit-identical outputs (tests/test_gpu_unet.py).
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include "mfpa_unet_args.h"

namespace mfpa_unet {
namespace {

using namespace mfpa_tile;
using namespace mfpa_tile::role_split;     // tile geometry and LDS plane layout (shared with conv_up_kernel)

constexpr int TAPS = 9;
constexpr int C1W = PW + 4, C1PROWS = 6;                               // C1SRC: a loader wave's part of the 1-channel source patch: <= 6 rows of PW + 4 columns
constexpr int C1LDS = (4 * C1PROWS * C1W + 128) * 4;                   // four wave-private patches + the first layer's (scale 64, shift 64)

// tile index of workgroup b's i-th tile.  Plain: b + i G.  XCD-aware: workgroups b and b + 8 share an XCD (round-robin dispatch: speed
// only), so within a round of G tiles XCD x = b % 8 takes the G / 8 consecutive tiles [x G / 8, (x + 1) G / 8).
__device__ __forceinline__ int tile_of(int b, int i, int G) {
  if ((G & 7) == 0) return i * G + (b & 7) * (G >> 3) + (b >> 3);
  return i * G + b;
}

// C1SRC: the 64 input channels are not read but COMPUTED by the loaders -- the UNet's first layer (1 -> 64 channels, 3x3, folded
// BatchNorm + ReLU; training/unet.py:16-18) applied to the 1-channel source, so `inc`'s 64-channel intermediate never exists in HBM.
template <bool C1SRC>
__global__ __launch_bounds__(THREADS, 1) void conv_ws64_kernel(ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int Cin = a.C0 + a.C1;
  const int nchunks = Cin / KC;
  const int ntiles = a.tiles_x * a.tiles_y * a.B;
  const int G = (int)gridDim.x;
  const int n0 = (int)blockIdx.y * 64;                                 // this workgroup's 64 output channels (Cout / 64 workgroup rows)
  // tiles this workgroup owns: i = 0 .. owned - 1 (tile_of is increasing in i; the launcher keeps G <= ntiles, so owned >= 1)
  const int first_tile = tile_of((int)blockIdx.x, 0, G);
  const int owned = first_tile < ntiles ? (ntiles - first_tile + G - 1) / G : 0;

  // LDS: [stage 0 | stage 1 | epilogue constants: scale 64, shift 64, w1x1 64, accumulator start values 64 | the epilogue's output tile 64 KB]
  float* const epi = reinterpret_cast<float*>(smem + 2 * STAGE);
  char* const outbuf = smem + 2 * STAGE + (256 + 16) * sizeof(float);
  float* const c1s = reinterpret_cast<float*>(outbuf + OUTBUF);        // C1SRC: [4 wave-private patches | scale 64 | shift 64]
  for (int i = tid; i < 64; i += THREADS) {
    epi[i] = a.scale ? a.scale[n0 + i] : 1.f;
    epi[64 + i] = a.shift ? a.shift[n0 + i] : 0.f;
    epi[128 + i] = a.w1x1 ? a.w1x1[i] : 0.f;
    epi[192 + i] = (a.scale == nullptr && a.shift != nullptr) ? a.shift[n0 + i] : 0.f;      // the accumulators' start values (see `initv`)
  }
  if constexpr (C1SRC) {
    for (int i = tid; i < 64; i += THREADS) {
      c1s[4 * C1PROWS * C1W + i] = a.c1_scale[i];
      c1s[4 * C1PROWS * C1W + 64 + i] = a.c1_shift[i];
    }
  }

  if (wave >= 4) {
    // =================================================================================================== LOADER waves
    // (tried in round 5, code retired: s_setprio for either role and in the epilogue, an s_sleep behind each halo request -- neither moved the
    //  kernel; DESIGN.md section 7, NOTES round 5)
    const int lt = tid - LTHREADS;
    const int aq = lt % SPP;
    struct Tile { int b, y0, x0; unsigned ain; unsigned t0, t1; bool interior; };   // t0 / t1: byte offset of the tile's HALO origin (pixel (-1, -1)) in source 0 / 1: may wrap
    // a thread's inside flags when the whole halo lies inside both sources (most tiles): only its padding slots (pix >= HP) are off
    unsigned ain_full = 0;
#pragma unroll
    for (int it = 0; it < A_F4; ++it) ain_full |= ((lt / SPP + it * PPI < HP) ? 1u : 0u) << it;
    ain_full |= ain_full << 16;
    auto make_tile = [&](int t) __attribute__((always_inline)) {
      Tile T;
      int bx = __builtin_amdgcn_readfirstlane(t);
      const int tx = bx % a.tiles_x; bx /= a.tiles_x;
      const int ty = bx % a.tiles_y; bx /= a.tiles_y;
      T.b = bx; T.y0 = ty * PH; T.x0 = tx * PW;
      T.t0 = (unsigned)(((T.y0 - 1) * a.W + (T.x0 - 1)) * a.C0) * 4u;
      T.t1 = (unsigned)(((T.y0 - 1 - a.oy1) * a.W1 + (T.x0 - 1 - a.ox1)) * a.C1) * 4u;
      // interior: every halo pixel inside source 0 and (if there is one) inside source 1 -- wave-uniform
      T.interior = T.y0 >= 1 && T.y0 + PH + 1 <= a.H && T.x0 >= 1 && T.x0 + PW + 1 <= a.W &&
                   (a.C1 == 0 || (T.y0 - 1 - a.oy1 >= 0 && T.y0 + PH - a.oy1 < a.H1 && T.x0 - 1 - a.ox1 >= 0 && T.x0 + PW - a.ox1 < a.W1));
      T.ain = ain_full;
      if (!T.interior) {
        T.ain = 0;
#pragma unroll
        for (int it = 0; it < A_F4; ++it) {
          const int pix = lt / SPP + it * PPI;
          const int gy = T.y0 + pix / HPW - 1, gx = T.x0 + halo_col(pix % HPW) - 1;   // (staged position -> halo column: see off0 / off1 below)
          const bool in = pix < HP && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
          const int y1 = gy - a.oy1, x1 = gx - a.ox1;
          const bool in1 = in && y1 >= 0 && y1 < a.H1 && x1 >= 0 && x1 < a.W1;
          T.ain |= (in ? 1u : 0u) << it | (in1 ? 1u : 0u) << (16 + it);
        }
      }
      return T;
    };

    const bool has_duty = a.y != nullptr || a.w1x1 != nullptr;
    // the epilogue's memory work for tile `t` out of the LDS tile the compute waves filled (see the header): the 64-channel rows as
    // 1 KB-per-wave coalesced stores (16 lanes = the 16 channel quads of a pixel, 4 pixels per wave instruction), then -- fused OutConv
    // -- one pixel per loader thread: 64 channels x their weights + bias.  The compute waves write the tile in THEIR group order: linear pixel
    // n = 32 row + column of the tile sits at LDS position m = (row >> 2) * 128 + ((column & 1) * 4 + (row & 3)) * 16 + (column >> 1), written
    // below as a per-thread part + a per-pass constant (as one expression of n hipcc kept an address pair per pass and spilled).
    auto duty = [&](int t) __attribute__((always_inline)) {
      int bx = __builtin_amdgcn_readfirstlane(t);
      const int tx = bx % a.tiles_x; bx /= a.tiles_x;
      const int ty = bx % a.tiles_y; bx /= a.tiles_y;
      const int ey0 = ty * PH, ex0 = tx * PW;
      if (a.y != nullptr && a.y_split) {
        // the SPLIT layout (mfpa_conv_desc.y_split): per pixel and 32-channel chunk [32 bf16 hi | 32 bf16 lo] -- a thread takes eight
        // channels (two pieces of the LDS tile), splits them exactly as a consumer's loader would, and stores the 16-byte hi piece and
        // the 16-byte lo piece: the next convolution's loaders only copy
        char* yb = reinterpret_cast<char*>(a.y + (size_t)bx * a.H * a.W * a.Cout + n0);
        const int kg8 = lt & 7;                                      // channels 8 kg8 .. 8 kg8 + 7 of this workgroup's 64
        const int col = lt >> 3;                                     // a pass is one tile row: m = (row >> 2) * 128 + (row & 3) * 16 + mt, m & 15 = col >> 1
        const char* const ob = outbuf + ((col & 1) * 64 + (col >> 1)) * 256;
        const int pc0 = ((2 * kg8) ^ (col >> 1)) << 4, pc1 = ((2 * kg8 + 1) ^ (col >> 1)) << 4;
        for (int pass = 0; pass < 8; pass += 2) {
          f32x4 v[2][2];
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int mrow = ((pass + u) >> 2) * 128 + ((pass + u) & 3) * 16;
            v[u][0] = *reinterpret_cast<const f32x4*>(ob + mrow * 256 + pc0);
            v[u][1] = *reinterpret_cast<const f32x4*>(ob + mrow * 256 + pc1);
          }
#pragma unroll
          for (int u = 0; u < 2; ++u) {
            const int n = (pass + u) * 32 + (lt >> 3);
            const int gy = ey0 + n / PW, gx = ex0 + n % PW;
            unsigned hi[4], lo[4];
#pragma unroll
            for (int h = 0; h < 2; ++h)
#pragma unroll
              for (int e = 0; e < 2; ++e)
                split_bf16x3(f32x2{v[u][h][2 * e], v[u][h][2 * e + 1]}, hi[2 * h + e], lo[2 * h + e]);
            if (gy < a.H && gx < a.W) {
              char* yp = yb + ((unsigned)gy * (unsigned)a.W + (unsigned)gx) * (unsigned)a.Cout * 4u + (unsigned)(kg8 >> 2) * 128u + (unsigned)(kg8 & 3) * 16u;
              *reinterpret_cast<uint4*>(yp) = uint4{hi[0], hi[1], hi[2], hi[3]};
              *reinterpret_cast<uint4*>(yp + 64) = uint4{lo[0], lo[1], lo[2], lo[3]};
            }
          }
        }
      } else if (a.y != nullptr) {
        char* yb = reinterpret_cast<char*>(a.y + (size_t)bx * a.H * a.W * a.Cout + n0);
        const int q = lt & 15, c4 = lt >> 4;
        // pass P = pass + u holds tile row P >> 1, columns (P & 1) * 16 + c4: m = (P >> 3) * 128 + ((P >> 1) & 3) * 16 + (P & 1) * 8 + mt with
        // mt = (c4 & 1) * 64 + (c4 >> 1), m & 15 = (c4 >> 1) + 8 (P & 1) -- the piece's swizzle has two values per thread
        const char* const ob0 = outbuf + ((c4 & 1) * 64 + (c4 >> 1)) * 256 + ((q ^ (c4 >> 1)) << 4);
        const char* const ob1 = outbuf + ((c4 & 1) * 64 + (c4 >> 1) + 8) * 256 + ((q ^ (c4 >> 1) ^ 8) << 4);
        for (int pass = 0; pass < 16; pass += 4) {                  // four LDS reads in flight, then their four stores
          f32x4 v[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int mrow = (pass >> 3) * 128 + (((pass >> 1) & 3) + (u >> 1)) * 16;
            v[u] = *reinterpret_cast<const f32x4*>(((u & 1) ? ob1 : ob0) + mrow * 256);
          }
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            const int n = (pass + u) * 16 + (lt >> 4);
            const int gy = ey0 + n / PW, gx = ex0 + n % PW;
            if (gy < a.H && gx < a.W) *reinterpret_cast<f32x4*>(yb + (((unsigned)gy * (unsigned)a.W + (unsigned)gx) * (unsigned)a.Cout + 4u * (unsigned)q) * 4u) = v[u];
          }
        }
      }
      if (a.w1x1 != nullptr) {
        const int m = lt;
        float sum = 0.f;
#pragma unroll 1
        for (int q0 = 0; q0 < 16; q0 += 4) {                         // (four pieces at a time: the whole row at once cost the kernel its register budget)
          f32x4 v[4], w[4];
#pragma unroll
          for (int u = 0; u < 4; ++u) {
            v[u] = *reinterpret_cast<const f32x4*>(outbuf + m * 256 + (((q0 + u) ^ (m & 15)) << 4));
            w[u] = *reinterpret_cast<const f32x4*>(epi + 128 + 4 * (q0 + u));
          }
#pragma unroll
          for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int k = 0; k < 4; ++k) sum = fmaf(v[u][k], w[u][k], sum);
        }
        // (the thread takes LDS POSITION m -- a wave instruction's 16-lane quarters keep 16 different m & 15: conflict-free -- which holds
        //  pixel (row, column) = (4 (m >> 7) + ((m >> 4) & 3), 2 (m & 15) + ((m >> 6) & 1)) of the tile)
        const int gy = ey0 + 4 * (m >> 7) + ((m >> 4) & 3), gx = ex0 + 2 * (m & 15) + ((m >> 6) & 1);
        if (gy < a.H && gx < a.W) a.y1x1[((size_t)bx * a.H + gy) * a.W + gx] = sum + a.b1x1;
      }
    };

    if constexpr (!C1SRC) {
      // a thread's staging slots map to fixed STAGED positions (pix = lt / 8 + 32 it: halo row pix / HPW, and in it halo column
      // halo_col(pix % HPW) -- the even columns, then the odd ones: mfpa_conv_tile.h); their byte offsets relative to the tile's HALO ORIGIN do
      // not depend on the tile (registers: the loader waves have room).  Raw buffer loads through a per-clip descriptor.  Edge tiles: halo
      // rows above / below the image fall outside the clip and return zero by themselves, a slot left / right of the image (or in a padded
      // column of the smaller source 1) is requested at an offset beyond the clip instead -- nothing is masked when it is split.
      unsigned off0[A_F4], off1[A_F4];                               // relative to the tile's halo origin: never negative
#pragma unroll
      for (int it = 0; it < A_F4; ++it) {
        const int pix = lt / SPP + it * PPI;
        const int py = pix / HPW, px = halo_col(pix % HPW);
        off0[it] = (unsigned)((py * a.W + px) * a.C0 + 4 * aq) * 4u;
        off1[it] = (unsigned)((py * a.W1 + px) * a.C1 + 4 * aq) * 4u;
        // a PADDING slot (pix >= HP: halo row PH + 2, which an interior tile's clip need not contain) is never inside: its VECTOR offset lies
        // beyond any clip, so the interior form's request (table entry + scalar tile offset) is out of range whether or not the range
        // check sees the scalar part; nothing reads what it returns (fragment reads stop at pixel HP - 1)
        if (pix >= HP) off0[it] = off1[it] = 0xfffffff0u;
      }
      const unsigned clip0 = (unsigned)a.H * (unsigned)a.W * (unsigned)a.C0 * 4u, clip1 = (unsigned)a.H1 * (unsigned)a.W1 * (unsigned)a.C1 * 4u;
      f32x4 areg[2][A_F4] = {};                                        // two staging sets: chunk k + 1 is split out of one while chunk k + 2 lands in the other
      // what a chunk's loads need besides the per-slot offsets: the clip's buffer descriptor, the tile-origin + channel offset, which offset
      // table (source 0 / 1) and where its inside flags sit -- wave-uniform, formed ONCE per turn
      struct Src { __amdgpu_buffer_rsrc_t rs; unsigned toff; bool from0; int ainsh; };
      auto make_src = [&](const Tile& T, int chunk) __attribute__((always_inline)) {
        Src S;
        const int c0 = chunk * KC;
        S.from0 = c0 < a.C0;
        const char* pb = reinterpret_cast<const char*>(S.from0 ? a.x0 : a.x1) + (size_t)T.b * (S.from0 ? clip0 : clip1);
        S.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pb), 0, (int)(S.from0 ? clip0 : clip1), 0x00020000);
        S.toff = S.from0 ? T.t0 + (unsigned)c0 * 4u : T.t1 + (unsigned)(c0 - a.C0) * 4u;
        S.ainsh = S.from0 ? 0 : 16;
        return S;
      };
      // a slot outside the image (left / right of it, or a padded column of the smaller source 1) is requested at an offset beyond the
      // clip: the buffer load returns zeros and the split needs no masking (rows above / below fall outside by themselves)
      auto issue_slot = [&](const Src& S, unsigned ain, auto SET, auto IT) __attribute__((always_inline)) {
        constexpr int it = decltype(IT)::value, set = decltype(SET)::value;
        unsigned o0 = off0[it], o1 = off1[it];
        asm("" : "+v"(o0), "+v"(o1));                                  // two VALUES, then a select (as `from0 ? off0[it] : off1[it]` hipcc indexed a selected
                                                                       // array base: both arrays went to scratch, a scratch load in front of every halo load)
        const bool inside = (ain >> (S.ainsh + it)) & 1u;
        const unsigned off = inside ? (S.from0 ? o0 : o1) + S.toff : 0xfffffff0u;
        areg[set][it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(S.rs, (int)off, 0, 0));
      };
      // interior tiles (no slot to zero): the table entry is the vector offset as it stands, the tile / channel offset rides in the
      // instruction's scalar offset -- no vector instruction at all per request
      auto issue_slot_interior = [&](const Src& S, auto FROM0, auto SET, auto IT) __attribute__((always_inline)) {
        constexpr int it = decltype(IT)::value, set = decltype(SET)::value;
        areg[set][it] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(S.rs, (int)(decltype(FROM0)::value ? off0[it] : off1[it]), (int)S.toff, 0));
      };
      // one staging slot: bf16 hi / lo split, two 8-byte stores into the (hi, k-group) and (lo, k-group) planes
      char* const wbase = smem + plane_off(0, aq >> 1) + (lt / SPP) * 16 + 8 * (aq & 1);
      // (a source in the SPLIT layout -- mfpa_conv_desc.x0_split / x1_split -- needs none of this: its 16 bytes at the very same offset ARE
      //  the (hi | lo, k-group) piece aq = 4 hl + kg of the pixel: one 16-byte store)
      char* const wbase_split = smem + plane_off(aq >> 2, aq & 3) + (lt / SPP) * 16;
      auto copy_slot = [&](auto SET, auto IT, int stage_off) __attribute__((always_inline)) {
        constexpr int it = decltype(IT)::value, set = decltype(SET)::value;
        *reinterpret_cast<f32x4*>(wbase_split + stage_off + it * PPI * 16) = areg[set][it];
      };
      auto split_slot = [&](auto SET, auto IT, int stage_off) __attribute__((always_inline)) {
        constexpr int it = decltype(IT)::value, set = decltype(SET)::value;
        const f32x4 v = areg[set][it];
        unsigned hi[2], lo[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) split_bf16x3(f32x2{v[2 * h], v[2 * h + 1]}, hi[h], lo[h]);
        char* at = wbase + stage_off + it * PPI * 16;
        *reinterpret_cast<uint2*>(at) = uint2{hi[0], hi[1]};
        *reinterpret_cast<uint2*>(at + HLS) = uint2{lo[0], lo[1]};
      };
      auto issue_all = [&](const Src& S, unsigned ain, bool interior, auto SET) __attribute__((always_inline)) {
        if (interior) {
          if (S.from0) each_index<A_F4>([&](auto IT) __attribute__((always_inline)) { issue_slot_interior(S, std::true_type{}, SET, IT); });
          else each_index<A_F4>([&](auto IT) __attribute__((always_inline)) { issue_slot_interior(S, std::false_type{}, SET, IT); });
          return;
        }
        each_index<A_F4>([&](auto IT) __attribute__((always_inline)) { issue_slot(S, ain, SET, IT); });
      };
      auto split_all = [&](auto SET, int stage_off, bool src_split) __attribute__((always_inline)) {
        if (src_split) {
          each_index<A_F4>([&](auto IT) __attribute__((always_inline)) { copy_slot(SET, IT, stage_off); });
          return;
        }
        each_index<A_F4>([&](auto IT) __attribute__((always_inline)) { split_slot(SET, IT, stage_off); });
      };
      // the chunk sequence of this workgroup: (tile i, chunk c), c fastest.  Q = the next chunk to REQUEST.
      int qi = 0, qc = 0;
      Tile TQ = make_tile(tile_of((int)blockIdx.x, 0, G));
      auto issue_next = [&](auto SET) __attribute__((always_inline)) {
        const Src S = make_src(TQ, qc);
        issue_all(S, TQ.ain, TQ.interior, SET);
        if (++qc == nchunks) {
          qc = 0; ++qi;
          if (qi < owned) TQ = make_tile(tile_of((int)blockIdx.x, qi, G));
        }
      };
      using SET0 = std::integral_constant<int, 0>;
      using SET1 = std::integral_constant<int, 1>;
      issue_next(SET0{});                                              // chunk 0 -> set 0
      int par = 0;
      const int total = owned * nchunks;                               // chunks this workgroup computes
      // iteration k = -1 (prologue: chunk 0 -> stage 0, then the barrier that starts the compute waves), then k = 0 .. total - 1: while
      // the compute waves work on chunk k the loaders REQUEST chunk k + 2 into set k & 1 and then split chunk k + 1 out of the other set
      // (requested one iteration ago: a whole chunk period in flight) into the stage the compute waves read next.  The output tile of
      // tile i (last chunk k_i = (i + 1) nchunks - 1) is written by the compute waves between barriers k_i and k_i + 1, so it is read
      // here in iteration k_i + 2 -- and once more after the last barrier for the last tile; the compute waves write the next one after
      // barrier k_i + nchunks >= k_i + 2, which the loaders reach only when that iteration's work is done.
      // is chunk number kk of this workgroup's sequence read from a source in the split layout?  (wave-uniform)
      auto src_split_of = [&](int kk) __attribute__((always_inline)) {
        const int c0 = (kk % nchunks) * KC;
        return (c0 < a.C0 ? a.x0_split : a.x1_split) != 0;
      };
      auto iteration = [&](int k, auto ISSUE_SET, auto SPLIT_SET) __attribute__((always_inline)) {
        if (k + 2 < total) issue_next(ISSUE_SET);
        __builtin_amdgcn_sched_barrier(0);                             // the requests first: hipcc sank them below the split
        if (k + 1 < total) split_all(SPLIT_SET, par * STAGE, src_split_of(k + 1));
        if (has_duty && k >= nchunks + 1 && (k - 1) % nchunks == 0) duty(tile_of((int)blockIdx.x, (k - 1) / nchunks - 1, G));
        __syncthreads();                                               // k = -1: stage 0 is ready; k >= 0: the compute waves' barrier of chunk k
        par ^= 1;
      };
      for (int k = -1; k < total; k += 2) {
        iteration(k, SET1{}, SET0{});                                  // odd k (and -1): chunk k + 2 is odd
        if (k + 1 < total) iteration(k + 1, SET0{}, SET1{});
      }
      if (has_duty) {
        // the last tile's read-out iteration lies beyond the loop (every other tile's does not: nchunks >= 2)
        __syncthreads();                                               // the compute waves' final barrier: the last tile's output is in LDS
        duty(tile_of((int)blockIdx.x, owned - 1, G));
      }
    } else {
      // ---- C1SRC: the 64 input channels are COMPUTED here -- the UNet's first layer (Conv2d(1, 64, 3, padding 1, bias False) + folded
      // BatchNorm + ReLU, training/unet.py:16-18) on the matrix cores.  The 340 halo pixels are 22 tiles of 16; loader wave w owns
      // tiles [6, 6, 5, 5] and keeps its own copy of the <= 6 source rows they need (no hand-off between the loader waves).  Per
      // (16-channel tile, 16-pixel tile): D[channel][pixel] = W[16 x K] . P[K x 16] with K = the nine taps padded to 16
      // (v_mfma_f32_16x16x16_bf16, bf16x3: three instructions of 8 cycles), then scale / shift / ReLU, zero outside the image (the second
      // layer's zero padding), bf16 hi | lo split and the same two 8-byte plane stores as the generic loader.  48 MFMAs per chunk and wave
      // against ~1300 vector instructions per chunk and thread in conv_mfma_kernel<.., C1SRC>'s loader.
      typedef short s16x4 __attribute__((ext_vector_type(4)));
      const int lw = wave - 4;
      const int pt0 = lw < 2 ? 6 * lw : 12 + 5 * (lw - 2), npt = lw < 2 ? 6 : 5;
      const int hr0 = (pt0 * 16) / HPW;                                  // first halo row of this wave's pixels = first patch row it keeps
      float* const patch = c1s + lw * (C1PROWS * C1W);
      const float* const c1c = c1s + 4 * C1PROWS * C1W;
      const int g = lane >> 4, p = lane & 15;
      // (a local wrapper on purpose: with split_bf16x3 called directly at the six sites hipcc allocates this kernel's registers differently)
      auto split2 = [&](float x0_, float x1_, unsigned& hi, unsigned& lo) __attribute__((always_inline)) { split_bf16x3(f32x2{x0_, x1_}, hi, lo); };
      // the first layer's weights as the A operand: lane (g, c) = channel 16 t + c, k = 4 g .. 4 g + 3 (tap k, zero from tap 9 on)
      s16x4 Ahi[4], Alo[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float w4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 4 * g + j;
          w4[j] = k < 9 ? a.c1_w[k * 64 + 16 * t + p] : 0.f;
        }
        unsigned h0, l0, h1, l1;
        split2(w4[0], w4[1], h0, l0);
        split2(w4[2], w4[3], h1, l1);
        Ahi[t] = __builtin_bit_cast(s16x4, uint2{h0, h1});
        Alo[t] = __builtin_bit_cast(s16x4, uint2{l0, l1});
      }
      // per lane, tile-independent: where pixel p of pixel tile t sits in the wave's patch (tap (0, 0)), its halo coordinates, and the
      // patch displacement of the lane's four taps.  A pixel tile is 16 consecutive STAGED positions hp (the generic loader's order: halo
      // row hp / HPW, halo column halo_col(hp % HPW)), so produce() stores pixel p of tile t at position (pt0 + t) * 16 + p as it stands.
      int pbase[6], pyx[6];
#pragma unroll
      for (int t = 0; t < 6; ++t) {
        const int hp = (pt0 + (t < npt ? t : 0)) * 16 + p;
        const int py = hp / HPW, px = halo_col(hp % HPW);
        pbase[t] = (py - hr0) * C1W + px;
        pyx[t] = (py << 8) | px | (hp < HP ? 0 : 0x10000);
      }
      int koff[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 4 * g + j;
        koff[j] = k < 9 ? (k / 3) * C1W + (k % 3) : -1;
      }
      // the wave's patch elements a lane carries from request to commit: i = lane + 64 j < 6 x 36
      double pvd[4];
      float pvf[4];
      unsigned pin = 0;
      double pden = 1.0;
      auto request_patch = [&](int t) __attribute__((always_inline)) {
        int bx = __builtin_amdgcn_readfirstlane(t);
        const int tx = bx % a.tiles_x; bx /= a.tiles_x;
        const int ty = bx % a.tiles_y; bx /= a.tiles_y;
        const int y0 = ty * PH, x0 = tx * PW;
        pden = a.c1_denom ? a.c1_denom[bx] : 1.0;
        pin = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = lane + 64 * j;
          const int gy = y0 - 2 + hr0 + i / C1W, gx = x0 - 2 + i % C1W;
          const bool in = i < C1PROWS * C1W && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
          pin |= (in ? 1u : 0u) << j;
          const size_t o = ((size_t)bx * a.H + min(max(gy, 0), a.H - 1)) * a.W + min(max(gx, 0), a.W - 1);      // clamped: the load is unconditional
          if (a.c1_spec64) pvd[j] = a.c1_spec64[o];
          else pvf[j] = a.c1_x32[o];
        }
      };
      auto commit_patch = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int i = lane + 64 * j;
          const float v = a.c1_spec64 ? (float)(pvd[j] / pden) : pvf[j];          // the fused spectrogram normalisation (peak_extractor.py:263-265)
          if (i < C1PROWS * C1W) patch[i] = ((pin >> j) & 1u) ? v : 0.f;            // zero = the first layer's own padding
        }
      };
      s16x4 Bh[6], Bl[6];
      unsigned inside = 0;                                             // bit t: pixel p of pixel tile t lies inside the image
      auto build_b = [&](int t) __attribute__((always_inline)) {
        int bx = __builtin_amdgcn_readfirstlane(t);
        const int tx = bx % a.tiles_x; bx /= a.tiles_x;
        const int ty = bx % a.tiles_y;
        const int y0 = ty * PH, x0 = tx * PW;
        inside = 0;
#pragma unroll
        for (int tt = 0; tt < 6; ++tt) {
          float v4[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) v4[j] = koff[j] >= 0 ? patch[pbase[tt] + koff[j]] : 0.f;
          unsigned h0, l0, h1, l1;
          split2(v4[0], v4[1], h0, l0);
          split2(v4[2], v4[3], h1, l1);
          Bh[tt] = __builtin_bit_cast(s16x4, uint2{h0, h1});
          Bl[tt] = __builtin_bit_cast(s16x4, uint2{l0, l1});
          const int gy = y0 - 1 + (pyx[tt] >> 8 & 0xff), gx = x0 - 1 + (pyx[tt] & 0xff);
          const bool in = !(pyx[tt] & 0x10000) && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
          inside |= (in ? 1u : 0u) << tt;
        }
      };
      // channels [32 c, 32 c + 32) of the current tile into the stage at `stage_off`
      auto produce = [&](int c, int stage_off) __attribute__((always_inline)) {
#pragma unroll
        for (int cth = 0; cth < 2; ++cth) {
          const int ct = 2 * c + cth;
          const f32x4 sc = *reinterpret_cast<const f32x4*>(c1c + 16 * ct + 4 * g);
          const f32x4 sh = *reinterpret_cast<const f32x4*>(c1c + 64 + 16 * ct + 4 * g);
          const s16x4 ah = c ? (cth ? Ahi[3] : Ahi[2]) : (cth ? Ahi[1] : Ahi[0]);
          const s16x4 al = c ? (cth ? Alo[3] : Alo[2]) : (cth ? Alo[1] : Alo[0]);
#pragma unroll
          for (int tt = 0; tt < 6; ++tt) {
            if (tt >= npt) continue;
            floatx4 d = {0.f, 0.f, 0.f, 0.f};
            d = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(al, Bh[tt], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, Bl[tt], d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(ah, Bh[tt], d, 0, 0, 0);
            const bool in = (inside >> tt) & 1u;
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = in ? fmaxf(fmaf(d[j], sc[j], sh[j]), 0.f) : 0.f;
            unsigned h0, l0, h1, l1;
            split2(v[0], v[1], h0, l0);
            split2(v[2], v[3], h1, l1);
            // channels 16 ct + 4 g .. + 3 of pixel hp: k-group (ct & 1) * 2 + (g >> 1) of the chunk, half g & 1 of its 16-byte piece
            char* at = smem + stage_off + plane_off(0, cth * 2 + (g >> 1)) + ((pt0 + tt) * 16 + p) * 16 + 8 * (g & 1);
            *reinterpret_cast<uint2*>(at) = uint2{h0, h1};
            *reinterpret_cast<uint2*>(at + HLS) = uint2{l0, l1};
          }
        }
      };
      const int total = owned * 2;                                     // two chunks per tile
      int par = 0;
      request_patch(tile_of((int)blockIdx.x, 0, G));
      for (int k = -1; k < total; ++k) {
        if (k + 1 < total) {
          const int i = (k + 1) >> 1, c = (k + 1) & 1;
          if (c == 0) {
            commit_patch();                                            // (wave-private copy: the wave's own DS instructions execute in order)
            build_b(tile_of((int)blockIdx.x, i, G));
            if (i + 1 < owned) request_patch(tile_of((int)blockIdx.x, i + 1, G));
          }
          produce(c, par * STAGE);
        }
        if (has_duty && k >= 3 && (k - 1) % 2 == 0) duty(tile_of((int)blockIdx.x, (k - 1) / 2 - 1, G));
        __syncthreads();
        par ^= 1;
      }
      if (has_duty) {
        __syncthreads();
        duty(tile_of((int)blockIdx.x, owned - 1, G));
      }
    }
    return;
  }

  // ===================================================================================================== COMPUTE waves
  const int wm = wave & 1, wn = wave >> 1;                             // pixel half (rows 4 wm .. 4 wm + 3), channel half
  const int p = lane & 15, g = lane >> 4;

  bf16x8 wq[3][2][2];                                                  // weight fragments: ring of three sets, [slot][16-channel tile][hi, lo]
  // through raw buffer loads, as in conv_up_kernel: the image's descriptor in scalar registers, ONE vector offset (lane * 16) for every load,
  // the (tap, chunk, channel-tile) block offset in the instruction's scalar offset -- no 64-bit vector address per request
  const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.w), 0, (int)(9u * (unsigned)a.Cout * (unsigned)Cin * 4u), 0x00020000);
  const unsigned wrow = (unsigned)(a.Cout / 16), wcol = (unsigned)(n0 / 16 + 2 * wn);
  const int wlane = lane * 16;
  auto load_w = [&](int chunk, int tap, auto SLOT) __attribute__((always_inline)) {
    constexpr int slot = decltype(SLOT)::value;
    const int so = (int)__builtin_amdgcn_readfirstlane((int)((((unsigned)tap * (unsigned)nchunks + (unsigned)chunk) * wrow + wcol) << 11));
    wq[slot][0][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane, so, 0));
    wq[slot][0][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane + 1024, so, 0));
    wq[slot][1][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane + 2048, so, 0));
    wq[slot][1][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs_w, wlane + 3072, so, 0));
  };
  struct XFrags { bf16x8 h[4], l[4]; };
  XFrags fx[2];
  // Pixel group pt = 4 px + j of the wave: tile row 4 wm + j, columns 2 p + px (conv_up_kernel's order: 16 pixels two columns apart).  Its
  // fragment at tap (ta, tb) is halo row 4 wm + j + ta, halo column 2 p + s with s = px + tb -> staged position (s & 1) * HALF + (s >> 1) + p
  // of that row: only s enters the address, so the column-odd groups at tap (ta, tb) and the column-even groups at tap (ta, tb + 1) read the
  // same bytes, and a tap row's six half-steps read FOUR distinct fragment sets s = 0 .. 3 (feeding 1, 2, 2, 1 consecutive half-steps) --
  // 12 sets of eight reads per chunk, not 18.  Set d = 4 ta + s of a chunk lives in fx[d & 1] (twelve sets: every chunk starts in fx[0]).
  // The next set's eight reads go under the half-steps that use the current one: all under a sole user, groups 0, 1 / 2, 3 under a first /
  // second user.  Which pixels share an instruction does not enter a pixel's sum: the outputs are bit for bit those of one read per half-step.
  const int xbase = ((4 * wm) * HPW + p) * 16 + plane_off(0, g);      // the lane's piece of row-0 group at set (0, 0) in plane (hi, g)
  constexpr int R_ALL = 0, R_FIRST = 1, R_SECOND = 2;                  // which groups of a set one half-step reads: 0 .. 3, 0 .. 1, 2 .. 3
  auto read_set = [&](XFrags& f, const char* stage, auto TA, auto S, auto PART) __attribute__((always_inline)) {
    constexpr int ta = decltype(TA)::value, s = decltype(S)::value, part = decltype(PART)::value;
#pragma unroll
    for (int j = (part == R_SECOND ? 2 : 0); j < (part == R_FIRST ? 2 : 4); ++j) {
      const char* r = stage + xbase + ((ta + j) * HPW + (s & 1) * HALF + (s >> 1)) * 16;
      f.l[j] = *reinterpret_cast<const bf16x8*>(r + HLS);
      f.h[j] = *reinterpret_cast<const bf16x8*>(r);
    }
  };
  floatx4 acc[2][PT];                                                  // per tile they start as the C operand of their first MFMA (see `initv`); the one
#pragma unroll                                                         // initialisation here only gives the values a definition (left undefined, their
  for (int ct = 0; ct < 2; ++ct)                                       // live ranges reached back to the kernel's entry and the prologue spilled)
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = floatx4{0.f, 0.f, 0.f, 0.f};
  // accumulator start values: zero -- or, when the output scale is folded into the weights (a.scale == nullptr), the per-channel shift, so
  // that the epilogue is a bare ReLU.  They enter as the C operand of an accumulator's FIRST MFMA of a tile (tap 0 of chunk 0 is its own
  // code: FIRST), so no accumulator is ever initialised by vector moves.  (Filled behind the first barrier: `epi` is written above.)
  floatx4 initv[2];
  auto mfma_half = [&](const XFrags& f, const bf16x8 (&w)[2][2], auto HALFI, auto FIRST) __attribute__((always_inline)) {
    constexpr int half = decltype(HALFI)::value;                       // column parity px of the four groups
    // term-major (lo x hi, hi x lo, hi x hi -- conv_wd16_kernel's order: bit-identical sums): an accumulator is touched every eighth instruction
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][1], f.h[i], decltype(FIRST)::value ? initv[ct] : acc[ct][4 * half + i], 0, 0, 0);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][0], f.l[i], acc[ct][4 * half + i], 0, 0, 0);
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[ct][4 * half + i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[ct][0], f.h[i], acc[ct][4 * half + i], 0, 0, 0);
  };
  constexpr int N_M = 24, N_W = 4;                                     // MFMAs of one half-step, weight loads of one tap
  using I0 = std::integral_constant<int, 0>;
  using I1 = std::integral_constant<int, 1>;
  using RAll = std::integral_constant<int, R_ALL>;
  using RFirst = std::integral_constant<int, R_FIRST>;
  using RSecond = std::integral_constant<int, R_SECOND>;
  // One tap (ta, tb), b = tb & 1.  Half A (column-even groups, set s = tb in fx[b]): MFMA || read set s + 1 into fx[b ^ 1] -- all of it when
  // tb = 0 (set 0 has this one user), else groups 2, 3 (half B of the previous tap read groups 0, 1) -- and request the weights of tap t + 2.
  // Half B (column-odd groups, set s = tb + 1 in fx[b ^ 1]): MFMA || read groups 0, 1 of set s + 1 into fx[b], or, when tb = 2 (set 3 has this
  // one user), all of the next tap row's set 0.  The chunk's one barrier sits between the halves of tap 8: behind it the other stage is
  // complete (the loaders arrived) and this one is read out (every compute wave's fragment reads of it have returned: lgkmcnt(0) in front of
  // it); half B of tap 8 reads the next chunk's set 0 out of that other stage.
  int kpar = 0;                                                        // parity of the stage the current chunk is read from
  auto tap_body = [&](auto TAP, int chunk, auto FIRST) __attribute__((always_inline)) {
    constexpr int tap = decltype(TAP)::value, ta = tap / 3, tb = tap % 3, b = tb & 1;
    using TA = std::integral_constant<int, ta>;
    using PART_A = std::conditional_t<tb == 0, RAll, RSecond>;
    using PART_B = std::conditional_t<tb == 2, RAll, RFirst>;
    constexpr int n_ra = tb == 0 ? 8 : 4, n_rb = tb == 2 ? 8 : 4;      // fragment reads (16 bytes each) under half A / half B
    const int chunk_n = chunk + 1 < nchunks ? chunk + 1 : 0;
    const char* cur = smem + kpar * STAGE;
    read_set(fx[b ^ 1], cur, TA{}, std::integral_constant<int, tb + 1>{}, PART_A{});
    mfma_half(fx[b], wq[tap % 3], I0{}, FIRST);
    load_w((tap + 2 >= TAPS) ? chunk_n : chunk, (tap + 2) % TAPS, std::integral_constant<int, (tap + 2) % 3>{});
    pin_reads<N_M - 1, n_ra>();
    constexpr int used_a = pin_read_slots(N_M - 1, n_ra);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, N_W, 0);
    if constexpr (N_M - used_a - 1 > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - used_a - 1, 0);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (tap == TAPS - 1) {
      __syncthreads();                                                 // (tried instead in round 5, code retired: hand-offs through LDS progress counters
                                                                       //  with no barrier in the loop -- did not move the kernel; DESIGN.md section 7, NOTES round 5)
      __builtin_amdgcn_sched_barrier(0);
      read_set(fx[b], smem + (kpar ^ 1) * STAGE, I0{}, I0{}, RAll{});
    } else if constexpr (tb == 2) {
      read_set(fx[b], cur, std::integral_constant<int, ta + 1>{}, I0{}, RAll{});
    } else {
      read_set(fx[b], cur, TA{}, std::integral_constant<int, tb + 2>{}, RFirst{});
    }
    mfma_half(fx[b ^ 1], wq[tap % 3], I1{}, FIRST);
    pin_reads<N_M, n_rb>();
    if constexpr (N_M - pin_read_slots(N_M, n_rb) > 0) __builtin_amdgcn_sched_group_barrier(0x008, N_M - pin_read_slots(N_M, n_rb), 0);
    __builtin_amdgcn_sched_barrier(0);
  };

  load_w(0, 0, std::integral_constant<int, 0>{});
  load_w(0, 1, std::integral_constant<int, 1>{});
  __syncthreads();                                                     // stage 0 holds chunk 0 of the first tile
  read_set(fx[0], smem, I0{}, I0{}, RAll{});
  for (int ti = 0; ti < owned; ++ti) {
    int bx = __builtin_amdgcn_readfirstlane(tile_of((int)blockIdx.x, ti, G));
    const int tx = bx % a.tiles_x; bx /= a.tiles_x;
    const int ty = bx % a.tiles_y; bx /= a.tiles_y;
    const int eb = bx, ey0 = ty * PH, ex0 = tx * PW;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {                                   // (per tile, out of LDS: eight registers live for one tap instead of the whole kernel)
      const f32x4 iv = *reinterpret_cast<const f32x4*>(epi + 192 + wn * 32 + ct * 16 + 4 * g);
      initv[ct] = floatx4{iv[0], iv[1], iv[2], iv[3]};
    }
    // chunk 0 is its own copy of the nine taps (its tap 0 starts the accumulators): inside ONE loop body the two forms of tap 0 were a
    // branch diamond across which hipcc spilled 62 registers
    auto chunk_body = [&](int chunk, auto FIRST) __attribute__((always_inline)) {
      tap_body(std::integral_constant<int, 0>{}, chunk, FIRST);
      each_index<TAPS - 1, 1>([&](auto TAP) __attribute__((always_inline)) { tap_body(TAP, chunk, std::false_type{}); });
      kpar ^= 1;
    };
    chunk_body(0, std::true_type{});
    for (int chunk = 1; chunk < nchunks; ++chunk) chunk_body(chunk, std::false_type{});
    // ---- epilogue: D[channel 4 g + j of tile ct][pixel p of tile pt]: out = relu(acc * scale + shift) -- or relu(acc) when the scale is in
    // the weights and the shift in the accumulators' start values.  ReLU as max(v, 0): NaN -> 0 like `v > 0 ? v : 0`; without ReLU nothing
    // touches the value (a NaN stays a NaN, as in the other kernels).
    if (a.scale != nullptr) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const int chl = wn * 32 + ct * 16 + 4 * g;
        const f32x4 sc = *reinterpret_cast<const f32x4*>(epi + chl);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(epi + 64 + chl);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ct][pt][j] = fmaf(acc[ct][pt][j], sc[j], sh[j]);
      }
    }
    if (a.relu) {
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt)
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[ct][pt][j] = fmaxf(acc[ct][pt][j], 0.f);
    }
    if (a.y != nullptr || a.w1x1 != nullptr) {
      // the tile goes to LDS as 16-byte pieces (position m = the wave's group order, channel quad q) at m * 256 + ((q ^ (m & 15)) << 4): a wave
      // instruction's 16 pixels of one quad hit 16 different 16-byte bank groups; the loaders un-permute (their `duty`), store it and form
      // the fused OutConv one barrier from now
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        const int m = wm * 128 + pt * 16 + p;                          // m & 15 == p
        char* row = outbuf + m * 256;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
          const int q = wn * 8 + ct * 4 + g;
          f32x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = acc[ct][pt][j];
          *reinterpret_cast<f32x4*>(row + ((q ^ p) << 4)) = o;
        }
      }
    }
    if (a.y_pool != nullptr) {
      // MaxPool2d(2) (floor): the window's two rows are two of the wave's pixel groups, its two columns (2 p, 2 p + 1) the same lane of the
      // column-even and the column-odd group of a row: four accumulators of one lane, every lane stores a pooled pixel.  (max over the rows
      // first, then over the columns, the even column's value first: the order of the DPP form this replaces)
      const int Ho = a.H / 2, Wo = a.W / 2;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int r = 0; r < 4; r += 2) {                               // tile rows 4 wm + r, + 1
          f32x4 v;
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = fmaxf(fmaxf(acc[ct][r][j], acc[ct][r + 1][j]), fmaxf(acc[ct][4 + r][j], acc[ct][4 + r + 1][j]));
          const int py = (ey0 + 4 * wm + r) / 2, px = ex0 / 2 + p;
          if (py < Ho && px < Wo) {
            float* pp = a.y_pool + (((size_t)eb * Ho + py) * Wo + px) * a.Cout + n0 + wn * 32;       // this pixel's 32-channel chunk (128 bytes)
            if (a.y_pool_split) {
              // split layout: channels 16 ct + 4 g .. + 3 of the chunk = half (g & 1) of k-group 2 ct + (g >> 1): 8 bytes of hi, 8 of lo
              unsigned hi[2], lo[2];
#pragma unroll
              for (int e = 0; e < 2; ++e) split_bf16x3(f32x2{v[2 * e], v[2 * e + 1]}, hi[e], lo[e]);
              char* at = reinterpret_cast<char*>(pp) + (2 * ct + (g >> 1)) * 16 + 8 * (g & 1);
              *reinterpret_cast<uint2*>(at) = uint2{hi[0], hi[1]};
              *reinterpret_cast<uint2*>(at + 64) = uint2{lo[0], lo[1]};
            } else {
              *reinterpret_cast<f32x4*>(pp + ct * 16 + 4 * g) = v;
            }
          }
        }
    }
  }
  if (a.y != nullptr || a.w1x1 != nullptr) __syncthreads();          // the last tile's output is in LDS: the loaders store it
}

}  // namespace

bool conv_ws64_serves(const ConvArgs& a) {
  const bool c1 = a.c1_x32 != nullptr || a.c1_spec64 != nullptr;
  if (a.Cout % 64 != 0 || (a.w1x1 != nullptr && a.Cout != 64) || a.w_frag != 2 || a.plain || a.in16 || a.in_scale0 || a.drop_thresh) return false;
  if (a.x0_bf16 || a.x1_bf16 || a.y_bf16 || a.stats_part || a.bz) return false;           // the training step's side outputs: conv_wd16_kernel<SIDE>
  if (a.yH != a.H || a.yW != a.W || a.W <= 16 || a.H < 8) return false;
  // (a slot outside the image is requested at byte offset 0xfffffff0: it must lie beyond a clip)
  // ... and an edge tile's halo origin is a WRAPPED negative offset (up to (W + 1) pixels in front of the clip): with a halo row's span added
  // it must still lie beyond the clip, never inside it
  if (4ull * a.H * a.W * a.C0 + 4ull * (a.W + 2) * (unsigned long long)a.C0 * 2ull >= 0xfffffff0ull ||
      4ull * a.H1 * a.W1 * a.C1 + 4ull * (a.W1 + 2) * (unsigned long long)a.C1 * 2ull >= 0xfffffff0ull) return false;
  if (36ull * a.Cout * (unsigned long long)(a.C0 + a.C1) >= 0x7fffffffull) return false;    // the weight image's buffer descriptor and 32-bit block offsets
  if (c1 && (a.C0 != 64 || a.C1 != 0 || a.Cout != 64 || a.w1x1 != nullptr || !a.c1_w || !a.c1_scale || !a.c1_shift)) return false;
  const long long ntiles = (long long)((a.W + PW - 1) / PW) * ((a.H + PH - 1) / PH) * a.B;
  if (ntiles > 0x7fffffffLL / 2) return false;                         // (tile_of's round arithmetic stays inside 31 bits; conv_wd16_kernel takes those)
  return a.C0 % KC == 0 && a.C1 % KC == 0 && a.C0 + a.C1 >= 64;
}

// (the caller has asked conv_ws64_serves: conv_route of csrc/unet.hip)
template <bool C1SRC>
int launch_conv_ws64(ConvArgs& a, hipStream_t s) {
  a.tiles_x = (a.W + PW - 1) / PW;
  a.tiles_y = (a.H + PH - 1) / PH;
  const long long ntiles = (long long)a.tiles_x * a.tiles_y * a.B;
  const size_t lds = 2 * (size_t)STAGE + (256 + 16) * sizeof(float) + (size_t)OUTBUF + (C1SRC ? (size_t)C1LDS : 0);
  const int cus = mfpa_current_device_cus();
  const unsigned gy = (unsigned)(a.Cout / 64);
  unsigned gx = (unsigned)(cus > 0 ? cus : 256) / gy;
  if (gx < 1) gx = 1;
  if ((long long)gx > ntiles) gx = (unsigned)ntiles;
  hipLaunchKernelGGL((conv_ws64_kernel<C1SRC>), dim3(gx, gy), dim3(THREADS), lds, s, a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
template int launch_conv_ws64<false>(ConvArgs&, hipStream_t);
template int launch_conv_ws64<true>(ConvArgs&, hipStream_t);

}  // namespace mfpa_unet
