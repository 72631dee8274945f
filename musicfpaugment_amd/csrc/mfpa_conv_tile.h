// What the MFMA convolution sources share: the vector types (csrc/unet.hip, unet_mfma.hip, unet_wd16.hip, unet_ws.hip, unet_up.hip), the chunk width KC,
// the DPP row-shift add of the fused reductions (unet_mfma.hip, unet_wd16.hip), the "one MFMA, then k LDS reads"
// scheduling pattern (also csrc/demucs_gemm.hip, with the vector types; csrc/lstm.hip and csrc/demucs_train.hip take the types too), the bf16 hi | lo split of the bf16x3 products, a compile-time index loop, and -- namespace
// mfpa_tile::role_split -- the tile geometry and LDS plane layout of the two role-split kernels (conv_ws64_kernel, conv_up_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace mfpa_tile {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr int KC = 32;        // channels per K chunk of every convolution kernel of the UNet family (and of the routing's divisibility rules)

template <int CTRL>
__device__ __forceinline__ float dpp_row_add(float v) {               // v + (v of the lane CTRL names; 0 where there is none)
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}

// sched_group_barrier pattern "one MFMA, then k LDS reads" with LEFT reads spread evenly over SLOTS MFMAs
template <int SLOTS, int LEFT, int I = 0>
__device__ __forceinline__ void pin_reads() {
  if constexpr (I < SLOTS && LEFT > 0) {
    constexpr int k = (LEFT + (SLOTS - I) - 1) / (SLOTS - I);
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, k, 0);
    pin_reads<SLOTS, LEFT - k, I + 1>();
  }
}
constexpr int pin_read_slots(int slots, int left) {      // how many MFMAs pin_reads placed
  int used = 0;
  for (int i = 0; i < slots && left > 0; ++i) {
    left -= (left + (slots - i) - 1) / (slots - i);
    ++used;
  }
  return used;
}

// bf16x3 operand split of a channel pair, x = hi + lo: one packed conversion, the two hi values back as floats by a shift and a mask, two
// subtractions, one packed conversion.  hi / lo each hold the pair as two packed bf16.
__device__ __forceinline__ void split_bf16x3(f32x2 x, unsigned& hi, unsigned& lo) {
  hi = __builtin_bit_cast(unsigned, __builtin_convertvector(x, bf16x2));
  const f32x2 r = {x[0] - __uint_as_float(hi << 16), x[1] - __uint_as_float(hi & 0xffff0000u)};
  lo = __builtin_bit_cast(unsigned, __builtin_convertvector(r, bf16x2));
}

// the bf16x3 product of one tile: lo.hi, hi.lo, hi.hi (small terms first; the order is part of the arithmetic model of tests/_gemm_oracle.py and of
// the exact-operand tests).  csrc/demucs_gemm.hip's seven bf16x3 kernels and convT_mfma_kernel (csrc/unet_mfma.hip); conv_mfma_kernel runs the same
// three terms over all of a wave's tiles each (its mfma_terms).
__device__ __forceinline__ void mfma_bf16x3(floatx16& acc, bf16x8 ah, bf16x8 al, bf16x8 bh, bf16x8 bl) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
}

// f(integral_constant<int, FIRST>{}, a...), ..., f(integral_constant<int, FIRST + N - 1>{}, a...): straight-line code, the index a compile-time
// constant
template <int FIRST, class F, int... I, class... A>
__device__ __forceinline__ void each_index_impl(F&& f, std::integer_sequence<int, I...>, A&&... a) {
  (f(std::integral_constant<int, FIRST + I>{}, a...), ...);
}
template <int N, int FIRST = 0, class F, class... A>
__device__ __forceinline__ void each_index(F&& f, A&&... a) {
  each_index_impl<FIRST>(f, std::make_integer_sequence<int, N>{}, a...);
}

// conv_ws64_kernel (csrc/unet_ws.hip) and conv_up_kernel (csrc/unet_up.hip): 8 x 32 output tiles, 4 compute + 4 loader waves, two LDS stages
// of eight planes [hi | lo][k-group] of (halo pixel x 16 B), a 64 KB output tile for the loaders to store
namespace role_split {
constexpr int PH = 8, PW = 32, HPW = PW + 2, HPH = PH + 2, HP = HPW * HPH;   // the halo patch: 10 x 34
constexpr int THREADS = 512, LTHREADS = 256;
constexpr int SPP = KC / 4;                                            // staging slots (16 B = 4 fp32 channels) per pixel and chunk
constexpr int PPI = LTHREADS / SPP;                                    // pixels per loader pass
constexpr int A_F4 = (HP + PPI - 1) / PPI;                             // staging slots per loader thread and chunk (11)
constexpr int HPS = A_F4 * PPI;                                        // staged pixels (>= HP)
constexpr int PLANE = ((HPS * 16 + 255) / 256) * 256;                  // bytes of one (hi | lo, k-group) plane, a multiple of 256
constexpr int HLS = 4 * PLANE + 256;                                   // hi -> lo distance (planes 2, 3 sit 128 B further)
constexpr int STAGE = 2 * HLS;
constexpr int PT = 8;                                                  // 16-pixel tiles (groups) per compute wave
constexpr int OUTBUF = PH * PW * 64 * 4;                               // the epilogue's LDS tile: 256 px x 64 ch fp32, piece (pixel m, channel quad q) at m * 256 + ((q ^ (m & 15)) << 4)

__device__ __forceinline__ constexpr int plane_off(int hl, int kg) { return hl * HLS + kg * PLANE + (kg >> 1) * 128; }

// Both kernels' 16-pixel groups are pixels TWO columns apart, so the loaders stage a halo row's columns DE-INTERLEAVED -- the 17 even halo
// columns, then the 17 odd ones -- and a group's fragment is still 16 consecutive 16-byte pieces of a plane: halo column hx sits at staged
// position (hx & 1) * HALF + (hx >> 1) of its row, staged position `pos` holds halo column halo_col(pos).
constexpr int HALF = HPW / 2;
__device__ __forceinline__ constexpr int halo_col(int pos) { return pos < HALF ? 2 * pos : 2 * (pos - HALF) + 1; }
}  // namespace role_split

}  // namespace mfpa_tile
