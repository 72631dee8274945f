// The GEMM family of the Demucs denoiser (layer layouts: csrc/demucs.hip): the batched strided MFMA GEMM behind mfpa_gemm_mfma -- six kernel
// templates, twelve instantiations, one shared epilogue, one route (gemm_route) and one launch table (GEMM_KERNELS) -- and the two fused
// end-level kernels (glu_convT_c1_kernel, c1_glu_kernel), which are the short-K bf16x3 GEMM with another loader and epilogue.
// Written once at the top of the file: the tile geometry of every kernel shape (read by the kernel and by its launch), the bf16 hi | lo
// split, the accumulator clear, the fragment pointer and the bf16x3 wave step.  A piece stays written out in a kernel
// where the shared spelling changes that kernel's instruction stream (hipcc simplifies a helper on its own before it inlines it); those
// places say so, and tools/same_kernels.py is the check.
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"
#include <type_traits>

namespace {

using namespace mfpa_tile;     // vector types, the bf16x3 product mfma_bf16x3, pin_reads ("one MFMA, then k LDS reads", LEFT reads spread over SLOTS MFMAs)

struct GemmArgs {
  const float* A; long long lda, strideA;      // A[b][m][k] = A[b*strideA + m*lda + k]
  const float* W;                              // [Npad][K], K contiguous, Npad multiple of 64 (zero rows beyond N)
  const float* bias;                           // [Npad] or null
  const float* addend; long long ldadd, strideAdd;   // mode 2: y += addend[b*strideAdd + m*ldadd + n]
  float* C; long long ldc, strideC;
  int nx, ny, nz;                              // tile grid (n tiles, m tiles, clips) of the 1-D launch
  float* C2; long long ldc2, strideC2;         // training: second output (mode 1: the packed GLU pre-activations; relu 2: relu(y) before the addition)
  int M, N, K, mode, relu;                     // mode 0: bias(+relu); 1: GLU (N = output columns = Npad_total/2 pairs); 2: + addend;
                                               // 3: * (addend > 0) -- the ReLU backward mask of the layer that produced addend
  // fp32 kernel only: A is not read but COMPUTED while it is staged -- the first encoder layer Conv1d(1 -> K, k8, s4) + ReLU
  // (conv1d_c1_kernel) of the waveform: A[b][m][c] = relu(c1_b[c] + sum_j c1_w[j][c] * c1_x[b][4 m + j])
  const float* c1_x; long long c1_lin;         // (batch, c1_lin) samples
  const float* c1_w; const float* c1_b;        // (8, K), (K)
};

// ---------------------------------------------------------------------------------- geometry, said once for a kernel and its launch
// A workgroup of THREADS owns a BM x BN tile; its LDS rows are ROW bytes apart; STAGES A + B tiles (and EXTRA bytes behind them) are the
// DYNAMIC LDS the launch asks for (0: the kernel's tiles are static arrays).
template <int BM_, int BN_, int THREADS_, int ROW_, int STAGES_ = 0, int EXTRA_ = 0>
struct GemmGeo {
  static constexpr int BM = BM_, BN = BN_, THREADS = THREADS_, ROW = ROW_;
  static constexpr int lds_bytes = STAGES_ * (BM_ + BN_) * ROW_ + EXTRA_;
};
constexpr int GKC = 16;            // K chunk of the fp32 kernel
constexpr int GLD = GKC + 4;       // its padded LDS row (floats): 80 B, conflict-free ds_read_b128 fragments
constexpr int HKC = 32, HROW = 144;   // bf16x3: K chunks of 32, LDS rows [32 hi | 32 lo | pad] = 144 B (the layout of conv_mfma_kernel<PREC 1>)
constexpr int shortk_row(int kw) { return 4 * kw + 16; }   // whole-K rows: KW floats, or [KW hi | KW lo] bf16, + pad: conflict-free b128 reads (208 B at 48)
using Fp32Geo = GemmGeo<128, 64, 256, 4 * GLD>;                               // gemm_mfma_kernel: 4 waves stacked along M, each 32 x 64
template <bool C1SRC, int K> using SmallKGeo = GemmGeo<128, 64, 256, shortk_row(K)>;        // gemm_smallk_kernel
using Bf16x3Geo = GemmGeo<128, 64, 256, HROW>;                                // gemm_bf16x3_kernel
using WideGeo = GemmGeo<128, 128, 256, HROW, 2>;                              // gemm_bf16x3_wide_kernel: four 64 x 64 wave tiles
using PipeGeo = GemmGeo<256, 128, 512, HROW, 2>;                              // gemm_bf16x3_pipe_kernel: 4 x 2 waves of 64 x 64
template <bool C1SRC, int K, int KCW> using ShortKGeo = GemmGeo<128, 64, 256, shortk_row(KCW), 1, C1SRC ? 9 * K * 4 : 0>;   // gemm_shortk_bf16x3_kernel (+ W1s)
using FusedGeo = GemmGeo<128, 128, 256, shortk_row(48)>;                      // glu_convT_c1_kernel, c1_glu_kernel: all 128 packed columns
constexpr int GBM = 128;           // rows of every tile whose epilogue goes through gemm_epilogue (the pipe kernel picks FULL itself)
static_assert(PipeGeo::lds_bytes == 110592 && WideGeo::lds_bytes == 73728, "dynamic LDS of the pipelined and the wide launch");
static_assert(ShortKGeo<false, 48, 48>::lds_bytes == 39936 && ShortKGeo<false, 96, 48>::lds_bytes == 39936 && ShortKGeo<true, 48, 48>::lds_bytes == 41664,
              "dynamic LDS of the short-K launches");
static_assert(Bf16x3Geo::lds_bytes == 0 && Fp32Geo::lds_bytes == 0 && SmallKGeo<false, 48>::lds_bytes == 0 && SmallKGeo<true, 48>::lds_bytes == 0 &&
              FusedGeo::lds_bytes == 0, "kernels with static tiles ask for no dynamic LDS");

// Tile of a workgroup in the 1-D launch.  Consecutive workgroup ids are dealt round-robin over the 8 XCDs, each with its own L2:
// with the plain order the n tiles that share an A tile land on 8 different XCDs and every one of them fetches that A tile from
// memory (PMC: the mid-level launches fetched 2.7x what they wrote).  Here XCD k owns a contiguous range of the (clip, m tile,
// n tile) order, n fastest, so the workgroups sharing an A tile run back to back on ONE XCD.
__device__ __forceinline__ bool gemm_tile_at(const GemmArgs& a, unsigned vb, int& bx, int& by, int& bz) {
  const unsigned total = (unsigned)a.nx * a.ny * a.nz;
  const unsigned per = (total + 7) / 8;
  if (vb / 8 >= per) return false;             // past the last virtual id (a persistent workgroup stepping by gridDim.x): NOT the next XCD's range
  const unsigned lin = (vb % 8) * per + vb / 8;
  if (lin >= total) return false;              // uniform over the workgroup, before any barrier
  bx = lin % a.nx;
  const unsigned rest = lin / a.nx;
  by = rest % a.ny;
  bz = rest / a.ny;
  return true;
}
__device__ __forceinline__ bool gemm_tile(const GemmArgs& a, int& bx, int& by, int& bz) { return gemm_tile_at(a, blockIdx.x, bx, by, bz); }

// ---------------------------------------------------------------------------------- pieces the kernels share
// (The whole-K staging loops and the "first encoder layer computed while A is staged" block of gemm_smallk_kernel and
// gemm_shortk_bf16x3_kernel and the chunk load / store of the two 256-thread bf16x3 kernels are NOT among them: as functions they moved every
// kernel that used them, by 135 .. 3759 instruction lines; NOTES.md, 2026-10-19.)
// bf16x3 operand split of four floats, v = hi + lo, into an LDS row [hi | lo]: quad q of the hi half, and of the lo half lo_off bytes on
__device__ __forceinline__ void split_store(char* row, int q, int lo_off, f32x4 v) {
  bf16x4 hi, lo;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hi[k] = (__bf16)v[k];
    lo[k] = (__bf16)(v[k] - (float)hi[k]);
  }
  *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
  *reinterpret_cast<bf16x4*>(row + lo_off + 8 * q) = lo;
}

template <int NT>
__device__ __forceinline__ void clear_acc(floatx16 (&acc)[NT]) {
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;
}

// this lane's fragment pointer into a tile of ROW-byte rows: row `row`, k half lh
__device__ __forceinline__ const char* frag_ptr(const char* tile, int row, int ROW, int lh) { return tile + row * ROW + 16 * lh; }

// One k-step (16 of K) of a 32-row x (32 NT)-column wave tile with bf16x3 products.  Ap / Bp: this lane's fragments OF THE STEP (the caller
// adds 32 s; with the step index as a parameter the K = 48 short-K forms' streams moved); rows of ROW bytes, the lo half LO bytes behind the hi
template <int NT, int ROW, int LO>
__device__ __forceinline__ void wave_step_bf16x3(floatx16 (&acc)[NT], const char* Ap, const char* Bp) {
  const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Ap);
  const bf16x8 al = *reinterpret_cast<const bf16x8*>(Ap + LO);
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) {
    const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bp + nt * 32 * ROW);
    const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bp + nt * 32 * ROW + LO);
    mfma_bf16x3(acc[nt], ah, al, bh, bl);
  }
}

// One k-step (8 of K) of a 32 x 64 wave tile with fp32 products: 2 x 4 v_mfma_f32_32x32x2f32 on the fragments the caller has read (af: four k of
// the A rows, b0 / b1: of the two n tiles' rows; as a function that reads them itself it moved gemm_mfma_kernel<false>'s stream)
__device__ __forceinline__ void wave_step_fp32(floatx16& acc0, floatx16& acc1, f32x4 af, f32x4 b0, f32x4 b1) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[k], b0[k], acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(af[k], b1[k], acc1, 0, 0, 0);
  }
}

// epilogue shared by all GEMM kernels: D[row = m][col = n]; a lane holds column li of both 32-wide n tiles.
// The short-K launches are bound by vector-instruction issue, and the first form of this epilogue was most of it (64-bit
// address arithmetic and an exec-mask branch per element, an IEEE division in the sigmoid): here every offset is a 32-bit byte
// offset from a per-clip scalar base (the host checks that a clip's tile fits 4 GB), full row tiles skip the row bounds checks
// (FULL), column predicates are hoisted out of the row loop, and the sigmoid uses v_rcp_f32.
__device__ __forceinline__ float gemm_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ void st_f32(char* base, unsigned boff, float v) { *reinterpret_cast<float*>(base + boff) = v; }
__device__ __forceinline__ float ld_f32(const char* base, unsigned boff) { return *reinterpret_cast<const float*>(base + boff); }

template <bool FULL>
__device__ __forceinline__ void gemm_epilogue_t(const GemmArgs& a, floatx16 (&acc)[2], int m0, int n0, int b, int wave, int li, int lh) {
  const float bias0 = a.bias ? a.bias[n0 + li] : 0.f;
  const float bias1 = a.bias ? a.bias[n0 + 32 + li] : 0.f;
  char* Cb = reinterpret_cast<char*>(a.C + (size_t)b * a.strideC);
  char* C2b = a.C2 ? reinterpret_cast<char*>(a.C2 + (size_t)b * a.strideC2) : nullptr;
  const unsigned ldc = (unsigned)a.ldc, ldc2 = (unsigned)a.ldc2;
  const int mbase = m0 + wave * 32 + 4 * lh;
  if (a.mode == 1) {                           // GLU: value * sigmoid(gate); output column = (tile index) * 32 + li
    const int n = (n0 / 64) * 32 + li;
    const bool ok = n < a.N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mbase + (r & 3) + 8 * (r >> 2);
      if (!FULL && m >= a.M) continue;
      const float v0 = acc[0][r] + bias0, v1 = acc[1][r] + bias1;
      if (C2b) {                               // the pre-activations in the packed [32 values | 32 gates] tile order
        const unsigned o = ((unsigned)m * ldc2 + (unsigned)(n0 + li)) * 4u;
        st_f32(C2b, o, v0);
        st_f32(C2b, o + 128u, v1);
      }
      if (ok) st_f32(Cb, ((unsigned)m * ldc + (unsigned)n) * 4u, v0 * gemm_sigmoid(v1));
    }
    return;
  }
  const int n = n0 + li;
  const bool ok0 = n < a.N, ok1 = n + 32 < a.N;
  const unsigned ldadd = (unsigned)a.ldadd;
  // modes 2 / 3: ALL of this lane's addend values are loaded before the first store -- the addend may alias C as far as the
  // compiler knows, so loads interleaved with the stores were serialised into 16 exposed memory round trips per wave (PMC: the
  // transposed-convolution launches spent 57 .. 70 % of their wave cycles in s_waitcnt)
  float ad0[16], ad1[16];
  if (a.mode >= 2) {
    const char* Adb = reinterpret_cast<const char*>(a.addend + (size_t)b * a.strideAdd);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mbase + (r & 3) + 8 * (r >> 2);
      const unsigned oa = ((unsigned)m * ldadd + (unsigned)n) * 4u;
      const bool rowok = FULL || m < a.M;
      ad0[r] = (rowok && ok0) ? ld_f32(Adb, oa) : 0.f;
      ad1[r] = (rowok && ok1) ? ld_f32(Adb, oa + 128u) : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = mbase + (r & 3) + 8 * (r >> 2);
    if (!FULL && m >= a.M) continue;
    float v0 = acc[0][r] + bias0, v1 = acc[1][r] + bias1;
    const unsigned o = ((unsigned)m * ldc + (unsigned)n) * 4u;
    if (a.relu == 2) {                         // ReLU before the skip addition
      v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f);
      if (C2b) {
        const unsigned o2 = ((unsigned)m * ldc2 + (unsigned)n) * 4u;
        if (ok0) st_f32(C2b, o2, v0);
        if (ok1) st_f32(C2b, o2 + 128u, v1);
      }
    }
    if (a.mode == 2) {
      v0 += ad0[r]; v1 += ad1[r];
    } else if (a.mode == 3) {
      if (C2b) {                               // the unmasked gradient as well (it is also the skip connection's gradient)
        const unsigned o2 = ((unsigned)m * ldc2 + (unsigned)n) * 4u;
        if (ok0) st_f32(C2b, o2, v0);
        if (ok1) st_f32(C2b, o2 + 128u, v1);
      }
      v0 = ad0[r] > 0.f ? v0 : 0.f;
      v1 = ad1[r] > 0.f ? v1 : 0.f;
    }
    if (a.relu == 1) { v0 = fmaxf(v0, 0.f); v1 = fmaxf(v1, 0.f); }
    if (ok0) st_f32(Cb, o, v0);
    if (ok1) st_f32(Cb, o + 128u, v1);
  }
}

__device__ __forceinline__ void gemm_epilogue(const GemmArgs& a, floatx16 (&acc)[2], int m0, int n0, int b, int wave, int li, int lh) {
  if (m0 + GBM <= a.M) gemm_epilogue_t<true>(a, acc, m0, n0, b, wave, li, lh);
  else gemm_epilogue_t<false>(a, acc, m0, n0, b, wave, li, lh);
}

// ---------------------------------------------------------------------------------- the GEMM kernels
template <bool C1SRC>
__global__ __launch_bounds__(256, 2) void gemm_mfma_kernel(GemmArgs a) {
  using G = Fp32Geo;
  __shared__ __attribute__((aligned(16))) float As[2][G::BM * GLD];
  __shared__ __attribute__((aligned(16))) float Bs[2][G::BN * GLD];
  __shared__ __attribute__((aligned(16))) float W1s[C1SRC ? 9 * 256 : 4];      // C1SRC: [8][K] taps then [K] bias, K <= 256
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int bx, by, b;
  if (!gemm_tile(a, bx, by, b)) return;
  const int n0 = bx * G::BN, m0 = by * G::BM;
  const float* Ab = a.A + (size_t)b * a.strideA;
  const int nk = a.K / GKC;

  // staging: A tile 128 rows x 4 float4, B tile 64 rows x 4 float4
  f32x4 ar[2], br;
  const int arow0 = tid >> 2, aq = tid & 3;             // rows arow0 and arow0 + 64
  const int brow = tid >> 2, bq = tid & 3;              // 64 rows
  f32x4 xr[2][2];                              // C1SRC: the 8 samples under each of this thread's two rows, loaded once
  if (C1SRC) {
    const float* xb = a.c1_x + (size_t)b * a.c1_lin;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + arow0 + 64 * i;
      xr[i][0] = xr[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (m < a.M) {
        xr[i][0] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m);
        xr[i][1] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m + 4);
      }
    }
    for (int i = tid; i < 8 * a.K; i += 256) W1s[i] = a.c1_w[i];
    for (int i = tid; i < a.K; i += 256) W1s[8 * a.K + i] = a.c1_b[i];
    __syncthreads();
  }
  auto load = [&](int kc) __attribute__((always_inline)) {
    if (C1SRC) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {             // conv1d_c1_kernel's arithmetic, same order: bias, then taps 0..7
        const int c = kc * GKC + 4 * aq;
        f32x4 v = *reinterpret_cast<const f32x4*>(&W1s[8 * a.K + c]);
#pragma unroll
        for (int j = 0; j < 8; ++j) v += xr[i][j >> 2][j & 3] * *reinterpret_cast<const f32x4*>(&W1s[j * a.K + c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
        ar[i] = (m0 + arow0 + 64 * i < a.M) ? v : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + arow0 + 64 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < a.M) v = *reinterpret_cast<const f32x4*>(Ab + (size_t)m * a.lda + kc * GKC + 4 * aq);
        ar[i] = v;
      }
    }
    br = *reinterpret_cast<const f32x4*>(a.W + (size_t)(n0 + brow) * a.K + kc * GKC + 4 * bq);
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *reinterpret_cast<f32x4*>(&As[buf][(arow0 + 64 * i) * GLD + 4 * aq]) = ar[i];
    *reinterpret_cast<f32x4*>(&Bs[buf][brow * GLD + 4 * bq]) = br;
  };

  floatx16 acc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;               // (written out: clear_acc moves this kernel's instruction stream)

  load(0);
  store(0);
  if (nk > 1) load(1);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) store(buf ^ 1);          // B/A(kc+1) registers -> the other LDS buffer (free since the last barrier)
    if (kc + 2 < nk) load(kc + 2);
    const float* Ap = &As[buf][(wave * 32 + li) * GLD + 4 * lh];
    const float* Bp = &Bs[buf][li * GLD + 4 * lh];
#pragma unroll
    for (int s = 0; s < GKC / 8; ++s) {
      const f32x4 af = *reinterpret_cast<const f32x4*>(Ap + 8 * s);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(Bp + 8 * s);
      const f32x4 b1 = *reinterpret_cast<const f32x4*>(Bp + 32 * GLD + 8 * s);
      wave_step_fp32(acc[0], acc[1], af, b0, b1);
    }
    __syncthreads();
  }

  gemm_epilogue(a, acc, m0, n0, b, wave, li, lh);
}

// Short-K form (the 48-channel 1x1 + GLU layers at the full-rate ends of the network: 16.4 M rows x 48 x 96, as much HBM time
// as MFMA time).  The whole K extent of both tiles is staged at once -- every global load of the workgroup is in flight
// together, one barrier, no chunk loop -- which is what a three-chunk pipeline cannot do: it exposed one memory latency
// per chunk.
template <bool C1SRC, int K>
__global__ __launch_bounds__(256, 3) void gemm_smallk_kernel(GemmArgs a) {
  using G = SmallKGeo<C1SRC, K>;
  constexpr int LD = G::ROW / 4, QPR = K / 4;           // LDS row (floats): 208 B for K = 48, conflict-free ds_read_b128
  constexpr int A_F4 = (G::BM * QPR + 255) / 256, B_F4 = (G::BN * QPR + 255) / 256;
  __shared__ __attribute__((aligned(16))) float As[G::BM * LD];
  __shared__ __attribute__((aligned(16))) float Bs[G::BN * LD];
  __shared__ __attribute__((aligned(16))) float W1s[C1SRC ? 9 * K : 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int bx, by, b;
  if (!gemm_tile(a, bx, by, b)) return;
  const int n0 = bx * G::BN, m0 = by * G::BM;
  f32x4 ar[A_F4], br[B_F4], x0[C1SRC ? A_F4 : 1], x1[C1SRC ? A_F4 : 1];
#pragma unroll
  for (int i = 0; i < B_F4; ++i) {
    const int idx = tid + 256 * i;
    br[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (idx < G::BN * QPR) br[i] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(n0 + idx / QPR) * K + 4 * (idx % QPR));
  }
  if (C1SRC) {
    const float* xb = a.c1_x + (size_t)b * a.c1_lin;
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      const int idx = tid + 256 * i, m = m0 + idx / QPR;
      x0[i] = x1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < G::BM * QPR && m < a.M) {
        x0[i] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m);
        x1[i] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m + 4);
      }
    }
    for (int i = tid; i < 8 * K; i += 256) W1s[i] = a.c1_w[i];
    for (int i = tid; i < K; i += 256) W1s[8 * K + i] = a.c1_b[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {              // conv1d_c1_kernel's arithmetic, same order: bias, then taps 0..7
      const int idx = tid + 256 * i, c = 4 * (idx % QPR);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < G::BM * QPR && m0 + idx / QPR < a.M) {
        v = *reinterpret_cast<const f32x4*>(&W1s[8 * K + c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v += x0[i][j] * *reinterpret_cast<const f32x4*>(&W1s[j * K + c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v += x1[i][j] * *reinterpret_cast<const f32x4*>(&W1s[(4 + j) * K + c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
      }
      ar[i] = v;
    }
  } else {
    const float* Ab = a.A + (size_t)b * a.strideA;
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      const int idx = tid + 256 * i, m = m0 + idx / QPR;
      ar[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < G::BM * QPR && m < a.M) ar[i] = *reinterpret_cast<const f32x4*>(Ab + (size_t)m * a.lda + 4 * (idx % QPR));
    }
  }
#pragma unroll
  for (int i = 0; i < A_F4; ++i) {
    const int idx = tid + 256 * i;
    if (idx < G::BM * QPR) *reinterpret_cast<f32x4*>(&As[(idx / QPR) * LD + 4 * (idx % QPR)]) = ar[i];
  }
#pragma unroll
  for (int i = 0; i < B_F4; ++i) {
    const int idx = tid + 256 * i;
    if (idx < G::BN * QPR) *reinterpret_cast<f32x4*>(&Bs[(idx / QPR) * LD + 4 * (idx % QPR)]) = br[i];
  }
  __syncthreads();
  floatx16 acc[2];
  clear_acc(acc);
  const float* Ap = &As[(wave * 32 + li) * LD + 4 * lh];
  const float* Bp = &Bs[li * LD + 4 * lh];
#pragma unroll
  for (int s = 0; s < K / 8; ++s) {
    const f32x4 af = *reinterpret_cast<const f32x4*>(Ap + 8 * s);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(Bp + 8 * s);
    const f32x4 b1 = *reinterpret_cast<const f32x4*>(Bp + 32 * LD + 8 * s);
    wave_step_fp32(acc[0], acc[1], af, b0, b1);
  }
  gemm_epilogue(a, acc, m0, n0, b, wave, li, lh);
}

// The same GEMM with bf16x3 products (precision 1): K chunks of 32 (HKC), LDS rows [32 hi | 32 lo | pad] (HROW), operands split while
// they are staged, 3 x v_mfma_f32_32x32x16_bf16 per fp32 product.
__global__ __launch_bounds__(256, 2) void gemm_bf16x3_kernel(GemmArgs a) {
  using G = Bf16x3Geo;
  __shared__ __attribute__((aligned(16))) char As[2][G::BM * HROW];
  __shared__ __attribute__((aligned(16))) char Bs[2][G::BN * HROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int bx, by, b;
  if (!gemm_tile(a, bx, by, b)) return;
  const int n0 = bx * G::BN, m0 = by * G::BM;
  const float* Ab = a.A + (size_t)b * a.strideA;
  const int nk = a.K / HKC;

  // staging: A tile 128 rows x 8 float4 (4 per thread), B tile 64 rows x 8 float4 (2 per thread)
  f32x4 ar[4], br[2];
  const int q = tid & 7, r0 = tid >> 3;                  // rows r0 + 32 i
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + r0 + 32 * i;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < a.M) v = *reinterpret_cast<const f32x4*>(Ab + (size_t)m * a.lda + kc * HKC + 4 * q);
      ar[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
      br[i] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(n0 + r0 + 32 * i) * a.K + kc * HKC + 4 * q);
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) split_store(&As[buf][(r0 + 32 * i) * HROW], q, 64, ar[i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) split_store(&Bs[buf][(r0 + 32 * i) * HROW], q, 64, br[i]);
  };

  floatx16 acc[2];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;               // (written out: clear_acc moves this kernel's instruction stream)

  load(0);
  store(0);
  if (nk > 1) load(1);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) store(buf ^ 1);
    if (kc + 2 < nk) load(kc + 2);
    const char* Ap = frag_ptr(As[buf], wave * 32 + li, HROW, lh);
    const char* Bp = frag_ptr(Bs[buf], li, HROW, lh);
#pragma unroll
    for (int s = 0; s < 2; ++s) wave_step_bf16x3<2, HROW, 64>(acc, Ap + 32 * s, Bp + 32 * s);
    __syncthreads();
  }
  gemm_epilogue(a, acc, m0, n0, b, wave, li, lh);
}

// The same with a 128 x 128 workgroup tile of four 64 x 64 wave tiles (2 x 2 MFMA tiles per wave): a wave reads 8 fragments per
// 12 MFMAs instead of 6 per 6 -- the 32 x 64 wave tile above keeps the LDS pipe as busy as the matrix pipe (PMC: 30 % of the wave
// cycles issue-stalled on the mid-level launches).  Used when the padded N is a multiple of 128.  73.7 KB of LDS, two workgroups
// per CU.
// WSPLIT: W arrives already split -- every 32-element chunk of a row as [32 bf16 hi | 32 bf16 lo] (ops_demucs.split_rows, for weights
// that do not change between calls): staging it is a 16-byte copy instead of 12 vector instructions per quad in every workgroup.
template <bool WSPLIT>
__global__ __launch_bounds__(256, 2) void gemm_bf16x3_wide_kernel(GemmArgs a) {
  using G = WideGeo;
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  char* As = wsm;                                    // [2][BM][HROW]
  char* Bs = wsm + 2 * G::BM * HROW;                 // [2][BN][HROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  int bx, by, b;
  if (!gemm_tile(a, bx, by, b)) return;
  const int n0 = bx * G::BN, m0 = by * G::BM;
  const float* Ab = a.A + (size_t)b * a.strideA;
  const int nk = a.K / HKC;

  f32x4 ar[4], br[4];
  const int q = tid & 7, r0 = tid >> 3;                  // rows r0 + 32 i
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + r0 + 32 * i;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (m < a.M) v = *reinterpret_cast<const f32x4*>(Ab + (size_t)m * a.lda + kc * HKC + 4 * q);
      ar[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      br[i] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(n0 + r0 + 32 * i) * a.K + kc * HKC + 4 * q);
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) split_store(As + (buf * G::BM + r0 + 32 * i) * HROW, q, 64, ar[i]);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (WSPLIT) *reinterpret_cast<f32x4*>(Bs + (buf * G::BN + r0 + 32 * i) * HROW + 16 * q) = br[i];
      else split_store(Bs + (buf * G::BN + r0 + 32 * i) * HROW, q, 64, br[i]);
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) clear_acc(acc[mt]);

  load(0);
  store(0);
  if (nk > 1) load(1);
  __syncthreads();
  for (int kc = 0; kc < nk; ++kc) {
    const int buf = kc & 1;
    if (kc + 1 < nk) store(buf ^ 1);
    if (kc + 2 < nk) load(kc + 2);
    const char* Ap = frag_ptr(As, buf * G::BM + wm * 64 + li, HROW, lh);
    const char* Bp = frag_ptr(Bs, buf * G::BN + wn * 64 + li, HROW, lh);
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        ah[t] = *reinterpret_cast<const bf16x8*>(Ap + t * 32 * HROW + 32 * s);
        al[t] = *reinterpret_cast<const bf16x8*>(Ap + t * 32 * HROW + 64 + 32 * s);
        bh[t] = *reinterpret_cast<const bf16x8*>(Bp + t * 32 * HROW + 32 * s);
        bl[t] = *reinterpret_cast<const bf16x8*>(Bp + t * 32 * HROW + 64 + 32 * s);
      }
#pragma unroll
      for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) mfma_bf16x3(acc[mt][nt], ah[mt], al[mt], bh[nt], bl[nt]);
    }
    __syncthreads();
  }
  // the shared epilogue takes a 32-row x 64-column wave tile at row (wave index) * 32: two calls per wave
#pragma unroll
  for (int mt = 0; mt < 2; ++mt) gemm_epilogue(a, acc[mt], m0, n0 + wn * 64, b, wm * 2 + mt, li, lh);
}

// The software-pipelined form of the wide kernel (the schedule of conv_mfma_kernel<PREC 1>'s tap body, unet_mfma.hip): 8 waves own a
// 256 x 128 tile (4 x 2 waves of 64 x 64), one workgroup per CU.  A K chunk of 32 is two k-steps; the fragments of a k-step are
// read from LDS one step AHEAD of the MFMAs that use them (two register sets of fragments), the barrier sits between the two
// k-steps of a chunk, and the global loads run two chunks ahead of their LDS stores through two register sets (straight-line
// code per chunk parity, so hipcc's vmcnt bookkeeping is exact: no s_waitcnt vmcnt(0) in the steady state).  Rows past M are
// clamped to row M - 1 when loaded (never stored), so every load is unconditional.  K must be a multiple of 64, at least 128.
template <bool WSPLIT>
__global__ __launch_bounds__(512, 1) void gemm_bf16x3_pipe_kernel(GemmArgs a) {
  using G = PipeGeo;
  extern __shared__ __attribute__((aligned(16))) char psm[];
  constexpr int ASZ = G::BM * HROW, BSZ = G::BN * HROW;
  char* As = psm;                                    // [2][BM][HROW]
  char* Bs = psm + 2 * ASZ;                          // [2][BN][HROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 3, wn = wave >> 2;
  const int nk = a.K / HKC;
  const int q = tid & 7, r0 = tid >> 3;              // staging: column quad, rows r0 + 64 i
  // PERSISTENT over tiles: workgroup w takes the virtual workgroup ids w, w + gridDim.x, ... (gridDim.x is a multiple of 8, so they all map
  // into the same XCD's range of gemm_tile_at).  One workgroup owns a CU (111 KB of LDS), so as one tile per workgroup nothing overlapped a
  // tile's first loads (a memory round trip before the first MFMA) and its epilogue (stores, addend loads) with anything: on the K = 192 .. 384
  // layers those two were as long as the main loop.  Here the first two chunks of the NEXT tile are requested before the epilogue of the
  // current one (their staging registers are free by then), so the round trip runs under the epilogue.
  struct TileP { const float* ap[4]; const float* bp[2]; int m0, n0, b; };
  auto tile_at = [&](unsigned vb, TileP& t) __attribute__((always_inline)) -> bool {
    int bx, by, b;
    if (!gemm_tile_at(a, vb, bx, by, b)) return false;
    t.n0 = bx * G::BN; t.m0 = by * G::BM; t.b = b;
    const float* Ab = a.A + (size_t)b * a.strideA;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int m = t.m0 + r0 + 64 * i;
      m = m < a.M ? m : a.M - 1;
      t.ap[i] = Ab + (size_t)m * a.lda + 4 * q;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) t.bp[i] = a.W + (size_t)(t.n0 + r0 + 64 * i) * a.K + 4 * q;
    return true;
  };
  struct Stage { f32x4 a[4], b[2]; };
  Stage st0, st1;
  auto load = [&](const TileP& t, int kc, Stage& st) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) st.a[i] = *reinterpret_cast<const f32x4*>(t.ap[i] + kc * HKC);
#pragma unroll
    for (int i = 0; i < 2; ++i) st.b[i] = *reinterpret_cast<const f32x4*>(t.bp[i] + kc * HKC);
  };
  auto store = [&](int buf, const Stage& st) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) split_store(As + buf * ASZ + (r0 + 64 * i) * HROW, q, 64, st.a[i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (WSPLIT) *reinterpret_cast<f32x4*>(Bs + buf * BSZ + (r0 + 64 * i) * HROW + 16 * q) = st.b[i];
      else split_store(Bs + buf * BSZ + (r0 + 64 * i) * HROW, q, 64, st.b[i]);
    }
  };
  struct Frags { bf16x8 ah[2], al[2], bh[2], bl[2]; };
  Frags fr0, fr1;
  const char* Ap = frag_ptr(As, wm * 64 + li, HROW, lh);
  const char* Bp = frag_ptr(Bs, wn * 64 + li, HROW, lh);
  auto read_frags = [&](Frags& f, int buf, int s) __attribute__((always_inline)) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      f.ah[t] = *reinterpret_cast<const bf16x8*>(Ap + buf * ASZ + t * 32 * HROW + 32 * s);
      f.al[t] = *reinterpret_cast<const bf16x8*>(Ap + buf * ASZ + t * 32 * HROW + 64 + 32 * s);
      f.bh[t] = *reinterpret_cast<const bf16x8*>(Bp + buf * BSZ + t * 32 * HROW + 32 * s);
      f.bl[t] = *reinterpret_cast<const bf16x8*>(Bp + buf * BSZ + t * 32 * HROW + 64 + 32 * s);
    }
  };
  floatx16 acc[2][2];
  auto mfma12 = [&](const Frags& f) __attribute__((always_inline)) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) mfma_bf16x3(acc[mt][nt], f.ah[mt], f.al[mt], f.bh[nt], f.bl[nt]);
  };
  constexpr int N_DSW = WSPLIT ? 10 : 12;            // LDS stores of one chunk per thread
  TileP cur;
  // one K chunk; SET = chunk parity = LDS buffer it is computed from; STORE: chunk kc + 1 (register set SET ^ 1) goes to the other
  // buffer; LOAD: that register set is refilled with chunk kc + 3
  auto body = [&](auto SET_, auto STORE_, auto LOAD_, int kc) __attribute__((always_inline)) {
    constexpr int SET = decltype(SET_)::value;
    constexpr bool STORE = decltype(STORE_)::value, LOAD = decltype(LOAD_)::value;
    Stage& other = SET ? st0 : st1;
    read_frags(fr1, SET, 1);
    mfma12(fr0);
    if constexpr (STORE) store(SET ^ 1, other);
    if constexpr (LOAD) load(cur, kc + 3, other);
    pin_reads<8, 8>();
    if constexpr (STORE) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, N_DSW / 2, 0);
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      __builtin_amdgcn_sched_group_barrier(0x200, N_DSW - N_DSW / 2, 0);
      if constexpr (LOAD) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x020, 6, 0);
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
      } else {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
      }
    } else {
      __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (STORE) read_frags(fr0, SET ^ 1, 0);
    mfma12(fr1);
    if constexpr (STORE) pin_reads<12, 8>();
    __builtin_amdgcn_sched_barrier(0);
  };
  using T = std::true_type;
  using F = std::false_type;
  using S0 = std::integral_constant<int, 0>;
  using S1 = std::integral_constant<int, 1>;
  unsigned vb = blockIdx.x;
  if (!tile_at(vb, cur)) return;                         // uniform over the workgroup, before any barrier
  // (the scheduling barriers keep the prologue's loads in the order the loop issues them, so the vmcnt state merged at the loop
  // header is the steady state's and the first stores of a trip do not wait for the newest loads)
  load(cur, 0, st0);
  __builtin_amdgcn_sched_barrier(0);
  load(cur, 1, st1);
  __builtin_amdgcn_sched_barrier(0);
  for (;;) {
    store(0, st0);
    __builtin_amdgcn_sched_barrier(0);
    load(cur, 2, st0);
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();
    read_frags(fr0, 0, 0);
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) clear_acc(acc[mt]);
    int kc = 0;
    for (; kc < nk - 4; kc += 2) {
      body(S0{}, T{}, T{}, kc);
      body(S1{}, T{}, T{}, kc + 1);
    }
    body(S0{}, T{}, T{}, kc);                               // kc = nk - 4: chunk nk - 1 is the last load
    body(S1{}, T{}, F{}, kc + 1);
    body(S0{}, T{}, F{}, kc + 2);
    body(S1{}, F{}, F{}, kc + 3);
    // the next tile's first two chunks go out now: both staging sets are free, and nobody reads LDS after the barrier inside the last body
    const int m0 = cur.m0, n0 = cur.n0, b = cur.b;
    vb += gridDim.x;
    const bool more = tile_at(vb, cur);
    if (more) {
      load(cur, 0, st0);
      __builtin_amdgcn_sched_barrier(0);
      load(cur, 1, st1);
      __builtin_amdgcn_sched_barrier(0);
    }
    const bool full = m0 + G::BM <= a.M;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
      if (full) gemm_epilogue_t<true>(a, acc[mt], m0, n0 + wn * 64, b, wm * 2 + mt, li, lh);
      else gemm_epilogue_t<false>(a, acc[mt], m0, n0 + wn * 64, b, wm * 2 + mt, li, lh);
    }
    if (!more) break;
  }
}

// Short-K layers with bf16x3 products (K = 48 and 96: the full-rate outer levels of the network; measured on 256 clips: forward
// 50.1 -> 46.8 ms with these two; the same form for K = 128 / 192 was slower than the fp32 kernel and is not instantiated).  With exact fp32 products
// these launches are bound by the fp32 MFMA rate (64 cycles per 32x32x2), not by HBM: e.g. the 1x1 + GLU of level 0 is 151 GFLOP
// per 256 clips = 1.2 ms of fp32 MFMA against 0.8 ms of HBM traffic.  Here EVERY global load of the workgroup (all NCH chunks
// of both tiles, up to 36 float4 per thread) is issued before anything is consumed; the chunks are then split to bf16 hi / lo and
// staged one at a time through a single small LDS buffer (40 .. 77 KB, two workgroups per CU), 3 x v_mfma_f32_32x32x16_bf16 per
// product.  Same tile (128 x 64, four 32 x 64 wave tiles) and epilogue as the other GEMM kernels.
template <bool C1SRC, int K, int KCW>
__global__ __launch_bounds__(256, 2) void gemm_shortk_bf16x3_kernel(GemmArgs a) {
  static_assert(K % KCW == 0 && KCW % 16 == 0 && (!C1SRC || K == KCW), "chunking");
  using G = ShortKGeo<C1SRC, K, KCW>;
  constexpr int NCH = K / KCW, QPR = KCW / 4, ROW = G::ROW;             // LDS row bytes: [KCW hi | KCW lo | pad]
  constexpr int A_F4 = (G::BM * QPR + 255) / 256, B_F4 = (G::BN * QPR + 255) / 256;
  extern __shared__ __attribute__((aligned(16))) char sksm[];
  char* As = sksm;                                                      // [BM][ROW]
  char* Bs = sksm + G::BM * ROW;                                        // [BN][ROW]
  float* W1s = reinterpret_cast<float*>(sksm + (G::BM + G::BN) * ROW);  // C1SRC: [8][K] taps then [K] bias
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  int bx, by, b;
  if (!gemm_tile(a, bx, by, b)) return;
  const int n0 = bx * G::BN, m0 = by * G::BM;
  f32x4 ar[NCH][A_F4], br[NCH][B_F4];
#pragma unroll
  for (int c = 0; c < NCH; ++c)
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
      const int idx = tid + 256 * i;
      br[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < G::BN * QPR) br[c][i] = *reinterpret_cast<const f32x4*>(a.W + (size_t)(n0 + idx / QPR) * K + c * KCW + 4 * (idx % QPR));
    }
  if (C1SRC) {
    f32x4 x0[A_F4], x1[A_F4];
    const float* xb = a.c1_x + (size_t)b * a.c1_lin;
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      const int idx = tid + 256 * i, m = m0 + idx / QPR;
      x0[i] = x1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (idx < G::BM * QPR && m < a.M) {
        x0[i] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m);
        x1[i] = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)m + 4);
      }
    }
    for (int i = tid; i < 8 * K; i += 256) W1s[i] = a.c1_w[i];
    for (int i = tid; i < K; i += 256) W1s[8 * K + i] = a.c1_b[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {              // conv1d_c1_kernel's arithmetic, same order: bias, then taps 0..7
      const int idx = tid + 256 * i, c = 4 * (idx % QPR);
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (idx < G::BM * QPR && m0 + idx / QPR < a.M) {
        v = *reinterpret_cast<const f32x4*>(&W1s[8 * K + c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v += x0[i][j] * *reinterpret_cast<const f32x4*>(&W1s[j * K + c]);
#pragma unroll
        for (int j = 0; j < 4; ++j) v += x1[i][j] * *reinterpret_cast<const f32x4*>(&W1s[(4 + j) * K + c]);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
      }
      ar[0][i] = v;
    }
  } else {
    const float* Ab = a.A + (size_t)b * a.strideA;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
#pragma unroll
      for (int i = 0; i < A_F4; ++i) {
        const int idx = tid + 256 * i, m = m0 + idx / QPR;
        ar[c][i] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (idx < G::BM * QPR && m < a.M) ar[c][i] = *reinterpret_cast<const f32x4*>(Ab + (size_t)m * a.lda + c * KCW + 4 * (idx % QPR));
      }
  }
  floatx16 acc[2];
  clear_acc(acc);
  const char* Ap = frag_ptr(As, wave * 32 + li, ROW, lh);
  const char* Bp = frag_ptr(Bs, li, ROW, lh);
#pragma unroll
  for (int c = 0; c < NCH; ++c) {
    if (c > 0) __syncthreads();                  // the previous chunk's fragment reads are done
#pragma unroll
    for (int i = 0; i < A_F4; ++i) {
      const int idx = tid + 256 * i;
      if (idx < G::BM * QPR) split_store(As + (idx / QPR) * ROW, idx % QPR, 2 * KCW, ar[c][i]);
    }
#pragma unroll
    for (int i = 0; i < B_F4; ++i) {
      const int idx = tid + 256 * i;
      if (idx < G::BN * QPR) split_store(Bs + (idx / QPR) * ROW, idx % QPR, 2 * KCW, br[c][i]);
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < KCW / 16; ++s) wave_step_bf16x3<2, ROW, 2 * KCW>(acc, Ap + 32 * s, Bp + 32 * s);
  }
  gemm_epilogue(a, acc, m0, n0, b, wave, li, lh);
}

// ---------------------------------------------------------------------------------- last decoder level in one launch
// Conv1d(1x1, C -> 2C) + GLU + ConvTranspose1d(C -> 1, k8, s4) of the last decoder level (model.py:80-88,316-318) without the
// (B, L, C) intermediate: as two launches that tensor (3.15 GB per 256 clips at C = 48) is written once and read twice.
// A workgroup owns 127 output groups of a clip (group t = samples 4t .. 4t+3 = taps 0..3 of g[t] + taps 4..7 of g[t-1]) and
// computes the 128 GLU rows g[127 by - 1 .. 127 by + 126] they need (one row of overlap instead of an exchange):
//   * the 1x1 + GLU is the short-K bf16x3 MFMA GEMM of gemm_shortk_bf16x3_kernel (K = C = 48 in one chunk, all 128 packed columns
//     in one workgroup, so a row's 48 GLU outputs meet in one place); W is staged once per workgroup and reused for TPW tiles;
//   * g goes to LDS in fp32 (over the A rows of the same wave: no extra barrier), a thread pair per row forms the 8 tap sums
//     p[t][j] = sum_c g[t][c] w[j][c] with fp32 FMAs, and y[4t + j] = bias + p[t][j] + p[t-1][j+4] is written coalesced.
constexpr int TT_K = 48, TT_ROW = FusedGeo::ROW, TT_OUT = 127, TT_TPW = 8;

__global__ MFPA_NO_PK_F32 __launch_bounds__(256, 2) void glu_convT_c1_kernel(const float* __restrict__ x, int L, const float* __restrict__ gw,
                                                              const float* __restrict__ gb, const float* __restrict__ wl, float bias,
                                                              float* __restrict__ y, int tiles_per_clip, int groups) {
  constexpr int K = TT_K, ROW = TT_ROW, QPR = K / 4, NQ = 128 * QPR / 256;      // 12 quads per row, 6 per thread
  __shared__ __attribute__((aligned(16))) char As[128 * ROW];                   // A rows (bf16 hi | lo), then g rows (fp32) of the same wave
  __shared__ __attribute__((aligned(16))) char Ws[128 * ROW];
  __shared__ __attribute__((aligned(16))) float wls[8 * K];
  __shared__ __attribute__((aligned(16))) float Ps[128 * 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y;
  const int tile0 = blockIdx.x * TT_TPW;
  const float* xb = x + (size_t)b * L * K;
  float* yb = y + (size_t)b * 4 * (L + 1);
  f32x4 ar[NQ];
  auto load_a = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int idx = tid + 256 * i;
      int t = tile * TT_OUT - 1 + idx / QPR;               // rows outside [0, L) are masked when g is written
      t = t < 0 ? 0 : (t < L ? t : L - 1);
      ar[i] = *reinterpret_cast<const f32x4*>(xb + (size_t)t * K + 4 * (idx % QPR));
    }
  };
  load_a(tile0);
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int idx = tid + 256 * i;
    split_store(Ws + (idx / QPR) * ROW, idx % QPR, 2 * K, *reinterpret_cast<const f32x4*>(gw + (size_t)(idx / QPR) * K + 4 * (idx % QPR)));
  }
  for (int i = tid; i < 8 * K; i += 256) wls[i] = wl[i];
  float gbias[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) gbias[nt] = gb[nt * 32 + li];
  const char* Ap = frag_ptr(As, wave * 32 + li, ROW, lh);
  const char* Bp = frag_ptr(Ws, li, ROW, lh);
  const int ntile = tiles_per_clip - tile0 < TT_TPW ? tiles_per_clip - tile0 : TT_TPW;
  for (int it = 0; it < ntile; ++it) {
    const int tile = tile0 + it;
    const int tbase = tile * TT_OUT - 1;                   // clip row of tile row 0
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int idx = tid + 256 * i;
      split_store(As + (idx / QPR) * ROW, idx % QPR, 2 * K, ar[i]);
    }
    if (it + 1 < ntile) load_a(tile + 1);
    __syncthreads();                                       // A (and, the first time, W / wl) staged
    floatx16 acc[4];
    clear_acc(acc);
#pragma unroll
    for (int s = 0; s < K / 16; ++s) wave_step_bf16x3<4, ROW, 2 * K>(acc, Ap + 32 * s, Bp + 32 * s);
    // GLU -> g rows in LDS (fp32, same 208-byte rows; this wave's own 32 rows, whose fragments it has just read)
    float* Gs = reinterpret_cast<float*>(As);
    constexpr int GLDF = ROW / 4;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
      const int t = tbase + row;
      const bool in = t >= 0 && t < L;
      const float g0 = (acc[0][r] + gbias[0]) * gemm_sigmoid(acc[1][r] + gbias[1]);
      Gs[row * GLDF + li] = in ? g0 : 0.f;
      if (li < K - 32) {
        const float g1 = (acc[2][r] + gbias[2]) * gemm_sigmoid(acc[3][r] + gbias[3]);
        Gs[row * GLDF + 32 + li] = in ? g1 : 0.f;
      }
    }
    // (rows tid / 2 of a wave's 64 threads are that wave's own 32 rows: only the wave's own LDS stores are needed here)
    {
      const int row = tid >> 1, half = tid & 1;
      const float* g = Gs + row * GLDF;
      const float* w = wls + half * 4 * K;
      f32x4 p = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
      for (int c = 0; c < K; c += 4) {
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const f32x4 wv = *reinterpret_cast<const f32x4*>(w + j * K + c);
          p[j] += gv[0] * wv[0] + gv[1] * wv[1] + gv[2] * wv[2] + gv[3] * wv[3];
        }
      }
      *reinterpret_cast<f32x4*>(Ps + row * 8 + 4 * half) = p;
    }
    __syncthreads();                                       // p of all 128 rows
    if (tid < 2 * TT_OUT) {
      const int i = 1 + (tid >> 1), j = (tid & 1) * 2;     // tile row of the group, first of its two samples
      const int t = tbase + i;                             // group index: 127 tile .. 127 tile + 126
      if (t < groups) {
        float2 o;
        o.x = bias + Ps[i * 8 + j] + Ps[(i - 1) * 8 + 4 + j];
        o.y = bias + Ps[i * 8 + j + 1] + Ps[(i - 1) * 8 + 5 + j];
        *reinterpret_cast<float2*>(yb + 4 * (size_t)t + j) = o;
      }
    }
    __syncthreads();                                       // p and g are free: the next tile's A may be staged
  }
}

// ---------------------------------------------------------------------------------- first encoder level in one launch
// Conv1d(1 -> C, k8, s4) + ReLU + Conv1d(C -> 2C, 1) + GLU of the first encoder level (model.py:66-75,303-307): x (B, Lin) -> h
// (B, Lout, C).  gemm_shortk_bf16x3_kernel<true, 48, 48> does the same with 128 x 64 tiles, i.e. TWO workgroups (the value /
// gate column pairs 0..31 and 32..47) each evaluate the first convolution for the same 128 rows; here a workgroup owns all 128
// packed columns: the first convolution (fp32 FMAs, bias then taps 0..7 -- conv1d_c1_kernel's order) and the bf16 split run once
// per row, W is staged once per workgroup and reused for TT_TPW tiles.
__global__ __launch_bounds__(256, 2) void c1_glu_kernel(const float* __restrict__ x, int Lin, int Lout, const float* __restrict__ w1,
                                                        const float* __restrict__ b1, const float* __restrict__ gw,
                                                        const float* __restrict__ gb, float* __restrict__ y, int tiles_per_clip) {
  constexpr int K = TT_K, ROW = TT_ROW, QPR = K / 4, NQ = 128 * QPR / 256;
  constexpr int NSLOT = 7;                                                      // rows per first-convolution thread: cr + 21 p
  __shared__ __attribute__((aligned(16))) char As[128 * ROW];
  __shared__ __attribute__((aligned(16))) char Ws[128 * ROW];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int b = blockIdx.y;
  const int tile0 = blockIdx.x * TT_TPW;
  const float* xb = x + (size_t)b * Lin;
  char* yb = reinterpret_cast<char*>(y + (size_t)b * Lout * K);
  // first-convolution slot of a thread: channel quad cq, rows cr + 21 p of every tile (252 of the 256 threads); the 8 samples under
  // a row come straight from memory (two aligned float4, L1 hits for the 11 other quads of the row), one tile ahead
  const int cq = tid % QPR, cr = tid / QPR;
  f32x4 xr[NSLOT][2];
  auto load_x = [&](int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int p = 0; p < NSLOT; ++p) {
      int m = tile * 128 + cr + 21 * p;
      m = m < Lout ? m : Lout - 1;                         // rows past Lout (and slots past row 127) are never used
      const float* px = xb + 4 * (size_t)m;
      xr[p][0] = *reinterpret_cast<const f32x4*>(px);
      xr[p][1] = *reinterpret_cast<const f32x4*>(px + 4);
    }
  };
  if (tid < 252) load_x(tile0);
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int idx = tid + 256 * i;
    split_store(Ws + (idx / QPR) * ROW, idx % QPR, 2 * K, *reinterpret_cast<const f32x4*>(gw + (size_t)(idx / QPR) * K + 4 * (idx % QPR)));
  }
  f32x4 wq[9];                                               // the quad's 8 taps and bias
#pragma unroll
  for (int j = 0; j < 8; ++j) wq[j] = *reinterpret_cast<const f32x4*>(w1 + j * K + 4 * cq);
  wq[8] = *reinterpret_cast<const f32x4*>(b1 + 4 * cq);
  float gbias[4];
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) gbias[nt] = gb[nt * 32 + li];
  const char* Ap = frag_ptr(As, wave * 32 + li, ROW, lh);
  const char* Bp = frag_ptr(Ws, li, ROW, lh);
  const int ntile = tiles_per_clip - tile0 < TT_TPW ? tiles_per_clip - tile0 : TT_TPW;
  for (int it = 0; it < ntile; ++it) {
    const int tile = tile0 + it;
    // A = relu(b1 + sum_j w1[j] * x[4 row + j]), bias then taps 0..7 (conv1d_c1_kernel's order), split into LDS
    if (tid < 252) {
#pragma unroll
      for (int p = 0; p < NSLOT; ++p) {
        const int row = cr + 21 * p;
        if (row < 128) {
          f32x4 v = wq[8];
          // One v_fma_f32 per element, kept from being paired (the empty asm).  Written as `v += x * wq[j]` hipcc emits
          // v_pk_fma_f32 with op_sel:[0,1,0] (the LOW lane takes the HIGH half of the sample pair) for the odd samples, and with
          // TWO workgroups per CU -- i.e. while the SIMD's other wave runs MFMAs -- the low lane of those instructions sporadically
          // came out wrong: wrong rows of A, different from run to run, only at > 256 workgroups; bit-exact with one workgroup per
          // CU, with this form, and in the 128 x 64-tile GEMM form, whose loader only uses the op_sel_hi:[1,0,1] broadcast
          // (profiles/r02_pk_fma_op_sel.md; tests/test_isa_scan.py keeps the packed form out of the library).
#pragma unroll
          for (int j = 0; j < 8; ++j)
#pragma unroll
            for (int k = 0; k < 4; ++k) {
              float t = __builtin_fmaf(xr[p][j >> 2][j & 3], wq[j][k], v[k]);
              asm volatile("" : "+v"(t));
              v[k] = t;
            }
#pragma unroll
          for (int k = 0; k < 4; ++k) v[k] = v[k] > 0.f ? v[k] : 0.f;
          split_store(As + row * ROW, cq, 2 * K, v);
        }
      }
      if (it + 1 < ntile) load_x(tile + 1);
    }
    __syncthreads();                                       // A (and, the first time, W) staged
    floatx16 acc[4];
    clear_acc(acc);
#pragma unroll
    for (int s = 0; s < K / 16; ++s) wave_step_bf16x3<4, ROW, 2 * K>(acc, Ap + 32 * s, Bp + 32 * s);
    const int mbase = tile * 128 + wave * 32 + 4 * lh;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = mbase + (r & 3) + 8 * (r >> 2);
      if (m < Lout) {
        const unsigned o = ((unsigned)m * K + (unsigned)li) * 4u;
        st_f32(yb, o, (acc[0][r] + gbias[0]) * gemm_sigmoid(acc[1][r] + gbias[1]));
        if (li < K - 32) st_f32(yb, o + 128u, (acc[2][r] + gbias[2]) * gemm_sigmoid(acc[3][r] + gbias[3]));
      }
    }
    __syncthreads();                                       // every wave has read its A fragments: the next tile may be staged
  }
}

// ---------------------------------------------------------------------------------- the launch table
// Every mfpa_gemm_mfma kernel that exists, in the order of the MFPA_GEMM_* ids (include/mfpa.h): each entry made from the kernel's own
// geometry, so the launch cannot ask for another tile or other LDS bytes than the kernel lays out.  persistent: the grid is clamped to the
// CUs and a workgroup walks the tiles.
struct GemmKernel { int id; void (*kernel)(GemmArgs); int threads, bm, bn, lds_bytes; bool persistent; };
template <class G> constexpr GemmKernel k_gemm(int id, void (*kernel)(GemmArgs), bool persistent = false) {
  return {id, kernel, G::THREADS, G::BM, G::BN, G::lds_bytes, persistent};
}
template <bool WSPLIT> constexpr GemmKernel k_pipe(int id) { return k_gemm<PipeGeo>(id, gemm_bf16x3_pipe_kernel<WSPLIT>, true); }
template <bool WSPLIT> constexpr GemmKernel k_wide(int id) { return k_gemm<WideGeo>(id, gemm_bf16x3_wide_kernel<WSPLIT>); }
template <bool C1SRC, int K, int KCW> constexpr GemmKernel k_shortk(int id) { return k_gemm<ShortKGeo<C1SRC, K, KCW>>(id, gemm_shortk_bf16x3_kernel<C1SRC, K, KCW>); }
template <bool C1SRC, int K> constexpr GemmKernel k_smallk(int id) { return k_gemm<SmallKGeo<C1SRC, K>>(id, gemm_smallk_kernel<C1SRC, K>); }
template <bool C1SRC> constexpr GemmKernel k_fp32(int id) { return k_gemm<Fp32Geo>(id, gemm_mfma_kernel<C1SRC>); }
constexpr GemmKernel GEMM_KERNELS[] = {
    k_pipe<false>(MFPA_GEMM_PIPE), k_pipe<true>(MFPA_GEMM_PIPE_WSPLIT), k_wide<false>(MFPA_GEMM_WIDE), k_wide<true>(MFPA_GEMM_WIDE_WSPLIT),
    k_gemm<Bf16x3Geo>(MFPA_GEMM_BF16X3, gemm_bf16x3_kernel),
    k_shortk<true, 48, 48>(MFPA_GEMM_SHORTK48_C1), k_shortk<false, 48, 48>(MFPA_GEMM_SHORTK48), k_shortk<false, 96, 48>(MFPA_GEMM_SHORTK96),
    k_smallk<true, 48>(MFPA_GEMM_SMALLK48_C1), k_smallk<false, 48>(MFPA_GEMM_SMALLK48), k_fp32<true>(MFPA_GEMM_MFMA_C1), k_fp32<false>(MFPA_GEMM_MFMA)};
constexpr int GEMM_NKERNELS = sizeof(GEMM_KERNELS) / sizeof(GEMM_KERNELS[0]);
constexpr bool gemm_kernels_in_id_order() {
  for (int i = 0; i < GEMM_NKERNELS; ++i)
    if (GEMM_KERNELS[i].id != i) return false;
  return true;
}
static_assert(gemm_kernels_in_id_order(), "GEMM_KERNELS is indexed by the MFPA_GEMM_* id");

}  // namespace

extern "C" {

constexpr int PIPE_MIN_M = 192;   // rows per clip from which the pipelined 256 x 128 kernel serves (rows past M are clamped when loaded: a 249-row clip fills 97 % of a 256-row tile)

// Validation and kernel choice of mfpa_gemm_mfma, host arithmetic only: MFPA_EINVAL, or MFPA_OK with *id = the MFPA_GEMM_* kernel that
// serves `d` (MFPA_GEMM_NONE: nothing to do).  The launcher below looks the id up in GEMM_KERNELS; the conditions exist here and nowhere else.
static int gemm_route(const mfpa_gemm_desc* d, int* id) {
  constexpr int GBN = 64, WBN = WideGeo::BN;   // the narrowest tile's columns (npad's unit) and the 128-column tiles'
  *id = MFPA_GEMM_NONE;
  if (!d) return MFPA_EINVAL;
  if (d->batch == 0 || d->M == 0) return MFPA_OK;
  if ((!d->A && !d->c1_x) || !d->W || !d->C || d->batch < 0 || d->M < 0 || d->N < 1 || d->K < GKC || d->K % GKC) return MFPA_EINVAL;
  if (d->c1_x && (!d->c1_w || !d->c1_b || d->K > 256 || (d->precision == 1 && d->K >= 128) || d->c1_lin < 4 * ((long long)d->M - 1) + 8 ||
                  d->c1_lin % 4)) return MFPA_EINVAL;
  if (d->npad < 64 || d->npad % 64 || d->mode < 0 || d->mode > 3 || (d->mode >= 2 && !d->addend)) return MFPA_EINVAL;
  if (d->lda % 4 || d->strideA % 4) return MFPA_EINVAL;   // float4 row loads
  {   // the epilogue addresses a clip's outputs with 32-bit byte offsets
    const long long lim = 0x3fffffffLL;      // floats
    if ((long long)d->M * d->ldc + d->npad > lim || (d->C2 && (long long)d->M * d->ldc2 + d->npad > lim) ||
        (d->mode >= 2 && (long long)d->M * d->ldadd + d->npad > lim)) return MFPA_EINVAL;
  }
  if (d->mode == 1 ? (d->N > d->npad / 2) : (d->N > d->npad)) return MFPA_EINVAL;
  if ((long long)(d->npad / GBN) * ((d->M + GBM - 1) / GBM) * d->batch > 0x3fffffffLL) return MFPA_EINVAL;
  if (d->precision < 0 || d->precision > 2) return MFPA_EINVAL;
  if (d->precision == 2 && !(d->K % HKC == 0 && d->K >= 128 && d->npad % WBN == 0 && !d->c1_x)) return MFPA_EINVAL;   // pre-split W: the wide kernel only
  // K >= 128: the chunked bf16x3 kernel.  (At first the K = 128 / 192 levels ran faster on the fp32 kernel; that was the
  // epilogue's serialised addend loads and 64-bit addressing, not the arithmetic: with those fixed the fp32 MFMA rate is what
  // bounds them -- PMC: 2.2 of 4.0 ms MFMA-busy on the K = 192 transposed convolution -- and bf16x3 is 10 % faster end to end.)
  // 128-column tiles whenever the padded N allows them (precision 2 always does, see above)
  const bool wide_ok = d->precision >= 1 && d->K % HKC == 0 && d->K >= 128 && d->npad % WBN == 0;
  if (wide_ok && d->K % (2 * HKC) == 0 && d->M >= PIPE_MIN_M) *id = d->precision == 2 ? MFPA_GEMM_PIPE_WSPLIT : MFPA_GEMM_PIPE;
  else if (wide_ok) *id = d->precision == 2 ? MFPA_GEMM_WIDE_WSPLIT : MFPA_GEMM_WIDE;
  else if (d->precision == 1 && d->K % HKC == 0 && d->K >= 128) *id = MFPA_GEMM_BF16X3;
  else if (d->precision == 1 && d->K == 48 && d->c1_x) *id = MFPA_GEMM_SHORTK48_C1;
  else if (d->precision == 1 && d->K == 48) *id = MFPA_GEMM_SHORTK48;
  else if (d->precision == 1 && d->K == 96 && !d->c1_x) *id = MFPA_GEMM_SHORTK96;
  else if (d->K == 48 && d->c1_x) *id = MFPA_GEMM_SMALLK48_C1;
  else if (d->K == 48) *id = MFPA_GEMM_SMALLK48;
  else if (d->c1_x) *id = MFPA_GEMM_MFMA_C1;
  else *id = MFPA_GEMM_MFMA;
  return MFPA_OK;
}

int mfpa_gemm_mfma_route(const mfpa_gemm_desc* d, int* kernel_id) {
  int id;
  const int rc = gemm_route(d, &id);
  if (kernel_id) *kernel_id = id;
  return rc;
}

int mfpa_gemm_mfma(const mfpa_gemm_desc* d, void* stream) {
  int id;
  const int rc = gemm_route(d, &id);
  if (rc != MFPA_OK || id == MFPA_GEMM_NONE) return rc;
  if (id < 0 || id >= GEMM_NKERNELS) return MFPA_EINVAL;   // an id without an entry
  const GemmKernel& k = GEMM_KERNELS[id];
  GemmArgs a{};
  a.A = d->A; a.lda = d->lda; a.strideA = d->strideA; a.W = d->W; a.bias = d->bias;
  a.addend = d->addend; a.ldadd = d->ldadd; a.strideAdd = d->strideAdd;
  a.C = d->C; a.ldc = d->ldc; a.strideC = d->strideC;
  a.C2 = d->C2; a.ldc2 = d->ldc2; a.strideC2 = d->strideC2;
  a.M = d->M; a.N = d->N; a.K = d->K; a.mode = d->mode; a.relu = d->relu;
  a.c1_x = d->c1_x; a.c1_lin = d->c1_lin; a.c1_w = d->c1_w; a.c1_b = d->c1_b;
  a.nx = d->npad / k.bn; a.ny = (d->M + k.bm - 1) / k.bm; a.nz = d->batch;
  unsigned grid = (unsigned)((((long long)a.nx * a.ny * a.nz + 7) / 8) * 8);   // the 1-D tile count, 8-aligned (gemm_tile_at's XCD ranges)
  if (k.persistent) {             // one workgroup per CU walks the tiles (a multiple of 8: XCD ranges)
    const unsigned cus8 = (unsigned)((mfpa_current_device_cus() + 7) / 8 * 8);
    if (cus8 >= 8 && grid > cus8) grid = cus8;
  }
  hipLaunchKernelGGL(k.kernel, dim3(grid), dim3(k.threads), k.lds_bytes, mfpa_stream(stream), a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

/* Last decoder level of Demucs in one launch (model.py:80-88: Conv1d(C, 2C, 1) + GLU + ConvTranspose1d(C, 1, 8, 4), no ReLU):
 * x (B, L, C) -> y (B, 4 (L + 1)).  gw / gb = the 1x1 weights and bias in the packed GLU tile order of mfpa_gemm_mfma mode 1
 * (128 rows x C for C = 48), wl (8, C) tap-major = weight[c][0][j], bias = the ConvTranspose1d bias.  C must be 48. */
int mfpa_glu_convT1d_c1(const float* x, int B, int L, int C, const float* gw, const float* gb, const float* wl, float bias, float* y,
                        void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !gw || !gb || !wl || !y || B < 0 || L < 1 || C != TT_K || B > 65535) return MFPA_EINVAL;
  const int groups = L + 1;
  const int tiles = (groups + TT_OUT - 1) / TT_OUT;
  hipLaunchKernelGGL(glu_convT_c1_kernel, dim3((tiles + TT_TPW - 1) / TT_TPW, B), dim3(FusedGeo::THREADS), FusedGeo::lds_bytes, mfpa_stream(stream), x, L,
                     gw, gb, wl, bias, y, tiles, groups);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

/* First encoder level of Demucs in one launch (model.py:66-75: Conv1d(1, C, 8, 4) + ReLU + Conv1d(C, 2C, 1) + GLU):
 * x (B, Lin) -> y (B, Lout, C), Lout = (Lin - 8) / 4 + 1.  w1 (8, C) tap-major and b1 (C) as for mfpa_conv1d_c1; gw (128, C) / gb
 * (128) in the packed GLU tile order of mfpa_gemm_mfma mode 1.  C must be 48. */
int mfpa_conv1d_c1_glu(const float* x, int B, int Lin, int Lout, int C, const float* w1, const float* b1, const float* gw,
                       const float* gb, float* y, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!x || !w1 || !b1 || !gw || !gb || !y || B < 0 || B > 65535 || C != TT_K || Lout < 1 || Lin < 4 * ((long long)Lout - 1) + 8 ||
      (long long)Lout * C * 4 > 0xffffffffLL || Lin % 4 != 0 || ((size_t)x & 15) != 0)        // the rows' samples are read as aligned float4
    return MFPA_EINVAL;
  const int tiles = (Lout + 127) / 128;
  hipLaunchKernelGGL(c1_glu_kernel, dim3((tiles + TT_TPW - 1) / TT_TPW, B), dim3(FusedGeo::THREADS), FusedGeo::lds_bytes, mfpa_stream(stream), x, Lin,
                     Lout, w1, b1, gw, gb, y, tiles);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
