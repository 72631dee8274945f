// Demucs training step, backward-pass kernels for MI355X (gfx950) -- SURVEY.md §8f-2 ("+ MRSTFT loss train step").
// Reference: training/train.py:275-312 (input_type == "audio": L1 + MultiResolutionSTFTLoss, loss.backward(), Adam) over
// training/model.py:163-326.  torch autograd is not used: every layer's adjoint is written out.
//
// Activations are time-major (B, L, C) like the forward (csrc/demucs.hip, csrc/demucs_gemm.hip).  Input gradients of every Conv1d /
// ConvTranspose1d / 1x1 / LSTM projection are again strided-window GEMMs served by mfpa_gemm_mfma (csrc/demucs_gemm.hip; a Conv1d's input
// gradient is a ConvTranspose1d of the output gradient and vice versa); its epilogue applies the ReLU mask of the layer
// below (mode 3).  The LSTM's backward recurrence is csrc/lstm.hip.  This file holds what else that kernel cannot express:
//   gemm_tn_kernel        weight gradients  dW[m][n] += sum_rows dY[row][m] * Xwin[row][n]  (K = every time step of the batch)
//   glu_bwd_kernel        GLU backward on the packed [32 values | 32 gates] pre-activation tiles the forward saved
//   downsample2 adjoint, the two 1-channel convolutions' weight gradients, column sums (bias gradients)
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"

namespace {

using mfpa_tile::bf16x4;
using mfpa_tile::bf16x8;
using mfpa_tile::f32x4;
using mfpa_tile::floatx16;

// ---------------------------------------------------------------------------------- weight-gradient GEMM ("TN")
// C[m][n] += sum_{b < batch} sum_{r < R} A[b*strideA + r*lda + m] * Bm[b*strideB + r*ldb + n]
// Both operands are K-major in memory (a row = one time step), which is exactly the fragment order of
// v_mfma_f32_32x32x2_f32: lane (i, k) of the A operand holds A[k][i], so the tiles are staged as they lie in HBM
// ([k][m] rows, 32-float pad so the two k rows a wave reads fall on disjoint banks) and read with ds_read_b32.
// K is split over blockIdx.y (row ranges that never straddle a clip); partial tiles are added with float atomics.
struct TnArgs {
  const float* A; long long lda, strideA;
  const float* Bm; long long ldb, strideB;
  float* C; long long ldc;
  float* colsum;               // optional: colsum[m] += sum over all rows of A[.][m] (the bias gradient), by the n-tile-0 workgroups
  int R, M, N;
  int rs, spb;                 // rows per split, splits per clip
  int tiles, nsplit;           // 1-D launch: tiles x nsplit workgroups
};

// (tile, split) of a workgroup.  Every tile of one K split reads the same rows of A and Bm; consecutive workgroup ids go round-robin
// over the 8 XCDs (one L2 each), so in the plain order each XCD fetched every split's rows.  Here XCD k owns a contiguous range
// of the (split, tile) order, tiles fastest: the tiles of a split run back to back on ONE XCD.
__device__ __forceinline__ bool tn_tile(const TnArgs& a, int& tile, int& split) {
  const unsigned total = (unsigned)a.tiles * a.nsplit;
  const unsigned per = (total + 7) / 8;
  const unsigned lin = (blockIdx.x % 8) * per + blockIdx.x / 8;
  if (lin >= total) return false;
  tile = lin % a.tiles;
  split = lin / a.tiles;
  return true;
}

// column sums of the A tiles a workgroup staged (every thread keeps the same column quad for all of its loads): combine the row
// lanes through LDS, one atomic per column
template <int QA>
__device__ __forceinline__ void tn_colsum_flush(float* red, f32x4 csum, int tid, int m0, int M, float* __restrict__ out) {
  __syncthreads();                                   // the operand buffers are free
  const int q = tid % QA, rl = tid / QA;
  *reinterpret_cast<f32x4*>(red + (rl * QA + q) * 4) = csum;
  __syncthreads();
  if (tid < QA * 4) {
    const int qq = tid >> 2, k = tid & 3;
    float sacc = 0.f;
#pragma unroll
    for (int r = 0; r < 256 / QA; ++r) sacc += red[(r * QA + qq) * 4 + k];
    const int m = m0 + 4 * qq + k;
    if (m < M) unsafeAtomicAdd(out + m, sacc);
  }
}

constexpr int TKC = 16;

template <int TM, int TN>
__global__ __launch_bounds__(256) void gemm_tn_kernel(TnArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int LDA_ = BM + 32, LDB_ = BN + 32;
  constexpr int QA = BM / 4, QB = BN / 4;                // float4 per staged row
  constexpr int FA = TKC * QA / 256, FB = TKC * QB / 256;  // float4 per thread per chunk (TM, TN)
  __shared__ __attribute__((aligned(16))) float As[2][TKC * LDA_];
  __shared__ __attribute__((aligned(16))) float Bs[2][TKC * LDB_];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int ntn = (a.N + BN - 1) / BN;
  int tile, split;
  if (!tn_tile(a, tile, split)) return;              // uniform, before any barrier
  const int n0 = (tile % ntn) * BN, m0 = (tile / ntn) * BM;
  const int b = split / a.spb;
  const int rbeg = (split % a.spb) * a.rs;
  const int rend = rbeg + a.rs < a.R ? rbeg + a.rs : a.R;
  const float* Ab = a.A + (size_t)b * a.strideA;
  const float* Bb = a.Bm + (size_t)b * a.strideB;
  const int nk = (rend - rbeg + TKC - 1) / TKC;

  f32x4 ar[FA], br[FB];
  const bool do_colsum = a.colsum != nullptr && n0 == 0;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
      const int idx = tid + 256 * i, row = idx / QA, q = idx % QA;
      const int r = rbeg + kc * TKC + row, m = m0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rend && m < a.M) v = *reinterpret_cast<const f32x4*>(Ab + (size_t)r * a.lda + m);
      ar[i] = v;
    }
#pragma unroll
    for (int i = 0; i < FB; ++i) {
      const int idx = tid + 256 * i, row = idx / QB, q = idx % QB;
      const int r = rbeg + kc * TKC + row, n = n0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rend && n < a.N) v = *reinterpret_cast<const f32x4*>(Bb + (size_t)r * a.ldb + n);
      br[i] = v;
    }
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&As[buf][(idx / QA) * LDA_ + 4 * (idx % QA)]) = ar[i];
      if (do_colsum) csum += ar[i];
    }
#pragma unroll
    for (int i = 0; i < FB; ++i) {
      const int idx = tid + 256 * i;
      *reinterpret_cast<f32x4*>(&Bs[buf][(idx / QB) * LDB_ + 4 * (idx % QB)]) = br[i];
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load(0);
    store(0);
    if (nk > 1) load(1);
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
      const int buf = kc & 1;
      if (kc + 1 < nk) store(buf ^ 1);
      if (kc + 2 < nk) load(kc + 2);
      const float* Ap = &As[buf][lh * LDA_ + wm * 32 * TM + li];
      const float* Bp = &Bs[buf][lh * LDB_ + wn * 32 * TN + li];
#pragma unroll
      for (int s = 0; s < TKC / 2; ++s) {
        float af[TM], bf[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) af[i] = Ap[2 * s * LDA_ + 32 * i];
#pragma unroll
        for (int j = 0; j < TN; ++j) bf[j] = Bp[2 * s * LDB_ + 32 * j];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i], bf[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  if (do_colsum) tn_colsum_flush<QA>(&As[0][0], csum, tid, m0, a.M, a.colsum);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * 32 * TN + 32 * j + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 * TM + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < a.M && n < a.N) unsafeAtomicAdd(a.C + (size_t)m * a.ldc + n, acc[i][j][r]);
      }
    }
}

// The same product on the bf16 matrix cores (precision 1: bf16x3, precision 2: plain bf16).  K is the ROW index and rows are
// what is contiguous in HBM, so the 8-consecutive-k fragments of v_mfma_f32_32x32x16_bf16 come from gfx950's transposing LDS
// read ds_read_b64_tr_b16 (lane i of a 16-lane group receives column i of a 4-row x 16-column block): the tiles stay in their
// natural [k][m] order.  LDS row = [BM bf16 hi | BM bf16 lo (bf16x3 only) | 64 B pad], which puts the four rows of a block on
// bank offsets 0 / 64 / 128 / 192.  Plain bf16 is the default for training: a weight gradient sums over every time step of the
// batch, so the 2^-9 product rounding averages out, and only the optimiser consumes the result (as for the UNet).
typedef short t_s16x4 __attribute__((ext_vector_type(4)));
constexpr int HKC_T = 32;

__device__ __forceinline__ bf16x8 tn_tr_frag(const char* p0, const char* p1) {
  typedef t_s16x4 __attribute__((address_space(3))) * lds_ptr;
  const t_s16x4 u = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p0));
  const t_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_ptr)(p1));
  union { short s[8]; bf16x8 b; } r;
#pragma unroll
  for (int j = 0; j < 4; ++j) { r.s[j] = u[j]; r.s[4 + j] = v[j]; }
  return r.b;
}

template <int TM, int TN, bool PLAIN>
__global__ __launch_bounds__(256) void gemm_tn_bf16_kernel(TnArgs a) {
  constexpr int BM = 64 * TM, BN = 64 * TN;
  constexpr int ROWA = (PLAIN ? 2 : 4) * BM + 64, ROWB = (PLAIN ? 2 : 4) * BN + 64;     // bytes
  constexpr int QA = BM / 4, QB = BN / 4;
  constexpr int FA = HKC_T * QA / 256, FB = HKC_T * QB / 256;
  extern __shared__ __attribute__((aligned(16))) char tsm[];
  char* As = tsm;                                  // [2][HKC_T][ROWA]
  char* Bs = tsm + 2 * HKC_T * ROWA;               // [2][HKC_T][ROWB]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int ntn = (a.N + BN - 1) / BN;
  int tile, split;
  if (!tn_tile(a, tile, split)) return;              // uniform, before any barrier
  const int n0 = (tile % ntn) * BN, m0 = (tile / ntn) * BM;
  const int b = split / a.spb;
  const int rbeg = (split % a.spb) * a.rs;
  const int rend = rbeg + a.rs < a.R ? rbeg + a.rs : a.R;
  const float* Ab = a.A + (size_t)b * a.strideA;
  const float* Bb = a.Bm + (size_t)b * a.strideB;
  const int nk = (rend - rbeg + HKC_T - 1) / HKC_T;
  // transposing read: lane 4q+p of a 16-lane group addresses row q, columns 4p..4p+3 of its block
  const int gl = lane & 15, tq = gl >> 2, tp = gl & 3, gsel = (lane >> 4) & 1;
  const int a_off = (8 * lh + tq) * ROWA + (wm * 32 * TM + 16 * gsel + 4 * tp) * 2;
  const int b_off = (8 * lh + tq) * ROWB + (wn * 32 * TN + 16 * gsel + 4 * tp) * 2;

  f32x4 ar[FA], br[FB];
  const bool do_colsum = a.colsum != nullptr && n0 == 0;
  f32x4 csum = {0.f, 0.f, 0.f, 0.f};
  auto load = [&](int kc) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
      const int idx = tid + 256 * i, row = idx / QA, q = idx % QA;
      const int r = rbeg + kc * HKC_T + row, m = m0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rend && m < a.M) v = *reinterpret_cast<const f32x4*>(Ab + (size_t)r * a.lda + m);
      ar[i] = v;
    }
#pragma unroll
    for (int i = 0; i < FB; ++i) {
      const int idx = tid + 256 * i, row = idx / QB, q = idx % QB;
      const int r = rbeg + kc * HKC_T + row, n = n0 + 4 * q;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (r < rend && n < a.N) v = *reinterpret_cast<const f32x4*>(Bb + (size_t)r * a.ldb + n);
      br[i] = v;
    }
  };
  auto split_store = [&](char* row, int q, int lo_off, f32x4 v) __attribute__((always_inline)) {
    bf16x4 hi, lo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      hi[k] = (__bf16)v[k];
      lo[k] = (__bf16)(v[k] - (float)hi[k]);
    }
    *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
    if (!PLAIN) *reinterpret_cast<bf16x4*>(row + lo_off + 8 * q) = lo;
  };
  auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < FA; ++i) {
      const int idx = tid + 256 * i;
      split_store(As + (buf * HKC_T + idx / QA) * ROWA, idx % QA, 2 * BM, ar[i]);
      if (do_colsum) csum += ar[i];
    }
#pragma unroll
    for (int i = 0; i < FB; ++i) {
      const int idx = tid + 256 * i;
      split_store(Bs + (buf * HKC_T + idx / QB) * ROWB, idx % QB, 2 * BN, br[i]);
    }
  };

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  if (nk > 0) {
    load(0);
    store(0);
    if (nk > 1) load(1);
    __syncthreads();
    for (int kc = 0; kc < nk; ++kc) {
      const int buf = kc & 1;
      if (kc + 1 < nk) store(buf ^ 1);
      if (kc + 2 < nk) load(kc + 2);
      const char* Ap = As + buf * HKC_T * ROWA + a_off;
      const char* Bp = Bs + buf * HKC_T * ROWB + b_off;
#pragma unroll
      for (int ks = 0; ks < HKC_T / 16; ++ks) {
        bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
          const char* p = Ap + 16 * ks * ROWA + 64 * i;
          ah[i] = tn_tr_frag(p, p + 4 * ROWA);
          if (!PLAIN) al[i] = tn_tr_frag(p + 2 * BM, p + 4 * ROWA + 2 * BM);
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const char* p = Bp + 16 * ks * ROWB + 64 * j;
          bh[j] = tn_tr_frag(p, p + 4 * ROWB);
          if (!PLAIN) bl[j] = tn_tr_frag(p + 2 * BN, p + 4 * ROWB + 2 * BN);
        }
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int j = 0; j < TN; ++j) {
            if (!PLAIN) {
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
              acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
            }
            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
          }
      }
      __syncthreads();
    }
  }
  if (do_colsum) tn_colsum_flush<QA>(reinterpret_cast<float*>(tsm), csum, tid, m0, a.M, a.colsum);
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * 32 * TN + 32 * j + li;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int m = m0 + wm * 32 * TM + 32 * i + (r & 3) + 8 * (r >> 2) + 4 * lh;
        if (m < a.M && n < a.N) unsafeAtomicAdd(a.C + (size_t)m * a.ldc + n, acc[i][j][r]);
      }
    }
}

// ---------------------------------------------------------------------------------- GLU backward
// u (rows, npad): packed pre-activations, tile t = [32 values | 32 gates] of output columns 32 t .. 32 t + 31 (< N).
// In place: u <- d(loss)/du given dg (rows, N columns, row pitch ldg).
__global__ __launch_bounds__(256) void glu_bwd_kernel(float* __restrict__ u, long long rows, int npad, int N,
                                                      const float* __restrict__ dg, long long ldg) {
  const int tiles = npad / 64;
  const long long total = rows * tiles * 8;              // one thread = 4 consecutive outputs of a tile
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
    const int q = (int)(e & 7);
    const long long rt = e >> 3;
    const int t = (int)(rt % tiles);
    const long long row = rt / tiles;
    float* up = u + row * npad + t * 64 + 4 * q;
    const f32x4 v = *reinterpret_cast<const f32x4*>(up), s = *reinterpret_cast<const f32x4*>(up + 32);
    const int n = t * 32 + 4 * q;
    f32x4 d = {0.f, 0.f, 0.f, 0.f};
    if (n < N) d = *reinterpret_cast<const f32x4*>(dg + row * ldg + n);   // N is a multiple of 4
    f32x4 dv, ds;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float sg = 1.f / (1.f + __expf(-s[k]));
      dv[k] = d[k] * sg;
      ds[k] = d[k] * v[k] * sg * (1.f - sg);
    }
    *reinterpret_cast<f32x4*>(up) = dv;
    *reinterpret_cast<f32x4*>(up + 32) = ds;
  }
}

// ---------------------------------------------------------------------------------- column sums (bias gradients)
// out[c] += sum_r x[r*ld + c], any C that is a multiple of 4 (48, 96, ... 3072).  A thread keeps float4 register
// accumulators for its column quad(s) and walks the rows of its block's range (four independent loads in flight); the
// row lanes are combined once per block through LDS, then one global atomic per column and block.
template <int NQ>
__global__ __launch_bounds__(256) void colsum_any_kernel(const float* __restrict__ x, long long rows, int C, long long ld,
                                                         float* __restrict__ out, long long rows_per_block) {
  extern __shared__ float accs[];
  const int tid = threadIdx.x;
  for (int c = tid; c < C; c += 256) accs[c] = 0.f;
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * rows_per_block;
  const long long r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
  const int Q = C / 4;
  const int QT = Q < 256 ? Q : 256;
  const int lanes = Q <= 256 ? 256 / Q : 1;
  const int q0 = tid % QT, rl = tid / QT;
  f32x4 acc[NQ];
#pragma unroll
  for (int i = 0; i < NQ; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (rl < lanes) {
    long long r = r0 + rl;
    for (; r + 3LL * lanes < r1; r += 4LL * lanes) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int q = q0 + 256 * i;
        if (q < Q) {
          const f32x4 v0 = *reinterpret_cast<const f32x4*>(x + r * ld + 4 * q);
          const f32x4 v1 = *reinterpret_cast<const f32x4*>(x + (r + lanes) * ld + 4 * q);
          const f32x4 v2 = *reinterpret_cast<const f32x4*>(x + (r + 2LL * lanes) * ld + 4 * q);
          const f32x4 v3 = *reinterpret_cast<const f32x4*>(x + (r + 3LL * lanes) * ld + 4 * q);
          acc[i] += (v0 + v1) + (v2 + v3);
        }
      }
    }
    for (; r < r1; r += lanes) {
#pragma unroll
      for (int i = 0; i < NQ; ++i) {
        const int q = q0 + 256 * i;
        if (q < Q) acc[i] += *reinterpret_cast<const f32x4*>(x + r * ld + 4 * q);
      }
    }
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
      const int q = q0 + 256 * i;
      if (q < Q) {
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(&accs[4 * q + k], acc[i][k]);
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) unsafeAtomicAdd(out + c, accs[c]);
}

// ---------------------------------------------------------------------------------- 1-channel convolutions' weight gradients
// dw[j][c] += sum_{b,t} x[b*ldx + 4t + j] * g[b*strideG + t*ldg + c],  j < 8, t < L   (w (8, C) tap-major)
// serves encoder.0.0 (x = the upsampled input, g = the masked gradient of its ReLU output) and the last
// ConvTranspose1d (x = the gradient of its output, g = the GLU output it consumed).
__global__ __launch_bounds__(256) void c1_wgrad_kernel(const float* __restrict__ x, long long ldx, const float* __restrict__ g,
                                                       long long ldg, long long strideG, int L, int C, float* __restrict__ dw,
                                                       int rows_per_block) {
  __shared__ float accs[8 * 256];                        // C <= 256
  const int tid = threadIdx.x, b = blockIdx.y;
  for (int i = tid; i < 8 * C; i += 256) accs[i] = 0.f;
  __syncthreads();
  const int Q = C / 4, lanes = 256 / Q;                  // row lanes per pass (Q = 12 for C = 48 -> 21 row lanes)
  const int q = tid % Q, rl = tid / Q;
  const int t0 = blockIdx.x * rows_per_block;
  const int t1 = t0 + rows_per_block < L ? t0 + rows_per_block : L;
  mfpa_f32x2 acc[8][2];                                  // [tap][channel pair]: packed FMAs without operand selection (mfpa_common.h)
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j][0] = acc[j][1] = mfpa_f32x2{0.f, 0.f};
  if (rl < lanes) {
    const float* xb = x + (size_t)b * ldx;
    const float* gb = g + (size_t)b * strideG;
    for (int t = t0 + rl; t < t1; t += lanes) {
      const f32x4 gv = *reinterpret_cast<const f32x4*>(gb + (size_t)t * ldg + 4 * q);
      const mfpa_f32x2 g01 = {gv[0], gv[1]}, g23 = {gv[2], gv[3]};
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)t), x1 = *reinterpret_cast<const f32x4*>(xb + 4 * (size_t)t + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const mfpa_f32x2 u = mfpa_bcast2(x0[j]), v = mfpa_bcast2(x1[j]);
        acc[j][0] += u * g01; acc[j][1] += u * g23;
        acc[4 + j][0] += v * g01; acc[4 + j][1] += v * g23;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) atomicAdd(&accs[j * C + 4 * q + k], acc[j][k >> 1][k & 1]);
  }
  __syncthreads();
  for (int i = tid; i < 8 * C; i += 256) unsafeAtomicAdd(dw + i, accs[i]);
}

// ---------------------------------------------------------------------------------- downsample2 adjoint
// forward (model.py:69-88): out[i] = sc * 0.5 * (x[2i] + sum_k xodd[i + k - 56] ker[k]), i < nout, xodd[j] = x[2j+1].
// adjoint: dx[2i] = g[i], dx[2j+1] = sum_k g[j + 56 - k] ker[k] with g[i] = 0.5 * sc * dy[i] (0 for i >= nout).
__global__ __launch_bounds__(256) void downsample2_adj_kernel(const float* __restrict__ dy, int ldy, int nout, const float* __restrict__ ker,
                                                              const float* __restrict__ scale, int T, float* __restrict__ dx) {
  __shared__ float kk[112];
  const int b = blockIdx.y, tid = threadIdx.x;
  if (tid < 112) kk[tid] = ker[tid];
  __syncthreads();
  const float sc = 0.5f * (scale ? scale[b] : 1.f);
  const float* dyb = dy + (size_t)b * ldy;
  float* dxb = dx + (size_t)b * T;
  for (int p = blockIdx.x * 256 + tid; p < T; p += gridDim.x * 256) {
    float v;
    if ((p & 1) == 0) {
      const int i = p >> 1;
      v = i < nout ? dyb[i] : 0.f;
    } else {
      const int j = p >> 1;
      float s = 0.f;
      for (int k = 0; k < 112; ++k) {
        const int i = j + 56 - k;
        if (i >= 0 && i < nout) s += dyb[i] * kk[k];
      }
      v = s;
    }
    dxb[p] = sc * v;
  }
}

}  // namespace

extern "C" {

int mfpa_gemm_tn(const mfpa_gemm_tn_desc* d, void* stream) {
  if (!d) return MFPA_EINVAL;
  if (d->batch == 0 || d->R == 0) return MFPA_OK;
  if (!d->A || !d->Bm || !d->C || d->batch < 0 || d->R < 0 || d->M < 4 || d->N < 4 || d->M % 4 || d->N % 4) return MFPA_EINVAL;
  if (d->lda % 4 || d->ldb % 4 || d->strideA % 4 || d->strideB % 4 || d->ldc < d->N) return MFPA_EINVAL;   // float4 row loads
  if (d->precision < 0 || d->precision > 2) return MFPA_EINVAL;
  const bool big = d->M > 64 && d->N > 64;
  const int BM = big ? 128 : 64, BN = big ? 128 : 64;
  const long long tiles = (long long)((d->M + BM - 1) / BM) * ((d->N + BN - 1) / BN);
  // rows per K split: about 2048 workgroups in all, at least 64 rows each, never across clips
  long long want = 2048 / tiles; if (want < 1) want = 1;
  long long rs = ((long long)d->batch * d->R + want - 1) / want;
  if (rs < 64) rs = 64;
  rs = (rs + HKC_T - 1) / HKC_T * HKC_T;
  long long spb = (d->R + rs - 1) / rs;
  if (tiles > 0x7fffffffLL) return MFPA_EINVAL;
  TnArgs a{};
  a.A = d->A; a.lda = d->lda; a.strideA = d->strideA; a.Bm = d->Bm; a.ldb = d->ldb; a.strideB = d->strideB;
  a.C = d->C; a.ldc = d->ldc; a.colsum = d->colsum; a.R = d->R; a.M = d->M; a.N = d->N; a.rs = (int)rs; a.spb = (int)spb;
  a.tiles = (int)tiles; a.nsplit = (int)(spb * d->batch);
  if (tiles * a.nsplit > 0x3fffffffLL) return MFPA_EINVAL;
  dim3 grid((unsigned)(((tiles * a.nsplit + 7) / 8) * 8));
  hipStream_t st = mfpa_stream(stream);
  if (d->precision == 0) {
    if (big) hipLaunchKernelGGL((gemm_tn_kernel<2, 2>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((gemm_tn_kernel<1, 1>), grid, dim3(256), 0, st, a);
  } else {
    const bool plain = d->precision == 2;
    const size_t lds = (size_t)2 * HKC_T * 2 * ((plain ? 2 : 4) * BM + 64);      // BM == BN
    if (big && plain) hipLaunchKernelGGL((gemm_tn_bf16_kernel<2, 2, true>), grid, dim3(256), lds, st, a);
    else if (big) hipLaunchKernelGGL((gemm_tn_bf16_kernel<2, 2, false>), grid, dim3(256), lds, st, a);
    else if (plain) hipLaunchKernelGGL((gemm_tn_bf16_kernel<1, 1, true>), grid, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((gemm_tn_bf16_kernel<1, 1, false>), grid, dim3(256), lds, st, a);
  }
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_glu_bwd(float* u, long long rows, int npad, int N, const float* dg, long long ldg, void* stream) {
  if (rows == 0) return MFPA_OK;
  if (!u || !dg || rows < 0 || npad < 64 || npad % 64 || N < 4 || N % 4 || N > npad / 2 || ldg < N || ldg % 4) return MFPA_EINVAL;
  const long long total = rows * (npad / 64) * 8;
  long long blocks = (total + 255) / 256; if (blocks > 65536) blocks = 65536;
  hipLaunchKernelGGL(glu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, mfpa_stream(stream), u, rows, npad, N, dg, ldg);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_colsum_any(const float* x, long long rows, int C, long long ld, float* out, void* stream) {
  if (rows == 0) return MFPA_OK;
  if (!x || !out || rows < 0 || C < 4 || C % 4 || C > 4096 || ld < C || ld % 4) return MFPA_EINVAL;
  long long blocks = (rows * (C / 4) + 256 * 32 - 1) / (256 * 32);      // about 32 float4 per thread
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  const long long rpb = (rows + blocks - 1) / blocks;
  blocks = (rows + rpb - 1) / rpb;
  if (C <= 1024)
    hipLaunchKernelGGL(colsum_any_kernel<1>, dim3((unsigned)blocks), dim3(256), (size_t)C * sizeof(float), mfpa_stream(stream), x, rows,
                       C, ld, out, rpb);
  else
    hipLaunchKernelGGL(colsum_any_kernel<4>, dim3((unsigned)blocks), dim3(256), (size_t)C * sizeof(float), mfpa_stream(stream), x, rows,
                       C, ld, out, rpb);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_c1_wgrad(const float* x, long long ldx, const float* g, long long ldg, long long strideG, int B, int L, int C, float* dw,
                  void* stream) {
  if (B == 0 || L == 0) return MFPA_OK;
  if (!x || !g || !dw || B < 0 || B > 65535 || L < 0 || C < 4 || C % 4 || C > 256 || ldx % 4 || ldg % 4 || strideG % 4 ||
      ldx < 4 * ((long long)L - 1) + 8) return MFPA_EINVAL;
  int gx = (L + 2047) / 2048; if (gx > 64) gx = 64;
  const int rpb = (L + gx - 1) / gx;
  gx = (L + rpb - 1) / rpb;
  hipLaunchKernelGGL(c1_wgrad_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), x, ldx, g, ldg, strideG, L, C, dw, rpb);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_downsample2_adjoint(const float* dy, int B, int ldy, int nout, const float* kernel112, const float* scale, int T, float* dx,
                             void* stream) {
  if (B == 0) return MFPA_OK;
  if (!dy || !kernel112 || !dx || B < 0 || B > 65535 || T < 2 || nout < 1 || nout > (T + 1) / 2 || ldy < nout) return MFPA_EINVAL;
  int gx = (T + 255) / 256; if (gx > 1024) gx = 1024;
  hipLaunchKernelGGL(downsample2_adj_kernel, dim3(gx, B), dim3(256), 0, mfpa_stream(stream), dy, ldy, nout, kernel112, scale, T, dx);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
