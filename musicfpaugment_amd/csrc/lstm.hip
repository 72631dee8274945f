// The LSTM recurrence of the Demucs denoiser for MI355X (gfx950), forward and backward -- torch.nn.LSTM of training/model.py:91-110
// of deezer/musicFPaugment: two layers, unidirectional, zero initial state.  The input projections of all steps are one GEMM
// (mfpa_gemm_mfma, csrc/demucs_gemm.hip); this file holds the recurrence, in both directions as one persistent launch per layer and time range or, where
// that grid cannot be resident, as one launch per time step:
//   lstm_step_kernel<MT>           forward step:  gates = h[t-1] W_hh^T + xp[t], then the cell update
//   lstm_seq_kernel<KS, MS>        forward range: W_hh in registers, h exchanged between workgroups in split form
//   lstm_step_bwd_kernel<MT, BUT>  backward step: dh = dhout[t] + dgates[t+1] W_hh, then the cell backward
//   lstm_bwd_seq_kernel<KS, MTB>   backward range: the forward range's scheme turned round
// and the thirteen mfpa_lstm_* entry points.  All products are bf16x3 (operands split hi + lo), fp32 accumulate.
#include "mfpa_common.h"
#include "mfpa_conv_tile.h"

namespace {

using mfpa_tile::bf16x4;
using mfpa_tile::bf16x8;
using mfpa_tile::f32x4;
using mfpa_tile::floatx16;

// ---------------------------------------------------------------------------------- what the four kernels share
constexpr int LKC = 128;                 // K chunk of the per-step kernels
constexpr int LROW = 4 * LKC + 16;       // their LDS row bytes: [128 hi | 128 lo | pad]
constexpr int LTHREADS = 512;            // their 8 waves
constexpr int LU = 16;                   // hidden units per workgroup (forward: 64 gate columns)
constexpr int QW = 8;                    // waves of the persistent kernels = K ranges

// Head of a persistent launch's work buffer, forward and backward alike: LSTM_SYNC_WORDS 32-bit words in front of the exchange buffers.
// The arrival counter of slab s is word LSTM_SLAB_STRIDE s (one 64-byte line each; every launch clears them), the error word is
// LSTM_ERR_WORD (sticky: the host clears it), so a launch has at most LSTM_MAX_SLABS slabs.
constexpr int LSTM_SYNC_WORDS = 1024;
constexpr int LSTM_ERR_WORD = 512;
constexpr int LSTM_SLAB_STRIDE = 16;
constexpr int LSTM_MAX_SLABS = LSTM_ERR_WORD / LSTM_SLAB_STRIDE;
constexpr unsigned LSTM_SPIN_LIMIT = 1u << 22;      // polls after which a wait gives up

// Workgroup id -> (major, minor) of `total` = majors x nminor workgroups, minor fastest.  Consecutive ids go round-robin over the 8 XCDs,
// so XCD k owns a contiguous range of that order.  false: a padding workgroup (grids are rounded up to 8), uniform over the workgroup
// and before any barrier.  The per-step kernels call it; the persistent kernels write the same lines out (see lstm_seq_kernel).
__device__ __forceinline__ bool lstm_xcd_decode(int total, int nminor, int& major, int& minor) {
  const int id = blockIdx.x;
  const int per_xcd = (total + 7) / 8;
  const int lin = (id % 8) * per_xcd + id / 8;
  if (lin >= total) return false;
  major = lin / nminor; minor = lin % nminor;
  return true;
}

// The per-step kernels' staging of four floats as bf16 hi | lo into an LDS row: column quad q
__device__ __forceinline__ void split_store(char* row, int q, f32x4 v) {
  bf16x4 hi, lo;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    hi[k] = (__bf16)v[k];
    lo[k] = (__bf16)(v[k] - (float)hi[k]);
  }
  *reinterpret_cast<bf16x4*>(row + 8 * q) = hi;
  *reinterpret_cast<bf16x4*>(row + 2 * LKC + 8 * q) = lo;
}

// The persistent kernels' exchange rows are [32 bf16 hi | 32 bf16 lo] per 32 columns: v[0 .. UPT-1] (1 or 2 consecutive columns) to the hi
// halves at buf + off, the lo halves 64 bytes on (the sum is formed at the stores, behind the conversions).  Agent-scope stores (sc1:
// written through to memory), so the release that follows needs no L2 write-back.
template <int UPT, class V>
__device__ __forceinline__ void put_split(char* buf, size_t off, const V& v) {
  if (UPT == 2) {
    const __bf16 h0 = (__bf16)v[0], h1 = (__bf16)v[UPT - 1];
    const __bf16 l0 = (__bf16)(v[0] - (float)h0), l1 = (__bf16)(v[UPT - 1] - (float)h1);
    const unsigned hi = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
    const unsigned lo = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
    __hip_atomic_store(reinterpret_cast<unsigned*>(buf + off), hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned*>(buf + off + 64), lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    const __bf16 h0 = (__bf16)v[0];
    const __bf16 l0 = (__bf16)(v[0] - (float)h0);
    __hip_atomic_store(reinterpret_cast<unsigned short*>(buf + off), __builtin_bit_cast(unsigned short, h0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned short*>(buf + off + 64), __builtin_bit_cast(unsigned short, l0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ---------------------------------------------------------------------------------- fused LSTM time step
// One launch per time step: gates = h[t-1] W_hh^T (+ xp[t], the input projection incl. both biases) AND the cell update,
// so the recurrence costs one short kernel per step instead of a GEMM + a cell kernel.
//   * a workgroup owns 64 clips x 16 hidden units = 64 x 64 gate columns [i16 | f16 | g16 | o16] (W_hh rows regrouped
//     on the host), K = H walked in chunks of 128 with the operands double-buffered in LDS and the next chunk's global
//     loads in flight during the MFMA block;
//   * bf16x3 products (operands split hi + lo while they are staged), fp32 accumulate, like conv_mfma_kernel<PREC 1>;
//   * workgroup id -> (XCD, slot): the 6 unit groups an XCD owns keep their W_hh slices (1.2 MB) in that XCD's L2 for
//     all 248 steps.
constexpr int LPF = 3;          // chunks of global loads in flight per thread (register ring)

// MT = 32-clip tiles per workgroup: 2 (64 clips; 8 waves = 2 clip halves x 2 gate-column halves x 2 k-step halves) or 1 (32
// clips; 2 gate-column halves x 4 k-step quarters).  The step streams h[t-1] and its W_hh slice from memory every launch and is
// bound by what the CUs that own it can pull, so small batches use the 32-clip form: twice the workgroups, half of h[t-1] each.
template <int MT>
__global__ __launch_bounds__(LTHREADS, 1) void lstm_step_kernel(const float* __restrict__ hprev, long long ldhp,
                                                           const float* __restrict__ whh, const float* xp,
                                                           long long ldxp, const float* cin, long long ldci, float* cout,
                                                           long long ldco, int B, int H,
                                                           float* __restrict__ hout, long long ldh, float* __restrict__ hsum,
                                                           const float* __restrict__ addend, long long ldadd, int mtiles,
                                                           float* gsave, long long ldgs) {
  constexpr int BMT = 32 * MT;               // clips per workgroup
  constexpr int WK = 4 / MT;                 // k-step groups
  constexpr int KS = 8 / WK;                 // k-steps of 16 per wave and 128-wide chunk
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  char* As = lsm;                            // [2][BMT][LROW]
  char* Bs = lsm + 2 * BMT * LROW;           // [2][64][LROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % MT, wn = (wave / MT) & 1, wk = wave / (2 * MT);
  int grp, mt;                               // (group-major, m-tile-minor) order
  if (!lstm_xcd_decode((H / LU) * mtiles, mtiles, grp, mt)) return;
  const int m0 = mt * BMT;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  if (hprev != nullptr) {
    const float* Wg = whh + (size_t)grp * 64 * H;
    const int nk = H / LKC;
    constexpr int FA = BMT * (LKC / 4) / LTHREADS;       // float4 per thread per chunk: h rows (2 MT)
    constexpr int FB = 64 * (LKC / 4) / LTHREADS;        // ... and W_hh rows (4)
    constexpr int RSTEP = LTHREADS / (LKC / 4);          // 16 rows per pass
    // register ring of LPF chunks of global loads
    f32x4 ar[LPF][FA], br[LPF][FB];
    const int q = tid % (LKC / 4), r0 = tid / (LKC / 4); // column quad, first row; rows r0 + 16 i
    auto load = [&](int kc, f32x4 (&a4)[FA], f32x4 (&b4)[FB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const int m = m0 + r0 + RSTEP * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < B) v = *reinterpret_cast<const f32x4*>(hprev + (size_t)m * ldhp + kc * LKC + 4 * q);
        a4[i] = v;
      }
#pragma unroll
      for (int i = 0; i < FB; ++i) b4[i] = *reinterpret_cast<const f32x4*>(Wg + (size_t)(r0 + RSTEP * i) * H + kc * LKC + 4 * q);
    };
    auto store = [&](int buf, f32x4 (&a4)[FA], f32x4 (&b4)[FB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FA; ++i) split_store(As + (buf * BMT + r0 + RSTEP * i) * LROW, q, a4[i]);
#pragma unroll
      for (int i = 0; i < FB; ++i) split_store(Bs + (buf * 64 + r0 + RSTEP * i) * LROW, q, b4[i]);
    };
#pragma unroll
    for (int j = 0; j < LPF; ++j)
      if (j < nk) load(j, ar[j], br[j]);
    for (int base = 0; base < nk; base += LPF) {
#pragma unroll
      for (int j = 0; j < LPF; ++j) {
        const int kc = base + j;
        if (kc < nk) {                                   // uniform over the workgroup
          const int buf = kc & 1;
          store(buf, ar[j], br[j]);                      // buffer (kc & 1) was last read for chunk kc - 2, before the previous barrier
          if (kc + LPF < nk) load(kc + LPF, ar[j], br[j]);
          __syncthreads();
          const char* Ap = As + (buf * BMT + wm * 32 + li) * LROW + 16 * lh;
          const char* Bp = Bs + (buf * 64 + wn * 32 + li) * LROW + 16 * lh;
#pragma unroll
          for (int s = KS * wk; s < KS * wk + KS; ++s) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Ap + 32 * s);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(Ap + 2 * LKC + 32 * s);
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bp + 32 * s);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bp + 2 * LKC + 32 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();                                     // the gate slabs below reuse the operand buffers
  }
  // the WK partial gate tiles -> LDS slabs [WK][BMT clips][64 + 4], summed by the cell threads
  float* G = reinterpret_cast<float*>(lsm);
  constexpr int GLDW = 68;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    G[(wk * BMT + m) * GLDW + wn * 32 + li] = acc[r];
  }
  __syncthreads();
  const int clip = tid >> 2, uq = tid & 3;
  const int m = m0 + clip;
  if (clip < BMT && m < B) {
    const int u0 = grp * LU + 4 * uq;
    const float* xr = xp + (size_t)m * ldxp;
    const f32x4 xi = *reinterpret_cast<const f32x4*>(xr + u0), xf = *reinterpret_cast<const f32x4*>(xr + H + u0);
    const f32x4 xg = *reinterpret_cast<const f32x4*>(xr + 2 * H + u0), xo = *reinterpret_cast<const f32x4*>(xr + 3 * H + u0);
    const f32x4 cp = cin ? *reinterpret_cast<const f32x4*>(cin + (size_t)m * ldci + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 gi4 = xi, gf4 = xf, gg4 = xg, go4 = xo;
#pragma unroll
    for (int w = 0; w < WK; ++w) {
      const float* g = G + (w * BMT + clip) * GLDW + 4 * uq;
      gi4 += *reinterpret_cast<const f32x4*>(g);
      gf4 += *reinterpret_cast<const f32x4*>(g + 16);
      gg4 += *reinterpret_cast<const f32x4*>(g + 32);
      go4 += *reinterpret_cast<const f32x4*>(g + 48);
    }
    f32x4 cn, hn, vi, vf, vg, vo;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float si = 1.f / (1.f + expf(-gi4[k])), sf = 1.f / (1.f + expf(-gf4[k])), so = 1.f / (1.f + expf(-go4[k]));
      const float tg = tanhf(gg4[k]);
      cn[k] = sf * cp[k] + si * tg;
      hn[k] = so * tanhf(cn[k]);
      vi[k] = si; vf[k] = sf; vg[k] = tg; vo[k] = so;
    }
    if (gsave) {                               // training: the gate activations the backward step needs (may alias xp)
      float* gr = gsave + (size_t)m * ldgs;
      *reinterpret_cast<f32x4*>(gr + u0) = vi;
      *reinterpret_cast<f32x4*>(gr + H + u0) = vf;
      *reinterpret_cast<f32x4*>(gr + 2 * H + u0) = vg;
      *reinterpret_cast<f32x4*>(gr + 3 * H + u0) = vo;
    }
    *reinterpret_cast<f32x4*>(cout + (size_t)m * ldco + u0) = cn;
    *reinterpret_cast<f32x4*>(hout + (size_t)m * ldh + u0) = hn;
    if (hsum) {
      const f32x4 ad = *reinterpret_cast<const f32x4*>(addend + (size_t)m * ldadd + u0);
      *reinterpret_cast<f32x4*>(hsum + (size_t)m * ldh + u0) = hn + ad;
    }
  }
}

// 32-clip tiles while they still leave the chip under-filled (<= 256 workgroups), 64-clip tiles for large batches
static int lstm_step_mt(int B, int H) { return ((long long)(H / LU) * ((B + 31) / 32) <= 256) ? 1 : 2; }

static int lstm_launch(const float* hprev, long long ldhp, const float* whh_grouped, const float* xp, long long ldxp, const float* cin,
                       long long ldci, float* cout, long long ldco, int B, int H, float* hout, long long ldh, float* hsum,
                       const float* addend, long long ldadd, float* gsave, long long ldgs, void* stream) {
  const int MT = lstm_step_mt(B, H);
  const int mtiles = (B + 32 * MT - 1) / (32 * MT);
  const long long total = (long long)(H / LU) * mtiles;
  if (total > 0x7fffff) return MFPA_EINVAL;
  const unsigned grid = (unsigned)(((total + 7) / 8) * 8);
  const size_t lds = (size_t)2 * (32 * MT + 64) * LROW;
  if (MT == 1)
    hipLaunchKernelGGL(lstm_step_kernel<1>, dim3(grid), dim3(LTHREADS), lds, mfpa_stream(stream), hprev, ldhp, whh_grouped, xp, ldxp, cin,
                       ldci, cout, ldco, B, H, hout, ldh, hsum, addend, ldadd, mtiles, gsave, ldgs);
  else
    hipLaunchKernelGGL(lstm_step_kernel<2>, dim3(grid), dim3(LTHREADS), lds, mfpa_stream(stream), hprev, ldhp, whh_grouped, xp, ldxp, cin,
                       ldci, cout, ldco, B, H, hout, ldh, hsum, addend, ldadd, mtiles, gsave, ldgs);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

// ---------------------------------------------------------------------------------- persistent LSTM layer
// The whole time range of one layer in ONE launch.  The per-step kernel above re-reads its W_hh slice (and splits it into
// bf16 hi / lo) in every one of the 248 steps and pays a launch per step; here
//   * a workgroup owns 64 clips x 16 hidden units (64 gate columns) for all steps.  Its W_hh slice lives in REGISTERS, already
//     split: wave w holds the MFMA B-fragments of K range [w H/8, (w+1) H/8) (H = 768: 2 column tiles x 6 k-steps x (hi, lo)
//     = 96 VGPRs), so W_hh is read from memory once per launch;
//   * h[t-1] is exchanged between workgroups through a ping-pong buffer that already holds the split form
//     ([32 bf16 hi | 32 bf16 lo] per 32 units, written once by the cell that produced it, not by each of its 48 readers);
//     a wave reads its A-fragments of it straight from global memory (L2) in MFMA layout: no LDS staging of operands;
//   * the 8 partial 64 x 64 gate tiles (one per K range) are summed through LDS by the cell threads, which keep c in registers;
//   * the workgroups of one slab meet at a counter in device memory after every step (release / acquire at agent scope: the other
//     XCDs' L2s see the new h).  Every wait is BOUNDED: after LSTM_SPIN_LIMIT polls a workgroup raises the error word and from then
//     on nobody waits, so the grid always drains; the host reads the word later (mfpa_lstm_seq_error_offset).
// The grid must be co-resident (one workgroup per CU: 136 KB of LDS): the host checks slabs x groups <= CUs, else the
// per-step kernels run.
constexpr int QGLD = 68;                     // floats per clip row of a partial gate slab (64 + pad)

struct LstmSeqArgs {
  const float* whh;       // grouped W_hh (4H, H)
  float* xp;              // (B, Tn, 4H) projections (+ biases); training: overwritten with the gate activations
  float* hseq;            // (B, Tn, H)
  float* cseq;            // training: (B, Tn, H)
  float* cstate;          // inference: (B, H), read at t0 > 0, written at the end
  float* xsum;            // optional (B, Tn, H): h + skip
  const float* skip;
  unsigned* sync;         // LSTM_SYNC_WORDS words
  char* hsplit;           // [2][B][H * 4 bytes]
  int B, Tn, H, t0, t1, train, nslab, ngroups;
};

// h[t-1] is read with agent-scope (sc1) buffer loads that do not trust the local caches, so a step needs no L1 / L2 invalidate
// (an invalidate per step + cached loads measured 7.83 vs 7.58 ms for both layers of 256 clips).
// MS = 32-clip MFMA row tiles per workgroup (slab = 32 MS clips): 2 for large batches; 1 while that still leaves half the chip free --
// twice the workgroups, each reading half as much of h per step (the step is bound by what a CU can pull, see the timing experiments).
template <int N> struct LFV { float v[N]; __device__ __forceinline__ float& operator[](int i) { return v[i]; } __device__ __forceinline__ const float& operator[](int i) const { return v[i]; } };
template <int N> __device__ __forceinline__ LFV<N> lfv_load(const float* p) { LFV<N> r;
#pragma unroll
  for (int i = 0; i < N; ++i) r.v[i] = p[i];
  return r; }
template <int N> __device__ __forceinline__ void lfv_store(float* p, const LFV<N>& x) {
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = x.v[i]; }

// The cell's sigmoid / tanh on v_exp_f32 + v_rcp_f32 (absolute error ~1e-7), not the library expf / tanhf.
__device__ __forceinline__ float lstm_sig(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float lstm_tanh(float x) {
  return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x));       // e^{2x} -> inf: 1; -> 0: -1
}

template <int KS, int MS>          // k-steps of 16 per wave: H = 128 KS
__global__ __launch_bounds__(64 * QW, 1) void lstm_seq_kernel(LstmSeqArgs a) {
  constexpr int SLAB = 32 * MS, UPT = MS, TPC = 16 / UPT;   // clips per workgroup; hidden units per cell thread; cell threads per clip
  typedef LFV<UPT> fv;
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  float* G = reinterpret_cast<float*>(lsm);                 // [QW][SLAB][QGLD]
  char* const PS = lsm + (size_t)QW * SLAB * QGLD * sizeof(float);   // [SLAB][64 B]: the step's new h, split, on its way out
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int H = a.H;
  int slab, grp;
  {   // lstm_xcd_decode, written out: as a call it moved these kernels' instruction streams
    const int id = blockIdx.x, total = a.nslab * a.ngroups;
    const int per_xcd = (total + 7) / 8;
    const int lin = (id % 8) * per_xcd + id / 8;            // slab-major: the workgroups of a slab sit in as few XCDs as possible
    if (lin >= total) return;                               // padding workgroups: they are not counted at the barrier
    slab = lin / a.ngroups; grp = lin % a.ngroups;
  }
  const int m0 = slab * SLAB;
  unsigned* cnt = a.sync + LSTM_SLAB_STRIDE * slab;
  unsigned* err = a.sync + LSTM_ERR_WORD;
  const unsigned members = (unsigned)a.ngroups;
  const size_t rowb = (size_t)H * 4;                        // bytes per clip row of the split exchange buffer
  const size_t bufb = (size_t)a.B * rowb;

  // ---- W_hh fragments, split once
  bf16x8 wh[2][KS], wl[2][KS];
  {
    const float* Wg = a.whh + (size_t)grp * 64 * H;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float* p = Wg + (size_t)(nt * 32 + li) * H + (wave * KS + s) * 16 + 8 * lh;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(p), v1 = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const __bf16 h0 = (__bf16)v0[k], h1 = (__bf16)v1[k];
          wh[nt][s][k] = h0; wh[nt][s][4 + k] = h1;
          wl[nt][s][k] = (__bf16)(v0[k] - (float)h0); wl[nt][s][4 + k] = (__bf16)(v1[k] - (float)h1);
        }
      }
  }
  // ---- cell threads: clip tid / TPC, hidden units u0 .. u0 + UPT - 1
  const int clip = tid / TPC, up = tid % TPC;
  const int m = m0 + clip;
  const bool live = m < a.B;
  const int u0 = grp * LU + UPT * up;
  const size_t ldh = (size_t)a.Tn * H, ldx = (size_t)a.Tn * 4 * H;
  const size_t split_off = (size_t)(live ? m : 0) * rowb + (size_t)(u0 >> 5) * 128 + (size_t)(u0 & 31) * 2;
  fv c;
#pragma unroll
  for (int k = 0; k < UPT; ++k) c[k] = 0.f;
  if (live) {
    fv hp;
#pragma unroll
    for (int k = 0; k < UPT; ++k) hp[k] = 0.f;
    if (a.t0 > 0) {
      hp = lfv_load<UPT>(a.hseq + (size_t)m * ldh + (size_t)(a.t0 - 1) * H + u0);
      c = a.train ? lfv_load<UPT>(a.cseq + (size_t)m * ldh + (size_t)(a.t0 - 1) * H + u0) : lfv_load<UPT>(a.cstate + (size_t)m * H + u0);
    }
    put_split<UPT>(a.hsplit + (size_t)((a.t0 + 1) & 1) * bufb, split_off, hp);          // h[t] lives in buffer t & 1
  }
  // ---- slab barrier: arrive after the stores above, wait until all `members` workgroups of the slab have arrived `round` times
  // (lambdas here and in lstm_bwd_seq_kernel: as shared functions they moved both kernels' instruction streams)
  bool dead = false;
  auto arrive = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");       // this wave's write-through stores of h have been acknowledged
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto wait = [&](unsigned round) __attribute__((always_inline)) {
    if (tid == 0) {
      if (!dead) {
        const unsigned target = round * members;
        unsigned n = 0;
        while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
          if ((++n & 63u) == 0u &&
              (n > LSTM_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
            __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            dead = true;
            break;
          }
          __builtin_amdgcn_s_sleep(1);
        }
      }
    }
    __syncthreads();
  };
  arrive();

  // A-fragment rows of this lane (clamped: rows past B compute garbage that is never stored)
  size_t arow[MS];
#pragma unroll
  for (int mt = 0; mt < MS; ++mt) {
    int r = m0 + mt * 32 + li;
    r = r < a.B ? r : a.B - 1;
    arow[mt] = (size_t)r * rowb + (size_t)wave * KS * 64 + 16 * lh;      // k = (wave KS + s) 16 + 8 lh -> chunk k / 32, 2 (k % 32)
  }
  constexpr int PF = KS < 3 ? KS : 3;                      // k-steps of A loads in flight
  const __amdgpu_buffer_rsrc_t hrsrc = __builtin_amdgcn_make_buffer_rsrc(a.hsplit, 0, (int)(2 * bufb), 0x00020000);
  for (int t = a.t0; t < a.t1; ++t) {
    // the projections do not depend on h: fetch them before the wait
    fv xg[4], ad;
#pragma unroll
    for (int k = 0; k < UPT; ++k) { xg[0][k] = xg[1][k] = xg[2][k] = xg[3][k] = 0.f; ad[k] = 0.f; }
    if (live) {
      const float* xr = a.xp + (size_t)m * ldx + (size_t)t * 4 * H + u0;
#pragma unroll
      for (int g = 0; g < 4; ++g) xg[g] = lfv_load<UPT>(xr + g * H);
      if (a.xsum) ad = lfv_load<UPT>(a.skip + (size_t)m * ldh + (size_t)t * H + u0);
    }
    wait((unsigned)(t - a.t0 + 1));
    floatx16 acc[MS][2];
#pragma unroll
    for (int i = 0; i < 2 * MS; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i >> 1][i & 1][r] = 0.f;
    bf16x8 fa[PF][MS][2];
    auto issue = [&](int s, bf16x8 (&f)[MS][2]) __attribute__((always_inline)) {
#pragma unroll
      for (int mt = 0; mt < MS; ++mt) {
        const size_t off = arow[mt] + (size_t)(s >> 1) * 128 + (size_t)(s & 1) * 32;
        const unsigned o = (unsigned)(((t + 1) & 1) * bufb + off);
        f[mt][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(hrsrc, o, 0, 16));
        f[mt][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(hrsrc, o + 64, 0, 16));
      }
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) issue(s, fa[s]);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int mt = 0; mt < MS; ++mt)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s % PF][mt][1], wh[nt][s], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s % PF][mt][0], wl[nt][s], acc[mt][nt], 0, 0, 0);
          acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[s % PF][mt][0], wh[nt][s], acc[mt][nt], 0, 0, 0);
        }
      if (s + PF < KS) issue(s + PF, fa[s % PF]);
    }
    // partial gate tiles -> LDS
#pragma unroll
    for (int mt = 0; mt < MS; ++mt)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int row = mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
          G[(wave * SLAB + row) * QGLD + nt * 32 + li] = acc[mt][nt][r];
        }
    __syncthreads();
    if (live) {
      fv gs[4] = {xg[0], xg[1], xg[2], xg[3]};
#pragma unroll
      for (int w = 0; w < QW; ++w) {
        const float* g = G + (w * SLAB + clip) * QGLD + UPT * up;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
          for (int k = 0; k < UPT; ++k) gs[q][k] += g[16 * q + k];
      }
      fv hn, vi, vf, vg, vo, hs;
#pragma unroll
      for (int k = 0; k < UPT; ++k) {
        const float si = lstm_sig(gs[0][k]), sf = lstm_sig(gs[1][k]), so = lstm_sig(gs[3][k]);
        const float tg = lstm_tanh(gs[2][k]);
        c[k] = sf * c[k] + si * tg;
        hn[k] = so * lstm_tanh(c[k]);
        hs[k] = hn[k] + ad[k];
        vi[k] = si; vf[k] = sf; vg[k] = tg; vo[k] = so;
      }
      {   // this thread's hi / lo halves into the workgroup's staging rows: [clip][16 units x bf16 hi | 16 units x bf16 lo]
        char* ps = PS + clip * 64 + UPT * up * 2;
        if (UPT == 2) {
          const __bf16 h0 = (__bf16)hn[0], h1 = (__bf16)hn[UPT - 1];
          const __bf16 l0 = (__bf16)(hn[0] - (float)h0), l1 = (__bf16)(hn[UPT - 1] - (float)h1);
          *reinterpret_cast<unsigned*>(ps) = (unsigned)__builtin_bit_cast(unsigned short, h0) | ((unsigned)__builtin_bit_cast(unsigned short, h1) << 16);
          *reinterpret_cast<unsigned*>(ps + 32) = (unsigned)__builtin_bit_cast(unsigned short, l0) | ((unsigned)__builtin_bit_cast(unsigned short, l1) << 16);
        } else {
          const __bf16 h0 = (__bf16)hn[0];
          *reinterpret_cast<unsigned short*>(ps) = __builtin_bit_cast(unsigned short, h0);
          *reinterpret_cast<unsigned short*>(ps + 32) = __builtin_bit_cast(unsigned short, (__bf16)(hn[0] - (float)h0));
        }
      }
      const size_t o = (size_t)m * ldh + (size_t)t * H + u0;
      lfv_store<UPT>(a.hseq + o, hn);
      if (a.xsum) lfv_store<UPT>(a.xsum + o, hs);
      if (a.train) {
        float* gr = a.xp + (size_t)m * ldx + (size_t)t * 4 * H + u0;
        lfv_store<UPT>(gr, vi);
        lfv_store<UPT>(gr + H, vf);
        lfv_store<UPT>(gr + 2 * H, vg);
        lfv_store<UPT>(gr + 3 * H, vo);
        lfv_store<UPT>(a.cseq + o, c);
      }
    }
    if (t + 1 < a.t1) {
      // the slab's new h as 16-byte write-through (sc1) stores (gathered through LDS: narrow sc1 stores are one fabric write each): thread j takes piece j & 3 (hi 0..7, hi 8..15, lo 0..7, lo 8..15) of clip j >> 2
      __syncthreads();
      if (tid < 4 * SLAB) {
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const int sc = tid >> 2, piece = tid & 3;
        const int sm = m0 + sc;
        if (sm < a.B) {
          const u32x4 v = *reinterpret_cast<const u32x4*>(PS + sc * 64 + piece * 16);
          const int ug = grp * LU;
          const unsigned off = (unsigned)((size_t)(t & 1) * bufb + (size_t)sm * rowb + (size_t)(ug >> 5) * 128 + (size_t)(ug & 31) * 2 + (size_t)(piece >> 1) * 64 +
                                          (size_t)(piece & 1) * 16);
          __builtin_amdgcn_raw_buffer_store_b128(v, hrsrc, off, 0, 16);
        }
      }
      arrive();
    }
  }
  if (live && !a.train) lfv_store<UPT>(a.cstate + (size_t)m * H + u0, c);
}

// Every lstm_seq_kernel that exists, by (k-steps per wave, 32-clip tiles per slab)
template <int KS, int MS> void launch_lstm_seq(const LstmSeqArgs& a, unsigned grid, hipStream_t st) {
  const size_t lds = (size_t)QW * 32 * MS * QGLD * sizeof(float) + (size_t)32 * MS * 64;
  hipLaunchKernelGGL((lstm_seq_kernel<KS, MS>), dim3(grid), dim3(64 * QW), lds, st, a);
}
struct LstmSeqKernel { int ks, ms; void (*launch)(const LstmSeqArgs&, unsigned, hipStream_t); };
template <int KS, int MS> constexpr LstmSeqKernel k_seq() { return {KS, MS, launch_lstm_seq<KS, MS>}; }
const LstmSeqKernel LSTM_SEQ_KERNELS[] = {k_seq<2, 1>(), k_seq<2, 2>(), k_seq<4, 1>(), k_seq<4, 2>(), k_seq<6, 1>(), k_seq<6, 2>(), k_seq<8, 1>(), k_seq<8, 2>()};

// The persistent forward launch for (B, H) under `wg_budget` (0 = one per CU): 32-clip slabs (ms = 1) while their workgroups leave half the
// chip free, else 64-clip slabs.  workgroups = nslab x ngroups, all resident at once; 0 (kernel = null) = the per-step path: no kernel for
// this (ks, ms), too many slabs, an exchange buffer beyond 32-bit offsets, or more workgroups than the budget.
struct LstmSeqPlan { int ms, nslab, ngroups, ks, workgroups; const LstmSeqKernel* kernel; };
static LstmSeqPlan lstm_seq_plan(int B, int H, int wg_budget) {
  const int cus = mfpa_current_device_cus();
  const int budget = (wg_budget > 0 && wg_budget < cus) ? wg_budget : cus;
  LstmSeqPlan p{};
  p.ks = H / 128; p.ngroups = H / LU;
  p.ms = ((long long)((B + 31) / 32) * p.ngroups <= (budget < cus / 2 ? budget : cus / 2)) ? 1 : 2;
  p.nslab = (B + 32 * p.ms - 1) / (32 * p.ms);
  if (H % 128 || p.nslab > LSTM_MAX_SLABS || (long long)B * H * 8 > 0x7fffffffLL || (long long)p.nslab * p.ngroups > budget) return p;
  for (const LstmSeqKernel& e : LSTM_SEQ_KERNELS)
    if (e.ks == p.ks && e.ms == p.ms) { p.kernel = &e; p.workgroups = p.nslab * p.ngroups; }
  return p;
}

// ---------------------------------------------------------------------------------- LSTM backward time step
// One launch per step t (t = T-1 .. 0):
//   dh    = dhout[t] + dgates[t+1] W_hh                      (GEMM, K = 4H; skipped at t = T-1)
//   do = dh tanh(c_t) o (1-o);  dc = dc_next + dh o (1 - tanh^2 c_t);  di = dc g i (1-i);  df = dc c_{t-1} f (1-f);
//   dg = dc i (1-g^2);  dc_next <- dc f;   dgates[t] overwrites the saved gate activations [i | f | g | o] of step t.
// A workgroup owns 64 clips x 32 hidden units: B operand = rows u of W_hh^T (H, 4H).  8 waves = (clip half) x (K quarter of
// every 128-wide chunk); bf16x3 products like the forward step; workgroup id -> (XCD, slot) so that an XCD's three unit
// groups keep their 1.2 MB of W_hh^T in that XCD's L2 for all steps.
constexpr int BU = 32;                   // hidden units per workgroup (BUT below: 32 or 16)
constexpr int BPF = 6;                   // chunks of global loads in flight per thread

// MT: 32-clip tiles per workgroup: 2 = (clip half) x (K quarter), 1 = K eighths (small batches: twice the workgroups).
// BUT: hidden units per workgroup, 32 or 16 (16: the matrix tile is half empty, but the step is bound by the bytes a workgroup
// streams -- 32 x 3072 gate gradients + BUT x 3072 weights -- and twice as many CUs pull them).
template <int MT, int BUT>
__global__ __launch_bounds__(LTHREADS, 1) void lstm_step_bwd_kernel(const float* __restrict__ dgnext, long long ldgn,
                                                                    const float* __restrict__ whhT, float* gs, long long ldgs,
                                                                    const float* __restrict__ ct, long long ldct,
                                                                    const float* __restrict__ cprev, long long ldcp,
                                                                    const float* __restrict__ dhout, long long lddh,
                                                                    float* __restrict__ dcstate, int B, int H, int mtiles) {
  constexpr int BBM = 32 * MT;               // clips per workgroup
  constexpr int WK = 8 / MT;                 // k-step groups
  constexpr int KS = 8 / WK;                 // k-steps of 16 per wave and chunk
  constexpr int FA = BBM * 32 / LTHREADS;    // float4 per thread per chunk for the dgates rows (2 MT)
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  char* As = lsm;                            // [2][BBM][LROW]
  char* Bs = lsm + 2 * BBM * LROW;           // [2][32][LROW]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 31, lh = lane >> 5;
  const int wm = wave % MT, wk = wave / MT;  // wk: k-steps KS wk .. of each chunk
  int grp, mt;
  if (!lstm_xcd_decode((H / BUT) * mtiles, mtiles, grp, mt)) return;
  const int m0 = mt * BBM;
  const int K = 4 * H;
  floatx16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  if (dgnext != nullptr) {
    const float* Wg = whhT + (size_t)grp * BUT * K;
    const int nk = K / LKC;
    constexpr int FB = BUT / 16;                       // float4 per thread per chunk for the weight rows
    if (BUT < 32) {                                    // rows BUT .. 31 of both weight buffers are never staged: keep them zero
      for (int i = tid; i < 2 * (32 - BUT) * (LROW / 16); i += LTHREADS) {
        const int buf = i / ((32 - BUT) * (LROW / 16)), rem = i % ((32 - BUT) * (LROW / 16));
        *reinterpret_cast<f32x4*>(Bs + (buf * 32 + BUT + rem / (LROW / 16)) * LROW + 16 * (rem % (LROW / 16))) = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    // register ring of BPF chunks of global loads (the step is latency-bound: dgates[t+1] was written by the previous launch)
    f32x4 ar[BPF][FA], br[BPF][FB];
    const int q = tid & 31, r0 = tid >> 5;             // column quad, first row; rows r0 + 16 i
    auto load = [&](int kc, f32x4 (&a4)[FA], f32x4 (&b2)[FB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FA; ++i) {
        const int m = m0 + r0 + 16 * i;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (m < B) v = *reinterpret_cast<const f32x4*>(dgnext + (size_t)m * ldgn + kc * LKC + 4 * q);
        a4[i] = v;
      }
#pragma unroll
      for (int i = 0; i < FB; ++i) b2[i] = *reinterpret_cast<const f32x4*>(Wg + (size_t)(r0 + 16 * i) * K + kc * LKC + 4 * q);
    };
    auto store = [&](int buf, f32x4 (&a4)[FA], f32x4 (&b2)[FB]) __attribute__((always_inline)) {
#pragma unroll
      for (int i = 0; i < FA; ++i) split_store(As + (buf * BBM + r0 + 16 * i) * LROW, q, a4[i]);
#pragma unroll
      for (int i = 0; i < FB; ++i) split_store(Bs + (buf * 32 + r0 + 16 * i) * LROW, q, b2[i]);
    };
#pragma unroll
    for (int j = 0; j < BPF; ++j)
      if (j < nk) load(j, ar[j], br[j]);
    for (int base = 0; base < nk; base += BPF) {
#pragma unroll
      for (int j = 0; j < BPF; ++j) {
        const int kc = base + j;
        if (kc < nk) {                                   // uniform over the workgroup
          const int buf = kc & 1;
          store(buf, ar[j], br[j]);                      // buffer (kc & 1) was last read for chunk kc - 2, before the previous barrier
          if (kc + BPF < nk) load(kc + BPF, ar[j], br[j]);
          __syncthreads();
          const char* Ap = As + (buf * BBM + wm * 32 + li) * LROW + 16 * lh;
          const char* Bp = Bs + (buf * 32 + li) * LROW + 16 * lh;
#pragma unroll
          for (int s = KS * wk; s < KS * wk + KS; ++s) {
            const bf16x8 ah = *reinterpret_cast<const bf16x8*>(Ap + 32 * s);
            const bf16x8 al = *reinterpret_cast<const bf16x8*>(Ap + 2 * LKC + 32 * s);
            const bf16x8 bh = *reinterpret_cast<const bf16x8*>(Bp + 32 * s);
            const bf16x8 bl = *reinterpret_cast<const bf16x8*>(Bp + 2 * LKC + 32 * s);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, acc, 0, 0, 0);
          }
        }
      }
    }
    __syncthreads();                                     // the slabs below reuse the operand buffers
  }
  // the WK partial tiles -> LDS slabs [WK][BBM clips][36], summed by the cell threads
  float* G = reinterpret_cast<float*>(lsm);
  constexpr int GLDW = 36;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
    G[(wk * BBM + m) * GLDW + li] = acc[r];
  }
  __syncthreads();
  constexpr int UQ = BUT / 4;                  // unit quads per clip
  const int clip = tid / UQ, uq = tid % UQ;
  const int m = m0 + clip;
  if (clip < BBM && m < B) {
    const int u0 = grp * BUT + 4 * uq;
    f32x4 dh = *reinterpret_cast<const f32x4*>(dhout + (size_t)m * lddh + u0);
#pragma unroll
    for (int w = 0; w < WK; ++w) dh += *reinterpret_cast<const f32x4*>(G + (w * BBM + clip) * GLDW + 4 * uq);
    float* gr = gs + (size_t)m * ldgs;
    const f32x4 vi = *reinterpret_cast<const f32x4*>(gr + u0), vf = *reinterpret_cast<const f32x4*>(gr + H + u0);
    const f32x4 vg = *reinterpret_cast<const f32x4*>(gr + 2 * H + u0), vo = *reinterpret_cast<const f32x4*>(gr + 3 * H + u0);
    const f32x4 c = *reinterpret_cast<const f32x4*>(ct + (size_t)m * ldct + u0);
    const f32x4 cp = cprev ? *reinterpret_cast<const f32x4*>(cprev + (size_t)m * ldcp + u0) : f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dcs = *reinterpret_cast<const f32x4*>(dcstate + (size_t)m * H + u0);
    f32x4 di, df, dg, dO;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float tc = tanhf(c[k]);
      dO[k] = dh[k] * tc * vo[k] * (1.f - vo[k]);
      const float dc = dcs[k] + dh[k] * vo[k] * (1.f - tc * tc);
      di[k] = dc * vg[k] * vi[k] * (1.f - vi[k]);
      df[k] = dc * cp[k] * vf[k] * (1.f - vf[k]);
      dg[k] = dc * vi[k] * (1.f - vg[k] * vg[k]);
      dcs[k] = dc * vf[k];
    }
    *reinterpret_cast<f32x4*>(gr + u0) = di;
    *reinterpret_cast<f32x4*>(gr + H + u0) = df;
    *reinterpret_cast<f32x4*>(gr + 2 * H + u0) = dg;
    *reinterpret_cast<f32x4*>(gr + 3 * H + u0) = dO;
    *reinterpret_cast<f32x4*>(dcstate + (size_t)m * H + u0) = dcs;
  }
}


// ---------------------------------------------------------------------------------- persistent LSTM backward layer
// The backward recurrence of a layer for steps t1-1 .. t0 in ONE launch: lstm_seq_kernel's scheme turned round.
//   dh[t] = dhout[t] + dgates[t+1] W_hh  is K = 4H long and 16 hidden units wide per workgroup, so the weights only fit the
//   registers with the 16 x 16 x 32 MFMA: wave w of 8 holds the B-fragments of W_hh^T rows u0 .. u0+15, K range [w 4H/8, ..):
//   KS = H / 64 k-steps x (hi, lo) x 4 VGPRs (96 at H = 768), read once per launch instead of once per step;
//   dgates[t+1] (64 clips x 4H, already split [32 hi | 32 lo] by the cells that produced it) is exchanged through a ping-pong
//   buffer with agent-scope stores / buffer loads, A-fragments read straight from it; the 8 partial 64 x 16 tiles meet in LDS;
//   a cell thread owns (clip, 2 units): dc lives in its registers, the saved gate activations / cell states / dhout of step t are
//   fetched before the wait; it writes dgates[t] over the activations (the weight-gradient GEMMs read them later) and into the
//   exchange buffer.  Slab counter, bounded waits and the error word as in lstm_seq_kernel.
constexpr int QB_GLD = 17;

struct LstmBwdSeqArgs {
  const float* whhT;      // (H, 4H)
  float* gates;           // (B, Tn, 4H): activations [i | f | g | o] in, pre-activation gradients out
  const float* cseq;      // (B, Tn, H)
  const float* dhout;     // (B, Tn, H)
  float* dcstate;         // (B, H): read when t1 < Tn, written at the end
  unsigned* sync;
  char* gsplit;           // [2][B][4H * 4 bytes]
  int B, Tn, H, t0, t1, nslab, ngroups;
};

// MTB = 16-clip MFMA row tiles per workgroup (slab = 16 MTB clips).  A workgroup reads its slab's WHOLE dgates[t+1] row block every
// step (K = 4H: 12 KB per clip), four times the forward's bytes, and a CU pulls ~60 GB/s of such loads: small batches therefore use
// small slabs, so that more CUs share the reading (64 clips: 192 workgroups of 16 clips instead of 48 of 64).
template <int KS, int MTB>          // k-steps of 32 per wave: 4H = 256 KS
__global__ __launch_bounds__(64 * QW, 1) void lstm_bwd_seq_kernel(LstmBwdSeqArgs a) {
  constexpr int SLAB = 16 * MTB;
  constexpr int UPT = MTB == 4 ? 2 : 1;                     // hidden units per cell thread
  constexpr int TPC = 16 / UPT;                             // cell threads per clip
  __shared__ __attribute__((aligned(16))) float G[QW * SLAB * QB_GLD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ln = lane & 15, kg = lane >> 4;
  const int H = a.H, K = 4 * a.H;
  int slab, grp;
  {
    const int id = blockIdx.x, total = a.nslab * a.ngroups;
    const int per_xcd = (total + 7) / 8;
    const int lin = (id % 8) * per_xcd + id / 8;
    if (lin >= total) return;                               // padding workgroups are not counted at the barrier
    slab = lin / a.ngroups; grp = lin % a.ngroups;
  }
  const int m0 = slab * SLAB, u0 = grp * 16;
  unsigned* cnt = a.sync + LSTM_SLAB_STRIDE * slab;
  unsigned* err = a.sync + LSTM_ERR_WORD;
  const unsigned members = (unsigned)a.ngroups;
  const size_t rowb = (size_t)K * 4, bufb = (size_t)a.B * rowb;

  // ---- W_hh^T fragments of this workgroup's 16 units, split once
  bf16x8 wh[KS], wl[KS];
  {
    const float* Wr = a.whhT + (size_t)(u0 + ln) * K + (size_t)wave * KS * 32 + 8 * kg;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(Wr + 32 * s), v1 = *reinterpret_cast<const f32x4*>(Wr + 32 * s + 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const __bf16 h0 = (__bf16)v0[k], h1 = (__bf16)v1[k];
        wh[s][k] = h0; wh[s][4 + k] = h1;
        wl[s][k] = (__bf16)(v0[k] - (float)h0); wl[s][4 + k] = (__bf16)(v1[k] - (float)h1);
      }
    }
  }
  // ---- cell threads: clip tid / TPC, hidden units u .. u + UPT - 1
  const int clip = tid / TPC, ui = tid % TPC;
  const int m = m0 + clip;
  const bool live = clip < SLAB && m < a.B;
  const int u = u0 + UPT * ui;
  const size_t ldg = (size_t)a.Tn * K, ldh = (size_t)a.Tn * H;
  auto put_gate = [&](char* buf, int q, const float (&v)[UPT]) __attribute__((always_inline)) {   // gate q of this thread's units -> the exchange rows
    const int col = q * H + u;
    put_split<UPT>(buf + (size_t)(live ? m : 0) * rowb + (size_t)(col >> 5) * 128 + (size_t)(col & 31) * 2, 0, v);
  };
  float dc[UPT];
#pragma unroll
  for (int k = 0; k < UPT; ++k) dc[k] = 0.f;
  if (live) {
    char* buf = a.gsplit + (size_t)(a.t1 & 1) * bufb;                // dgates[t] live in buffer t & 1
    if (a.t1 < a.Tn) {                                               // a later range has run: its dgates[t1] and dc
      const float* gr = a.gates + (size_t)m * ldg + (size_t)a.t1 * K + u;
#pragma unroll
      for (int k = 0; k < UPT; ++k) dc[k] = a.dcstate[(size_t)m * H + u + k];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float v[UPT];
#pragma unroll
        for (int k = 0; k < UPT; ++k) v[k] = gr[q * H + k];
        put_gate(buf, q, v);
      }
    } else {
      float z[UPT];
#pragma unroll
      for (int k = 0; k < UPT; ++k) z[k] = 0.f;
#pragma unroll
      for (int q = 0; q < 4; ++q) put_gate(buf, q, z);
    }
  }
  bool dead = false;
  auto arrive = [&]() __attribute__((always_inline)) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  };
  auto wait = [&](unsigned round) __attribute__((always_inline)) {
    if (tid == 0 && !dead) {
      const unsigned target = round * members;
      unsigned n = 0;
      while (__hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
        if ((++n & 63u) == 0u && (n > LSTM_SPIN_LIMIT || __hip_atomic_load(err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)) {
          __hip_atomic_store(err, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          dead = true;
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
    }
    __syncthreads();
  };
  arrive();

  unsigned arow[MTB];
#pragma unroll
  for (int mt = 0; mt < MTB; ++mt) {
    int r = m0 + mt * 16 + ln;
    r = r < a.B ? r : a.B - 1;
    arow[mt] = (unsigned)((size_t)r * rowb + (size_t)wave * KS * 128 + 16 * kg);          // k-step s = chunk wave KS + s of the row
  }
  const __amdgpu_buffer_rsrc_t grsrc = __builtin_amdgcn_make_buffer_rsrc(a.gsplit, 0, (int)(2 * bufb), 0x00020000);
  constexpr int PF = (MTB == 4) ? 2 : (KS < 4 ? KS : 4);    // k-steps of A loads in flight (8 MTB VGPRs each)
  for (int t = a.t1 - 1; t >= a.t0; --t) {
    // what the cell needs of step t does not depend on the recurrence: fetch it before the wait
    float gv[4][UPT], ct[UPT], cp[UPT], dho[UPT];
#pragma unroll
    for (int k = 0; k < UPT; ++k) { gv[0][k] = gv[1][k] = gv[2][k] = gv[3][k] = 0.f; ct[k] = cp[k] = dho[k] = 0.f; }
    if (live) {
      const float* gr = a.gates + (size_t)m * ldg + (size_t)t * K + u;
      const size_t o = (size_t)m * ldh + (size_t)t * H + u;
#pragma unroll
      for (int k = 0; k < UPT; ++k) {
#pragma unroll
        for (int q = 0; q < 4; ++q) gv[q][k] = gr[q * H + k];
        ct[k] = a.cseq[o + k];
        if (t > 0) cp[k] = a.cseq[o + k - H];
        dho[k] = a.dhout[o + k];
      }
    }
    wait((unsigned)(a.t1 - t));
    const unsigned pb = (unsigned)(((t + 1) & 1) * bufb);
    f32x4 acc[MTB];
#pragma unroll
    for (int mt = 0; mt < MTB; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 fa[PF][MTB][2];
    auto issue = [&](int s, bf16x8 (&f)[MTB][2]) __attribute__((always_inline)) {
#pragma unroll
      for (int mt = 0; mt < MTB; ++mt) {
        const unsigned o = pb + arow[mt] + (unsigned)s * 128u;
        f[mt][0] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(grsrc, o, 0, 16));
        f[mt][1] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(grsrc, o + 64, 0, 16));
      }
    };
#pragma unroll
    for (int s = 0; s < PF; ++s) issue(s, fa[s]);
#pragma unroll
    for (int s = 0; s < KS; ++s) {
#pragma unroll
      for (int mt = 0; mt < MTB; ++mt) {
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[s % PF][mt][1], wh[s], acc[mt], 0, 0, 0);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[s % PF][mt][0], wl[s], acc[mt], 0, 0, 0);
        acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[s % PF][mt][0], wh[s], acc[mt], 0, 0, 0);
      }
      if (s + PF < KS) issue(s + PF, fa[s % PF]);
    }
    // partial tiles -> LDS: D[row = 4 kg + j][col = ln] of m-tile mt
#pragma unroll
    for (int mt = 0; mt < MTB; ++mt)
#pragma unroll
      for (int j = 0; j < 4; ++j) G[(wave * SLAB + mt * 16 + 4 * kg + j) * QB_GLD + ln] = acc[mt][j];
    __syncthreads();
    if (live) {
      float dg_[4][UPT];
#pragma unroll
      for (int k = 0; k < UPT; ++k) {
        float dh = dho[k];
#pragma unroll
        for (int w = 0; w < QW; ++w) dh += G[(w * SLAB + clip) * QB_GLD + UPT * ui + k];
        const float vi = gv[0][k], vf = gv[1][k], vg = gv[2][k], vo = gv[3][k];
        const float tc = tanhf(ct[k]);
        dg_[3][k] = dh * tc * vo * (1.f - vo);
        const float dcv = dc[k] + dh * vo * (1.f - tc * tc);
        dg_[0][k] = dcv * vg * vi * (1.f - vi);
        dg_[1][k] = dcv * cp[k] * vf * (1.f - vf);
        dg_[2][k] = dcv * vi * (1.f - vg * vg);
        dc[k] = dcv * vf;
      }
      char* buf = a.gsplit + (size_t)(t & 1) * bufb;
      float* gr = a.gates + (size_t)m * ldg + (size_t)t * K + u;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        put_gate(buf, q, dg_[q]);
#pragma unroll
        for (int k = 0; k < UPT; ++k) gr[q * H + k] = dg_[q][k];
      }
    }
    if (t > a.t0) arrive();                                  // (its __syncthreads also frees the partial-tile slabs)
  }
  if (live) {
#pragma unroll
    for (int k = 0; k < UPT; ++k) a.dcstate[(size_t)m * H + u + k] = dc[k];
  }
}

// Every lstm_bwd_seq_kernel that exists, by (k-steps per wave, 16-clip tiles per slab)
template <int KS, int MTB> void launch_lstm_bwd_seq(const LstmBwdSeqArgs& a, unsigned grid, hipStream_t st) {
  hipLaunchKernelGGL((lstm_bwd_seq_kernel<KS, MTB>), dim3(grid), dim3(64 * QW), 0, st, a);
}
struct LstmBwdSeqKernel { int ks, mtb; void (*launch)(const LstmBwdSeqArgs&, unsigned, hipStream_t); };
template <int KS, int MTB> constexpr LstmBwdSeqKernel k_bwd_seq() { return {KS, MTB, launch_lstm_bwd_seq<KS, MTB>}; }
const LstmBwdSeqKernel LSTM_BWD_SEQ_KERNELS[] = {k_bwd_seq<4, 1>(),  k_bwd_seq<4, 2>(),  k_bwd_seq<4, 4>(),  k_bwd_seq<8, 1>(), k_bwd_seq<8, 2>(),
                                                 k_bwd_seq<8, 4>(),  k_bwd_seq<12, 1>(), k_bwd_seq<12, 2>(), k_bwd_seq<12, 4>()};

// The persistent backward launch for (B, H) under `wg_budget` (0 = one per CU): the smallest slab (mtb x 16 clips, mtb = 1, 2, 4) whose
// workgroups still fit the budget, so that more CUs share the reading of dgates[t+1].  workgroups = 0 (kernel = null) = the per-step path.
struct LstmBwdSeqPlan { int mtb, nslab, ngroups, ks, workgroups; const LstmBwdSeqKernel* kernel; };
static LstmBwdSeqPlan lstm_bwd_seq_plan(int B, int H, int wg_budget) {
  const int cus = mfpa_current_device_cus();
  const int budget = (wg_budget > 0 && wg_budget < cus) ? wg_budget : cus;
  LstmBwdSeqPlan p{};
  p.ks = (H % 64 == 0) ? H / 64 : 0; p.ngroups = H / 16;
  for (int c = 1; c <= 4 && !p.mtb; c *= 2)
    if ((long long)((B + 16 * c - 1) / (16 * c)) * p.ngroups <= budget) p.mtb = c;
  p.nslab = p.mtb ? (B + 16 * p.mtb - 1) / (16 * p.mtb) : 0;
  if (!p.mtb || p.nslab > LSTM_MAX_SLABS || (long long)B * H * 32 > 0x7fffffffLL || (long long)p.nslab * p.ngroups > budget) return p;
  for (const LstmBwdSeqKernel& e : LSTM_BWD_SEQ_KERNELS)
    if (e.ks == p.ks && e.mtb == p.mtb) { p.kernel = &e; p.workgroups = p.nslab * p.ngroups; }
  return p;
}

// The per-step backward kernel for (B, H): 32-clip tiles (mt = 1) while they leave the chip under-filled, and then 16-unit groups while even
// those leave half the chip free
struct LstmStepBwdTile { int mt, but; };
static LstmStepBwdTile lstm_step_bwd_tile(int B, int H) {
  const int mt = ((long long)(H / BU) * ((B + 31) / 32) <= 256) ? 1 : 2;
  return {mt, (mt == 1 && (long long)(H / 16) * ((B + 31) / 32) <= 128) ? 16 : 32};
}

}  // namespace

extern "C" {

int mfpa_lstm_step(const float* hprev, long long ldhp, const float* whh_grouped, const float* xp, long long ldxp, float* c,
                   int B, int H, float* hout, long long ldh, float* hsum, const float* addend, long long ldadd, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!whh_grouped || !xp || !c || !hout || B < 0 || H < LKC || H % LKC) return MFPA_EINVAL;
  if (ldhp % 4 || ldxp % 4 || ldh % 4 || ldadd % 4 || (hsum && !addend)) return MFPA_EINVAL;   // float4 rows
  return lstm_launch(hprev, ldhp, whh_grouped, xp, ldxp, c, (long long)H, c, (long long)H, B, H, hout, ldh, hsum, addend, ldadd,
                     nullptr, 0LL, stream);
}

int mfpa_lstm_step_train(const float* hprev, long long ldhp, const float* whh_grouped, const float* xp, long long ldxp,
                         const float* cprev, long long ldcp, float* cout, long long ldco, int B, int H, float* hout, long long ldh,
                         float* hsum, const float* addend, long long ldadd, float* gsave, long long ldgs, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!whh_grouped || !xp || !cout || !hout || !gsave || B < 0 || H < LKC || H % LKC) return MFPA_EINVAL;
  if (ldhp % 4 || ldxp % 4 || ldh % 4 || ldadd % 4 || ldcp % 4 || ldco % 4 || ldgs % 4 || (hsum && !addend)) return MFPA_EINVAL;
  return lstm_launch(hprev, ldhp, whh_grouped, xp, ldxp, cprev, ldcp, cout, ldco, B, H, hout, ldh, hsum, addend, ldadd, gsave, ldgs,
                     stream);
}

/* A whole LSTM layer: the Tn time steps of mfpa_lstm_step / mfpa_lstm_step_train launched from one host loop (one call across
 * the ABI instead of Tn: the Python-side cost of 2 x 248 launches was a third of a 16-clip training step). */
int mfpa_lstm_layer_range(const float* whh_grouped, float* xp, float* hseq, float* cseq, float* cstate, int B, int Tn, int H,
                          float* xsum, const float* skip, int train, int t0, int t1, void* stream) {
  if (B == 0 || Tn == 0 || t1 <= t0) return MFPA_OK;
  if (!whh_grouped || !xp || !hseq || B < 0 || Tn < 0 || H < LKC || H % LKC || (xsum && !skip) || t0 < 0 || t1 > Tn) return MFPA_EINVAL;
  if (train ? !cseq : !cstate) return MFPA_EINVAL;
  const long long ldh = (long long)Tn * H, ldx = (long long)Tn * 4 * H;
  if (!train && t0 == 0) MFPA_HIP(hipMemsetAsync(cstate, 0, (size_t)B * H * sizeof(float), mfpa_stream(stream)));
  for (int t = t0; t < t1; ++t) {
    const float* hprev = t ? hseq + (size_t)(t - 1) * H : nullptr;
    float* xt = xp + (size_t)t * 4 * H;
    int rc;
    if (train)
      rc = lstm_launch(hprev, ldh, whh_grouped, xt, ldx, t ? cseq + (size_t)(t - 1) * H : nullptr, ldh, cseq + (size_t)t * H, ldh, B, H,
                       hseq + (size_t)t * H, ldh, xsum ? xsum + (size_t)t * H : nullptr, skip ? skip + (size_t)t * H : nullptr, ldh, xt, ldx,
                       stream);
    else
      rc = lstm_launch(hprev, ldh, whh_grouped, xt, ldx, cstate, (long long)H, cstate, (long long)H, B, H, hseq + (size_t)t * H, ldh,
                       xsum ? xsum + (size_t)t * H : nullptr, skip ? skip + (size_t)t * H : nullptr, ldh, nullptr, 0LL, stream);
    if (rc != MFPA_OK) return rc;
  }
  return MFPA_OK;
}

/* The persistent form of mfpa_lstm_layer_range (lstm_seq_kernel): one launch for steps [t0, t1).  `work` = device scratch of
 * mfpa_lstm_seq_work_bytes(B, H) bytes, private to this layer while the call is in flight; its error word (mfpa_lstm_seq_error)
 * must be zero before the first use (hipMemset the buffer once).  Shapes the persistent kernel does not take (H not 128 KS for
 * KS in {2, 4, 6, 8}, more 64-clip slabs x H / 16 groups than CUs) run the per-step kernels: the result is the same either way. */
int mfpa_lstm_seq_work_bytes(int B, int H, long long* bytes) {
  if (!bytes || B < 0 || H < 0) return MFPA_EINVAL;
  *bytes = (long long)LSTM_SYNC_WORDS * 4 + 2LL * B * H * 4;
  return MFPA_OK;
}

int mfpa_lstm_seq_error_offset(void) { return LSTM_ERR_WORD * 4; }

int mfpa_lstm_seq_workgroups(int B, int H, int wg_budget, int* workgroups) {
  if (!workgroups || B < 0 || H < LKC || H % LKC) return MFPA_EINVAL;
  *workgroups = B > 0 ? lstm_seq_plan(B, H, wg_budget).workgroups : 0;
  return MFPA_OK;
}

int mfpa_lstm_layer_seq(const float* whh_grouped, float* xp, float* hseq, float* cseq, float* cstate, int B, int Tn, int H, float* xsum,
                        const float* skip, int train, int t0, int t1, int wg_budget, void* work, void* stream) {
  if (B == 0 || Tn == 0 || t1 <= t0) return MFPA_OK;
  if (!whh_grouped || !xp || !hseq || !work || B < 0 || Tn < 0 || H < LKC || H % LKC || (xsum && !skip) || t0 < 0 || t1 > Tn) return MFPA_EINVAL;
  if (train ? !cseq : !cstate) return MFPA_EINVAL;
  // every workgroup of the launch must be resident at once: the plan keeps them within `wg_budget` (0 = one per CU of the current
  // device; a caller running two such launches side by side -- the chunked two-stream pipeline -- passes half the CU count)
  const LstmSeqPlan p = lstm_seq_plan(B, H, wg_budget);
  if (p.workgroups == 0)
    return mfpa_lstm_layer_range(whh_grouped, xp, hseq, cseq, cstate, B, Tn, H, xsum, skip, train, t0, t1, stream);
  LstmSeqArgs a;
  a.whh = whh_grouped; a.xp = xp; a.hseq = hseq; a.cseq = cseq; a.cstate = cstate; a.xsum = xsum; a.skip = skip;
  a.sync = reinterpret_cast<unsigned*>(work);
  a.hsplit = reinterpret_cast<char*>(work) + (size_t)LSTM_SYNC_WORDS * 4;
  a.B = B; a.Tn = Tn; a.H = H; a.t0 = t0; a.t1 = t1; a.train = train; a.nslab = p.nslab; a.ngroups = p.ngroups;
  hipStream_t st = mfpa_stream(stream);
  MFPA_HIP(hipMemsetAsync(work, 0, (size_t)LSTM_ERR_WORD * 4, st));          // the slab counters; the error word stays
  p.kernel->launch(a, (unsigned)(((p.workgroups + 7) / 8) * 8), st);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_lstm_step_bwd(const float* dgnext, long long ldgn, const float* whhT, float* gates, long long ldg, const float* ct,
                       long long ldct, const float* cprev, long long ldcp, const float* dhout, long long lddh, float* dcstate, int B,
                       int H, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!whhT || !gates || !ct || !dhout || !dcstate || B < 0 || H < LKC || H % LKC) return MFPA_EINVAL;
  if (ldgn % 4 || ldg % 4 || ldct % 4 || ldcp % 4 || lddh % 4) return MFPA_EINVAL;
  const LstmStepBwdTile tile = lstm_step_bwd_tile(B, H);
  const int MT = tile.mt, but = tile.but;
  const int mtiles = (B + 32 * MT - 1) / (32 * MT);
  const long long total = (long long)(H / but) * mtiles;
  if (total > 0x7fffff) return MFPA_EINVAL;
  const unsigned grid = (unsigned)(((total + 7) / 8) * 8);
  const size_t lds = (size_t)2 * (32 * MT + 32) * LROW;
  if (MT == 1 && but == 16)
    hipLaunchKernelGGL((lstm_step_bwd_kernel<1, 16>), dim3(grid), dim3(LTHREADS), lds, mfpa_stream(stream), dgnext, ldgn, whhT, gates, ldg,
                       ct, ldct, cprev, ldcp, dhout, lddh, dcstate, B, H, mtiles);
  else if (MT == 1)
    hipLaunchKernelGGL((lstm_step_bwd_kernel<1, 32>), dim3(grid), dim3(LTHREADS), lds, mfpa_stream(stream), dgnext, ldgn, whhT, gates, ldg,
                       ct, ldct, cprev, ldcp, dhout, lddh, dcstate, B, H, mtiles);
  else
    hipLaunchKernelGGL((lstm_step_bwd_kernel<2, 32>), dim3(grid), dim3(LTHREADS), lds, mfpa_stream(stream), dgnext, ldgn, whhT, gates, ldg,
                       ct, ldct, cprev, ldcp, dhout, lddh, dcstate, B, H, mtiles);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

/* The backward recurrence of a whole LSTM layer: mfpa_lstm_step_bwd for t = Tn-1 .. 0 from one host loop.  gates / cseq / dhout
 * are (B, Tn, .) as mfpa_lstm_layer_range(train = 1) left them; dcstate (B, H) scratch (zeroed here). */
int mfpa_lstm_layer_bwd_range(const float* whhT, float* gates, const float* cseq, const float* dhout, float* dcstate, int B, int Tn,
                              int H, int t0, int t1, void* stream) {
  if (B == 0 || Tn == 0 || t1 <= t0) return MFPA_OK;
  if (!whhT || !gates || !cseq || !dhout || !dcstate || B < 0 || Tn < 0 || t0 < 0 || t1 > Tn) return MFPA_EINVAL;
  if (t1 == Tn) MFPA_HIP(hipMemsetAsync(dcstate, 0, (size_t)B * H * sizeof(float), mfpa_stream(stream)));
  const long long ldg = (long long)Tn * 4 * H, ldh = (long long)Tn * H;
  for (int t = t1 - 1; t >= t0; --t) {
    const int rc = mfpa_lstm_step_bwd(t + 1 < Tn ? gates + (size_t)(t + 1) * 4 * H : nullptr, ldg, whhT, gates + (size_t)t * 4 * H, ldg,
                                      cseq + (size_t)t * H, ldh, t ? cseq + (size_t)(t - 1) * H : nullptr, ldh, dhout + (size_t)t * H, ldh,
                                      dcstate, B, H, stream);
    if (rc != MFPA_OK) return rc;
  }
  return MFPA_OK;
}

/* mfpa_lstm_layer_bwd_range as ONE persistent launch (lstm_bwd_seq_kernel): same arguments and results; `work` = device scratch of the
 * size mfpa_lstm_bwd_seq_work_bytes reports, owned by this layer while the call runs, zeroed once before its first use; the error
 * word (bounded waits, as for mfpa_lstm_layer_seq) sits at the same byte offset.  Shapes outside the persistent kernel's range
 * (H / 64 not in {4, 8, 12}, more workgroups than `wg_budget` even with 64-clip slabs) take the per-step path inside the same call.
 * wg_budget: how many workgroups this launch may keep resident (0 = one per CU); a caller running two such launches at once passes half. */
int mfpa_lstm_bwd_seq_work_bytes(int B, int H, long long* bytes) {
  if (!bytes || B < 0 || H < 0) return MFPA_EINVAL;
  *bytes = (long long)LSTM_SYNC_WORDS * 4 + 2LL * B * 4 * H * 4;
  return MFPA_OK;
}

int mfpa_lstm_bwd_seq_workgroups(int B, int H, int wg_budget, int* workgroups) {
  if (!workgroups || B < 0 || H < 64) return MFPA_EINVAL;
  *workgroups = B > 0 ? lstm_bwd_seq_plan(B, H, wg_budget).workgroups : 0;
  return MFPA_OK;
}

int mfpa_lstm_layer_bwd_seq(const float* whhT, float* gates, const float* cseq, const float* dhout, float* dcstate, int B, int Tn, int H,
                            int t0, int t1, int wg_budget, void* work, void* stream) {
  if (B == 0 || Tn == 0 || t1 <= t0) return MFPA_OK;
  if (!whhT || !gates || !cseq || !dhout || !dcstate || !work || B < 0 || Tn < 0 || t0 < 0 || t1 > Tn || H < 64) return MFPA_EINVAL;
  const LstmBwdSeqPlan p = lstm_bwd_seq_plan(B, H, wg_budget);
  if (p.workgroups == 0)
    return mfpa_lstm_layer_bwd_range(whhT, gates, cseq, dhout, dcstate, B, Tn, H, t0, t1, stream);
  LstmBwdSeqArgs a;
  a.whhT = whhT; a.gates = gates; a.cseq = cseq; a.dhout = dhout; a.dcstate = dcstate;
  a.sync = reinterpret_cast<unsigned*>(work);
  a.gsplit = reinterpret_cast<char*>(work) + (size_t)LSTM_SYNC_WORDS * 4;
  a.B = B; a.Tn = Tn; a.H = H; a.t0 = t0; a.t1 = t1; a.nslab = p.nslab; a.ngroups = p.ngroups;
  hipStream_t st = mfpa_stream(stream);
  MFPA_HIP(hipMemsetAsync(work, 0, (size_t)LSTM_ERR_WORD * 4, st));          // the slab counters; the error word stays
  p.kernel->launch(a, (unsigned)(((p.workgroups + 7) / 8) * 8), st);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
