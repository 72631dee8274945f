// Dynamic range compression for MI355X (gfx950): a feed-forward, log-domain compressor with the smooth decoupled peak detector of
// Giannoulis, Massberg and Reiss (JAES 2012), float64 state and arithmetic, float32 or float64 samples (include/mfpa.h has the
// formula).  Two recurrences per sample, the second fed by the first:
//   release   y1 <- max(xl, aR y1 + (1 - aR) xl)      a map y -> max(c, a y + b); (a2, b2, c2) after (a1, b1, c1) is
//                                                     (a2 a1, a2 b1 + b2, max(c2, a2 c1 + b2)): the family is closed
//   attack    yL <- aA yL + (1 - aA) y1               affine: (a2, b2) after (a1, b1) is (a2 a1, a2 b1 + b2)
// so both are scans, csrc/iir.hip's scheme inside a wavefront: a lane owns L = 16 consecutive samples of a super-chunk of 64 x 16,
// folds them into its composite map, an inclusive shuffle scan over the lanes composes the maps, the map of the lanes before a lane is
// applied ONCE to the super-chunk's carry (the state itself is never pushed through the scan), and the lane reruns its 16 samples
// with the recurrence itself: only a lane's start state carries the rounding of the scan.  The attack stage needs the release
// stage's true output, so the order is release scan, release true pass, attack scan, attack true pass, all in registers.
//
// Mapping: one workgroup of P wavefronts = one row (iir.hip's single wavefront per row takes one wavefront's serial walk whatever the
// batch).  Wavefront w owns a contiguous part of the row, ceil(ceil(T / 1024) / P) whole super-chunks, and the row is walked three
// times with a workgroup barrier and the parts' carries in LDS between the walks:
//   1. every wavefront composes the release map of its part; the parts' start states y1 follow by applying the maps of the parts
//      before, in wavefront order, to the row's initial state (every wavefront does this itself: same operations, same bits);
//   2. every wavefront reruns the release stage from its true start and composes the attack map of its part; the start states yL
//      follow in the same way;
//   3. every wavefront runs both stages from its true starts, applies the gain and stores.
// The level xl is recomputed in every walk: there is no work buffer and the second and third reads of the row come from L2.  A
// wavefront whose part is empty carries the identity map (1, 0, -DBL_MAX) / (1, 0), as do the samples past T inside a super-chunk.  No
// atomics, no workgroup waits for another one, every fold has a fixed order: a row's bits do not depend on B, on the row's position
// or on the run.
//
// Arithmetic: compiled with -ffp-contract=off (csrc/build.py): every product and sum is rounded on its own, in the order of the
// formula, which is the order of tests/_dynamics_oracle.py.  log10 and exp10 are the device library's.
//
// Loads and stores: as in iir.hip a super-chunk is read coalesced (16 loads of 64 consecutive elements) and transposed through LDS in
// the sample type, sample p at element (p / 16) * 17 + p % 16: a stride of 17 elements keeps the lanes' own reads on different banks.
#include "mfpa_common.h"

#include <cfloat>

namespace {

constexpr int P = 8;                                     // wavefronts per row
constexpr int L = 16;                                    // samples per lane
constexpr int SUPER = MFPA_WAVE * L;                     // samples per super-chunk
constexpr int LDS_STRIDE = L + 1;                        // elements per lane in LDS
constexpr int SCAN_STEPS = 6;                            // offsets 2^k, k < 6: 64 lanes

__device__ __forceinline__ int lds_slot(int p) { return (p >> 4) * LDS_STRIDE + (p & (L - 1)); }

// LDS written by one lane and read by another lane of the SAME wavefront (iir.hip)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Rel {                                             // y -> max(c, a y + b)
  double a, b, c;
};
struct Aff {                                             // y -> a y + b
  double a, b;
};

__device__ __forceinline__ Rel rel_identity() { return Rel{1.0, 0.0, -DBL_MAX}; }
__device__ __forceinline__ Aff aff_identity() { return Aff{1.0, 0.0}; }
__device__ __forceinline__ Rel then(const Rel& first, const Rel& next) {
  return Rel{next.a * first.a, next.a * first.b + next.b, fmax(next.c, next.a * first.c + next.b)};
}
__device__ __forceinline__ Aff then(const Aff& first, const Aff& next) { return Aff{next.a * first.a, next.a * first.b + next.b}; }
__device__ __forceinline__ double apply(const Rel& m, double y) { return fmax(m.c, m.a * y + m.b); }
__device__ __forceinline__ double apply(const Aff& m, double y) { return m.a * y + m.b; }
__device__ __forceinline__ Rel shuffle_up(const Rel& m, int d) { return Rel{__shfl_up(m.a, d), __shfl_up(m.b, d), __shfl_up(m.c, d)}; }
__device__ __forceinline__ Aff shuffle_up(const Aff& m, int d) { return Aff{__shfl_up(m.a, d), __shfl_up(m.b, d)}; }
__device__ __forceinline__ Rel from_lane(const Rel& m, int l) { return Rel{__shfl(m.a, l), __shfl(m.b, l), __shfl(m.c, l)}; }
__device__ __forceinline__ Aff from_lane(const Aff& m, int l) { return Aff{__shfl(m.a, l), __shfl(m.b, l)}; }

// lane l: the lanes' maps composed in lane order, lanes 0..l
template <typename M>
__device__ __forceinline__ M scan(M m, int lane) {
#pragma unroll
  for (int k = 0; k < SCAN_STEPS; ++k) {
    const M before = shuffle_up(m, 1 << k);
    if (lane >= (1 << k)) m = then(before, m);
  }
  return m;
}

// the lane's start state: the map of the lanes before it applied once to the super-chunk's carry
template <typename M>
__device__ __forceinline__ double start_state(const M& scanned, int lane, double carry) {
  const M before = shuffle_up(scanned, 1);
  return lane ? apply(before, carry) : carry;
}

struct Params {
  double threshold, slope, knee, attack, release, makeup;
};

// the gain reduction wanted, dB
__device__ __forceinline__ double level_of(double x, const Params& p) {
  const double xg = 20.0 * log10(fmax(fabs(x), 1e-10));
  const double o = xg - p.threshold;
  if (2.0 * o <= -p.knee) return 0.0;
  if (2.0 * fabs(o) < p.knee) {
    const double t = o + p.knee / 2.0;
    return p.slope * (t * t) / (2.0 * p.knee);
  }
  return p.slope * o;
}

// The super-chunk at c0: x[i] = the lane's own 16 samples (sample c0 + 16 lane + i), lv[i] their levels.  Samples past n are copies
// of the row's last one; the caller masks them by its count of real samples.
template <typename T, bool LEVEL_IN>
__device__ __forceinline__ void load_super(const T* __restrict__ xr, long long c0, long long n, T* tile, int lane, const Params& p,
                                           double (&x)[L], double (&lv)[L]) {
  T raw[L];
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const long long g = c0 + (long long)j * MFPA_WAVE + lane;
    raw[j] = xr[g < n ? g : n - 1];
  }
#pragma unroll
  for (int j = 0; j < L; ++j) tile[lds_slot(j * MFPA_WAVE + lane)] = raw[j];
  wave_sync();
#pragma unroll
  for (int i = 0; i < L; ++i) x[i] = (double)tile[lane * LDS_STRIDE + i];
  wave_sync();
#pragma unroll
  for (int i = 0; i < L; ++i) lv[i] = LEVEL_IN ? x[i] : level_of(x[i], p);
}

template <typename T>
__device__ __forceinline__ void store_super(T* __restrict__ yr, long long c0, long long n, T* tile, int lane, const double (&v)[L]) {
#pragma unroll
  for (int i = 0; i < L; ++i) tile[lane * LDS_STRIDE + i] = (T)v[i];
  wave_sync();
#pragma unroll
  for (int j = 0; j < L; ++j) {
    const long long g = c0 + (long long)j * MFPA_WAVE + lane;
    if (g < n) yr[g] = tile[lds_slot(j * MFPA_WAVE + lane)];
  }
  wave_sync();
}

__device__ __forceinline__ Rel fold_release(const double (&lv)[L], int nv, double aR, double bR) {
  Rel m = rel_identity();
#pragma unroll
  for (int i = 0; i < L; ++i)
    if (i < nv) m = then(m, Rel{aR, bR * lv[i], lv[i]});
  return m;
}

// the release stage itself over the lane's real samples from y1: lv[i] <- y1 after sample i; returns the state after the last one
__device__ __forceinline__ double run_release(double (&lv)[L], int nv, double aR, double bR, double y1) {
#pragma unroll
  for (int i = 0; i < L; ++i)
    if (i < nv) {
      y1 = fmax(lv[i], aR * y1 + bR * lv[i]);
      lv[i] = y1;
    }
  return y1;
}

__device__ __forceinline__ Aff fold_attack(const double (&y1)[L], int nv, double aA, double bA) {
  Aff m = aff_identity();
#pragma unroll
  for (int i = 0; i < L; ++i)
    if (i < nv) m = then(m, Aff{aA, bA * y1[i]});
  return m;
}

__device__ __forceinline__ double run_attack(double (&y1)[L], int nv, double aA, double bA, double yL) {
#pragma unroll
  for (int i = 0; i < L; ++i)
    if (i < nv) {
      yL = aA * yL + bA * y1[i];
      y1[i] = yL;
    }
  return yL;
}

template <typename T, bool LEVEL_IN>
__global__ __launch_bounds__(MFPA_WAVE* P) void dynamics_kernel(const T* __restrict__ x, long long n, const double* __restrict__ params,
                                                                 int params_per_row, const unsigned char* __restrict__ apply_row,
                                                                 const double* __restrict__ zi, double* __restrict__ zf, T* __restrict__ y,
                                                                 T* __restrict__ gr) {
  __shared__ T tiles[P][MFPA_WAVE * LDS_STRIDE];
  __shared__ double part_release[P][3];
  __shared__ double part_attack[P][2];
  const int lane = threadIdx.x & (MFPA_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int row = blockIdx.x;
  const T* xr = x + (size_t)row * n;
  T* yr = y + (size_t)row * n;
  T* gr_row = gr ? gr + (size_t)row * n : nullptr;
  const double z1 = zi ? zi[(size_t)row * 2] : 0.0, z2 = zi ? zi[(size_t)row * 2 + 1] : 0.0;

  if (apply_row && !apply_row[row]) {                     // the gate, the whole workgroup alike: the row itself and its state unchanged
    for (long long i = threadIdx.x; i < n; i += MFPA_WAVE * P) {
      yr[i] = xr[i];
      if (gr_row) gr_row[i] = (T)0.0;
    }
    if (zf && threadIdx.x == 0) {
      zf[(size_t)row * 2] = z1;
      zf[(size_t)row * 2 + 1] = z2;
    }
    return;
  }
  const double* q = params + (params_per_row ? (size_t)row * 6 : 0);
  const Params p{q[0], q[1], q[2], q[3], q[4], q[5]};
  const double aA = p.attack, bA = 1.0 - p.attack, aR = p.release, bR = 1.0 - p.release;
  T* tile = tiles[wave];

  const long long chunks = (n + SUPER - 1) / SUPER, per_wave = (chunks + P - 1) / P;
  const long long part_begin = (long long)wave * per_wave * SUPER;
  const long long part_end = part_begin + per_wave * SUPER < n ? part_begin + per_wave * SUPER : n;   // <= part_begin: an empty part
  const int last_wave = (int)((chunks - 1) / per_wave);  // the wavefront that owns sample n - 1

  double xs[L], lv[L];
  // walk 1: the release map of the part
  Rel part1 = rel_identity();
  for (long long c0 = part_begin; c0 < part_end; c0 += SUPER) {
    const long long left = n - (c0 + (long long)lane * L);
    const int nv = left < 0 ? 0 : (left < L ? (int)left : L);
    load_super<T, LEVEL_IN>(xr, c0, n, tile, lane, p, xs, lv);
    const Rel m = scan(fold_release(lv, nv, aR, bR), lane);
    part1 = then(part1, from_lane(m, MFPA_WAVE - 1));
  }
  if (lane == 0) {
    part_release[wave][0] = part1.a;
    part_release[wave][1] = part1.b;
    part_release[wave][2] = part1.c;
  }
  __syncthreads();
  double carry1 = z1;
  for (int j = 0; j < wave; ++j) carry1 = apply(Rel{part_release[j][0], part_release[j][1], part_release[j][2]}, carry1);

  // walk 2: the release stage from its true start, the attack map of the part
  Aff part2 = aff_identity();
  {
    double c1 = carry1;
    for (long long c0 = part_begin; c0 < part_end; c0 += SUPER) {
      const long long left = n - (c0 + (long long)lane * L);
      const int nv = left < 0 ? 0 : (left < L ? (int)left : L);
      const long long real = n - c0 < SUPER ? n - c0 : SUPER;
      load_super<T, LEVEL_IN>(xr, c0, n, tile, lane, p, xs, lv);
      const Rel m = scan(fold_release(lv, nv, aR, bR), lane);
      const double end1 = run_release(lv, nv, aR, bR, start_state(m, lane, c1));
      c1 = __shfl(end1, (int)((real - 1) >> 4));           // the state after the super-chunk's last real sample: from the recurrence
      const Aff m2 = scan(fold_attack(lv, nv, aA, bA), lane);
      part2 = then(part2, from_lane(m2, MFPA_WAVE - 1));
    }
  }
  if (lane == 0) {
    part_attack[wave][0] = part2.a;
    part_attack[wave][1] = part2.b;
  }
  __syncthreads();
  double carry2 = z2;
  for (int j = 0; j < wave; ++j) carry2 = apply(Aff{part_attack[j][0], part_attack[j][1]}, carry2);

  // walk 3: both stages from their true starts, the gain, the stores
  for (long long c0 = part_begin; c0 < part_end; c0 += SUPER) {
    const long long left = n - (c0 + (long long)lane * L);
    const int nv = left < 0 ? 0 : (left < L ? (int)left : L);
    const long long real = n - c0 < SUPER ? n - c0 : SUPER;
    const int tail_lane = (int)((real - 1) >> 4);
    load_super<T, LEVEL_IN>(xr, c0, n, tile, lane, p, xs, lv);
    const Rel m = scan(fold_release(lv, nv, aR, bR), lane);
    const double end1 = run_release(lv, nv, aR, bR, start_state(m, lane, carry1));
    carry1 = __shfl(end1, tail_lane);
    const Aff m2 = scan(fold_attack(lv, nv, aA, bA), lane);
    const double end2 = run_attack(lv, nv, aA, bA, start_state(m2, lane, carry2));
    carry2 = __shfl(end2, tail_lane);
    if (LEVEL_IN) {
      store_super<T>(yr, c0, n, tile, lane, lv);
    } else {
      if (gr_row) store_super<T>(gr_row, c0, n, tile, lane, lv);
#pragma unroll
      for (int i = 0; i < L; ++i) lv[i] = xs[i] * exp10((p.makeup - lv[i]) / 20.0);
      store_super<T>(yr, c0, n, tile, lane, lv);
    }
  }
  if (zf && wave == last_wave && lane == 0) {
    zf[(size_t)row * 2] = carry1;
    zf[(size_t)row * 2 + 1] = carry2;
  }
}

template <typename T>
void launch(const void* x, int B, long long n, const double* params, int params_per_row, const unsigned char* apply_row, const double* zi,
            double* zf, int level_in, void* y, void* gr, hipStream_t st) {
  const dim3 grid(B), block(MFPA_WAVE * P);
  if (level_in)
    hipLaunchKernelGGL((dynamics_kernel<T, true>), grid, block, 0, st, static_cast<const T*>(x), n, params, params_per_row, apply_row, zi, zf,
                       static_cast<T*>(y), static_cast<T*>(nullptr));
  else
    hipLaunchKernelGGL((dynamics_kernel<T, false>), grid, block, 0, st, static_cast<const T*>(x), n, params, params_per_row, apply_row, zi, zf,
                       static_cast<T*>(y), static_cast<T*>(gr));
}

}  // namespace

extern "C" {

int mfpa_dynamics(const void* x, int x_f64, int B, long long T, const double* params, int params_per_row, const unsigned char* apply,
                  const double* zi, double* zf, int level_in, void* y, void* gr, void* stream) {
  if (B < 0 || B > 65535 || T < 1 || T > (1LL << 30) || (x_f64 != 0 && x_f64 != 1) || (params_per_row != 0 && params_per_row != 1) ||
      (level_in != 0 && level_in != 1) || (level_in && gr))
    return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!x || !y || !params) return MFPA_EINVAL;
  const uintptr_t elem = x_f64 ? 7 : 3;
  if ((reinterpret_cast<uintptr_t>(x) & elem) || (reinterpret_cast<uintptr_t>(y) & elem) || (reinterpret_cast<uintptr_t>(gr) & elem) ||
      (reinterpret_cast<uintptr_t>(params) & 7) || (reinterpret_cast<uintptr_t>(zi) & 7) || (reinterpret_cast<uintptr_t>(zf) & 7))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  if (x_f64)
    launch<double>(x, B, T, params, params_per_row, apply, zi, zf, level_in, y, gr, st);
  else
    launch<float>(x, B, T, params, params_per_row, apply, zi, zf, level_in, y, gr, st);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
