// Model-free spectral noise suppression for MI355X (gfx950): a windowed minimum-statistics noise tracker per frequency bin (Martin
// 2001, plain form), the decision-directed a-priori SNR of Ephraim and Malah (1984) and a Wiener gain, on (B, F, nF) STFT
// magnitudes with the frames contiguous (include/mfpa.h has the formula).  The work is B x F independent serial walks over nF frames:
// two recurrences (the smoothed periodogram s, and xi through the previous gain) with a sliding minimum of s between them that looks
// `ahead` frames into the future.
//
// Mapping: one workgroup of ONE wavefront owns BINS = 16 consecutive bins of one clip (17 workgroups per clip at F = 257).  Frames are
// contiguous in memory and the recurrences want a bin per lane, so every tile of BINS x CHUNK = 16 x 64 values goes through LDS
// transposed: loaded and stored with the 64 lanes along the frames (coalesced, a row of the tile per instruction), walked by lanes
// 0..15 with a lane per bin.  A tile row is TILE_STRIDE = 65 doubles: the walkers' reads of one frame fall on banks 2 bin (+ t), the
// loads' writes of one bin on consecutive banks -- no conflict either way.
//
// The gain walk must lag the s walk by `ahead` frames.  It lags by D = ceil(ahead / 64) whole chunks instead: in step c the walkers
// run s over chunk c into a ring in LDS (slot = frame mod R, R = back + 64 D + 64 frames, RING_STRIDE = 17 doubles per frame so that
// the four frame groups of the minimum's readers fall on different banks), then the gains of chunk c - D, whose windows
// [t - back, t + ahead] are all in the ring by then.  The magnitudes of that older chunk are read again (from L2): there is no work
// buffer.  With a noise PSD given there is no tracker, no ring and no lag.
//
// LDS: the tiles of m / y (in place) and n are static, 2 x 16 x 65 x 8 = 16 640 B; the ring and, only when g is asked for, a third tile
// are dynamic: R x 136 B (+ 8 320 B).  Default window: R = 176, 40 576 B, four workgroups per compute unit (48 896 B and three with
// g); the largest window (W = MFPA_DENOISE_MAX_WINDOW = 128): R <= 254, at most 59 504 B -- everything stays below 64 KB.  LDS, not
// registers (89-91 VGPRs, no scratch), bounds the residency: a bin needs (R + 130) x 8 B whatever the geometry.
//
// Sliding minimum: min and max select and never round, so any order gives the same bits, and it is taken off the serial chain: all
// 64 lanes work, lane = (bin, group of GROUP = 16 consecutive frames).  The 16 windows of a group share W - 15 frames; their minimum
// is taken once, and the 15 frames to its left and right enter through suffix and prefix minima (the block scheme of van Herk and
// Gil-Werman with the group as the block): (W + 15) / 16 LDS reads and about 3 operations per frame instead of W reads.  Windows
// shorter than GROUP are read directly.  Frames outside [0, nF) count as +inf.
//
// Arithmetic: float64, compiled with -ffp-contract=off (csrc/build.py): every product, sum and quotient is rounded on its own in the
// order of include/mfpa.h, which tests/_denoise_oracle.py restates in numpy; `/` is the IEEE division.  No atomics, no work buffer, no
// workgroup reads what another one wrote: a row's bits do not depend on B, on the row's position or on the grid.
#include "mfpa_common.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int BINS = 16;                                 // bins per workgroup
constexpr int CHUNK = MFPA_WAVE;                         // frames per tile
constexpr int TILE_STRIDE = CHUNK + 1;                   // doubles per bin in a tile
constexpr int RING_STRIDE = BINS + 1;                    // doubles per frame in the ring
constexpr int GROUP = 16;                                // frames per lane in the sliding minimum
constexpr int MAX_FRAMES = 16384;
static_assert(BINS * (CHUNK / GROUP) == MFPA_WAVE, "a lane per (bin, frame group)");
// R = back + 64 ceil(ahead / 64) + 64 <= (W - 1) + 63 + 64 frames
static_assert(3 * BINS * TILE_STRIDE * 8 + (MFPA_DENOISE_MAX_WINDOW + 2 * CHUNK) * RING_STRIDE * 8 <= 64 * 1024, "LDS budget");

struct Params {
  double alpha, one_minus_alpha, bias, a, one_minus_a, xi_min, g_floor;
  int back, ahead;
};

// tile[j][lane] <- m[row j][t0 + lane], lanes along the frames
template <typename TI>
__device__ __forceinline__ void load_tile(const TI* __restrict__ rows, int nb, int nF, int t0, double* tile, int lane) {
  const int t = t0 + lane;
  if (t < nF)
    for (int j = 0; j < nb; ++j) tile[j * TILE_STRIDE + lane] = (double)rows[(size_t)j * nF + t];
}

template <typename TO>
__device__ __forceinline__ void store_tile(TO* __restrict__ rows, int nb, int nF, int t0, const double* tile, int lane) {
  const int t = t0 + lane;
  if (t < nF)
    for (int j = 0; j < nb; ++j) rows[(size_t)j * nF + t] = (TO)tile[j * TILE_STRIDE + lane];
}

// the windowed minima of the GROUP frames from t0 of one bin: out[i] <- bias * min{ s[u] : t0 + i - back <= u <= t0 + i + ahead, 0 <= u < nF }
__device__ __forceinline__ void group_minima(const double* ring, int R, int nF, int t0, const Params& p, double* out) {
  const int W = p.back + p.ahead + 1;
  const double inf = __builtin_huge_val();
  int u = t0 - p.back;
  int slot = ((u % R) + R) % R;
  auto next = [&]() {                                    // s[u], then u + 1
    const double v = (u >= 0 && u < nF) ? ring[slot * RING_STRIDE] : inf;
    ++u;
    slot = slot + 1 == R ? 0 : slot + 1;
    return v;
  };
  if (W >= GROUP) {
    double left[GROUP - 1], right[GROUP - 1];
#pragma unroll
    for (int j = 0; j < GROUP - 1; ++j) left[j] = next();
    double common = inf;
#pragma unroll 8
    for (int j = 0; j < W - (GROUP - 1); ++j) common = fmin(common, next());                // unrolled: the reads of a pass in flight together
#pragma unroll
    for (int j = 0; j < GROUP - 1; ++j) right[j] = next();
#pragma unroll
    for (int j = GROUP - 3; j >= 0; --j) left[j] = fmin(left[j], left[j + 1]);       // left[j] = min of the left frames j..14
#pragma unroll
    for (int j = 1; j < GROUP - 1; ++j) right[j] = fmin(right[j], right[j - 1]);     // right[j] = min of the right frames 0..j
#pragma unroll
    for (int i = 0; i < GROUP; ++i) {
      double v = common;
      if (i < GROUP - 1) v = fmin(v, left[i]);
      if (i > 0) v = fmin(v, right[i - 1]);
      if (t0 + i < nF) out[i] = p.bias * v;
    }
  } else {
    for (int i = 0; i < GROUP && t0 + i < nF; ++i) {
      u = t0 + i - p.back;
      slot = ((u % R) + R) % R;
      double v = inf;
      for (int j = 0; j < W; ++j) v = fmin(v, next());
      out[i] = p.bias * v;
    }
  }
}

template <typename TI, typename TO>
__global__ __launch_bounds__(MFPA_WAVE) void suppress_kernel(const TI* __restrict__ m, int F, int nF, Params p, const double* __restrict__ noise,
                                                             const double* __restrict__ denom, const double* __restrict__ row_floor,
                                                             const unsigned char* __restrict__ apply_row, TO* __restrict__ y,
                                                             double* __restrict__ g_out, double* __restrict__ n_out) {
  __shared__ double mt[BINS * TILE_STRIDE];              // magnitudes in, y out (in place)
  __shared__ double nt[BINS * TILE_STRIDE];              // the noise PSD n
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* ring = reinterpret_cast<double*>(smem);        // R frames of s, RING_STRIDE doubles each; absent with a noise PSD
  const int lane = threadIdx.x;
  const int b = blockIdx.y, k0 = blockIdx.x * BINS;
  const int nb = F - k0 < BINS ? F - k0 : BINS;
  const size_t row0 = ((size_t)b * F + k0) * nF;
  const TI* rows = m + row0;
  TO* yrows = y + row0;
  double* grows = g_out ? g_out + row0 : nullptr;
  double* nrows = n_out ? n_out + row0 : nullptr;
  const bool divide = denom != nullptr;
  const double den = divide ? denom[b] : 1.0;
  const int chunks = (nF + CHUNK - 1) / CHUNK;

  if (apply_row && !apply_row[b]) {                      // the gate, the whole workgroup alike: g = 1, n = 0
    for (int c = 0; c < chunks; ++c) {
      const int t = c * CHUNK + lane;
      if (t < nF)
        for (int j = 0; j < nb; ++j) {
          const double v = (double)rows[(size_t)j * nF + t];
          yrows[(size_t)j * nF + t] = (TO)(divide ? v / den : v);
          if (grows) grows[(size_t)j * nF + t] = 1.0;
          if (nrows) nrows[(size_t)j * nF + t] = 0.0;
        }
    }
    return;
  }

  if (row_floor) p.g_floor = row_floor[b];
  const bool tracked = noise == nullptr;
  const int D = tracked ? (p.ahead + CHUNK - 1) / CHUNK : 0;
  const int R = p.back + CHUNK * D + CHUNK;
  double* gt = grows ? ring + (tracked ? R * RING_STRIDE : 0) : nullptr;   // the gain g: a tile behind the ring, only when it is asked for
  const bool walker = lane < nb;
  const double fixed_n = (!tracked && walker) ? noise[(size_t)b * F + k0 + lane] : 0.0;
  double s = 0.0, carry = 0.0;                           // s[t - 1]; (g[t-1] g[t-1]) q[t-1]

  for (int c = 0; c < chunks + D; ++c) {
    if (tracked && c < chunks) {                         // s over chunk c into the ring
      load_tile<TI>(rows, nb, nF, c * CHUNK, mt, lane);
      __syncthreads();
      if (walker) {
        const int t0 = c * CHUNK, n_here = nF - t0 < CHUNK ? nF - t0 : CHUNK;
        int slot = t0 % R;
#pragma unroll 8
        for (int i = 0; i < n_here; ++i) {
          const double v = mt[lane * TILE_STRIDE + i];
          const double pw = v * v;
          s = (t0 + i == 0) ? pw : p.alpha * s + p.one_minus_alpha * pw;
          ring[slot * RING_STRIDE + lane] = s;
          slot = slot + 1 == R ? 0 : slot + 1;
        }
      }
      __syncthreads();
    }
    const int gc = c - D;
    if (gc < 0) continue;
    const int t0 = gc * CHUNK, n_here = nF - t0 < CHUNK ? nF - t0 : CHUNK;
    if (D > 0 || !tracked) {                             // with D = 0 the tile still holds chunk gc
      load_tile<TI>(rows, nb, nF, t0, mt, lane);
    }
    if (tracked) {
      const int bin = lane & (BINS - 1), group = lane >> 4;
      if (bin < nb && group * GROUP < n_here)
        group_minima(ring + bin, R, nF, t0 + group * GROUP, p, nt + bin * TILE_STRIDE + group * GROUP);
    }
    __syncthreads();
    if (walker) {
#pragma unroll 8
      for (int i = 0; i < n_here; ++i) {
        const double v = mt[lane * TILE_STRIDE + i];
        const double pw = v * v;
        const double n = tracked ? nt[lane * TILE_STRIDE + i] : fixed_n;
        const double d = fmax(n, DBL_MIN);
        const double q = pw / d;
        const double inst = fmax(q - 1.0, 0.0);
        const double dd = (t0 + i == 0) ? p.a : p.a * carry;
        const double xi = fmax(dd + p.one_minus_a * inst, p.xi_min);
        const double g = fmax(1.0 - 1.0 / (1.0 + xi), p.g_floor);
        carry = (g * g) * q;
        const double gm = g * v;
        mt[lane * TILE_STRIDE + i] = divide ? gm / den : gm;
        if (gt) gt[lane * TILE_STRIDE + i] = g;
        nt[lane * TILE_STRIDE + i] = n;
      }
    }
    __syncthreads();
    store_tile<TO>(yrows, nb, nF, t0, mt, lane);
    if (gt) store_tile<double>(grows, nb, nF, t0, gt, lane);
    if (nrows) store_tile<double>(nrows, nb, nF, t0, nt, lane);
    __syncthreads();
  }
}

template <typename TI, typename TO>
void launch(const void* m, int B, int F, int nF, const Params& p, const double* noise, const double* denom, const double* row_floor,
            const unsigned char* apply, void* y, double* g_out, double* n_out, hipStream_t st) {
  const int D = noise ? 0 : (p.ahead + CHUNK - 1) / CHUNK;
  const size_t ring_bytes = (noise ? 0 : (size_t)(p.back + CHUNK * D + CHUNK) * RING_STRIDE * sizeof(double)) +
                            (g_out ? (size_t)BINS * TILE_STRIDE * sizeof(double) : 0);
  const dim3 grid((unsigned)((F + BINS - 1) / BINS), (unsigned)B), block(MFPA_WAVE);
  hipLaunchKernelGGL((suppress_kernel<TI, TO>), grid, block, ring_bytes, st, static_cast<const TI*>(m), F, nF, p, noise, denom, row_floor, apply,
                     static_cast<TO*>(y), g_out, n_out);
}

inline bool flag(int v) { return v == 0 || v == 1; }
inline bool misaligned(const void* q, uintptr_t mask) { return (reinterpret_cast<uintptr_t>(q) & mask) != 0; }

}  // namespace

extern "C" {

int mfpa_spectral_suppress(const void* m, int m_f64, int B, int F, int nF, double alpha, int back, int ahead, double bias, double a,
                           double xi_min, double g_floor, const double* row_floor, const double* noise, const double* denom,
                           const unsigned char* apply, void* y, int y_f64, double* g_out, double* n_out, void* stream) {
  if (B < 1 || B > 65535 || F < 1 || F > (1 << 20) || nF < 1 || nF > MAX_FRAMES || !flag(m_f64) || !flag(y_f64)) return MFPA_EINVAL;
  if (!(alpha >= 0.0 && alpha < 1.0) || !(a >= 0.0 && a < 1.0) || !(xi_min > 0.0 && std::isfinite(xi_min)) ||
      !(g_floor >= 0.0 && g_floor <= 1.0) || !(bias > 0.0 && std::isfinite(bias)))
    return MFPA_EINVAL;
  if (back < 0 || ahead < 0 || back > MFPA_DENOISE_MAX_WINDOW || ahead > MFPA_DENOISE_MAX_WINDOW || back + ahead + 1 > MFPA_DENOISE_MAX_WINDOW)
    return MFPA_EINVAL;
  if (!m || !y) return MFPA_EINVAL;
  if (misaligned(m, m_f64 ? 7 : 3) || misaligned(y, y_f64 ? 7 : 3) || misaligned(noise, 7) || misaligned(denom, 7) || misaligned(row_floor, 7) || misaligned(g_out, 7) ||
      misaligned(n_out, 7))
    return MFPA_EINVAL;
  const Params p{alpha, 1.0 - alpha, bias, a, 1.0 - a, xi_min, g_floor, back, ahead};
  hipStream_t st = mfpa_stream(stream);
  if (m_f64) {
    if (y_f64)
      launch<double, double>(m, B, F, nF, p, noise, denom, row_floor, apply, y, g_out, n_out, st);
    else
      launch<double, float>(m, B, F, nF, p, noise, denom, row_floor, apply, y, g_out, n_out, st);
  } else {
    if (y_f64)
      launch<float, double>(m, B, F, nF, p, noise, denom, row_floor, apply, y, g_out, n_out, st);
    else
      launch<float, float>(m, B, F, nF, p, noise, denom, row_floor, apply, y, g_out, n_out, st);
  }
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
