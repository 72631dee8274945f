// Delay lines for MI355X (gfx950): a time-varying fractional delay without feedback (mfpa_varidelay) and a comb with an integer
// delay and feedback (mfpa_comb); float64 arithmetic, float32 or float64 samples (include/mfpa.h has both formulas).
//
// varidelay_kernel.  One workgroup of four wavefronts = MFPA_VARIDELAY_TILE consecutive outputs of one row, one per lane; the voices
// are walked in order and a lane adds its own sample's taps in index order, so there is nothing to combine between lanes.  Per voice:
//   1. every lane forms p = n - d and decides on the double whether its window meets the row (live); the tile reduces the smallest
//      and largest live p (shuffles inside a wavefront, one LDS slot per wavefront and voice, one barrier);
//   2. if [floor(min p) - half, floor(max p) + half + 1] holds at most MFPA_VARIDELAY_WINDOW samples, the workgroup stages it once
//      in LDS as float64, zeros outside the row (a second barrier), and the taps read LDS: consecutive lanes read consecutive
//      doubles for a smooth delay, which ds_read_b64 serves without a bank conflict; otherwise (random or steep delays) the taps read
//      global memory.  The staged value is the global one converted exactly, and both paths run the SAME tap function, so the bits
//      agree.  The decision is the tile's and uniform, the data of a tile never depend on another tile;
//   3. one sinpi and one sincospi per lane and voice; the Hann window per tap comes from the table of cospi / sinpi(j / half) in LDS by
//      the angle sum, as in csrc/rir.hip.
// A lane that is not live (n >= T, a delay that is not finite, a window wholly outside the row) adds g * 0.  The window buffer is
// rewritten only after barrier 1 of the next voice, which every lane passes after its taps.
//
// comb_kernel.  The residue classes n mod D are independent: lane r < D walks n = r, r + D, ... with x[n - D] and y[n - D] in
// registers.  Loads and stores are coalesced over consecutive residues; no LDS, no barrier.  A small D uses few lanes (DESIGN.md
// section 3.18 has what that costs).
//
// Arithmetic: compiled with -ffp-contract=off (csrc/build.py): every product and sum is rounded on its own in the order of the formula,
// which is the order of tests/_delay_oracle.py; the comb is compared with it bit for bit.
#include "mfpa_common.h"

namespace {

constexpr int TILE = MFPA_VARIDELAY_TILE;
constexpr int WINDOW = MFPA_VARIDELAY_WINDOW;
constexpr int MAX_VOICES = MFPA_DELAY_MAX_VOICES;
constexpr int WAVES = TILE / MFPA_WAVE;
constexpr int MAX_FILTER = 255;
constexpr long long MAX_SAMPLES = 1LL << 30;
constexpr long long MAX_COMB_DELAY = 1LL << 24;
constexpr double PI = 3.14159265358979323846;
static_assert(WAVES == 4 && WINDOW >= TILE + MAX_FILTER + 1, "a tile of constant delay must fit the staged window");

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o));
  return v;
}

// The taps of one output sample at whole + frac.  STAGED: src is the LDS window, element i = sample base + i, zeros outside the row
// already in place.  Otherwise src is the row itself.
template <bool STAGED, typename S>
__device__ __forceinline__ double taps(const S* __restrict__ src, int base, int T, int whole, double frac, int half, const double* win_cos,
                                       const double* win_sin) {
  const double dhalf = (double)half;
  const double sf = sinpi(frac);
  double sw, cw;
  sincospi(frac / dhalf, &sw, &cw);
  double s = 0.0;
  for (int j = -half; j <= half + 1; ++j) {
    const double t = (double)j - frac;
    const int ji = j + half;
    const double w = 0.5 * (1.0 + (win_cos[ji] * cw + win_sin[ji] * sw));
    const double sinc = t == 0.0 ? 1.0 : ((j & 1) ? sf : -sf) / (PI * t);
    const int k = whole + j;
    double xv;
    if (STAGED)
      xv = (double)src[k - base];
    else
      xv = (k >= 0 && k < T) ? (double)src[k] : 0.0;
    if (fabs(t) <= dhalf) s += xv * (w * sinc);
  }
  return s;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(TILE) void varidelay_kernel(const TI* __restrict__ x, long long ldx, int T, const double* __restrict__ delay,
                                                         long long d_row, long long d_voice, int d_time, int V,
                                                         const double* __restrict__ gains, const double* __restrict__ dry,
                                                         const unsigned char* __restrict__ apply_row, int half, TO* __restrict__ y) {
  __shared__ double window[WINDOW];
  __shared__ double win_cos[MAX_FILTER + 1], win_sin[MAX_FILTER + 1];          // j = -half .. half + 1
  __shared__ double tile_min[MAX_VOICES][WAVES], tile_max[MAX_VOICES][WAVES];
  const int row = blockIdx.y;
  const int n = blockIdx.x * TILE + (int)threadIdx.x;                        // < 2^30 + TILE
  const bool inside = n < T;
  const TI* xr = x + (size_t)row * ldx;
  TO* yr = y + (size_t)row * T;
  if (apply_row && !apply_row[row]) {                                         // the whole workgroup alike
    if (inside) yr[n] = (TO)xr[n];
    return;
  }
  for (int t = threadIdx.x; t <= 2 * half + 1; t += TILE) {
    const double u = (double)(t - half) / (double)half;
    win_cos[t] = cospi(u);
    win_sin[t] = sinpi(u);
  }
  const int lane = threadIdx.x & (MFPA_WAVE - 1);
  const int wave = threadIdx.x >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  const double lo_bound = -(double)(half + 1), hi_bound = (double)T + (double)half;
  const double* drow = delay + (size_t)row * d_row;
  double acc = inside ? dry[row] * (double)xr[n] : 0.0;
  for (int v = 0; v < V; ++v) {
    // a lane past the row reads nothing; a NaN fails both comparisons
    const double p = inside ? (double)n - drow[(size_t)v * d_voice + (size_t)n * d_time] : inf;
    const bool live = p > lo_bound && p < hi_bound;
    const double mn = wave_min(live ? p : inf), mx = mfpa_wave_max(live ? p : -inf);
    if (lane == 0) {
      tile_min[v][wave] = mn;
      tile_max[v][wave] = mx;
    }
    __syncthreads();                                      // barrier 1: also the table's, and every lane is done with the last window
    const double pmin = fmin(fmin(tile_min[v][0], tile_min[v][1]), fmin(tile_min[v][2], tile_min[v][3]));
    const double pmax = fmax(fmax(tile_max[v][0], tile_max[v][1]), fmax(tile_max[v][2], tile_max[v][3]));
    double s = 0.0;
    if (pmin <= pmax) {                                   // somebody is live: both lie inside (lo_bound, hi_bound), so they fit an int
      const int base = (int)floor(pmin) - half, last = (int)floor(pmax) + half + 1;
      const bool staged = last - base < WINDOW;           // last - base + 1 samples
      const double whole = floor(live ? p : 0.0);
      const double frac = (live ? p : 0.0) - whole;
      if (staged) {
        for (int i = threadIdx.x; i <= last - base; i += TILE) {
          const int k = base + i;
          window[i] = (k >= 0 && k < T) ? (double)xr[k] : 0.0;
        }
        __syncthreads();                                  // barrier 2
        if (live) s = taps<true>(window, base, T, (int)whole, frac, half, win_cos, win_sin);
      } else if (live) {
        s = taps<false>(xr, 0, T, (int)whole, frac, half, win_cos, win_sin);
      }
    }
    acc += gains[(size_t)row * V + v] * s;
  }
  if (inside) yr[n] = (TO)acc;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void comb_kernel(const TI* __restrict__ x, long long ldx, long long T, const double* __restrict__ params,
                                                   int params_per_row, long long max_delay, const unsigned char* __restrict__ apply_row,
                                                   TO* __restrict__ y) {
  const int row = blockIdx.y;
  const TI* xr = x + (size_t)row * ldx;
  TO* yr = y + (size_t)row * T;
  const long long first = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
  if (apply_row && !apply_row[row]) {
    for (long long i = first; i < T; i += step) yr[i] = (TO)xr[i];
    return;
  }
  const double* q = params + (params_per_row ? (size_t)row * 4 : 0);
  const double Dd = q[0], b0 = q[1], bD = q[2], aD = q[3];
  // the row's delay: truncated, and held inside [1, max_delay] whatever the device holds (a NaN gives 1)
  const long long D = Dd >= (double)max_delay ? max_delay : (Dd >= 1.0 ? (long long)Dd : 1);
  const long long residues = D < T ? D : T;
  for (long long r = first; r < residues; r += step) {    // one pass unless the row's D exceeds the grid (it never does: max_delay sizes it)
    double xp = 0.0, yp = 0.0;
    for (long long i = r; i < T; i += D) {
      const double xv = (double)xr[i];
      const double yv = b0 * xv + (bD * xp + aD * yp);
      yr[i] = (TO)yv;
      xp = xv;
      yp = yv;
    }
  }
}

bool aligned(const void* p, int f64) { return (reinterpret_cast<uintptr_t>(p) & (f64 ? 7 : 3)) == 0; }
bool flag(int v) { return v == 0 || v == 1; }

}  // namespace

extern "C" {

int mfpa_varidelay(const void* x, int x_f64, long long ldx, int B, long long T, const double* delay, long long delay_row_stride,
                   long long delay_voice_stride, int delay_time_stride, int V, const double* gains, const double* dry,
                   const unsigned char* apply, int filter_len, void* y, int y_f64, void* stream) {
  if (B < 1 || B > 65535 || T < 1 || T > MAX_SAMPLES || ldx < T || V < 1 || V > MAX_VOICES || filter_len < 3 || filter_len > MAX_FILTER ||
      !(filter_len & 1) || delay_row_stride < 0 || delay_voice_stride < 0 || !flag(delay_time_stride) || !flag(x_f64) || !flag(y_f64))
    return MFPA_EINVAL;
  if (!x || !delay || !gains || !dry || !y || !aligned(x, x_f64) || !aligned(y, y_f64) || !aligned(delay, 1) || !aligned(gains, 1) ||
      !aligned(dry, 1))
    return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const dim3 grid((unsigned)((T + TILE - 1) / TILE), B), block(TILE);
  const int half = (filter_len - 1) / 2, t = (int)T;
#define MFPA_VARIDELAY_LAUNCH(TI, TO)                                                                                                   \
  hipLaunchKernelGGL((varidelay_kernel<TI, TO>), grid, block, 0, st, static_cast<const TI*>(x), ldx, t, delay, delay_row_stride,         \
                     delay_voice_stride, delay_time_stride, V, gains, dry, apply, half, static_cast<TO*>(y))
  if (x_f64 && y_f64)
    MFPA_VARIDELAY_LAUNCH(double, double);
  else if (x_f64)
    MFPA_VARIDELAY_LAUNCH(double, float);
  else if (y_f64)
    MFPA_VARIDELAY_LAUNCH(float, double);
  else
    MFPA_VARIDELAY_LAUNCH(float, float);
#undef MFPA_VARIDELAY_LAUNCH
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_comb(const void* x, int x_f64, long long ldx, int B, long long T, const double* params, int params_per_row, long long max_delay,
              const unsigned char* apply, void* y, int y_f64, void* stream) {
  if (B < 1 || B > 65535 || T < 1 || T > MAX_SAMPLES || ldx < T || max_delay < 1 || max_delay > MAX_COMB_DELAY || !flag(x_f64) ||
      !flag(y_f64) || !flag(params_per_row))
    return MFPA_EINVAL;
  if (!x || !params || !y || !aligned(x, x_f64) || !aligned(y, y_f64) || !aligned(params, 1)) return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const long long residues = max_delay < T ? max_delay : T;
  const dim3 grid((unsigned)((residues + 255) / 256), B), block(256);
#define MFPA_COMB_LAUNCH(TI, TO)                                                                                                        \
  hipLaunchKernelGGL((comb_kernel<TI, TO>), grid, block, 0, st, static_cast<const TI*>(x), ldx, T, params, params_per_row, max_delay,   \
                     apply, static_cast<TO*>(y))
  if (x_f64 && y_f64)
    MFPA_COMB_LAUNCH(double, double);
  else if (x_f64)
    MFPA_COMB_LAUNCH(double, float);
  else if (y_f64)
    MFPA_COMB_LAUNCH(float, double);
  else
    MFPA_COMB_LAUNCH(float, float);
#undef MFPA_COMB_LAUNCH
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
