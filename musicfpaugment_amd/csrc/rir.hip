// Room impulse responses for MI355X (gfx950): the image-source method for a shoebox room (Allen and Berkley), every image a
// Hann-windowed sinc of filter_len taps at its fractional delay, float64 throughout (include/mfpa.h has the formula).
//
// Mapping: one workgroup of four wavefronts = 64 consecutive output samples (a tile) of one room, no atomics.  Wavefront w takes the
// image rows ix = -N + w, -N + w + 4, ...; a lane keeps ONE output sample in a register and adds to it the taps of its wavefront's
// images in a fixed order, and wavefront 0 adds the four partial sums in the order ((0 + 1) + 2) + 3 through LDS: a row's bits depend
// neither on the run nor on the batch the room sits in.  (One wavefront per tile walking every image took 3.6 to 3.9 times as long for
// one room and 1.5 times for 64 rooms at order 47: a tile is one chain of dependent float64 operations per image, and late tiles meet
// thousands of images.  DESIGN.md section 3.16.)
//   1. tables: per axis and signed reflection index i in [-N, N] the squared distance X[i] of the image coordinate to the
//      microphone's and the wall gain G[i], 3 x (2N + 1) doubles each, built by the workgroup in LDS; beside them cos and sin of
//      pi j / half, j = -half .. half, for the window.
//   2. walk: the wavefront walks the (ix, iy) columns in index order, the lanes spread over iz (64 at a time, index order).  A
//      row ix or a column is left out whole when X, or X + Y, already lies beyond the tile's distance window, or X + Y plus the
//      column's largest Z falls short of it (the image coordinate grows with i, so the largest Z of [-R, R] sits at an end).  The
//      bounds are slack (one sample and 1e-9 of the distance): they only save work, the decision is taken per image on tau.
//   3. candidates: every lane forms d, tau = (d fs) / c and a ballot picks the images whose window can meet the tile; those lanes
//      form amp, floor(tau), frac = tau - floor(tau) (exact) and sin(pi frac), cos / sin(pi frac / half).
//   4. taps: for each set bit in lane order the five values are read from that lane (v_readlane) and every lane adds its own
//      sample's tap.  With j = k - floor(tau), x = j - frac rounds to the very double k - tau rounds to;
//      sin(pi x) = -(-1)^j sin(pi frac), so there is one sine per image, and cos(pi x / half) comes from the j table by the angle
//      sum.  A lane outside the window (|x| > half) or the row adds nothing.
// Arithmetic: compiled with -ffp-contract=off (csrc/build.py), so the tables, d and tau are tests/_rir_oracle.py's float64
// values operation for operation; the sine of the fraction is more accurate than the oracle's sin(pi (k - tau)).
#include "mfpa_common.h"

namespace {

constexpr int MAX_ORDER = 128;
constexpr int MAX_FILTER = 255;
constexpr int MAX_LENGTH = 262144;
constexpr int WAVES = 4;                                  // wavefronts (tiles of 64 samples) per workgroup
constexpr int AXIS = 2 * MAX_ORDER + 1;
constexpr double PI = 3.14159265358979323846;
constexpr double FOUR_PI = 4.0 * PI;
constexpr double SLACK = 1e-9;

__device__ __forceinline__ double from_lane(double v, int src) {          // src is the same in every lane
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

template <typename T>
__global__ __launch_bounds__(64 * WAVES) void rir_shoebox_kernel(const double* __restrict__ geom, int N, int length, double fs, double c,
                                                                 int half, int reversed, T* __restrict__ out, long long ldo) {
  __shared__ double dist2[3][AXIS];
  __shared__ double gain[3][AXIS];
  __shared__ double win_cos[MAX_FILTER], win_sin[MAX_FILTER];
  __shared__ double partial[WAVES][MFPA_WAVE];
  const double* g = geom + (size_t)blockIdx.y * 15;       // room, source, mic, absorption x0 x1 y0 y1 z0 z1
  const int side = 2 * N + 1;
  for (int t = threadIdx.x; t < 3 * side; t += 64 * WAVES) {
    const int a = t / side, i = t % side - N;
    const double L = g[a], s = g[3 + a], m = g[6 + a];
    const double b0 = __dsqrt_rn(1.0 - g[9 + 2 * a]), b1 = __dsqrt_rn(1.0 - g[10 + 2 * a]);
    const int p = i & 1, n = (i + p) / 2;                 // i + p is even
    const double img = p ? (double)(i + 1) * L - s : s + (double)i * L;
    const double dd = img - m;
    dist2[a][i + N] = dd * dd;
    gain[a][i + N] = pow(b0, (double)abs(n - p)) * pow(b1, (double)abs(n));      // pow(0, 0) = 1: a fully absorbing wall nobody hits
  }
  for (int t = threadIdx.x; t <= 2 * half; t += 64 * WAVES) {
    const double u = (double)(t - half) / (double)half;
    win_cos[t] = cospi(u);
    win_sin[t] = sinpi(u);
  }
  __syncthreads();

  const int lane = threadIdx.x & (MFPA_WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int k0 = blockIdx.x * MFPA_WAVE;                  // < length: the grid has ceil(length / 64) tiles
  const int kend = min(k0 + MFPA_WAVE - 1, length - 1);
  const int k = k0 + lane;
  // the tile's window in samples (tau) and, slack, in squared metres
  const double tlo = (double)(k0 - half - 1), thi = (double)(kend + half + 1);
  const double dhi = thi * (c / fs) * (1.0 + SLACK), dlo = tlo * (c / fs) * (1.0 - SLACK);
  const double dhi2 = dhi * dhi, dlo2 = dlo > 0.0 ? dlo * dlo : -1.0;
  const double dhalf = (double)half;
  double h = 0.0;
  for (int ix = -N + wave; ix <= N; ix += WAVES) {
    const double X = dist2[0][ix + N];
    if (X > dhi2) continue;
    const double gx = gain[0][ix + N];
    const int ny = N - abs(ix);
    for (int iy = -ny; iy <= ny; ++iy) {
      const double XY = X + dist2[1][iy + N];
      if (XY > dhi2) continue;
      const int R = ny - abs(iy);
      if (XY + fmax(dist2[2][N + R], dist2[2][N - R]) < dlo2) continue;
      const double gxy = gx * gain[1][iy + N];
      for (int z0 = -R; z0 <= R; z0 += MFPA_WAVE) {
        const int iz = z0 + lane;
        const bool live = iz <= R;
        const int zi = live ? iz + N : N;
        const double d = __dsqrt_rn(XY + dist2[2][zi]);
        const double G = gxy * gain[2][zi];
        const double tau = (d * fs) / c;
        // an image at distance 0 or with no gain left contributes nothing; a NaN fails the comparisons
        const bool cand = live && tau > tlo && tau < thi && d > 0.0 && G != 0.0;
        unsigned long long todo = __ballot(cand);
        if (!todo) continue;
        const double amp = G / (FOUR_PI * d);
        const double whole = floor(cand ? tau : 0.0);      // within (-half - 1, length + half + 1) for a candidate: fits an int
        const double frac = (cand ? tau : 0.0) - whole;
        const int first = (int)whole;
        const double sin_frac = sinpi(frac);
        double sin_win, cos_win;
        sincospi(frac / dhalf, &sin_win, &cos_win);
        while (todo) {
          const int src = __ffsll(todo) - 1;
          todo &= todo - 1;
          const double a = from_lane(amp, src), fr = from_lane(frac, src), s1 = from_lane(sin_frac, src);
          const double sw = from_lane(sin_win, src), cw = from_lane(cos_win, src);
          const int j = k - __builtin_amdgcn_readlane(first, src);
          const double x = (double)j - fr;
          const int ji = min(max(j + half, 0), 2 * half);
          const double w = 0.5 * (1.0 + (win_cos[ji] * cw + win_sin[ji] * sw));
          const double sinc = x == 0.0 ? 1.0 : ((j & 1) ? s1 : -s1) / (PI * x);
          if (fabs(x) <= dhalf) h += a * w * sinc;
        }
      }
    }
  }
  partial[wave][lane] = h;
  __syncthreads();
  if (wave == 0 && k < length) {
    h = ((partial[0][lane] + partial[1][lane]) + partial[2][lane]) + partial[3][lane];
    out[(size_t)blockIdx.y * ldo + (reversed ? length - 1 - k : k)] = (T)h;
  }
}

bool finite_positive(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }

}  // namespace

extern "C" {

int mfpa_rir_image_count(int max_order, long long* out) {
  if (!out || max_order < 0 || max_order > MAX_ORDER) return MFPA_EINVAL;
  const long long n = max_order;
  *out = (2 * n + 1) * (2 * n * n + 2 * n + 3) / 3;
  return MFPA_OK;
}

int mfpa_rir_shoebox(const double* geom, int B, int max_order, int length, double fs, double c, int filter_len, int reversed, int out_f64,
                     void* out, long long ldo, void* stream) {
  if (B < 0 || B > 65535 || max_order < 0 || max_order > MAX_ORDER || length < 1 || length > MAX_LENGTH || ldo < length ||
      filter_len < 3 || filter_len > MAX_FILTER || !(filter_len & 1) || !finite_positive(fs) || !finite_positive(c) ||
      (reversed != 0 && reversed != 1) || (out_f64 != 0 && out_f64 != 1))
    return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!geom || !out || (reinterpret_cast<uintptr_t>(geom) & 7) || (reinterpret_cast<uintptr_t>(out) & (out_f64 ? 7 : 3))) return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const dim3 grid((length + MFPA_WAVE - 1) / MFPA_WAVE, B), block(64 * WAVES);
  const int half = (filter_len - 1) / 2;
  if (out_f64)
    hipLaunchKernelGGL(rir_shoebox_kernel<double>, grid, block, 0, st, geom, max_order, length, fs, c, half, reversed, static_cast<double*>(out), ldo);
  else
    hipLaunchKernelGGL(rir_shoebox_kernel<float>, grid, block, 0, st, geom, max_order, length, fs, c, half, reversed, static_cast<float*>(out), ldo);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
