// Lossy coding for MI355X (gfx950): an MDCT transform codec with a masking-shaped noise allocation (mfpa_transform_codec) and
// mu-law companding (mfpa_mulaw); float64 arithmetic, float32 or float64 samples (include/mfpa.h has both definitions).
//
// codec_kernel.  One workgroup of four wavefronts = MFPA_CODEC_FRAMES + 1 consecutive frames of one row = the MFPA_CODEC_FRAMES
// blocks of 256 outputs between them; eight lanes per frame, so all lanes of a frame sit in one wavefront and talk through LDS
// without a workgroup barrier.  The grid's neighbour transforms the shared edge frame again (32 transforms per 31 blocks) instead of
// exchanging it, so every workgroup writes its own blocks with plain stores.
//   1. Thread i of the workgroup folds sample i of every frame: the 512 windowed samples of an MDCT frame fold to the 256 inputs u of
//      a DCT-IV (u[n] = -z[383 - n] - z[384 + n] below 128, z[n - 128] - z[383 - n] from 128 on).  Coalesced row reads, zeros
//      outside the row.
//   2. The DCT-IV of 256 reals is a 128-point complex transform: t[n] = (u[2n] + i u[255 - 2n]) o[n], o[n] = exp(-i pi (8n + 1) / 2048),
//      c = o FFT128(t), X[2k] = Re c[k], X[255 - 2k] = -Im c[k].  Lane l holds n = l + 8 j: a 16-point transform in registers
//      (mfpa_fft16.h), twiddles, one exchange through a padded 16 x 8 LDS tile, two 8-point transforms.  The outputs land on the
//      indices the lane started from, so the quantiser and the inverse (the same DCT-IV) need no further exchange.
//   3. The allocation runs in the frame's own lanes: lane l owns bands l, l + 8, ...; band sums in ascending k from the frame's
//      spectrum in LDS, then thresholds, candidates and steps through 4 x 32 doubles of LDS.
//   LDS: a frame owns 256 doubles, which hold in turn its folded input, the exchange tile (while the values are in registers), its
//   spectrum, three of the allocation's four tables (the spectrum is read by the band sums alone), the exchange tile again and the
//   inverse's output; with the fourth table and the twiddles 80.8 KB per workgroup, so two workgroups share a compute unit.
//   4. The inverse DCT-IV, its 256 values to LDS; thread i then forms sample i of every block from the two frames that cover it, the
//      earlier one first.
// No atomics, no work buffer; nothing depends on the batch or on the grid.
//
// mulaw_kernel.  Elementwise, grid-stride.
//
// Arithmetic: compiled with -ffp-contract=off (csrc/build.py): every product and sum of the allocation and of the quantiser is rounded
// on its own in the order of the formula, which is the order of tests/_codec_oracle.py.
#include "mfpa_fft16.h"

#include <cmath>

namespace {

constexpr int M = 256;
constexpr int G = MFPA_CODEC_FRAMES;
constexpr int SLOTS = G + 1;
constexpr int MAX_BANDS = MFPA_CODEC_MAX_BANDS;
constexpr int EX = 16 * 9;                      // padded 16 x 8 exchange tile of doubles: inside the frame's own 256 doubles, free meanwhile
constexpr long long MAX_SAMPLES = 1LL << 30;
static_assert(SLOTS * 8 == 256 && EX <= M && 3 * MAX_BANDS <= M, "eight lanes per frame; the exchange tile and the band statistics reuse the frame's slot");

struct Bands {
  int n;
  int edges[MAX_BANDS + 1];
  double up[MAX_BANDS], down[MAX_BANDS];        // 10^(-up_db d / 10), 10^(-down_db d / 10), d = 0 .. 31
};

// LDS, in doubles
constexpr int OFF_BUF = 0;                      // [SLOTS][256]: folded input, then spectrum, then the inverse's output
constexpr int OFF_VAR = OFF_BUF + SLOTS * M;    // [SLOTS][32]: band variances, then the steps
constexpr int OFF_WIN = OFF_VAR + SLOTS * MAX_BANDS;   // [256]: the window's first half, w[n] = w[511 - n]
constexpr int OFF_OM = OFF_WIN + 256;           // [128] complex
constexpr int OFF_TW = OFF_OM + 256;            // [128] complex
constexpr int OFF_UP = OFF_TW + 256;            // [32]
constexpr int OFF_DOWN = OFF_UP + MAX_BANDS;    // [32]
constexpr int OFF_INT = OFF_DOWN + MAX_BANDS;   // ints from here: edges [33], then band_of [256] as bytes
constexpr size_t LDS_BYTES = sizeof(double) * OFF_INT + sizeof(int) * (MAX_BANDS + 4) + 256;
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per compute unit");

// In-place 8-point DFT, natural order in and out.
__device__ __forceinline__ void dft8(cd (&v)[8]) {
  constexpr double R2 = 0.70710678118654752440;
  dft4(v[0], v[2], v[4], v[6]);                 // E[k] at v[2k]
  dft4(v[1], v[3], v[5], v[7]);                 // O[k] at v[2k + 1]
  const cd e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
  const cd o0 = v[1], o1 = cmul(v[3], cd{R2, -R2}), o2 = cd{v[5].im, -v[5].re}, o3 = cmul(v[7], cd{-R2, -R2});
  v[0] = e0 + o0;
  v[1] = e1 + o1;
  v[2] = e2 + o2;
  v[3] = e3 + o3;
  v[4] = e0 - o0;
  v[5] = e1 - o1;
  v[6] = e2 - o2;
  v[7] = e3 - o3;
}

// 128-point forward DFT over the 8 lanes l = 0..7 of one frame.  In: a[j] = t[l + 8 j].  Out: z[m] = T[l + 8 m].  ex: the frame's EX
// doubles of LDS; tw[2m], tw[2m+1] = cos, -sin of 2 pi m / 128.  Real and imaginary parts go through the same slots one after the other.
__device__ __forceinline__ void fft128_lanes(cd (&a)[16], cd (&z)[16], double* ex, int l, const double* tw) {
  dft16(a);                                     // A[k1] at a[4*(k1&3) + (k1>>2)]
  double tim[16];
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) {
    const int m = (l * k1) & 127;
    const cd v = cmul(a[4 * (k1 & 3) + (k1 >> 2)], cd{tw[2 * m], tw[2 * m + 1]});
    ex[k1 * 9 + l] = v.re;
    tim[k1] = v.im;
  }
  wave_sync();
  cd r0[8], r1[8];                              // k1 = l and k1 = l + 8 over the lanes
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    r0[q].re = ex[l * 9 + q];
    r1[q].re = ex[(l + 8) * 9 + q];
  }
  wave_sync();
#pragma unroll
  for (int k1 = 0; k1 < 16; ++k1) ex[k1 * 9 + l] = tim[k1];
  wave_sync();
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    r0[q].im = ex[l * 9 + q];
    r1[q].im = ex[(l + 8) * 9 + q];
  }
  wave_sync();
  dft8(r0);                                     // T[l + 16 k2]
  dft8(r1);                                     // T[l + 8 + 16 k2]
#pragma unroll
  for (int k2 = 0; k2 < 8; ++k2) {
    z[2 * k2] = r0[k2];
    z[2 * k2 + 1] = r1[k2];
  }
}

// DCT-IV of 256 reals over the 8 lanes of a frame, in place: e[j] = u[2n], o[j] = u[255 - 2n] at n = l + 8 j, in and out.
__device__ __forceinline__ void dct4_lanes(double (&e)[16], double (&o)[16], double* ex, int l, const double* om, const double* tw) {
  cd a[16], z[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = l + 8 * j;
    a[j] = cmul(cd{e[j], o[j]}, cd{om[2 * n], om[2 * n + 1]});
  }
  fft128_lanes(a, z, ex, l, tw);
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const int k = l + 8 * m;
    const cd c = cmul(z[m], cd{om[2 * k], om[2 * k + 1]});
    e[m] = c.re;
    o[m] = -c.im;
  }
}

// One coefficient through the band's quantiser; st < 0: the band is not coded.
__device__ __forceinline__ double quantise(double X, double st, int& count) {
  if (!(st >= 0.0)) return 0.0;
  const double t = fabs(X) / st;
  if (!(t < 0x1p52)) {                          // finer than a double resolves (a step that underflowed included): the value itself
    count += X != 0.0;
    return X;
  }
  const double q = floor(t + 0.5);
  count += q != 0.0;
  const double s = X > 0.0 ? 1.0 : (X < 0.0 ? -1.0 : 0.0);
  return s * q * st;
}

template <typename TI, typename TO>
__global__ __launch_bounds__(256) void codec_kernel(const TI* __restrict__ x, long long ldx, int T, int F, double rate,
                                                    const double* __restrict__ row_rates, const Bands bands,
                                                    const unsigned char* __restrict__ apply_row, TO* __restrict__ y,
                                                    double* __restrict__ lambda_out, int* __restrict__ coded_out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* lds = reinterpret_cast<double*>(smem);
  double* buf = lds + OFF_BUF;
  double* win = lds + OFF_WIN;
  double* om = lds + OFF_OM;
  double* tw = lds + OFF_TW;
  double* s_up = lds + OFF_UP;
  double* s_down = lds + OFF_DOWN;
  int* s_edges = reinterpret_cast<int*>(lds + OFF_INT);
  unsigned char* band_of = reinterpret_cast<unsigned char*>(s_edges + MAX_BANDS + 4);

  const int tid = threadIdx.x, l = tid & 7, s = tid >> 3;
  const int row = blockIdx.y, f0 = blockIdx.x * G;
  const int n_blocks = F - 1;
  const int nb = bands.n;
  const TI* xr = x + (size_t)row * ldx;
  TO* yr = y + (size_t)row * T;
  const int f = f0 + s;
  const bool owns_stats = l == 0 && f < F && (s < G || f == F - 1);
  const double nan = __longlong_as_double(0x7ff8000000000000LL), inf = __longlong_as_double(0x7ff0000000000000LL);

  if (apply_row && !apply_row[row]) {           // the whole workgroup alike
    for (int r = 0; r < G; ++r) {
      const int h = f0 + r, pos = h * M + tid;
      if (h >= n_blocks) break;
      if (pos < T) yr[pos] = (TO)xr[pos];
    }
    if (owns_stats) {
      if (lambda_out) lambda_out[(size_t)row * F + f] = nan;
      if (coded_out) coded_out[(size_t)row * F + f] = 0;
    }
    return;
  }

  // 0. tables
  win[tid] = sinpi(((double)tid + 0.5) / 512.0);
  if (tid < 128) {
    om[2 * tid] = cospi((double)(8 * tid + 1) / 2048.0);
    om[2 * tid + 1] = -sinpi((double)(8 * tid + 1) / 2048.0);
    tw[2 * tid] = cospi((double)tid / 64.0);
    tw[2 * tid + 1] = -sinpi((double)tid / 64.0);
  }
  if (tid < MAX_BANDS) {
    s_up[tid] = bands.up[tid];
    s_down[tid] = bands.down[tid];
  }
  if (tid <= MAX_BANDS) s_edges[tid] = bands.edges[tid < nb ? tid : nb];
  {
    int b = 0;
    for (int j = 1; j < nb; ++j) b += tid >= bands.edges[j];
    band_of[tid] = (unsigned char)b;
  }
  __syncthreads();

  // 1. fold: thread tid forms u[tid] of every frame
  for (int fs = 0; fs < SLOTS; ++fs) {
    const int base = (f0 + fs - 1) * M;         // the row's index of the frame's sample 0
    int na, nbb;
    if (tid < 128) {
      na = 383 - tid;
      nbb = 384 + tid;
    } else {
      na = tid - 128;
      nbb = 383 - tid;
    }
    const int ia = base + na, ib = base + nbb;
    const double za = win[na < M ? na : 511 - na] * ((ia >= 0 && ia < T) ? (double)xr[ia] : 0.0);
    const double zb = win[nbb < M ? nbb : 511 - nbb] * ((ib >= 0 && ib < T) ? (double)xr[ib] : 0.0);
    buf[fs * M + tid] = tid < 128 ? -za - zb : za - zb;
  }
  __syncthreads();

  // 2. analysis
  double* fb = buf + s * M;
  double* ex = fb;                              // the exchange tile: the slot itself, whose values are in registers while it is used
  double e[16], o[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int n = l + 8 * j;
    e[j] = fb[2 * n];
    o[j] = fb[255 - 2 * n];
  }
  wave_sync();
  dct4_lanes(e, o, ex, l, om, tw);

  // 3. allocation and quantiser
  const double R = row_rates ? row_rates[row] : rate;
  double lam = -inf;
  int count = 0;
  if (!(R == inf)) {                            // the row's, so the workgroup's
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int k = l + 8 * m;
      fb[2 * k] = e[m];
      fb[255 - 2 * k] = o[m];
    }
    wave_sync();
    double* s_var = lds + OFF_VAR + s * MAX_BANDS;   // later the steps
    double* s_L = fb;                            // the spectrum in LDS is read by the band sums alone
    double* s_m = fb + MAX_BANDS;
    double* s_cand = fb + 2 * MAX_BANDS;
    for (int b = l; b < nb; b += 8) {
      const int k0 = s_edges[b], k1 = s_edges[b + 1];
      double acc = 0.0;
      for (int k = k0; k < k1; ++k) acc += fb[k] * fb[k];
      s_var[b] = acc / (double)(k1 - k0);
    }
    wave_sync();
    for (int b = l; b < nb; b += 8) {
      double mx = 0.0;
      for (int bp = 0; bp < nb; ++bp) mx = fmax(mx, s_var[bp] * (b >= bp ? s_up[b - bp] : s_down[bp - b]));
      const double var = s_var[b];
      s_L[b] = var > 0.0 ? log2(var) - log2(mx) : nan;
      s_m[b] = mx;
    }
    wave_sync();
    for (int j = l; j < nb; j += 8) {
      const double Lj = s_L[j];
      double cand = nan;
      if (Lj == Lj) {
        double S = 0.0, P = 0.0;
        for (int b = 0; b < nb; ++b) {
          const double Lb = s_L[b];
          if (Lb >= Lj) {
            const double W = (double)(s_edges[b + 1] - s_edges[b]);
            S += W;
            P += W * Lb;
          }
        }
        const double lj = (P - 2.0 * R) / S;
        if (lj < Lj) cand = lj;
      }
      s_cand[j] = cand;
    }
    wave_sync();
    lam = nan;
    double best = inf;
    for (int j = 0; j < nb; ++j) {
      const double c = s_cand[j], Lj = s_L[j];
      if (c == c && Lj < best) {
        best = Lj;
        lam = c;
      }
    }
    for (int b = l; b < nb; b += 8) s_var[b] = s_L[b] > lam ? sqrt(12.0 * (s_m[b] * exp2(lam))) : -1.0;
    wave_sync();
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const int k = l + 8 * m;
      e[m] = quantise(e[m], s_var[band_of[2 * k]], count);
      o[m] = quantise(o[m], s_var[band_of[255 - 2 * k]], count);
    }
    count += __shfl_xor(count, 1);
    count += __shfl_xor(count, 2);
    count += __shfl_xor(count, 4);
    wave_sync();                                // the exchange tile is the inverse's again
  }
  if (owns_stats) {
    if (lambda_out) lambda_out[(size_t)row * F + f] = lam;
    if (coded_out) coded_out[(size_t)row * F + f] = count;
  }

  // 4. synthesis: the same DCT-IV; the scale 2 / M rides on the window below
  dct4_lanes(e, o, ex, l, om, tw);
#pragma unroll
  for (int m = 0; m < 16; ++m) {
    const int k = l + 8 * m;
    fb[2 * k] = e[m];
    fb[255 - 2 * k] = o[m];
  }
  __syncthreads();
  // y_f[256 + i] = (2 / M) w[256 + i] * -(i < 128 ? v[127 - i] : v[i - 128]);  y_f[i] = (2 / M) w[i] * (i < 128 ? v[128 + i] : -v[383 - i])
  const double wa = win[255 - tid], wb = win[tid];
  const int ja = tid < 128 ? 127 - tid : tid - 128, jb = tid < 128 ? 128 + tid : 383 - tid;
  constexpr double SCALE = 2.0 / M;
  for (int r = 0; r < G; ++r) {
    const int h = f0 + r, pos = h * M + tid;
    if (h >= n_blocks) break;
    if (pos < T) {
      const double va = -buf[r * M + ja];
      const double vb = tid < 128 ? buf[(r + 1) * M + jb] : -buf[(r + 1) * M + jb];
      yr[pos] = (TO)(SCALE * (wa * va) + SCALE * (wb * vb));
    }
  }
}

// MODE 0: encode (TO = int), 1: decode (TI = int), 2: both
template <typename TI, typename TO, int MODE>
__global__ __launch_bounds__(256) void mulaw_kernel(const TI* __restrict__ x, long long n, long long T, double mu, double l1p,
                                                    const unsigned char* __restrict__ apply_row, TO* __restrict__ y) {
  const long long step = (long long)gridDim.x * 256;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
    if (MODE == 2 && apply_row && !apply_row[i / T]) {
      y[i] = (TO)x[i];
      continue;
    }
    double code;
    if (MODE != 1) {
      const double v = fmin(fmax((double)x[i], -1.0), 1.0);
      const double sg = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
      const double c = sg * log1p(mu * fabs(v)) / l1p;
      code = floor((c + 1.0) / 2.0 * mu + 0.5);
    } else {
      code = (double)x[i];
    }
    if (MODE == 0) {
      y[i] = (TO)code;
    } else {
      const double v = 2.0 * code / mu - 1.0;
      const double sg = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
      y[i] = (TO)(sg * (exp(fabs(v) * l1p) - 1.0) / mu);
    }
  }
}

bool aligned(const void* p, int f64) { return (reinterpret_cast<uintptr_t>(p) & (f64 ? 7 : 3)) == 0; }
bool flag(int v) { return v == 0 || v == 1; }

}  // namespace

extern "C" {

int mfpa_transform_codec(const void* x, int x_f64, long long ldx, int B, long long T, double rate, const double* row_rates,
                         const int* band_edges, int n_bands, double up_db, double down_db, const unsigned char* apply, void* y, int y_f64,
                         double* lambda_out, int* coded_out, void* stream) {
  if (B < 1 || B > 65535 || T < 1 || T > MAX_SAMPLES || ldx < T || !flag(x_f64) || !flag(y_f64) || n_bands < 1 || n_bands > MAX_BANDS)
    return MFPA_EINVAL;
  if (!x || !y || !band_edges || !aligned(x, x_f64) || !aligned(y, y_f64) || !aligned(row_rates, 1) || !aligned(lambda_out, 1) ||
      !aligned(coded_out, 0))
    return MFPA_EINVAL;
  if (!(up_db >= 0.0) || !(down_db >= 0.0) || std::isinf(up_db) || std::isinf(down_db)) return MFPA_EINVAL;
  if (!row_rates && rate != rate) return MFPA_EINVAL;
  Bands bands;
  bands.n = n_bands;
  if (band_edges[0] != 0 || band_edges[n_bands] != M) return MFPA_EINVAL;
  for (int b = 0; b < n_bands; ++b)
    if (band_edges[b + 1] <= band_edges[b]) return MFPA_EINVAL;
  for (int b = 0; b <= MAX_BANDS; ++b) bands.edges[b] = band_edges[b < n_bands ? b : n_bands];
  for (int d = 0; d < MAX_BANDS; ++d) {
    bands.up[d] = pow(10.0, -(up_db * (double)d) / 10.0);
    bands.down[d] = pow(10.0, -(down_db * (double)d) / 10.0);
  }
  hipStream_t st = mfpa_stream(stream);
  const int n_blocks = (int)((T + M - 1) / M), F = n_blocks + 1, t = (int)T;
  const dim3 grid((unsigned)((n_blocks + G - 1) / G), B), block(256);
#define MFPA_CODEC_LAUNCH(TI, TO)                                                                                                      \
  hipLaunchKernelGGL((codec_kernel<TI, TO>), grid, block, LDS_BYTES, st, static_cast<const TI*>(x), ldx, t, F, rate, row_rates, bands,  \
                     apply, static_cast<TO*>(y), lambda_out, coded_out)
  if (x_f64 && y_f64)
    MFPA_CODEC_LAUNCH(double, double);
  else if (x_f64)
    MFPA_CODEC_LAUNCH(double, float);
  else if (y_f64)
    MFPA_CODEC_LAUNCH(float, double);
  else
    MFPA_CODEC_LAUNCH(float, float);
#undef MFPA_CODEC_LAUNCH
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_mulaw(const void* x, int x_f64, int B, long long T, int channels, int mode, const unsigned char* apply, void* y, int y_f64,
               void* stream) {
  if (B < 1 || B > 65535 || T < 1 || T > MAX_SAMPLES || channels < 2 || channels > 65536 || !flag(x_f64) || !flag(y_f64))
    return MFPA_EINVAL;
  if (mode != MFPA_MULAW_ENCODE && mode != MFPA_MULAW_DECODE && mode != MFPA_MULAW_ROUNDTRIP) return MFPA_EINVAL;
  if ((mode == MFPA_MULAW_ENCODE && y_f64) || (mode == MFPA_MULAW_DECODE && x_f64) || (mode != MFPA_MULAW_ROUNDTRIP && apply))
    return MFPA_EINVAL;
  if (!x || !y || !aligned(x, x_f64) || !aligned(y, y_f64)) return MFPA_EINVAL;
  hipStream_t st = mfpa_stream(stream);
  const long long n = (long long)B * T;
  const long long want = (n + 255) / 256;
  const dim3 grid((unsigned)(want < 65536 ? want : 65536)), block(256);
  const double mu = (double)(channels - 1), l1p = log1p(mu);
#define MFPA_MULAW_LAUNCH(TI, TO, MODE)                                                                                                 \
  hipLaunchKernelGGL((mulaw_kernel<TI, TO, MODE>), grid, block, 0, st, static_cast<const TI*>(x), n, T, mu, l1p, apply, static_cast<TO*>(y))
  if (mode == MFPA_MULAW_ENCODE) {
    if (x_f64)
      MFPA_MULAW_LAUNCH(double, int, 0);
    else
      MFPA_MULAW_LAUNCH(float, int, 0);
  } else if (mode == MFPA_MULAW_DECODE) {
    if (y_f64)
      MFPA_MULAW_LAUNCH(int, double, 1);
    else
      MFPA_MULAW_LAUNCH(int, float, 1);
  } else if (x_f64 && y_f64) {
    MFPA_MULAW_LAUNCH(double, double, 2);
  } else if (x_f64) {
    MFPA_MULAW_LAUNCH(double, float, 2);
  } else if (y_f64) {
    MFPA_MULAW_LAUNCH(float, double, 2);
  } else {
    MFPA_MULAW_LAUNCH(float, float, 2);
  }
#undef MFPA_MULAW_LAUNCH
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
