// Device side of the composable waveform transforms (augmentation/transformations/*.py, augmentation/composition.py of
// deezer/musicFPaugment) that csrc/augment.hip does not already cover:
//   bandpass_taps_kernel   julius 0.2.7 BandPassFilter restated: two windowed-sinc low-passes on ONE window, subtracted.  One pass of
//                          mfpa_fir over these taps is the band-pass (out_mode 0) or the band-stop x - bandpass (out_mode 1).
//   colored_noise_kernel   AddColoredNoise._gen_noise (colored_noise.py:12-38): rfft of N white samples, power-law mask, irfft,
//                          RMS normalisation, tiling to T samples -- one workgroup per example, the whole transform in LDS.
//
// The real FFT of N samples is a complex FFT of M = N/2 points (even samples real part, odd samples imaginary part) and one
// split pass; the inverse is the mirror image.  The complex engine is a Stockham autosort FFT with radices 5, 3, 4, 2 (in that
// order) over ONE LDS buffer of M complex floats: a pass reads all its inputs into registers, the workgroup meets at a
// barrier, and the pass writes its outputs -- so the buffer needs no twin, and N = 16000 fits the classic 64 KiB.
//   pass(R, Ns):  butterfly j < M/R reads  in[j + t M/R] * W^(t k),  k = j mod Ns,  W = exp(-2 pi i / (Ns R)),  t < R
//                 and writes out[(j / Ns) Ns R + k + t Ns]
// Reads are contiguous over j (ds_read_b64, no bank conflict).  Writes are runs of Ns contiguous complex values R * Ns apart:
// contiguous enough once Ns >= 32.  Before that, by the addresses (not measured): a stride of 3 or 5 complex values visits every
// bank once (odd multiples of two dwords), so 5 and 3 go first; a power-of-two size pays a 4-way conflict in its first two
// radix-4 passes (Ns = 1, 4) and a 2-way one in the third (Ns = 16), of seven passes per transform.
// Twiddles come from a table the host computes in float64 and rounds once (mfpa_rfft_twiddles): tw[q] = exp(-2 pi i q / N).
// Every sum has a fixed order and there is no atomic: an example's output depends on its N samples, f_decay and N alone.
#include <math.h>

#include "mfpa_common.h"

namespace {

constexpr int RFFT_THREADS = 1024;
constexpr int RFFT_MAX_M = MFPA_RFFT_MAX_N / 2;                  // complex points the LDS buffer holds
constexpr int RFFT_LDS_BYTES = RFFT_MAX_M * 8 + 64;              // + 16 floats of cross-wave reduction scratch

// A complex float.  Not HIP's float2: its constructors are functions of the HIP headers, which the compiler will not inline into a
// kernel compiled under MFPA_NO_PK_F32 (another target attribute) -- every brace would become a call through scratch.
struct __attribute__((aligned(8))) cf32 {
  float x, y;
};

// __syncthreads() and __shfl_xor() are header functions as well: spelled with the builtins they wrap, for the same reason.
__device__ __forceinline__ void wg_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ float wave_xor(float v, int mask) {
  const int lane = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  return __int_as_float(__builtin_amdgcn_ds_bpermute((lane ^ mask) << 2, __float_as_int(v)));
}

struct rfft_plan {
  int n;
  int radix[MFPA_RFFT_MAX_RADICES];
};

// The passes of an M-point FFT, or false: 5s, then 3s, then 4s, then at most one 2.
bool make_plan(int N, rfft_plan* p) {
  if (N < 4 || (N & 1) || N > MFPA_RFFT_MAX_N) return false;
  int m = N / 2, n = 0;
  int r[32];
  while (m % 5 == 0) { r[n++] = 5; m /= 5; }
  while (m % 3 == 0) { r[n++] = 3; m /= 3; }
  while (m % 4 == 0) { r[n++] = 4; m /= 4; }
  if (m % 2 == 0) { r[n++] = 2; m /= 2; }
  if (m != 1 || n > MFPA_RFFT_MAX_RADICES) return false;
  p->n = n;
  for (int i = 0; i < MFPA_RFFT_MAX_RADICES; ++i) p->radix[i] = i < n ? r[i] : 0;
  return true;
}

__device__ __forceinline__ cf32 cmul(cf32 a, cf32 w) { return cf32{a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x}; }
__device__ __forceinline__ cf32 cadd(cf32 a, cf32 b) { return cf32{a.x + b.x, a.y + b.y}; }
__device__ __forceinline__ cf32 csub(cf32 a, cf32 b) { return cf32{a.x - b.x, a.y - b.y}; }
__device__ __forceinline__ cf32 cmul_mi(cf32 a) { return cf32{a.y, -a.x}; }       // a * (-i)

template <int R>
__device__ __forceinline__ void butterfly(cf32* v);

template <>
__device__ __forceinline__ void butterfly<2>(cf32* v) {
  const cf32 a = v[0], b = v[1];
  v[0] = cadd(a, b);
  v[1] = csub(a, b);
}

template <>
__device__ __forceinline__ void butterfly<3>(cf32* v) {
  const float s3 = 0.8660254037844386f;                                 // sin(pi / 3)
  const cf32 s = cadd(v[1], v[2]), d = cmul_mi(csub(v[1], v[2]));     // d = -i (v1 - v2)
  const cf32 m = cf32{v[0].x - 0.5f * s.x, v[0].y - 0.5f * s.y};
  v[0] = cadd(v[0], s);
  v[1] = cf32{m.x + s3 * d.x, m.y + s3 * d.y};
  v[2] = cf32{m.x - s3 * d.x, m.y - s3 * d.y};
}

template <>
__device__ __forceinline__ void butterfly<4>(cf32* v) {
  const cf32 a = cadd(v[0], v[2]), b = csub(v[0], v[2]), c = cadd(v[1], v[3]), d = cmul_mi(csub(v[1], v[3]));
  v[0] = cadd(a, c);
  v[1] = cadd(b, d);
  v[2] = csub(a, c);
  v[3] = csub(b, d);
}

template <>
__device__ __forceinline__ void butterfly<5>(cf32* v) {
  const float c1 = 0.30901699437494745f, c2 = -0.8090169943749475f;     // cos(2 pi / 5), cos(4 pi / 5)
  const float s1 = 0.9510565162951535f, s2 = 0.5877852522924731f;       // sin(2 pi / 5), sin(4 pi / 5)
  const cf32 a1 = cadd(v[1], v[4]), a2 = cadd(v[2], v[3]);
  const cf32 b1 = cmul_mi(csub(v[1], v[4])), b2 = cmul_mi(csub(v[2], v[3]));            // -i (difference)
  const cf32 p1 = cf32{v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y};
  const cf32 p2 = cf32{v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y};
  const cf32 q1 = cf32{s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y};
  const cf32 q2 = cf32{s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y};
  v[0] = cadd(v[0], cadd(a1, a2));
  v[1] = cadd(p1, q1);
  v[4] = csub(p1, q1);
  v[2] = cadd(p2, q2);
  v[3] = csub(p2, q2);
}

// One Stockham pass of radix R over buf[0..M) (see the head of the file).  `last`: the value written is (re * scale, -im * scale)
// -- the conjugate that turns the forward engine into the inverse transform, and the 1/N of the irfft.
template <int R>
__device__ __forceinline__ void fft_pass(cf32* buf, int M, int Ns, int N, const cf32* __restrict__ tw, bool last, float scale) {
  constexpr int ROUNDS = (RFFT_MAX_M / R + RFFT_THREADS - 1) / RFFT_THREADS;
  const int nb = M / R, tid = threadIdx.x;
  cf32 v[ROUNDS][R];
#pragma unroll
  for (int rr = 0; rr < ROUNDS; ++rr) {
    const int j = tid + rr * RFFT_THREADS, jj = j < nb ? j : 0;     // an idle slot reads butterfly 0 and writes nothing
#pragma unroll
    for (int t = 0; t < R; ++t) v[rr][t] = buf[jj + t * nb];
  }
  wg_barrier();
  const int twstep = N / (Ns * R);
#pragma unroll
  for (int rr = 0; rr < ROUNDS; ++rr) {
    const int j = tid + rr * RFFT_THREADS;
    if (j < nb) {
      const int blk = j / Ns, k = j - blk * Ns;
#pragma unroll
      for (int t = 1; t < R; ++t) v[rr][t] = cmul(v[rr][t], tw[t * k * twstep]);
      butterfly<R>(v[rr]);
      cf32* o = buf + blk * Ns * R + k;
#pragma unroll
      for (int t = 0; t < R; ++t) o[t * Ns] = last ? cf32{v[rr][t].x * scale, -v[rr][t].y * scale} : v[rr][t];
    }
  }
  wg_barrier();
}

__device__ __forceinline__ void fft(cf32* buf, int M, int N, const rfft_plan& plan, const cf32* __restrict__ tw, bool inverse,
                                    float scale) {
  int Ns = 1;
  for (int p = 0; p < plan.n; ++p) {
    const int r = plan.radix[p];
    const bool last = inverse && p == plan.n - 1;
    if (r == 5) fft_pass<5>(buf, M, Ns, N, tw, last, scale);
    else if (r == 3) fft_pass<3>(buf, M, Ns, N, tw, last, scale);
    else if (r == 4) fft_pass<4>(buf, M, Ns, N, tw, last, scale);
    else fft_pass<2>(buf, M, Ns, N, tw, last, scale);
    Ns *= r;
  }
}

// 1 / linspace(1, sqrt(N/2), M + 1)[k] ** f_decay in float32, torch.linspace's two-sided form (from the start below the middle,
// from the end above it).
__device__ __forceinline__ float noise_mask(int k, int M, float end, float step, float f_decay) {
  const int steps = M + 1;
  const float base = k < steps / 2 ? 1.f + step * (float)k : end - step * (float)(steps - 1 - k);
  return 1.f / powf(base, f_decay);
}

__global__ MFPA_NO_PK_F32 __launch_bounds__(RFFT_THREADS) void colored_noise_kernel(const float* __restrict__ white, int N,
                                                                                    const float* __restrict__ f_decay, int T,
                                                                                    const cf32* __restrict__ tw, rfft_plan plan,
                                                                                    float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) cf32 buf[RFFT_MAX_M];
  __shared__ float red[16];
  const int b = blockIdx.x, tid = threadIdx.x, M = N / 2;
  const float* xb = white + (size_t)b * N;
  for (int j = tid; j < M; j += RFFT_THREADS) buf[j] = cf32{xb[2 * j], xb[2 * j + 1]};
  wg_barrier();
  fft(buf, M, N, plan, tw, false, 1.f);
  // Z -> twice the real spectrum X[k], X[M-k] -> mask -> four times the packed spectrum of the inverse, stored conjugated.
  // A thread owns the pair (k, M - k): it reads and writes no other slot, so the step is in place.
  const float fd = f_decay[b];
  const float end = (float)sqrt((double)N / 2.0), step = (end - 1.f) / (float)M;
  for (int k = tid; 2 * k <= M; k += RFFT_THREADS) {
    if (k == 0) {
      const cf32 z = buf[0];
      const float y0 = noise_mask(0, M, end, step, fd) * (2.f * (z.x + z.y));
      const float ym = noise_mask(M, M, end, step, fd) * (2.f * (z.x - z.y));
      buf[0] = cf32{y0 + ym, -(y0 - ym)};
      continue;
    }
    const cf32 A = buf[k], Bc = cf32{buf[M - k].x, -buf[M - k].y}, w = tw[k];
    const cf32 e = cadd(A, Bc), o = cmul(cmul_mi(csub(A, Bc)), w);           // 2 Xe, 2 w Xo
    const float mk = noise_mask(k, M, end, step, fd), mm = noise_mask(M - k, M, end, step, fd);
    const cf32 xk = cadd(e, o), xm = csub(e, o);                             // 2 X[k], conj(2 X[M-k])
    const cf32 yk = cf32{mk * xk.x, mk * xk.y}, ymc = cf32{mm * xm.x, mm * xm.y};       // Y[k], conj(Y[M-k])
    const cf32 ye = cadd(yk, ymc), yo = cmul(csub(yk, ymc), cf32{w.x, -w.y});
    // Z'[k] = ye + i yo,  Z'[M-k] = conj(ye) + i conj(yo);  both stored conjugated
    buf[k] = cf32{ye.x - yo.y, -(ye.y + yo.x)};
    if (k != M - k) buf[M - k] = cf32{ye.x + yo.y, -(yo.x - ye.y)};
  }
  wg_barrier();
  fft(buf, M, N, plan, tw, true, (float)(0.5 / (double)N));
  // buf viewed as floats is now x[0..N): RMS in a fixed order (thread-strided partial, xor tree in the wave, 16 waves in turn)
  const float* xs = reinterpret_cast<const float*>(buf);
  float s = 0.f;
  for (int i = tid; i < N; i += RFFT_THREADS) s += xs[i] * xs[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += wave_xor(s, o);
  if ((tid & 63) == 0) red[tid >> 6] = s;
  wg_barrier();
  float tot = red[0];
  for (int w = 1; w < 16; ++w) tot += red[w];
  const float r = sqrtf(tot / (float)N) + 1e-8f;
  // out[t] = x[t mod N] / r: scalar stores up to the row's first 16-byte boundary, float4 stores after it, scalar tail
  float* ob = out + (size_t)b * T;
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(ob) >> 2) & 3)) & 3);
  if (head > T) head = T;
  if (tid < head) ob[tid] = xs[tid % N] / r;
  const int nvec = (T - head) / 4;
  for (int q = tid; q < nvec; q += RFFT_THREADS) {
    const int t = head + 4 * q;
    int i = t % N;
    mfpa_f32x4 v;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      v[c] = xs[i] / r;
      i = i + 1 == N ? 0 : i + 1;
    }
    *reinterpret_cast<mfpa_f32x4*>(ob + t) = v;
  }
  const int t = head + 4 * nvec + tid;
  if (tid < 4 && t < T) ob[t] = xs[t % N] / r;
}

// taps[k] = hi[k] / sum(hi) - lo[k] / sum(lo), each c in {lo, hi}: 2c hann(k) sinc(2c pi (k - half)), k = 0..2*half, in the
// arithmetic of lowpass_taps_kernel (csrc/augment.hip) -- float32 taps, float64 sums, one float32 reciprocal per filter -- but for
// the sine's argument, which is reduced first (below).
__device__ __forceinline__ float sinc_tap(float c, int k, int h, int n) {
  const float win = 0.5f - 0.5f * cosf(6.283185307179586f * (float)k / (float)(n - 1));   // hann_window(n, periodic=False)
  const float t = (float)(k - h);
  const float arg = 2.f * c * 3.141592653589793f * t;
  // sin(2 pi c t) of the phase reduced to [-1/2, 1/2]: c * t is exact in float64 (24 x 32 bits), so is its distance from the nearest
  // integer.  lowpass_taps_kernel takes sinf(arg) directly; on a window of 64 001 points (|arg| up to 4e4, half an ulp of it 2e-3
  // rad) that puts 1e-6 on the unit sum of the wider low-pass and 4e-7 on its centre taps -- measured, and gone with the reduction.
  const double turns = (double)c * (double)(k - h);
  const float sinc = (k == h) ? 1.f : sinf(6.283185307179586f * (float)(turns - rint(turns))) / arg;
  return 2.f * c * win * sinc;
}

__global__ __launch_bounds__(256) void bandpass_taps_kernel(const float* __restrict__ cut_lo, const float* __restrict__ cut_hi,
                                                            const int* __restrict__ half, const long long* __restrict__ tap_off,
                                                            float* __restrict__ taps) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const int h = half[b], n = 2 * h + 1;
  const float cl = cut_lo[b], ch = cut_hi[b];
  float* T = taps + tap_off[b];
  double sl = 0.0, sh_ = 0.0;
  for (int k = tid; k < n; k += 256) {
    sl += (double)sinc_tap(cl, k, h, n);
    sh_ += (double)sinc_tap(ch, k, h, n);
  }
  __shared__ double sh[2][256];
  sh[0][tid] = sl;
  sh[1][tid] = sh_;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      sh[0][tid] += sh[0][tid + o];
      sh[1][tid] += sh[1][tid + o];
    }
    __syncthreads();
  }
  const float il = (float)(1.0 / sh[0][0]), ih = (float)(1.0 / sh[1][0]);
  for (int k = tid; k < n; k += 256) T[k] = __fsub_rn(__fmul_rn(sinc_tap(ch, k, h, n), ih), __fmul_rn(sinc_tap(cl, k, h, n), il));
}

}  // namespace

extern "C" {

int mfpa_bandpass_taps(const float* cut_lo, const float* cut_hi, const int* half, const long long* tap_off, int B, float* taps,
                       void* stream) {
  if (!cut_lo || !cut_hi || !half || !tap_off || !taps || B < 0) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  hipLaunchKernelGGL(bandpass_taps_kernel, dim3(B), dim3(256), 0, mfpa_stream(stream), cut_lo, cut_hi, half, tap_off, taps);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_rfft_plan(int N, int* radices, int* n_radices, int* lds_bytes) {
  rfft_plan p;
  if (!make_plan(N, &p)) return MFPA_EINVAL;
  if (radices)
    for (int i = 0; i < MFPA_RFFT_MAX_RADICES; ++i) radices[i] = p.radix[i];
  if (n_radices) *n_radices = p.n;
  if (lds_bytes) *lds_bytes = RFFT_LDS_BYTES;
  return MFPA_OK;
}

int mfpa_rfft_twiddles(int N, float* out) {
  rfft_plan p;
  if (!out || !make_plan(N, &p)) return MFPA_EINVAL;
  for (int q = 0; q < N; ++q) {
    const double a = 2.0 * M_PI * (double)q / (double)N;
    out[2 * q] = (float)cos(a);
    out[2 * q + 1] = (float)-sin(a);
  }
  return MFPA_OK;
}

int mfpa_colored_noise(const float* white, int B, int N, const float* f_decay, int T, const float* twiddles, float* out,
                       void* stream) {
  rfft_plan p;
  if (!white || !f_decay || !twiddles || !out || B < 0 || T < 1 || !make_plan(N, &p)) return MFPA_EINVAL;
  if ((reinterpret_cast<uintptr_t>(twiddles) & 7) != 0) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  hipLaunchKernelGGL(colored_noise_kernel, dim3(B), dim3(RFFT_THREADS), 0, mfpa_stream(stream), white, N, f_decay, T,
                     reinterpret_cast<const cf32*>(twiddles), p, out);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
