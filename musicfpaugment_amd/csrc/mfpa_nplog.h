// numpy's float32 natural logarithm, restated: the value np.log returns for a float32 argument where numpy dispatches its SIMD kernel
// (AVX512F, or AVX2 + FMA3; numpy/_core/src/umath/loops_exponent_log.dispatch.c.src).  The reference takes np.log of a FLOAT32 array on
// the denoised branch (afp/audfprint/peak_extractor.py:265-276, afp/dejavu/fingerprint.py:70-79), and that kernel is not correctly
// rounded: it differs from the float64 log rounded once to float32 (mfpa_log_t, the pickers' default) on 22 % of the float32 arguments in
// (1e-6, 1].  With this function the denoised branch's log values are the reference's bit for bit.
//   (m, e) = frexp(x), m in [0.5, 1); m <= sqrt(1/2): m = 2m, e = e - 1;  t = m - 1
//   log x = e * ln2 + P(t) / Q(t), P and Q of degree 5 evaluated by Horner with fused multiply-adds, one correctly rounded division,
//   one last fused multiply-add; every operation and every constant in float32.
// tools/make_nplog_golden.py --exhaustive compares it with np.log on every non-negative float32 (0 differences, NOTES.md);
// tests/test_nplog_host.py compiles this very header with gcc (define MFPA_NPLOG_HOST before including, build with -ffp-contract=off).
// frexp is done on the bit pattern and a denormal is normalised with a leading-zero count, so the result does not depend on the
// denormal mode; nothing but the marked fused multiply-adds may be contracted.
#pragma once
#ifdef MFPA_NPLOG_HOST
#include <math.h>
#define MFPA_NPLOG_FN static inline
#define MFPA_NPLOG_DIV(a, b) ((a) / (b))
#else
#include <hip/hip_runtime.h>
#define MFPA_NPLOG_FN __device__ __forceinline__
#define MFPA_NPLOG_DIV(a, b) __fdiv_rn((a), (b))
#endif

MFPA_NPLOG_FN float mfpa_nplogf(float x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  unsigned int ix;
  __builtin_memcpy(&ix, &x, 4);
  if (ix - 0x00800000u >= 0x7f000000u) {                    // zero, denormal, inf, nan or negative
    if (x != x) return x + x;                               // nan (quiet)
    if ((ix << 1) == 0u) return -__builtin_inff();          // +-0
    if (ix >> 31) return __builtin_nanf("");                // negative
    if (ix == 0x7f800000u) return x;                        // +inf
  }
  unsigned int mant = ix & 0x007fffffu;
  int e = (int)(ix >> 23) - 126;
  if ((ix >> 23) == 0u) {                                   // denormal: mant != 0, leading one moved to bit 23
    const int shift = __builtin_clz(mant) - 8;
    mant = (mant << shift) & 0x007fffffu;
    e = -125 - shift;
  }
  const unsigned int im = mant | 0x3f000000u;
  float m;
  __builtin_memcpy(&m, &im, 4);
  if (m <= 0.70710678118654752440f) {
    m += m;
    e -= 1;
  }
  const float t = m - 1.0f;
  float num = 2.589979117907922693523e-02f;
  num = __builtin_fmaf(num, t, 3.808837741388407920751e-01f);
  num = __builtin_fmaf(num, t, 1.480000633576506585156e+00f);
  num = __builtin_fmaf(num, t, 2.112677543073053063722e+00f);
  num = __builtin_fmaf(num, t, 9.999999999999998702752e-01f);
  num = __builtin_fmaf(num, t, 0.0f);
  float den = 5.875095403124574342950e-03f;
  den = __builtin_fmaf(den, t, 1.546476374983906719538e-01f);
  den = __builtin_fmaf(den, t, 9.864942958519418960339e-01f);
  den = __builtin_fmaf(den, t, 2.453006071784736363091e+00f);
  den = __builtin_fmaf(den, t, 2.612677543073109236779e+00f);
  den = __builtin_fmaf(den, t, 1.0f);
  const float p = MFPA_NPLOG_DIV(num, den);
  return __builtin_fmaf((float)e, 0.693147180559945309417232121458176568f, p);
}
