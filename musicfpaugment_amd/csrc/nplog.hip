// Element-wise numpy float32 logarithm for MI355X (gfx950): y[i] = np.log(x[i]) as numpy's SIMD float32 kernel returns it, bit for
// bit (mfpa_nplog.h).  The bit-level test surface of that function, and an entry point for callers that post-process float32
// spectrograms themselves (the reference takes np.log of the UNet's float32 output: afp/audfprint/peak_extractor.py:265-276,
// afp/dejavu/fingerprint.py:70-79).  Memory-bound: 16-byte loads and stores, the last n % 4 elements one by one.
// Compiled with -ffp-contract=off like the pickers (the function also switches contraction off itself).
#include "mfpa_common.h"
#include "mfpa_nplog.h"

namespace {

constexpr int NPLOG_THREADS = 256;

// VEC: x and y are both 16-byte aligned (the launcher checks); otherwise every element goes through the scalar loop
template <bool VEC>
__global__ __launch_bounds__(NPLOG_THREADS) void nplog_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
  const long long tid = (long long)blockIdx.x * NPLOG_THREADS + threadIdx.x;
  const long long stride = (long long)gridDim.x * NPLOG_THREADS;
  const long long nvec = VEC ? n / 4 : 0;
  if (VEC) {
    const float4* xv = reinterpret_cast<const float4*>(x);
    float4* yv = reinterpret_cast<float4*>(y);
    for (long long i = tid; i < nvec; i += stride) {
      const float4 v = xv[i];
      yv[i] = float4{mfpa_nplogf(v.x), mfpa_nplogf(v.y), mfpa_nplogf(v.z), mfpa_nplogf(v.w)};
    }
  }
  for (long long i = 4 * nvec + tid; i < n; i += stride) y[i] = mfpa_nplogf(x[i]);
}

}  // namespace

extern "C" {

int mfpa_nplog_f32(const float* x, float* y, long long n, void* stream) {
  if (n == 0) return MFPA_OK;
  if (!x || !y || n < 0) return MFPA_EINVAL;
  {  // the kernel's pointers are __restrict__: the two ranges must not overlap (in place included)
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), ya = reinterpret_cast<uintptr_t>(y), bytes = (uintptr_t)n * sizeof(float);
    if (xa < ya + bytes && ya < xa + bytes) return MFPA_EINVAL;
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  const long long work = vec ? (n + 3) / 4 : n;
  const long long blocks = (work + NPLOG_THREADS - 1) / NPLOG_THREADS;
  const dim3 grid((unsigned)(blocks > 4096 ? 4096 : blocks));
  if (vec) hipLaunchKernelGGL(nplog_kernel<true>, grid, dim3(NPLOG_THREADS), 0, mfpa_stream(stream), x, y, n);
  else hipLaunchKernelGGL(nplog_kernel<false>, grid, dim3(NPLOG_THREADS), 0, mfpa_stream(stream), x, y, n);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
