// Workgroup-wide scan and bitonic sort helpers shared by the matchers (match.hip, dejavu_match.hip).
// Every helper is called by all threads of one workgroup of BLOCK threads and ends on a barrier.
#pragma once
#include <hip/hip_runtime.h>

namespace mfpa_sort {

// Block-wide exclusive scan of one value per thread (int or long long); *total gets the sum.  sh holds BLOCK values.
template <int BLOCK, typename T>
__device__ __forceinline__ T block_excl_scan(T v, T* sh, T* total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int off = 1; off < BLOCK; off <<= 1) {
    const T x = tid >= off ? sh[tid - off] : T(0);
    __syncthreads();
    sh[tid] += x;
    __syncthreads();
  }
  const T incl = sh[tid];
  *total = sh[BLOCK - 1];
  __syncthreads();
  return incl - v;
}

// Bitonic compare-exchange passes j = jstart .. 1 of stage k on s[0, len), global index of s[0] = gbase.
// K needs a strict `>`; equal keys are never exchanged.
template <int BLOCK, typename K>
__device__ __forceinline__ void lds_bitonic(K* s, int len, long long gbase, long long k, int jstart) {
  for (int j = jstart; j > 0; j >>= 1) {
    for (int i = threadIdx.x; i < len; i += BLOCK) {
      const int l = i ^ j;
      if (l > i) {
        const bool asc = ((gbase + i) & k) == 0;
        const K a = s[i], b = s[l];
        if ((a > b) == asc) {
          s[i] = b;
          s[l] = a;
        }
      }
    }
    __syncthreads();
  }
}

// Ascending sort of keys[0, P), P a power of two, in global memory: CHUNK-key pieces in the LDS buffer sk, global passes
// only for strides >= CHUNK.
template <int BLOCK, int CHUNK, typename K>
__device__ __forceinline__ void sort_keys(K* keys, long long P, K* sk) {
  const int tid = threadIdx.x;
  if (P <= CHUNK) {
    for (int i = tid; i < P; i += BLOCK) sk[i] = keys[i];
    __syncthreads();
    for (long long k = 2; k <= P; k <<= 1) lds_bitonic<BLOCK>(sk, (int)P, 0, k, (int)(k >> 1));
    for (int i = tid; i < P; i += BLOCK) keys[i] = sk[i];
    __syncthreads();
    return;
  }
  for (long long c = 0; c < P; c += CHUNK) {
    for (int i = tid; i < CHUNK; i += BLOCK) sk[i] = keys[c + i];
    __syncthreads();
    for (long long k = 2; k <= CHUNK; k <<= 1) lds_bitonic<BLOCK>(sk, CHUNK, c, k, (int)(k >> 1));
    for (int i = tid; i < CHUNK; i += BLOCK) keys[c + i] = sk[i];
    __syncthreads();
  }
  for (long long k = 2 * CHUNK; k <= P; k <<= 1) {
    for (long long j = k >> 1; j >= CHUNK; j >>= 1) {
      for (long long i = tid; i < P; i += BLOCK) {
        const long long l = i ^ j;
        if (l > i) {
          const bool asc = (i & k) == 0;
          const K a = keys[i], b = keys[l];
          if ((a > b) == asc) {
            keys[i] = b;
            keys[l] = a;
          }
        }
      }
      __syncthreads();
    }
    for (long long c = 0; c < P; c += CHUNK) {
      for (int i = tid; i < CHUNK; i += BLOCK) sk[i] = keys[c + i];
      __syncthreads();
      lds_bitonic<BLOCK>(sk, CHUNK, c, k, CHUNK >> 1);
      for (int i = tid; i < CHUNK; i += BLOCK) keys[c + i] = sk[i];
      __syncthreads();
    }
  }
}

}  // namespace mfpa_sort
