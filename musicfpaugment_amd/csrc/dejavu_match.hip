// Dejavu fingerprint store and matcher for MI355X (gfx950): the fingerprints table of PostgreSQLDatabase (INSERT ... ON
// CONFLICT DO NOTHING under UNIQUE(song_id, offset, hash), afp/dejavu/postgres_database.py:125-178, :288-295),
// CommonDatabase.return_matches (:180-229) and Dejavu.align_matches (afp/dejavu/dejavu.py:312-378).  Integer only.
//
// Table: rows [w0, w1, w2, sid, offset] int32, w0..w2 the 10-byte digest as big-endian words (bytes 8-9 in the high half of
// w2), so the unsigned word order is the byte order of the hash.  Rows are sorted by (hash, sid, offset) and unique; their
// bytes depend only on the SET of rows.  directory[b] = the first row whose leading `dirbits` hash bits are >= b
// (b = 0 .. 2^dirbits), so a lookup is two directory reads and a binary search on all 80 bits inside one bucket.
//
// store: the caller orders the rows by (hash, sid, offset) (a torch sort); three launches flag the rows that differ from
//   their predecessor, scan the per-workgroup counts and write the kept rows at their ranks; a fourth fills the directory.
//
// match: one workgroup per query, all of it in the query's slice of a global scratch buffer:
//   1. pairs   (hash, t1) pairs as 128-bit keys, bitonic-sorted: equal pairs are adjacent (the query is a set,
//              file_recognizer.py:20-27) and the pairs of one hash are contiguous (the `mapper` of return_matches);
//   2. groups  distinct pairs and distinct hashes by block scans;
//   3. lookup  the row range of each distinct hash; hits = sum over hashes of rows x query offsets;
//   4. emit    one key per (row, query offset): sid << 40 | (diff + 2^31) << 1 | first-offset flag.  The flag marks one key
//              per table row, so the flags of a song count its rows (dedup_hashes[sid]); a query whose hits exceed the
//              scratch capacity writes only -1 markers (the caller retries with a larger one);
//   5. sort    the keys; runs of equal (sid, diff) are the counts of align_matches' groupby, the first maximum of a song
//              is its smallest diff among the tied maxima;
//   6. rank    songs by that count descending, ties to the smaller sid (the stable sort of align_matches); the first K.
#include "mfpa_common.h"
#include "mfpa_sort.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk64 = 4096;        // uint64 keys per LDS sort chunk (32 KiB)
constexpr int kChunk128 = 2048;       // 128-bit pair keys per LDS sort chunk (the same 32 KiB)
constexpr long long kMaxHcap = 1ll << 26;
constexpr int kMaxCap = 1 << 24;

struct Key128 {
  unsigned long long hi, lo;
};
__device__ __forceinline__ bool operator>(const Key128& a, const Key128& b) {
  return a.hi > b.hi || (a.hi == b.hi && a.lo > b.lo);
}

__device__ __forceinline__ void digest_words(const uint8_t* d, uint32_t w[3]) {
  w[0] = ((uint32_t)d[0] << 24) | ((uint32_t)d[1] << 16) | ((uint32_t)d[2] << 8) | d[3];
  w[1] = ((uint32_t)d[4] << 24) | ((uint32_t)d[5] << 16) | ((uint32_t)d[6] << 8) | d[7];
  w[2] = ((uint32_t)d[8] << 24) | ((uint32_t)d[9] << 16);
}

// -------------------------------------------------------------------------------------------------------------- store
struct StoreIn {
  const uint8_t* dig;
  const int32_t* sid;
  const int32_t* off;
  const int64_t* order;
  long long n;
};

__device__ __forceinline__ int row_is_new(const StoreIn& in, long long j) {
  if (j >= in.n) return 0;
  if (j == 0) return 1;
  const long long a = in.order[j], b = in.order[j - 1];
  if (in.sid[a] != in.sid[b] || in.off[a] != in.off[b]) return 1;
  for (int k = 0; k < 10; ++k)
    if (in.dig[10 * a + k] != in.dig[10 * b + k]) return 1;
  return 0;
}

__global__ __launch_bounds__(kBlock) void store_count_kernel(StoreIn in, int32_t* __restrict__ blk) {
  __shared__ int sh[kBlock];
  const int f = row_is_new(in, (long long)blockIdx.x * kBlock + threadIdx.x);
  int tot;
  mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
  if (threadIdx.x == 0) blk[blockIdx.x] = tot;
}

// One workgroup: exclusive scan of the per-workgroup counts in place; *n_rows = the number of unique rows.
__global__ __launch_bounds__(kBlock) void store_scan_kernel(int32_t* __restrict__ blk, int nblk, int32_t* __restrict__ n_rows) {
  __shared__ int sh[kBlock];
  int carry = 0;
  for (int base = 0; base < nblk; base += kBlock) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? blk[i] : 0;
    int tot;
    const int ex = mfpa_sort::block_excl_scan<kBlock>(v, sh, &tot);
    if (i < nblk) blk[i] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) *n_rows = carry;
}

__global__ __launch_bounds__(kBlock) void store_place_kernel(StoreIn in, const int32_t* __restrict__ blk,
                                                              int32_t* __restrict__ table) {
  __shared__ int sh[kBlock];
  const long long j = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int f = row_is_new(in, j);
  int tot;
  const int ex = mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
  if (!f) return;
  const long long a = in.order[j];
  uint32_t w[3];
  digest_words(in.dig + 10 * a, w);
  int32_t* row = table + 5ll * (blk[blockIdx.x] + ex);
  row[0] = (int32_t)w[0];
  row[1] = (int32_t)w[1];
  row[2] = (int32_t)w[2];
  row[3] = in.sid[a];
  row[4] = in.off[a];
}

__global__ __launch_bounds__(kBlock) void store_dir_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ n_rows,
                                                            int dirbits, int32_t* __restrict__ dir) {
  const long long b = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (b > (1ll << dirbits)) return;
  int lo = 0, hi = *n_rows;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((long long)((uint32_t)table[5ll * mid] >> (32 - dirbits)) < b)
      lo = mid + 1;
    else
      hi = mid;
  }
  dir[b] = lo;
}

// -------------------------------------------------------------------------------------------------------------- lookup
__device__ __forceinline__ bool row_less(const int32_t* r, const uint32_t w[3]) {
  const uint32_t a0 = (uint32_t)r[0], a1 = (uint32_t)r[1], a2 = (uint32_t)r[2];
  return a0 < w[0] || (a0 == w[0] && (a1 < w[1] || (a1 == w[1] && a2 < w[2])));
}
__device__ __forceinline__ bool row_greater(const int32_t* r, const uint32_t w[3]) {
  const uint32_t a0 = (uint32_t)r[0], a1 = (uint32_t)r[1], a2 = (uint32_t)r[2];
  return a0 > w[0] || (a0 == w[0] && (a1 > w[1] || (a1 == w[1] && a2 > w[2])));
}

// Rows [*first, *first + *count) of the table carry the hash w (SELECT ... WHERE hash IN (...), postgres_database.py:212-219).
__device__ __forceinline__ void lookup_range(const int32_t* table, const int32_t* dir, int dirbits, const uint32_t w[3],
                                             int* first, int* count) {
  const uint32_t bkt = w[0] >> (32 - dirbits);
  int lo = dir[bkt], hi = dir[bkt + 1];
  const int end = hi;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (row_less(table + 5ll * mid, w))
      lo = mid + 1;
    else
      hi = mid;
  }
  const int f = lo;
  hi = end;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (row_greater(table + 5ll * mid, w))
      hi = mid;
    else
      lo = mid + 1;
  }
  *first = f;
  *count = lo - f;
}

__global__ __launch_bounds__(kBlock) void lookup_kernel(const int32_t* __restrict__ table, const int32_t* __restrict__ dir,
                                                        int dirbits, const uint8_t* __restrict__ dig, int n,
                                                        int32_t* __restrict__ ranges) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w[3];
  digest_words(dig + 10ll * i, w);
  int f, c;
  lookup_range(table, dir, dirbits, w, &f, &c);
  ranges[2 * i] = f;
  ranges[2 * i + 1] = f + c;
}

// -------------------------------------------------------------------------------------------------------------- match
struct MatchArgs {
  const int32_t* table;
  const int32_t* dir;
  int dirbits;
  const uint8_t* dig;
  const int32_t* t1;
  const int32_t* nq;
  int cap;
  long long p2, hcap, per_query;
  unsigned char* scratch;
  int K;
  int32_t* out;
  int32_t* info;
};

__device__ __forceinline__ unsigned long long pair_hash_lo(const Key128& k) { return k.lo >> 32; }
__device__ __forceinline__ bool same_hash(const Key128& a, const Key128& b) {
  return a.hi == b.hi && pair_hash_lo(a) == pair_hash_lo(b);
}
__device__ __forceinline__ int key_sid(unsigned long long k) { return (int)(k >> 40); }
__device__ __forceinline__ int key_diff(unsigned long long k) {
  return (int)((long long)((k >> 1) & 0xFFFFFFFFull) - 0x80000000ll);
}

__global__ __launch_bounds__(kBlock) void match_kernel(MatchArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long P2 = a.p2, hcap = a.hcap;
  unsigned char* base = a.scratch + (size_t)b * (size_t)a.per_query;
  Key128* pk = reinterpret_cast<Key128*>(base);                        // [P2] sorted (hash, t1) pairs
  long long* gofs = reinterpret_cast<long long*>(pk + P2);             // [P2 + 1] first hit of each hash group
  int32_t* dpos = reinterpret_cast<int32_t*>(gofs + P2 + 1);           // [P2] sorted index of each distinct pair
  int32_t* gs = dpos + P2;                                             // [P2 + 1] first distinct pair of each hash group
  int32_t* glo = gs + P2 + 1;                                          // [P2] first table row of the group's hash
  int32_t* gn = glo + P2;                                              // [P2] table rows of the group's hash
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(base + 48 * P2 + 16);   // [hcap] (sid, diff, flag) keys
  int32_t* rstart = reinterpret_cast<int32_t*>(keys + hcap);           // [hcap + 1] first key of each (sid, diff) run
  int32_t* sstart = rstart + hcap + 1;                                 // [hcap + 1] first run of each song
  int32_t* sbest = sstart + hcap + 1;                                  // [hcap] per song: count of its best diff
  int32_t* sdiff = sbest + hcap;                                       //        its best diff
  int32_t* shm = sdiff + hcap;                                         //        table rows matched (dedup_hashes)

  __shared__ unsigned long long sk[kChunk64];
  __shared__ int sh[kBlock];
  __shared__ long long sh64[kBlock];
  __shared__ int rc[kBlock], rsid[kBlock], ridx[kBlock];

  int32_t* info = a.info + (size_t)b * 4;
  int32_t* out = a.out + (size_t)b * a.K * 4;

  // ---- 1. pairs
  const int n = min(max(a.nq[b], 0), a.cap);
  long long P = 1;
  while (P < n) P <<= 1;
  const uint8_t* D = a.dig + (size_t)b * a.cap * 10;
  const int32_t* T1 = a.t1 + (size_t)b * a.cap;
  for (long long i = tid; i < P; i += kBlock) {
    Key128 k;
    if (i < n) {
      uint32_t w[3];
      digest_words(D + 10 * i, w);
      k.hi = ((unsigned long long)w[0] << 32) | w[1];
      k.lo = ((unsigned long long)(w[2] >> 16) << 32) | (uint32_t)T1[i];
    } else {
      k.hi = ~0ull;
      k.lo = ~0ull;
    }
    pk[i] = k;
  }
  __syncthreads();
  if (n > 1) mfpa_sort::sort_keys<kBlock, kChunk128>(pk, P, reinterpret_cast<Key128*>(sk));

  // ---- 2. distinct pairs, then distinct hashes
  int Q = 0;
  for (int base_i = 0; base_i < n; base_i += kBlock) {
    const int i = base_i + tid;
    const int f = i < n && (i == 0 || pk[i].hi != pk[i - 1].hi || pk[i].lo != pk[i - 1].lo);
    int tot;
    const int ex = mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
    if (f) dpos[Q + ex] = i;
    Q += tot;
  }
  __syncthreads();
  int G = 0;
  for (int base_q = 0; base_q < Q; base_q += kBlock) {
    const int q = base_q + tid;
    const int f = q < Q && (q == 0 || !same_hash(pk[dpos[q]], pk[dpos[q - 1]]));
    int tot;
    const int ex = mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
    if (f) gs[G + ex] = q;
    G += tot;
  }
  if (tid == 0) gs[G] = Q;
  __syncthreads();

  // ---- 3. lookup; gofs = exclusive prefix of rows x offsets over the groups
  long long H = 0;
  for (int base_g = 0; base_g < G; base_g += kBlock) {
    const int g = base_g + tid;
    long long hits = 0;
    if (g < G) {
      const Key128 k = pk[dpos[gs[g]]];
      const uint32_t w[3] = {(uint32_t)(k.hi >> 32), (uint32_t)k.hi, (uint32_t)pair_hash_lo(k) << 16};
      int f, c;
      lookup_range(a.table, a.dir, a.dirbits, w, &f, &c);
      glo[g] = f;
      gn[g] = c;
      hits = (long long)c * (gs[g + 1] - gs[g]);
    }
    long long tot;
    const long long ex = mfpa_sort::block_excl_scan<kBlock>(hits, sh64, &tot);
    if (g < G) gofs[g] = H + ex;
    H += tot;
  }
  if (tid == 0) gofs[G] = H;
  __syncthreads();
  if (H > hcap) {                                          // reported, never truncated: the caller retries with a larger hcap
    if (tid == 0) {
      info[0] = (int32_t)min(H, (long long)INT32_MAX);
      info[1] = -1;
      info[2] = -1;
      info[3] = -1;
    }
    return;
  }
  const int NH = (int)H;
  if (NH == 0) {
    if (tid == 0) {
      info[0] = 0;
      info[1] = Q;
      info[2] = 0;
      info[3] = 0;
    }
    return;
  }

  // ---- 4. emit: hit h belongs to group g (gofs[g] <= h < gofs[g + 1]), row glo[g] + l / m, query offset l % m
  for (int h = tid; h < NH; h += kBlock) {
    int lo = 0, hi = G;                                    // the last g with gofs[g] <= h
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (gofs[mid] <= h)
        lo = mid;
      else
        hi = mid;
    }
    const int g = lo, m = gs[g + 1] - gs[g];
    const int l = h - (int)gofs[g];
    const int r = glo[g] + l / m, qo = l % m;
    const int32_t* row = a.table + 5ll * r;
    const int t = (int)(uint32_t)pk[dpos[gs[g] + qo]].lo;
    const unsigned long long biased = (unsigned long long)((long long)row[4] - t + 0x80000000ll) & 0xFFFFFFFFull;
    keys[h] = ((unsigned long long)((uint32_t)row[3] & 0xFFFFFFu) << 40) | (biased << 1) | (qo == 0 ? 1ull : 0ull);
  }
  __syncthreads();

  // ---- 5. sort the keys, (sid, diff) runs, songs
  if (NH > 1) {
    long long PH = 1;
    while (PH < NH) PH <<= 1;
    for (long long i = NH + tid; i < PH; i += kBlock) keys[i] = ~0ull;
    __syncthreads();
    mfpa_sort::sort_keys<kBlock, kChunk64>(keys, PH, sk);
  }
  int R = 0;
  for (int base_i = 0; base_i < NH; base_i += kBlock) {
    const int i = base_i + tid;
    const int f = i < NH && (i == 0 || (keys[i] >> 1) != (keys[i - 1] >> 1));
    int tot;
    const int ex = mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
    if (f) rstart[R + ex] = i;
    R += tot;
  }
  if (tid == 0) rstart[R] = NH;
  __syncthreads();
  int S = 0;
  for (int base_r = 0; base_r < R; base_r += kBlock) {
    const int r = base_r + tid;
    const int f = r < R && (r == 0 || key_sid(keys[rstart[r]]) != key_sid(keys[rstart[r - 1]]));
    int tot;
    const int ex = mfpa_sort::block_excl_scan<kBlock>(f, sh, &tot);
    if (f) sstart[S + ex] = r;
    S += tot;
  }
  if (tid == 0) sstart[S] = R;
  __syncthreads();
  // per song: the first maximum over its runs in diff order (dejavu.py:338-345), and its flagged keys = rows matched
  for (int s = tid; s < S; s += kBlock) {
    int best = 0, bdiff = 0, rows = 0;
    for (int r = sstart[s]; r < sstart[s + 1]; ++r) {
      const int rs = rstart[r], re = rstart[r + 1];
      if (re - rs > best) {
        best = re - rs;
        bdiff = key_diff(keys[rs]);
      }
      int lo = rs, hi = re;                                // the run's flag-0 keys sort before its flag-1 keys
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] & 1ull)
          hi = mid;
        else
          lo = mid + 1;
      }
      rows += re - lo;
    }
    sbest[s] = best;
    sdiff[s] = bdiff;
    shm[s] = rows;
  }
  __syncthreads();

  // ---- 6. the first K songs by count descending, ties to the smaller sid: K rounds of a block arg-max
  const int W = min(a.K, S);
  int pc = INT32_MAX, psid = -1;                           // previous pick; the next one comes strictly after it
  for (int c = 0; c < W; ++c) {
    int bc = -1, bsid = INT32_MAX, bs = -1;
    for (int s = tid; s < S; s += kBlock) {
      const int cs = sbest[s], sid = key_sid(keys[rstart[sstart[s]]]);
      const bool after_prev = cs < pc || (cs == pc && sid > psid);
      if (after_prev && (cs > bc || (cs == bc && sid < bsid))) {
        bc = cs;
        bsid = sid;
        bs = s;
      }
    }
    rc[tid] = bc;
    rsid[tid] = bsid;
    ridx[tid] = bs;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const int c2 = rc[tid + o], s2 = rsid[tid + o];
        if (c2 > rc[tid] || (c2 == rc[tid] && s2 < rsid[tid])) {
          rc[tid] = c2;
          rsid[tid] = s2;
          ridx[tid] = ridx[tid + o];
        }
      }
      __syncthreads();
    }
    pc = rc[0];
    psid = rsid[0];
    if (tid == 0) {
      const int s = ridx[0];
      int32_t* o = out + (size_t)c * 4;
      o[0] = psid;
      o[1] = sdiff[s];
      o[2] = sbest[s];
      o[3] = shm[s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    info[0] = NH;
    info[1] = Q;
    info[2] = W;
    info[3] = S;
  }
}

bool valid_hcap(long long hcap) { return hcap >= 64 && hcap <= kMaxHcap && (hcap & (hcap - 1)) == 0; }

long long pair_pow2(int cap) {
  long long p = 1;
  while (p < cap) p <<= 1;
  return p;
}

}  // namespace

extern "C" int mfpa_dejavu_store(const uint8_t* digests, const int32_t* sids, const int32_t* offsets, const int64_t* order,
                                 long long n, int dirbits, int32_t* work, int32_t* table, int32_t* n_rows, int32_t* directory,
                                 void* stream) {
  if (n < 0 || n > INT32_MAX - kBlock || dirbits < 1 || dirbits > 24) return MFPA_EINVAL;
  if (!work || !table || !n_rows || !directory) return MFPA_EINVAL;
  if (n > 0 && (!digests || !sids || !offsets || !order)) return MFPA_EINVAL;
  const int nblk = (int)((n + kBlock - 1) / kBlock);
  const StoreIn in{digests, sids, offsets, order, n};
  hipStream_t s = mfpa_stream(stream);
  if (nblk > 0) {
    hipLaunchKernelGGL(store_count_kernel, dim3(nblk), dim3(kBlock), 0, s, in, work);
    MFPA_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(store_scan_kernel, dim3(1), dim3(kBlock), 0, s, work, nblk, n_rows);
  MFPA_CHECK_LAUNCH();
  if (nblk > 0) {
    hipLaunchKernelGGL(store_place_kernel, dim3(nblk), dim3(kBlock), 0, s, in, (const int32_t*)work, table);
    MFPA_CHECK_LAUNCH();
  }
  const long long nd = (1ll << dirbits) + 1;
  hipLaunchKernelGGL(store_dir_kernel, dim3((unsigned)((nd + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, (const int32_t*)table,
                     (const int32_t*)n_rows, dirbits, directory);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

extern "C" int mfpa_dejavu_lookup(const int32_t* table, const int32_t* directory, int dirbits, const uint8_t* digests, int n,
                                  int32_t* ranges, void* stream) {
  if (n < 0 || dirbits < 1 || dirbits > 24) return MFPA_EINVAL;
  if (n == 0) return MFPA_OK;
  if (!table || !directory || !digests || !ranges) return MFPA_EINVAL;
  hipLaunchKernelGGL(lookup_kernel, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, mfpa_stream(stream), table, directory,
                     dirbits, digests, n, ranges);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

extern "C" int mfpa_dejavu_match_scratch_bytes(int cap, long long hcap, long long* bytes) {
  if (!bytes || cap < 0 || cap > kMaxCap || !valid_hcap(hcap)) return MFPA_EINVAL;
  *bytes = 48 * pair_pow2(cap) + 16 + 32 * hcap;
  return MFPA_OK;
}

extern "C" int mfpa_dejavu_match(const int32_t* table, const int32_t* directory, int dirbits, const uint8_t* digests,
                                 const int32_t* t1, const int32_t* nq, int B, int cap, long long hcap, void* scratch, int K,
                                 int32_t* out, int32_t* info, void* stream) {
  if (B < 0 || cap < 0 || cap > kMaxCap || dirbits < 1 || dirbits > 24 || K < 1 || !valid_hcap(hcap)) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!table || !directory || !digests || !t1 || !nq || !scratch || !out || !info) return MFPA_EINVAL;
  MatchArgs a;
  a.table = table;
  a.dir = directory;
  a.dirbits = dirbits;
  a.dig = digests;
  a.t1 = t1;
  a.nq = nq;
  a.cap = cap;
  a.p2 = pair_pow2(cap);
  a.hcap = hcap;
  a.per_query = 48 * a.p2 + 16 + 32 * hcap;
  a.scratch = static_cast<unsigned char*>(scratch);
  a.K = K;
  a.out = out;
  a.info = info;
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(kBlock), 0, mfpa_stream(stream), a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
