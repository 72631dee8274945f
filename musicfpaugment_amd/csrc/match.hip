// Audfprint hash table and matcher for MI355X (gfx950): HashTable.store / get_hits and
// Matcher._best_count_ids / _approx_match_counts / the final sort of match_hashes
// (afp/audfprint/hash_table.py:72-113, :222-247; afp/audfprint/audfprint_match.py:105-137, :236-320, :322-346).
// Integer arithmetic throughout except the weighted count rawcount / hashesperid, one float64 division as in numpy.
//
// store: one thread per (bucket) segment of a batch of entries already grouped by bucket in arrival order (a stable sort
//   done by the caller).  The thread walks its segment in arrival order, so in-bucket slots are arrival ranks exactly as
//   the reference assigns them; a full bucket takes the reservoir step (slot uniform over 0..count, stored only when
//   slot < depth) with the slot drawn from a counter-based generator keyed by (seed, bucket, arrival index in the bucket)
//   instead of Python's global `random` -- DESIGN.md §3.8.
//
// match: one workgroup per query, all of it in the query's slice of a global scratch buffer:
//   1. gather  every table entry of every query hash -> 64-bit key (id << 32 | biased dt); the count is reported, and a
//              query whose hits exceed the scratch capacity writes nothing else (the caller retries with a larger one);
//   2. sort    bitonic: LDS chunks of 4096 keys, global passes only for strides >= one chunk;
//   3. runs    run lengths of equal keys = the sparse dt histogram of each id (rcnt), run lengths of equal ids = rawcounts;
//   4. rank    ids ordered by rawcount / hashesperid (float64) descending, ties larger id first (numpy's argsort(...)[::-1]
//              on a stable order); the first min(#(rawcount > threshcount), search_depth) are the candidates;
//   5. modes   one wave per candidate: locmax on the sparse histogram (implicit zeros between runs), repeated first-index
//              argmax, windowed sum of the unfiltered counts, zeroing of the window, at most max_alignments + 1 modes;
//   6. order   rows by filtered count descending, ties by (candidate rank, mode order); the first K are written.
//
// match_ex (exact_count / find_time_range / hashesfor, audfprint_match.py:131-233, :293-296, :343-349) runs the same body
// with three more regions of scratch per query and these steps after 4:
//   4x. regather  the query's hits once more, keeping those of the <= 256 candidates, keyed
//                 candidate rank (8 bits) | biased dt (32) | query row (15): sorted, every window [mode - w, mode + w] of a
//                 candidate is one contiguous key range;
//   5x. modes     exact: every run that is a local maximum with rcnt >= threshcount, dt ascending (find_modes), no cap;
//   5w. windows   the workgroup takes the modes one by one: the window's packed values query_time + (hash << timebits)
//                 sorted in `wbuf`, distinct neighbours counted (_unique_match_hashes); the window's query times sorted, the
//                 two order statistics read (_calculate_time_ranges); exact rows with count < threshcount dropped;
//   7.  hashes    the sorted distinct packed values of result row `hashesfor`, unpacked, to the caller's buffer.
#include "mfpa_common.h"
#include "mfpa_sort.h"

namespace {

constexpr int kBlock = 256;
constexpr int kChunk = 4096;          // uint64 keys per LDS sort chunk (32 KiB)
constexpr int kMaxCand = 256;         // search_depth limit (LDS candidate arrays)

__device__ __forceinline__ unsigned long long splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__global__ __launch_bounds__(kBlock) void store_kernel(const int32_t* __restrict__ rows, const int32_t* __restrict__ ids,
                                                        const int64_t* __restrict__ order, const int32_t* __restrict__ seg,
                                                        int n_seg, uint32_t hmask, int timebits, int depth,
                                                        unsigned long long seed, uint32_t* __restrict__ table,
                                                        int32_t* __restrict__ counts) {
  const int s = blockIdx.x * kBlock + threadIdx.x;
  if (s >= n_seg) return;
  const int lo = seg[s], hi = seg[s + 1];
  if (lo >= hi) return;
  const uint32_t bucket = (uint32_t)rows[2 * order[lo] + 1] & hmask;
  const uint32_t tmask = (1u << timebits) - 1u;
  uint32_t* row = table + (size_t)bucket * depth;
  int c = counts[bucket];
  for (int j = lo; j < hi; ++j, ++c) {
    const long long i = order[j];
    const uint32_t val = ((uint32_t)(ids[i] + 1) << timebits) | ((uint32_t)rows[2 * i] & tmask);
    if (c < depth) {
      row[c] = val;
    } else {
      // hash_table.py:99-103: slot = random.randint(0, count); stored only if slot < depth
      const unsigned long long r = splitmix64(seed ^ splitmix64(((unsigned long long)bucket << 32) | (uint32_t)c));
      const unsigned long long slot = __umul64hi(r, (unsigned long long)c + 1ull);
      if (slot < (unsigned long long)depth) row[slot] = val;
    }
  }
  counts[bucket] = c;
}

__device__ __forceinline__ int block_excl_scan(int v, int* sh, int* total) {
  return mfpa_sort::block_excl_scan<kBlock>(v, sh, total);
}

__device__ __forceinline__ void sort_keys(unsigned long long* keys, long long P, unsigned long long* sk) {
  mfpa_sort::sort_keys<kBlock, kChunk>(keys, P, sk);
}

__device__ __forceinline__ int key_id(unsigned long long k) { return (int)(uint32_t)(k >> 32); }
__device__ __forceinline__ int key_dt(unsigned long long k) { return (int)((uint32_t)k ^ 0x80000000u); }

struct MatchArgs {
  const uint32_t* table;
  const int32_t* counts;
  const int32_t* hashesperid;
  int n_ids, timebits, depth;
  uint32_t hmask;
  const int32_t* hashes;
  const int32_t* nq;
  int cap, thresh, search_depth, window, max_modes;
  long long hcap;
  unsigned char* scratch;
  int K;
  int32_t* out;
  int32_t* info;
};

// The extended path's arguments (mfpa_audfprint_match_ex); the default kernel never reads them.
struct MatchExArgs {
  int flags;                  // kExact | kTimeRange
  double quantile;            // time_quantile in [0, 1)
  uint32_t p2mask;            // bit k: numpy's ceil(log(2^k) / log(2)) is k + 1
  int hashesfor, hf_cap;      // result row whose matching hashes are wanted (-1: none), rows of hf_out per query
  int32_t* hf_out;
  int32_t* hf_count;
};
constexpr int kExact = 1, kTimeRange = 2;
constexpr int kBytesPerHit = 32, kBytesPerHitEx = 56;   // scratch per unit of hcap
constexpr int kRowBits = 15;                            // query row in the regathered key: cap <= 2^15

// encpowerof2 (audfprint_match.py:17-21) of v >= 1: exact for every v that is no power of two; for 2^k numpy's float64
// quotient decides, and the host hands its 32 answers over in p2mask.
__device__ __forceinline__ int encpowerof2(int v, uint32_t p2mask) {
  if ((v & (v - 1)) == 0) {
    const int k = __ffs(v) - 1;
    return k + (int)((p2mask >> k) & 1u);
  }
  return 32 - __clz(v);
}

// First index in the sorted keys[0, n) whose key is >= k.
__device__ __forceinline__ int lower_bound(const unsigned long long* keys, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The regathered hits of one query (phase 4x) and what turns one of their windows into sorted values.
struct Windows {
  const unsigned long long* keys2;   // sorted: candidate rank | biased dt | query row
  int n2, window;
  unsigned long long* wbuf;
  const int32_t* Q;                  // the query's (time, hash) rows
  uint32_t hmask;
  int tb;                            // timebits of the packing
};

// The window [dtm - window, dtm + window] of candidate c as a range of keys2: returns its length, *lo its start.
__device__ __forceinline__ int window_range(const Windows& w, int c, int dtm, int* lo) {
  const unsigned long long base = (unsigned long long)c << (32 + kRowBits);
  long long bl = (long long)dtm - w.window + 0x80000000ll, bh = (long long)dtm + w.window + 1 + 0x80000000ll;
  if (bl < 0) bl = 0;
  if (bh > 0x100000000ll) bh = 0x100000000ll;
  *lo = lower_bound(w.keys2, w.n2, base + ((unsigned long long)bl << kRowBits));
  return lower_bound(w.keys2, w.n2, base + ((unsigned long long)bh << kRowBits)) - *lo;
}

// wbuf[0, nw) = the window's values, ascending: the packed query_time + (hash << timebits) of _unique_match_hashes, or
// the query times alone, as int64 with the sign bit flipped (unsigned order = numpy's signed order; a negative query time
// packs as it does there).  Called by the whole workgroup; ends on a barrier.
constexpr unsigned long long kSignBit = 1ull << 63;
__device__ __forceinline__ long long window_value(unsigned long long v) { return (long long)(v ^ kSignBit); }
__device__ __forceinline__ void sort_window(const Windows& w, int lo, int nw, bool packed, unsigned long long* sk) {
  int P = 1;
  while (P < nw) P <<= 1;
  for (int j = threadIdx.x; j < P; j += kBlock) {
    unsigned long long v = ~0ull;
    if (j < nw) {
      const int i = (int)(w.keys2[lo + j] & ((1u << kRowBits) - 1u));
      const long long t = w.Q[2 * i];
      const long long h = (uint32_t)w.Q[2 * i + 1] & w.hmask;
      v = (unsigned long long)(packed ? t + (h << w.tb) : t) ^ kSignBit;
    }
    w.wbuf[j] = v;
  }
  __syncthreads();
  if (P > 1) sort_keys(w.wbuf, (long long)P, sk);
}

template <bool EX>
__device__ __forceinline__ void match_body(const MatchArgs& a, const MatchExArgs& x) {
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long hcap = a.hcap;
  unsigned long long* keys =
      reinterpret_cast<unsigned long long*>(a.scratch + (size_t)b * (size_t)hcap * (EX ? kBytesPerHitEx : kBytesPerHit));
  unsigned long long* rkey = keys + hcap;                 // run keys
  int32_t* rcnt = reinterpret_cast<int32_t*>(rkey + hcap); // run lengths = unfiltered histogram values
  int32_t* rfilt = rcnt + hcap;                            // run start (phase 3), then the filtered histogram
  int32_t* idrun = rfilt + hcap;                           // first run of each distinct id
  int32_t* idraw = idrun + hcap;                           // rawcount of each distinct id
  double* wts = reinterpret_cast<double*>(keys);           // phase 4 (keys are dead after phase 3)
  int32_t* rows = reinterpret_cast<int32_t*>(keys);        // phase 5-6: (count, dt) pairs at the candidate's run indices
  // extended path only: the regathered candidate hits, the window being sorted, (min_time, max_time) beside `rows`
  unsigned long long* keys2 = EX ? reinterpret_cast<unsigned long long*>(idraw + hcap) : nullptr;
  unsigned long long* wbuf = keys2 + hcap;
  int32_t* mt = reinterpret_cast<int32_t*>(wbuf + hcap);

  __shared__ unsigned long long sk[kChunk];
  __shared__ int sh[kBlock];
  __shared__ double rw[kBlock];
  __shared__ int rid[kBlock], rm[kBlock];
  __shared__ int c_m[kMaxCand], c_nrow[kMaxCand], c_off[kMaxCand + 1];
  __shared__ long long s_n;
  __shared__ int x_id[EX ? kMaxCand : 1], x_sid[EX ? kMaxCand : 1], x_srank[EX ? kMaxCand : 1];   // candidate ids, and sorted by id
  __shared__ int x_n2, x_tmax, x_hf[2];

  // ---- 1. gather (hash_table.py:222-247): query hashes masked to hashbits, query times not masked
  const int n = min(max(a.nq[b], 0), a.cap);
  const int32_t* Q = a.hashes + (size_t)b * a.cap * 2;
  if (tid == 0) s_n = 0;
  __syncthreads();
  const uint32_t tmask = (1u << a.timebits) - 1u;
  for (int i = tid; i < n; i += kBlock) {
    const int t = Q[2 * i];
    const uint32_t h = (uint32_t)Q[2 * i + 1] & a.hmask;
    const int nb = min(max(a.counts[h], 0), a.depth);
    if (nb == 0) continue;
    const long long pos = (long long)atomicAdd(reinterpret_cast<unsigned long long*>(&s_n), (unsigned long long)nb);
    const uint32_t* tv = a.table + (size_t)h * a.depth;
    for (int s = 0; s < nb && pos + s < hcap; ++s) {
      const uint32_t v = tv[s];
      const int id = (int)(v >> a.timebits) - 1;
      const int dt = (int)(v & tmask) - t;
      keys[pos + s] = ((unsigned long long)(uint32_t)id << 32) | ((uint32_t)dt ^ 0x80000000u);
    }
  }
  __syncthreads();
  const long long nh = s_n;
  int32_t* info = a.info + (size_t)b * 3;
  if (nh > hcap) {                                         // reported, never truncated: the caller retries with a larger hcap
    if (tid == 0) {
      info[0] = (int32_t)min(nh, (long long)INT32_MAX);
      info[1] = -1;
      info[2] = -1;
    }
    return;
  }

  // ---- 2. sort (id, dt) keys
  if (nh > 1) {
    long long P = 1;
    while (P < nh) P <<= 1;
    for (long long i = nh + tid; i < P; i += kBlock) keys[i] = ~0ull;
    __syncthreads();
    sort_keys(keys, P, sk);
  }
  const int NH = (int)nh;

  // ---- 3. runs: sparse per-id dt histograms (np.bincount, audfprint_match.py:275) and rawcounts (:117)
  int R = 0;
  for (int base = 0; base < NH; base += kBlock) {
    const int i = base + tid;
    const int flag = i < NH && (i == 0 || keys[i] != keys[i - 1]);
    int tot;
    const int ex = block_excl_scan(flag, sh, &tot);
    if (flag) {
      rkey[R + ex] = keys[i];
      rfilt[R + ex] = i;
    }
    R += tot;
  }
  __syncthreads();
  for (int r = tid; r < R; r += kBlock) rcnt[r] = (r + 1 < R ? rfilt[r + 1] : NH) - rfilt[r];
  int M = 0;
  for (int base = 0; base < R; base += kBlock) {
    const int r = base + tid;
    const int flag = r < R && (r == 0 || key_id(rkey[r]) != key_id(rkey[r - 1]));
    int tot;
    const int ex = block_excl_scan(flag, sh, &tot);   // its barriers also order the rcnt writes above
    if (flag) idrun[M + ex] = r;
    M += tot;
  }
  __syncthreads();
  for (int m = tid; m < M; m += kBlock) {
    const int e = m + 1 < M ? idrun[m + 1] : R;
    idraw[m] = (e < R ? rfilt[e] : NH) - rfilt[idrun[m]];
  }
  __syncthreads();
  // locmax (audfprint_match.py:24-40): >= the left neighbour, > the right one; zeros between runs are implicit
  for (int r = tid; r < R; r += kBlock) {
    const int id = key_id(rkey[r]), dt = key_dt(rkey[r]), c = rcnt[r];
    const int left = (r > 0 && key_id(rkey[r - 1]) == id && key_dt(rkey[r - 1]) == dt - 1) ? rcnt[r - 1] : 0;
    const int right = (r + 1 < R && key_id(rkey[r + 1]) == id && key_dt(rkey[r + 1]) == dt + 1) ? rcnt[r + 1] : 0;
    rfilt[r] = (c >= left && c > right) ? c : 0;
  }

  // ---- 4. candidates (_best_count_ids, audfprint_match.py:105-137)
  int above = 0;
  for (int m = tid; m < M; m += kBlock) {
    const int id = key_id(rkey[idrun[m]]);
    const bool ok = id >= 0 && id < a.n_ids;
    wts[m] = ok ? (double)idraw[m] / (double)a.hashesperid[id] : -1.0;
    above += ok && idraw[m] > a.thresh;
  }
  int n_above;
  block_excl_scan(above, sh, &n_above);
  const int D = min(n_above, a.search_depth);
  double pw = INFINITY;
  int pid = INT32_MAX;                                     // previous pick: (weight, id); the next one comes strictly after it
  for (int c = 0; c < D; ++c) {
    double bw = -1.0;
    int bid = -1, bm = -1;
    for (int m = tid; m < M; m += kBlock) {
      const double w = wts[m];
      if (w < 0) continue;
      const int id = key_id(rkey[idrun[m]]);
      const bool after_prev = w < pw || (w == pw && id < pid);
      const bool better = w > bw || (w == bw && id > bid);
      if (after_prev && better) {
        bw = w;
        bid = id;
        bm = m;
      }
    }
    rw[tid] = bw;
    rid[tid] = bid;
    rm[tid] = bm;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
      if (tid < o) {
        const double w2 = rw[tid + o];
        const int id2 = rid[tid + o];
        if (w2 > rw[tid] || (w2 == rw[tid] && id2 > rid[tid])) {
          rw[tid] = w2;
          rid[tid] = id2;
          rm[tid] = rm[tid + o];
        }
      }
      __syncthreads();
    }
    pw = rw[0];
    pid = rid[0];
    if (tid == 0) c_m[c] = rm[0];
    __syncthreads();
  }

  const bool exact = EX && (x.flags & kExact), trange = EX && (x.flags & kTimeRange);
  const bool windows = exact || trange || (EX && x.hashesfor >= 0);
  int n2 = 0, tb = 1;
  if (windows) {
    // ---- 4x. the candidates' hits again, with the query row as payload
    if (tid == 0) {
      x_n2 = 0;
      x_tmax = 1;                                          // timebits = max(1, encpowerof2(max(1, largest query time with a hit)))
    }
    for (int c = tid; c < D; c += kBlock) x_id[c] = key_id(rkey[idrun[c_m[c]]]);
    __syncthreads();
    for (int c = tid; c < D; c += kBlock) {
      int pos = 0;
      for (int c2 = 0; c2 < D; ++c2) pos += x_id[c2] < x_id[c];
      x_sid[pos] = x_id[c];
      x_srank[pos] = c;
    }
    __syncthreads();
    for (int i = tid; i < n; i += kBlock) {
      const int t = Q[2 * i];
      const uint32_t h = (uint32_t)Q[2 * i + 1] & a.hmask;
      const int nb = min(max(a.counts[h], 0), a.depth);
      if (nb == 0) continue;
      atomicMax(&x_tmax, t);
      const uint32_t* tv = a.table + (size_t)h * a.depth;
      for (int s = 0; s < nb; ++s) {
        const uint32_t v = tv[s];
        const int id = (int)(v >> a.timebits) - 1;
        int lo = 0, hi = D;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if (x_sid[mid] < id) lo = mid + 1; else hi = mid;
        }
        if (lo == D || x_sid[lo] != id) continue;
        const int dt = (int)(v & tmask) - t;
        const int pos = atomicAdd(&x_n2, 1);               // at most the nh <= hcap hits of phase 1
        keys2[pos] = ((unsigned long long)x_srank[lo] << (32 + kRowBits)) |
                     ((unsigned long long)((uint32_t)dt ^ 0x80000000u) << kRowBits) | (unsigned long long)i;
      }
    }
    __syncthreads();
    n2 = x_n2;
    tb = max(1, encpowerof2(x_tmax, x.p2mask));
    if (n2 > 1) {
      long long P = 1;
      while (P < n2) P <<= 1;
      for (long long i = n2 + tid; i < P; i += kBlock) keys2[i] = ~0ull;
      __syncthreads();
      sort_keys(keys2, P, sk);
    }
  }
  const Windows w = {keys2, n2, a.window, wbuf, Q, a.hmask, tb};

  if (exact) {
    // ---- 5x. modes (find_modes, audfprint_match.py:54-68): every local maximum >= threshcount, dt ascending
    for (int c = wave; c < D; c += kBlock / 64) {
      const int m = c_m[c];
      const int s = idrun[m], e = m + 1 < M ? idrun[m + 1] : R;
      int nrow = 0;
      for (int base = s; base < e; base += 64) {
        const int r = base + lane;
        const bool ok = r < e && rfilt[r] > 0 && rcnt[r] >= a.thresh;
        const unsigned long long ball = __ballot(ok);
        if (ok) {
          const int p = s + nrow + __popcll(ball & ((1ull << lane) - 1ull));
          rows[2 * p] = 0;
          rows[2 * p + 1] = key_dt(rkey[r]);
        }
        nrow += __popcll(ball);
      }
      if (lane == 0) c_nrow[c] = nrow;
    }
  } else
  // ---- 5. modes (_approx_match_counts, audfprint_match.py:281-318), one wave per candidate
  for (int c = wave; c < D; c += kBlock / 64) {
    const int m = c_m[c];
    const int s = idrun[m], e = m + 1 < M ? idrun[m + 1] : R;
    int nrow = 0;
    for (int found = 0; found < a.max_modes; ++found) {
      int v = 0, idx = -1;
      for (int r = s + lane; r < e; r += 64) {
        const int f = rfilt[r];
        if (f > v) {
          v = f;
          idx = r;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const int v2 = __shfl_xor(v, o), i2 = __shfl_xor(idx, o);
        if (v2 > v || (v2 == v && i2 >= 0 && (idx < 0 || i2 < idx))) {
          v = v2;
          idx = i2;
        }
      }
      if (v <= a.thresh) break;                            // first-index argmax of the filtered histogram <= threshcount
      const int dtm = key_dt(rkey[idx]);
      int count = 0;
      for (int r = idx; r >= s && key_dt(rkey[r]) >= dtm - a.window; --r) {
        count += rcnt[r];
        if (((r - s) & 63) == lane) rfilt[r] = 0;          // each lane clears only the runs it scans above
      }
      for (int r = idx + 1; r < e && key_dt(rkey[r]) <= dtm + a.window; ++r) {
        count += rcnt[r];
        if (((r - s) & 63) == lane) rfilt[r] = 0;
      }
      if (lane == 0) {
        rows[2 * (s + nrow)] = count;
        rows[2 * (s + nrow) + 1] = dtm;
      }
      ++nrow;
    }
    if (lane == 0) c_nrow[c] = nrow;
  }
  __syncthreads();

  if (exact || trange) {
    // ---- 5w. the workgroup takes the modes one by one (_exact_match_counts :210-232, _calculate_time_ranges :155-181)
    for (int c = 0; c < D; ++c) {
      const int s = idrun[c_m[c]];
      for (int k = 0; k < c_nrow[c]; ++k) {
        int lo;
        const int nw = window_range(w, c, rows[2 * (s + k) + 1], &lo);
        int count = rows[2 * (s + k)];
        if (exact) {
          sort_window(w, lo, nw, true, sk);
          int u = 0;
          for (int j = tid; j < nw; j += kBlock) u += j == 0 || wbuf[j] != wbuf[j - 1];
          block_excl_scan(u, sh, &count);
        }
        int t0 = 0, t1 = 0;
        if (trange && nw > 0 && count >= (exact ? a.thresh : 0)) {
          sort_window(w, lo, nw, false, sk);
          const int i0 = min((int)((double)nw * x.quantile), nw - 1);
          const int i1 = (int)((double)nw * (1.0 - x.quantile)) - 1;      // -1 is Python's last element
          t0 = (int)window_value(wbuf[i0]);
          t1 = (int)window_value(wbuf[i1 < 0 ? nw - 1 : i1]);
        }
        __syncthreads();                                   // wbuf is read above and rewritten by the next mode
        if (tid == 0) {
          rows[2 * (s + k)] = count;
          mt[2 * (s + k)] = t0;
          mt[2 * (s + k) + 1] = t1;
        }
      }
    }
    __syncthreads();
    if (exact) {                                           // filtcount >= threshcount (:214)
      for (int c = tid; c < D; c += kBlock) {
        const int s = idrun[c_m[c]];
        int j = 0;
        for (int k = 0; k < c_nrow[c]; ++k) {
          if (rows[2 * (s + k)] < a.thresh) continue;
          rows[2 * (s + j)] = rows[2 * (s + k)];
          rows[2 * (s + j) + 1] = rows[2 * (s + k) + 1];
          mt[2 * (s + j)] = mt[2 * (s + k)];
          mt[2 * (s + j) + 1] = mt[2 * (s + k) + 1];
          ++j;
        }
        c_nrow[c] = j;
      }
      __syncthreads();
    }
  }

  // ---- 6. final order (match_hashes, audfprint_match.py:336): filtered count descending, ties (rank, mode order)
  if (tid == 0) {
    if (EX) x_hf[0] = -1;
    int o = 0;
    for (int c = 0; c < D; ++c) {
      c_off[c] = o;
      o += c_nrow[c];
    }
    c_off[D] = o;
  }
  __syncthreads();
  const int Rt = c_off[D];
  int32_t* out = a.out + (size_t)b * a.K * 7;
  for (int f = tid; f < Rt; f += kBlock) {
    int c = 0;
    while (c_off[c + 1] <= f) ++c;
    const int m = c_m[c], s = idrun[m], k = f - c_off[c];
    const int cnt = rows[2 * (s + k)];
    int pos = 0;
    for (int c2 = 0; c2 < D; ++c2) {
      const int s2 = idrun[c_m[c2]];
      for (int k2 = 0; k2 < c_nrow[c2]; ++k2) {
        const int cg = rows[2 * (s2 + k2)];
        pos += cg > cnt || (cg == cnt && c_off[c2] + k2 < f);
      }
    }
    if (pos < a.K) {
      int32_t* o = out + (size_t)pos * 7;
      o[0] = key_id(rkey[s]);
      o[1] = cnt;
      o[2] = rows[2 * (s + k) + 1];
      o[3] = idraw[m];
      o[4] = c;
      o[5] = trange ? mt[2 * (s + k)] : 0;
      o[6] = trange ? mt[2 * (s + k) + 1] : 0;
    }
    if (EX && pos == x.hashesfor) {
      x_hf[0] = c;
      x_hf[1] = rows[2 * (s + k) + 1];
    }
  }
  if (tid == 0) {
    info[0] = NH;
    info[1] = min(Rt, a.K);
    info[2] = Rt;
  }
  if (EX && x.hashesfor >= 0) {
    // ---- 7. the matching hashes of result row `hashesfor` (match_hashes :345-349, _unique_match_hashes)
    __syncthreads();
    const int c = x_hf[0];
    if (c < 0) {
      if (tid == 0) x.hf_count[b] = -1;                    // no such row
      return;
    }
    int lo;
    const int nw = window_range(w, c, x_hf[1], &lo);
    sort_window(w, lo, nw, true, sk);
    int u = 0, nu;
    for (int j = tid; j < nw; j += kBlock) u += j == 0 || wbuf[j] != wbuf[j - 1];
    block_excl_scan(u, sh, &nu);
    if (tid == 0) x.hf_count[b] = nu;                      // reported, never truncated: past hf_cap nothing is written
    if (nu > x.hf_cap) return;
    int32_t* ho = x.hf_out + (size_t)b * x.hf_cap * 2;
    const long long timemask = (1ll << tb) - 1ll;
    int U = 0;
    for (int base = 0; base < nw; base += kBlock) {
      const int j = base + tid;
      const int flag = j < nw && (j == 0 || wbuf[j] != wbuf[j - 1]);
      int tot;
      const int ex = block_excl_scan(flag, sh, &tot);
      if (flag) {
        ho[2 * (U + ex)] = (int32_t)(window_value(wbuf[j]) & timemask);
        ho[2 * (U + ex) + 1] = (int32_t)(window_value(wbuf[j]) >> tb);
      }
      U += tot;
    }
  }
}

__global__ __launch_bounds__(kBlock) void match_kernel(MatchArgs a) { match_body<false>(a, MatchExArgs{}); }

__global__ __launch_bounds__(kBlock) void match_ex_kernel(MatchArgs a, MatchExArgs x) { match_body<true>(a, x); }

bool valid_table(int hashbits, int timebits, int depth) {
  return hashbits >= 1 && hashbits <= 24 && timebits >= 1 && timebits <= 20 && depth >= 1 && depth <= 4096;
}

}  // namespace

extern "C" int mfpa_audfprint_store(const int32_t* rows, const int32_t* ids, const int64_t* order, const int32_t* seg_start,
                                    int n_seg, int hashbits, int timebits, int depth, unsigned long long seed,
                                    uint32_t* table, int32_t* counts, void* stream) {
  if (n_seg < 0 || !valid_table(hashbits, timebits, depth)) return MFPA_EINVAL;
  if (n_seg == 0) return MFPA_OK;
  if (!rows || !ids || !order || !seg_start || !table || !counts) return MFPA_EINVAL;
  hipLaunchKernelGGL(store_kernel, dim3((n_seg + kBlock - 1) / kBlock), dim3(kBlock), 0, mfpa_stream(stream), rows, ids,
                     order, seg_start, n_seg, (uint32_t)((1ull << hashbits) - 1), timebits, depth, seed, table, counts);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

namespace {

bool valid_hcap(long long hcap) { return hcap >= 64 && hcap <= (1ll << 26) && !(hcap & (hcap - 1)); }   // a power of two: the bitonic sort pads to one

// Argument checks shared by mfpa_audfprint_match and mfpa_audfprint_match_ex, all on the host before any launch.
// *launch is 0 for an empty batch.
int match_args(const uint32_t* table, const int32_t* counts, const int32_t* hashesperid, int n_ids, int hashbits, int timebits,
               int depth, const int32_t* hashes, const int32_t* nq, int B, int cap, int threshcount, int search_depth, int window,
               int max_alignments, long long hcap, void* scratch, int K, int32_t* out, int32_t* info, MatchArgs* a, int* launch) {
  *launch = 0;
  if (B < 0 || cap < 0 || n_ids < 0 || !valid_table(hashbits, timebits, depth)) return MFPA_EINVAL;
  if (threshcount < 0 || search_depth < 0 || search_depth > kMaxCand || window < 0 || window > 1024 || max_alignments < 0 ||
      max_alignments >= INT32_MAX || K < 1)
    return MFPA_EINVAL;
  if (!valid_hcap(hcap)) return MFPA_EINVAL;
  if (B == 0) return MFPA_OK;
  if (!table || !counts || !hashesperid || !hashes || !nq || !scratch || !out || !info) return MFPA_EINVAL;
  a->table = table;
  a->counts = counts;
  a->hashesperid = hashesperid;
  a->n_ids = n_ids;
  a->timebits = timebits;
  a->depth = depth;
  a->hmask = (uint32_t)((1ull << hashbits) - 1);
  a->hashes = hashes;
  a->nq = nq;
  a->cap = cap;
  a->thresh = threshcount;
  a->search_depth = search_depth;
  a->window = window;
  a->max_modes = max_alignments + 1;
  a->hcap = hcap;
  a->scratch = static_cast<unsigned char*>(scratch);
  a->K = K;
  a->out = out;
  a->info = info;
  *launch = 1;
  return MFPA_OK;
}

}  // namespace

extern "C" int mfpa_audfprint_match_scratch_bytes(long long hcap, long long* bytes) {
  if (!bytes || !valid_hcap(hcap)) return MFPA_EINVAL;
  *bytes = hcap * kBytesPerHit;
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_match_ex_scratch_bytes(long long hcap, long long* bytes) {
  if (!bytes || !valid_hcap(hcap)) return MFPA_EINVAL;
  *bytes = hcap * kBytesPerHitEx;
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_match(const uint32_t* table, const int32_t* counts, const int32_t* hashesperid, int n_ids,
                                    int hashbits, int timebits, int depth, const int32_t* hashes, const int32_t* nq, int B,
                                    int cap, int threshcount, int search_depth, int window, int max_alignments,
                                    long long hcap, void* scratch, int K, int32_t* out, int32_t* info, void* stream) {
  MatchArgs a;
  int launch;
  const int rc = match_args(table, counts, hashesperid, n_ids, hashbits, timebits, depth, hashes, nq, B, cap, threshcount,
                            search_depth, window, max_alignments, hcap, scratch, K, out, info, &a, &launch);
  if (rc != MFPA_OK || !launch) return rc;
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(kBlock), 0, mfpa_stream(stream), a);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_match_ex(const uint32_t* table, const int32_t* counts, const int32_t* hashesperid, int n_ids,
                                       int hashbits, int timebits, int depth, const int32_t* hashes, const int32_t* nq, int B,
                                       int cap, int threshcount, int search_depth, int window, int max_alignments, int flags,
                                       double time_quantile, uint32_t pow2_roundup_mask, int hashesfor, int hf_cap,
                                       int32_t* hf_out, int32_t* hf_count, long long hcap, void* scratch, int K, int32_t* out,
                                       int32_t* info, void* stream) {
  if (flags < 0 || flags > (kExact | kTimeRange) || !(time_quantile >= 0.0 && time_quantile < 1.0) || hashesfor < -1)
    return MFPA_EINVAL;
  if ((flags & kExact) && threshcount < 1) return MFPA_EINVAL;   // find_modes: empty bins would qualify as modes
  if (cap > (1 << kRowBits)) return MFPA_EINVAL;                 // the query row's field of the regathered key
  if (hashesfor >= 0 && hf_cap < 1) return MFPA_EINVAL;
  MatchArgs a;
  int launch;
  const int rc = match_args(table, counts, hashesperid, n_ids, hashbits, timebits, depth, hashes, nq, B, cap, threshcount,
                            search_depth, window, max_alignments, hcap, scratch, K, out, info, &a, &launch);
  if (rc != MFPA_OK || !launch) return rc;
  if (hashesfor >= 0 && (!hf_out || !hf_count)) return MFPA_EINVAL;
  MatchExArgs x;
  x.flags = flags;
  x.quantile = time_quantile;
  x.p2mask = pow2_roundup_mask;
  x.hashesfor = hashesfor;
  x.hf_cap = hf_cap;
  x.hf_out = hf_out;
  x.hf_count = hf_count;
  hipLaunchKernelGGL(match_ex_kernel, dim3(B), dim3(kBlock), 0, mfpa_stream(stream), a, x);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
