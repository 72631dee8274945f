// Maintenance of the Audfprint hash table on MI355X (gfx950): HashTable.remove and HashTable.retrieve
// (afp/audfprint/hash_table.py:277-295, :297-316).  Integer only; results equal the reference's exactly.
//
// The table is match.hip's: (2^hashbits, depth) uint32 of ((id + 1) << timebits) | time, counts (2^hashbits) int32 that may
// exceed depth.  With n = min(counts[b], depth), a MATCH is a slot j < n of bucket b whose (table[b][j] >> timebits) - 1,
// taken on the unsigned value, is in the requested set.
//
// INVARIANT: both operations are specified on tables in which every slot at or beyond min(counts[b], depth) is zero --
// what store, reset, load and the reference's save produce.  Behaviour on other tables is unspecified.
//
// All three passes walk the table the same way: one wavefront per run of buckets, the counts of 64 buckets in one
// coalesced load, then bucket by bucket the first n slots in rounds of 64 (lane = slot, 256 contiguous bytes per round; the
// next bucket's first round is in flight while this one is worked on).  Buckets with n = 0 are never read.
// MFPA_MAINTAIN_FULL_ROWS reads all `depth` slots of every bucket instead (same results under the invariant; DESIGN.md §3.8
// has the two measured).
//
// remove   : a set of ids (byte map) in one pass.  A round's kept entries move to kept_so_far + prefix popcount of the
//            round's keep ballot -- never beyond a slot this wave has already read -- so the row is compacted in place and
//            in order; a bucket with a match then gets zeros from the kept count to `depth` and counts[b] = kept (the
//            entries dropped by the reservoir are forgotten, hash_table.py:289-290); a bucket without one is not written.
//            removed[id] sums per wave (runs of one id across the wave's buckets) before the atomic add.
// retrieve : rows (time, bucket) of K distinct ids, concatenated in request order, bucket ascending then slot ascending
//            (:309-315).  Deterministic by construction, no sort: the buckets are cut into C contiguous chunks, one wave
//            each.  (1) count: work[rank][chunk] = matches; (2) scan: exclusive over the chunks of each rank, then over the
//            ranks -> offsets (K + 1); (3) scatter: each wave walks its chunk again and takes positions
//            offsets[rank] + work[rank][chunk]++ in walking order.  A cell of `work` belongs to one wave, so the order in
//            which atomics arrive cannot change a position.
#include "mfpa_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / MFPA_WAVE;
constexpr int kMaxRemoveWaves = 1 << 14;
constexpr int kMaxChunks = 4096;            // retrieve: waves, and columns of `work`
constexpr long long kWorkBudget = 1ll << 22;   // retrieve: at most this many int32 of `work` once K > 1024

// match.hip's valid_table
bool valid_table(int hashbits, int timebits, int depth) {
  return hashbits >= 1 && hashbits <= 24 && timebits >= 1 && timebits <= 20 && depth >= 1 && depth <= 4096;
}

__device__ __forceinline__ unsigned long long lanes_below(int lane) { return (1ull << lane) - 1ull; }

// Buckets [b0, b1) by one wavefront, in order.  For bucket b with n = min(max(counts[b], 0), depth) valid slots it calls
// op.round(b, row, n, j0, v) for j0 = 0, 64, ... (v = row[j0 + lane], 0 past the slots read), then op.end(b, row).
// All arguments but v are wave-uniform.  Slots read: n, or `depth` with `full`.
template <class Op>
__device__ __forceinline__ void walk(uint32_t* table, const int32_t* counts, long long b0, long long b1, int depth, bool full,
                                     Op& op) {
  const int lane = threadIdx.x & 63;
  for (long long g = b0; g < b1; g += 64) {
    const bool in = g + lane < b1;
    const int nl = in ? min(max(counts[g + lane], 0), depth) : 0;
    const int rl = in && full ? depth : nl;
    unsigned long long todo = __ballot(rl > 0);
    uint32_t vpre = 0;
    if (todo) {
      const int i = __ffsll((long long)todo) - 1;
      if (lane < __shfl(rl, i)) vpre = table[(size_t)(g + i) * depth + lane];
    }
    while (todo) {
      const int i = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int n = __shfl(nl, i), r = __shfl(rl, i);
      uint32_t* row = table + (size_t)(g + i) * depth;
      uint32_t v = vpre;
      vpre = 0;
      if (todo) {                                          // another bucket's row: no alias with what op writes to this one
        const int i2 = __ffsll((long long)todo) - 1;
        if (lane < __shfl(rl, i2)) vpre = table[(size_t)(g + i2) * depth + lane];
      }
      for (int j0 = 0; j0 < r; j0 += 64) {
        if (j0) v = j0 + lane < r ? row[j0 + lane] : 0u;
        op.round(g + i, row, n, j0, v);
      }
      op.end(g + i, row);
    }
  }
}

// Sums per id (or per cell) over one wave: consecutive hits of one key are added up in a wave-uniform register pair and
// reach memory as one atomic add when the key changes or the wave ends.
struct RunSum {
  int32_t* base;
  long long key = -1;
  int sum = 0;
  __device__ __forceinline__ void add(long long k, int c) {           // wave-uniform arguments
    if (k != key) {
      flush();
      key = k;
    }
    sum += c;
  }
  __device__ __forceinline__ void flush() {
    if (key >= 0 && sum > 0 && (threadIdx.x & 63) == 0) atomicAdd(base + key, sum);
    sum = 0;
  }
};

struct RemoveOp {
  const uint8_t* in_set;
  uint32_t n_ids;
  int timebits, depth;
  int32_t* counts;
  RunSum removed;
  int kept = 0, dropped = 0;

  __device__ __forceinline__ void round(long long, uint32_t* row, int n, int j0, uint32_t v) {
    const int lane = threadIdx.x & 63, j = j0 + lane;
    const uint32_t id = (v >> timebits) - 1u;              // an empty slot gives 0xffffffff: in no set
    const bool valid = j < n;
    const bool hit = valid && id < n_ids && in_set[id] != 0;
    const bool keep = valid && !hit;
    unsigned long long hb = __ballot(hit);
    const unsigned long long kb = __ballot(keep);
    if (hb | (unsigned long long)dropped) {                // something before this entry is gone: it moves down
      const int pos = kept + __popcll(kb & lanes_below(lane));
      if (keep && pos != j) row[pos] = v;
    }
    kept += __popcll(kb);
    dropped += __popcll(hb);
    while (hb) {                                           // one group of lanes per distinct id of the round
      const uint32_t lid = (uint32_t)__shfl((int)id, __ffsll((long long)hb) - 1);
      const unsigned long long same = __ballot(hit && id == lid);
      removed.add((long long)lid, __popcll(same));
      hb &= ~same;
    }
  }
  __device__ __forceinline__ void end(long long b, uint32_t* row) {
    if (dropped) {
      const int lane = threadIdx.x & 63;
      for (int j = kept + lane; j < depth; j += 64) row[j] = 0u;
      if (lane == 0) counts[b] = kept;
    }
    kept = dropped = 0;
  }
};

__global__ __launch_bounds__(kBlock) void remove_kernel(uint32_t* __restrict__ table, int32_t* counts, long long nb,
                                                         long long per, int depth, int timebits, int full,
                                                         const uint8_t* __restrict__ in_set, int n_ids,
                                                         int32_t* __restrict__ removed) {
  const long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  const long long b0 = w * per;
  if (b0 >= nb) return;
  RemoveOp op{in_set, (uint32_t)n_ids, timebits, depth, counts, RunSum{removed}};
  walk(table, counts, b0, min(nb, b0 + per), depth, full != 0, op);
  op.removed.flush();
}

// Retrieve's two walks.  SCATTER false: work[rank * C + chunk] += matches.  SCATTER true: the same cell, by now the number
// of the rank's rows in earlier chunks, hands out the positions.
template <bool SCATTER>
struct RetrieveOp {
  const int32_t* rank;
  uint32_t n_ids;
  int K, timebits;
  int32_t* cells;                                          // work + chunk, stride C
  long long C;
  const int32_t* offsets;
  int32_t* rows;
  int n_rows;
  RunSum sums;

  __device__ __forceinline__ void round(long long b, uint32_t*, int n, int j0, uint32_t v) {
    const int lane = threadIdx.x & 63;
    const uint32_t id = (v >> timebits) - 1u;
    int rk = -1;
    if (j0 + lane < n && id < n_ids) rk = rank[id];
    if (rk >= K) rk = -1;                                  // not a rank of this request: never an index
    unsigned long long hb = __ballot(rk >= 0);
    while (hb) {
      const int leader = __ffsll((long long)hb) - 1;
      const int lrk = __shfl(rk, leader);
      const unsigned long long same = __ballot(rk == lrk);
      const int c = __popcll(same);
      if (SCATTER) {
        int base = 0;
        if (lane == leader) base = atomicAdd(cells + (long long)lrk * C, c);
        base = __shfl(base, leader);
        const long long pos = (long long)offsets[lrk] + base + __popcll(same & lanes_below(lane));
        if (rk == lrk && pos < n_rows) {
          rows[2 * pos] = (int32_t)(v & ((1u << timebits) - 1u));
          rows[2 * pos + 1] = (int32_t)b;
        }
      } else {
        sums.add((long long)lrk * C, c);
      }
      hb &= ~same;
    }
  }
  __device__ __forceinline__ void end(long long, uint32_t*) {}
};

template <bool SCATTER>
__global__ __launch_bounds__(kBlock) void retrieve_kernel(const uint32_t* __restrict__ table, const int32_t* __restrict__ counts,
                                                           long long nb, long long per, int C, int depth, int timebits, int full,
                                                           const int32_t* __restrict__ rank, int n_ids, int K, int32_t* work,
                                                           const int32_t* __restrict__ offsets, int32_t* __restrict__ rows,
                                                           int n_rows) {
  const long long w = (long long)blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (w >= C) return;
  const long long b0 = w * per;
  RetrieveOp<SCATTER> op{rank, (uint32_t)n_ids, K, timebits, work + w, C, offsets, rows, n_rows, RunSum{work + w}};
  walk(const_cast<uint32_t*>(table), counts, b0, min(nb, b0 + per), depth, full != 0, op);   // neither Op writes the table
  if (!SCATTER) op.sums.flush();
}

__device__ __forceinline__ int wave_incl_scan(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o);
    if (lane >= o) v += u;
  }
  return v;
}

// One wave per rank: its C chunk counts become exclusive prefixes; the rank's total goes to offsets[rank + 1].
__global__ __launch_bounds__(kBlock) void scan_chunks_kernel(int32_t* __restrict__ work, int C, int K, int32_t* __restrict__ offsets) {
  const int k = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  int32_t* w = work + (size_t)k * C;
  int carry = 0;
  for (int c0 = 0; c0 < C; c0 += 64) {
    const int c = c0 + lane;
    const int x = c < C ? w[c] : 0;
    const int s = wave_incl_scan(x);
    if (c < C) w[c] = carry + s - x;
    carry += __shfl(s, 63);
  }
  if (lane == 0) offsets[k + 1] = carry;
}

// One wave: offsets[0] = 0, offsets[k + 1] = the totals up to and including rank k.
__global__ __launch_bounds__(MFPA_WAVE) void scan_ranks_kernel(int32_t* __restrict__ offsets, int K) {
  const int lane = threadIdx.x;
  if (lane == 0) offsets[0] = 0;
  int carry = 0;
  for (int k0 = 0; k0 < K; k0 += 64) {
    const int k = k0 + lane;
    const int s = wave_incl_scan(k < K ? offsets[k + 1] : 0);
    if (k < K) offsets[k + 1] = carry + s;
    carry += __shfl(s, 63);
  }
}

// Chunks of retrieve's two walks and buckets per chunk: host arithmetic on (hashbits, K) alone, so both walks agree.
void retrieve_chunks(int hashbits, int K, int* C, long long* per) {
  const long long nb = 1ll << hashbits;
  long long c = kWorkBudget / (K > 0 ? K : 1);
  c = c < 1 ? 1 : c > kMaxChunks ? kMaxChunks : c;
  if (c > nb) c = nb;
  *per = (nb + c - 1) / c;
  *C = (int)((nb + *per - 1) / *per);
}

// Every row index fits int32.
bool retrieve_fits(int hashbits, int depth) { return ((long long)depth << hashbits) <= (long long)INT32_MAX; }

bool valid_flags(int flags) { return flags == 0 || flags == MFPA_MAINTAIN_FULL_ROWS; }

}  // namespace

extern "C" int mfpa_audfprint_remove(uint32_t* table, int32_t* counts, int hashbits, int timebits, int depth,
                                     const uint8_t* in_set, int n_ids, int flags, int32_t* removed, void* stream) {
  if (n_ids < 0 || !valid_flags(flags) || !valid_table(hashbits, timebits, depth)) return MFPA_EINVAL;
  if (n_ids == 0) return MFPA_OK;                          // the empty set
  if (!table || !counts || !in_set || !removed) return MFPA_EINVAL;
  const long long nb = 1ll << hashbits, groups = (nb + 63) / 64;
  const long long waves = groups < kMaxRemoveWaves ? groups : kMaxRemoveWaves;
  const long long per = 64 * ((groups + waves - 1) / waves);
  MFPA_HIP(hipMemsetAsync(removed, 0, (size_t)n_ids * sizeof(int32_t), mfpa_stream(stream)));
  hipLaunchKernelGGL(remove_kernel, dim3((unsigned)((waves + kWaves - 1) / kWaves)), dim3(kBlock), 0, mfpa_stream(stream), table,
                     counts, nb, per, depth, timebits, flags, in_set, n_ids, removed);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_retrieve_work_ints(int hashbits, int K, long long* ints) {
  if (!ints || K < 0 || hashbits < 1 || hashbits > 24) return MFPA_EINVAL;
  int C;
  long long per;
  retrieve_chunks(hashbits, K, &C, &per);
  *ints = (long long)K * C;
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_retrieve_count(const uint32_t* table, const int32_t* counts, int hashbits, int timebits, int depth,
                                             const int32_t* rank, int n_ids, int K, int flags, int32_t* work, int32_t* offsets,
                                             void* stream) {
  if (K < 0 || n_ids < 0 || K > n_ids || !valid_flags(flags) || !valid_table(hashbits, timebits, depth) ||
      !retrieve_fits(hashbits, depth))
    return MFPA_EINVAL;
  if (K == 0) return MFPA_OK;
  if (!table || !counts || !rank || !work || !offsets) return MFPA_EINVAL;
  int C;
  long long per;
  retrieve_chunks(hashbits, K, &C, &per);
  MFPA_HIP(hipMemsetAsync(work, 0, (size_t)K * C * sizeof(int32_t), mfpa_stream(stream)));
  hipLaunchKernelGGL(retrieve_kernel<false>, dim3((C + kWaves - 1) / kWaves), dim3(kBlock), 0, mfpa_stream(stream), table, counts,
                     1ll << hashbits, per, C, depth, timebits, flags, rank, n_ids, K, work, (const int32_t*)nullptr,
                     (int32_t*)nullptr, 0);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_chunks_kernel, dim3((K + kWaves - 1) / kWaves), dim3(kBlock), 0, mfpa_stream(stream), work, C, K, offsets);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(scan_ranks_kernel, dim3(1), dim3(MFPA_WAVE), 0, mfpa_stream(stream), offsets, K);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

extern "C" int mfpa_audfprint_retrieve(const uint32_t* table, const int32_t* counts, int hashbits, int timebits, int depth,
                                       const int32_t* rank, int n_ids, int K, int flags, int32_t* work, const int32_t* offsets,
                                       int32_t* rows, int n_rows, void* stream) {
  if (K < 0 || n_ids < 0 || K > n_ids || n_rows < 0 || !valid_flags(flags) || !valid_table(hashbits, timebits, depth) ||
      !retrieve_fits(hashbits, depth))
    return MFPA_EINVAL;
  if (K == 0 || n_rows == 0) return MFPA_OK;
  if (!table || !counts || !rank || !work || !offsets || !rows) return MFPA_EINVAL;
  int C;
  long long per;
  retrieve_chunks(hashbits, K, &C, &per);
  hipLaunchKernelGGL(retrieve_kernel<true>, dim3((C + kWaves - 1) / kWaves), dim3(kBlock), 0, mfpa_stream(stream), table, counts,
                     1ll << hashbits, per, C, depth, timebits, flags, rank, n_ids, K, work, offsets, rows, n_rows);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}
