// Landmark pairing and hashing for MI355X (gfx950) -- the step right after the peak pickers
// (SURVEY.md §8f-1).  Integer-only, so results are identical to the reference's.
//
//   audfprint: peaks2landmarks (afp/audfprint/peak_extractor.py:313-346), landmarks2hashes (:40-58) and the
//              duplicate removal of wavfile2hashes (:443-460: merge to time<<32|hash, unique, sort).
//              Clips (mfpa_audfprint_landmarks): one workgroup per clip, up to 8192 landmarks -- one LDS sort.
//              Whole tracks (mfpa_audfprint_landmarks_track, up to 16384 frames, any number of landmarks): tiles of 256 frames
//              (+ a halo of targetdt - 1 frames of peak lists).  A tile holds <= 256 * 8 * maxpairs <= 8192 landmarks, so the
//              same LDS sort holds any tile; the sort key is time << 32 | hash and a tile owns a contiguous time range, so
//              tiles sorted on their own and written in tile order ARE the globally sorted list, and duplicates can only meet
//              inside one tile.  Three launches: per-tile counts, an exclusive scan over the tiles of a clip, emission at those
//              offsets (the tile is computed again).  The launches are ordered by the stream: no workgroup reads what another
//              wrote in the same launch.  Both kernels are built from the same pieces below.
//   dejavu   : generate_hashes (afp/dejavu/fingerprint.py:174-213): peaks in time order, each paired with its next
//              fan_value-1 peaks, SHA-1("f1|f2|dt") truncated to 20 hex digits (10 bytes).
//
// The peak mask never leaves the device between the picker and the hash list.
#include "mfpa_common.h"
#include "mfpa_sort.h"

namespace {

constexpr int HT = 256;            // threads (= frames of a tile)
constexpr int MAXPK = 8;           // peaks per frame (the pruner keeps <= 8)
constexpr int SORT_CAP = 8192;     // clip kernel: landmarks of a clip
constexpr int CLIP_MAX_PAIRS = 3;
constexpr int TILE_W = HT;
constexpr int MAX_PAIRS = 4;       // tiles: 256 * 8 * 4 = 8192 landmarks per tile at the most
constexpr int MAX_TARGETDT = 256;  // halo frames of peak lists per tile: targetdt - 1

struct AudLds {
  size_t pk, npk, col_off, sh, keys, total;
};
__host__ __device__ inline AudLds aud_lds(int T, int npow) {   // byte offsets of the clip kernel's LDS carve
  AudLds l;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  l.pk = 0;
  l.npk = up(l.pk + sizeof(short) * (size_t)T * MAXPK);
  l.col_off = up(l.npk + sizeof(short) * (size_t)T);
  l.sh = up(l.col_off + sizeof(int) * (size_t)T);
  l.keys = up(l.sh + sizeof(int) * (HT + 2));
  l.total = l.keys + sizeof(unsigned long long) * (size_t)npow;
  return l;
}

struct TileLds {
  size_t pk, npk, sh, keys, total;
};
__host__ __device__ inline TileLds tile_lds(int nfr, int npow) {   // byte offsets of the tile kernel's LDS carve; nfr = TILE_W + targetdt - 1
  TileLds l;
  auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
  l.pk = 0;
  l.npk = up(l.pk + sizeof(short) * (size_t)nfr * MAXPK);
  l.sh = up(l.npk + sizeof(short) * (size_t)nfr);
  l.keys = up(l.sh + sizeof(int) * (HT + 2));
  l.total = l.keys + sizeof(unsigned long long) * (size_t)npow;
  return l;
}

__host__ __device__ inline int pow2_at_least(int v) {
  int p = 1;
  while (p < v) p <<= 1;
  return p;
}

// exclusive scan over HT threads (all of them call); sh[HT + 1]; the total in sh[HT]
__device__ __forceinline__ int tile_excl_scan(int v, int* sh, int tid) {
  __syncthreads();                                             // (sh may still be read from the previous scan)
  sh[tid] = v;
  __syncthreads();
  if (tid < 64) {                                              // one wavefront: four values per lane, a shuffle scan across the lanes
    int a[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { a[k] = sh[4 * tid + k]; s += a[k]; }
    int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (tid >= o) incl += t;
    }
    int acc = incl - s;
#pragma unroll
    for (int k = 0; k < 4; ++k) { sh[4 * tid + k] = acc; acc += a[k]; }
    if (tid == 63) sh[HT] = incl;
  }
  __syncthreads();
  return sh[tid];
}

// ------------------------------------------------------------------------------------------ audfprint: the shared pieces
// Per-frame peak lists (bins ascending) of frames [0, nfr) of M (bin rows of pitch T): thread = frame, consecutive threads read
// consecutive bytes of a bin row.  *flag (LDS, zeroed by the caller) is set when one of the first nflag frames holds more than
// MAXPK peaks.  Ends on a barrier.
__device__ __forceinline__ void peak_lists(const uint8_t* M, int R, int T, int nfr, int nflag, short* pk, short* npk, int* flag, int tid) {
  for (int c = tid; c < nfr; c += HT) {
    int n = 0;
    for (int r = 0; r < R; ++r) {
      if (M[(size_t)r * T + c]) {
        if (n < MAXPK) pk[c * MAXPK + n] = (short)r;
        ++n;
      }
    }
    if (n > MAXPK) {
      if (c < nflag) atomicOr(flag, 1);
      n = MAXPK;
    }
    npk[c] = (short)n;
  }
  __syncthreads();
}

struct PairRule {
  int mindt, targetdt, targetdf, maxpairs;
};

// Landmarks of peak i of frame c of the lists, scanning col2 then bin2 ascending (peak_extractor.py:313-346; `scols` there is only a
// loop bound -- frames beyond the last peak hold no peaks -- so the number of readable frames, c_stop, serves).  t_first: the absolute
// time of frame 0 of the lists.  out (nullable): 4 * maxpairs values (time, bin, bin2, dt).
__device__ __forceinline__ int pairs_of(const short* pk, const short* npk, int c, int i, int t_first, int c_stop, PairRule q, int32_t* out) {
  const int p = pk[c * MAXPK + i];
  int pairs = 0;
  const int c_end = min(c_stop, c + q.targetdt);
  for (int c2 = c + q.mindt; c2 < c_end && pairs < q.maxpairs; ++c2) {
    const int n2 = npk[c2];
    for (int k = 0; k < n2 && pairs < q.maxpairs; ++k) {
      const int p2 = pk[c2 * MAXPK + k];
      const int d = p2 - p;
      if ((d < 0 ? -d : d) < q.targetdf) {
        if (out) { out[4 * pairs] = t_first + c; out[4 * pairs + 1] = p; out[4 * pairs + 2] = p2; out[4 * pairs + 3] = c2 - c; }
        ++pairs;
      }
    }
  }
  return pairs;
}

// landmarks2hashes: 8 bits of bin, 6 of the bin difference, 6 of the time difference
__device__ __forceinline__ int32_t landmark_hash(const int32_t* lm) {
  return ((lm[1] & 255) << 12) | (((lm[2] - lm[1]) & 63) << 6) | (lm[3] & 63);
}
__device__ __forceinline__ unsigned long long sort_key(int32_t time, int32_t hash) {
  return ((unsigned long long)(unsigned)time << 32) + (unsigned long long)(unsigned)hash;
}

// ascending bitonic sort of npow (a power of two) keys in LDS; ends on a barrier
__device__ __forceinline__ void sort_lds(unsigned long long* keys, int npow) {
  for (int k = 2; k <= npow; k <<= 1) mfpa_sort::lds_bitonic<HT>(keys, npow, 0, k, k >> 1);
}

// Unique compaction of keys[0, total) (sorted ascending; the padding ~0 never equals a real key): the rows (time, hash) to UQ when it is
// not null; returns their number.  All threads call.
__device__ __forceinline__ int unique_rows(const unsigned long long* keys, int total, int32_t* UQ, int* sh, int tid) {
  const int per = (total + HT - 1) / HT;
  const int i0 = min(total, tid * per), i1 = min(total, i0 + per);
  int cnt = 0;
  for (int i = i0; i < i1; ++i) cnt += (i == 0 || keys[i] != keys[i - 1]);
  int off = tile_excl_scan(cnt, sh, tid);
  if (UQ) {
    for (int i = i0; i < i1; ++i) {
      if (i == 0 || keys[i] != keys[i - 1]) {
        UQ[2 * off] = (int32_t)(keys[i] >> 32);
        UQ[2 * off + 1] = (int32_t)(keys[i] & 0xFFFFFFFFull);
        ++off;
      }
    }
  }
  return sh[HT];
}

// ------------------------------------------------------------------------------------------ audfprint: clips
// One workgroup per clip.  mask (R, T) uint8, R <= 256.  landmarks (cap, 4) int32 in the reference's list order, hashes (cap, 2) int32 in
// the same order, uniq (cap, 2) int32 sorted unique, counts[0] = landmarks (or -1 on overflow), counts[1] = unique.
__global__ __launch_bounds__(HT) void audfprint_landmarks_kernel(const uint8_t* __restrict__ mask, int R, int T, int cap, PairRule q,
                                                                 int32_t* __restrict__ landmarks, int32_t* __restrict__ hashes,
                                                                 int32_t* __restrict__ uniq, int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const AudLds L = aud_lds(T, 1);
  short* pk = reinterpret_cast<short*>(smem + L.pk);             // [T][MAXPK]
  short* npk = reinterpret_cast<short*>(smem + L.npk);           // [T]
  int* col_off = reinterpret_cast<int*>(smem + L.col_off);       // [T]
  int* sh = reinterpret_cast<int*>(smem + L.sh);                 // [HT + 2] scan scratch; sh[HT + 1]: the ">8 peaks" flag
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + L.keys);  // [pow2 >= n]

  const int tid = threadIdx.x, b = blockIdx.x;
  int32_t* LM = landmarks + (size_t)b * cap * 4;
  int32_t* HS = hashes + (size_t)b * cap * 2;
  if (tid == 0) sh[HT + 1] = 0;
  __syncthreads();
  peak_lists(mask + (size_t)b * R * T, R, T, T, T, pk, npk, &sh[HT + 1], tid);

  // pass 1: landmarks per frame -> offsets
  int total = 0;
  {
    // frames are distributed in contiguous chunks so the block scan yields list order
    const int per = (T + HT - 1) / HT;
    const int c0 = tid * per, c1 = min(T, c0 + per);
    int mine = 0;
    for (int c = c0; c < c1; ++c) {
      int cc = 0;
      for (int i = 0; i < npk[c]; ++i) cc += pairs_of(pk, npk, c, i, 0, T, q, nullptr);
      col_off[c] = cc;
      mine += cc;
    }
    int off = tile_excl_scan(mine, sh, tid);
    total = sh[HT];
    for (int c = c0; c < c1; ++c) {
      const int cc = col_off[c];
      col_off[c] = off;
      off += cc;
    }
  }
  __syncthreads();
  if (total > cap || total > SORT_CAP || sh[HT + 1]) {
    if (tid == 0) { counts[2 * b] = -1; counts[2 * b + 1] = -1; }
    return;
  }
  // pass 2: emit landmarks + hashes in list order, keys for the unique/sort step
  const int npow = pow2_at_least(total);
  for (int i = tid; i < npow; i += HT) keys[i] = ~0ull;
  __syncthreads();
  for (int c = tid; c < T; c += HT) {
    int off = col_off[c];
    for (int i = 0; i < npk[c]; ++i) {
      int32_t tmp[4 * CLIP_MAX_PAIRS];
      const int n = pairs_of(pk, npk, c, i, 0, T, q, tmp);
      for (int k = 0; k < n; ++k) {
        const int e = off + k;
        const int32_t h = landmark_hash(tmp + 4 * k);
        LM[4 * e] = tmp[4 * k]; LM[4 * e + 1] = tmp[4 * k + 1]; LM[4 * e + 2] = tmp[4 * k + 2]; LM[4 * e + 3] = tmp[4 * k + 3];
        HS[2 * e] = tmp[4 * k];
        HS[2 * e + 1] = h;
        keys[e] = sort_key(tmp[4 * k], h);
      }
      off += n;
    }
  }
  __syncthreads();
  sort_lds(keys, npow);
  const int nuniq = unique_rows(keys, total, uniq + (size_t)b * cap * 2, sh, tid);
  if (tid == 0) { counts[2 * b] = total; counts[2 * b + 1] = nuniq; }
}

// ------------------------------------------------------------------------------------------ audfprint: whole tracks
// One tile of one clip: frames [t0, t0 + 256) pair with frames < t0 + 256 + targetdt - 1.
// EMIT = false: tiles[b][tile] = {landmarks, unique rows} of the tile; landmarks = -1 when a frame of the tile holds more than 8 peaks.
// EMIT = true : tiles[b][tile] holds the tile's offsets {first landmark, first unique row} (tile_scan_kernel); the landmarks and
//               hashes go out in list order (skipped when the pointers are null), the unique rows sorted; a flagged clip (counts[2b] < 0)
//               writes nothing.
template <bool EMIT>
__global__ __launch_bounds__(HT) void landmarks_tile_kernel(const uint8_t* __restrict__ mask, int R, int T, int ntiles, int cap_lds,
                                                            PairRule q, int cap, int32_t* __restrict__ tiles,
                                                            int32_t* __restrict__ landmarks, int32_t* __restrict__ hashes,
                                                            int32_t* __restrict__ uniq, const int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nfr_max = TILE_W + q.targetdt - 1;
  const TileLds L = tile_lds(nfr_max, 1);
  short* pk = reinterpret_cast<short*>(smem + L.pk);             // [nfr][MAXPK]
  short* npk = reinterpret_cast<short*>(smem + L.npk);           // [nfr]
  int* sh = reinterpret_cast<int*>(smem + L.sh);                 // [HT + 2] scan scratch; sh[HT + 1]: the ">8 peaks" flag
  unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + L.keys);  // [cap_lds]: a power of two >= the tile's landmarks

  const int tid = threadIdx.x, b = blockIdx.x, tile = blockIdx.y;
  int32_t* tc = tiles + ((size_t)b * ntiles + tile) * 2;
  if (EMIT && counts[2 * b] < 0) return;                         // (uniform)
  const int t0 = tile * TILE_W;
  const int nown = min(TILE_W, T - t0);                          // frames this tile owns
  const int nfr = min(nfr_max, T - t0);                          // ... and reads
  if (tid == 0) sh[HT + 1] = 0;
  __syncthreads();
  peak_lists(mask + (size_t)b * R * T + t0, R, T, nfr, nown, pk, npk, &sh[HT + 1], tid);   // (a halo frame is flagged by the tile that owns it)
  if (sh[HT + 1]) {
    if (!EMIT && tid == 0) { tc[0] = -1; tc[1] = 0; }
    return;                                                      // (EMIT: unreachable, the clip is flagged)
  }

  // thread = frame: the scan over the threads yields list order
  int mine = 0;
  if (tid < nown)
    for (int i = 0; i < npk[tid]; ++i) mine += pairs_of(pk, npk, tid, i, t0, nfr, q, nullptr);
  int off = tile_excl_scan(mine, sh, tid);
  const int total = sh[HT];                                      // <= 256 * 8 * maxpairs <= 8192
  if (total > cap || total > cap_lds) {                          // more than the caller's capacity in ONE tile: the clip overflows
    if (!EMIT && tid == 0) { tc[0] = total; tc[1] = total; }     // (the scan flags the clip: its landmark total exceeds cap)
    return;
  }
  const int npow = pow2_at_least(total);
  for (int i = tid; i < npow; i += HT) keys[i] = ~0ull;
  __syncthreads();
  const size_t lm0 = EMIT ? (size_t)b * cap + tc[0] : 0, uq0 = EMIT ? (size_t)b * cap + tc[1] : 0;
  const bool lists = EMIT && landmarks != nullptr && hashes != nullptr;
  if (tid < nown) {
    for (int i = 0; i < npk[tid]; ++i) {
      int32_t tmp[4 * MAX_PAIRS];
      const int n = pairs_of(pk, npk, tid, i, t0, nfr, q, tmp);
      for (int k = 0; k < n; ++k) {
        const int e = off + k;
        const int32_t h = landmark_hash(tmp + 4 * k);
        if (lists) {
          int32_t* LM = landmarks + (lm0 + e) * 4;
          int32_t* HS = hashes + (lm0 + e) * 2;
          LM[0] = tmp[4 * k]; LM[1] = tmp[4 * k + 1]; LM[2] = tmp[4 * k + 2]; LM[3] = tmp[4 * k + 3];
          HS[0] = tmp[4 * k];
          HS[1] = h;
        }
        keys[e] = sort_key(tmp[4 * k], h);
      }
      off += n;
    }
  }
  __syncthreads();
  sort_lds(keys, npow);
  const int nuniq = unique_rows(keys, total, EMIT ? uniq + uq0 * 2 : nullptr, sh, tid);
  if (!EMIT && tid == 0) { tc[0] = total; tc[1] = nuniq; }
}

// tiles (B, ntiles, 2): per-tile counts -> exclusive offsets in place; counts[b] = {landmarks, unique rows} of the clip, or {-1, -1} when a
// frame holds more than 8 peaks or the clip more than `cap` landmarks.  A thread per clip: at most 64 tiles.
__global__ __launch_bounds__(64) void tile_scan_kernel(int32_t* __restrict__ tiles, int B, int ntiles, int cap, int32_t* __restrict__ counts) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  int32_t* tc = tiles + (size_t)b * ntiles * 2;
  long long lm = 0, uq = 0;
  bool bad = false;
  for (int t = 0; t < ntiles; ++t) {
    const int n = tc[2 * t], u = tc[2 * t + 1];
    bad = bad || n < 0;
    tc[2 * t] = (int)(lm < cap ? lm : cap);                       // (never used beyond cap: the clip is flagged then)
    tc[2 * t + 1] = (int)(uq < cap ? uq : cap);
    lm += n < 0 ? 0 : n;
    uq += u;
  }
  bad = bad || lm > cap;
  counts[2 * b] = bad ? -1 : (int)lm;
  counts[2 * b + 1] = bad ? -1 : (int)uq;
}

// ------------------------------------------------------------------------------------------ dejavu + SHA-1
__device__ __forceinline__ uint32_t rol(uint32_t x, int s) { return (x << s) | (x >> (32 - s)); }

__device__ int put_dec(unsigned char* m, int pos, int v) {   // decimal digits of v >= 0
  char tmp[12];
  int n = 0;
  do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (n) m[pos++] = (unsigned char)tmp[--n];
  return pos;
}

// SHA-1 of the ASCII string "f1|f2|dt" (<= 55 bytes: one block); writes the first 10 digest bytes.
__device__ void sha1_trunc10(int f1, int f2, int dt, uint8_t* out10) {
  unsigned char m[64];
#pragma unroll
  for (int i = 0; i < 64; ++i) m[i] = 0;
  int len = put_dec(m, 0, f1);
  m[len++] = '|';
  len = put_dec(m, len, f2);
  m[len++] = '|';
  len = put_dec(m, len, dt);
  m[len] = 0x80;
  const unsigned bits = (unsigned)len * 8u;
  m[62] = (unsigned char)(bits >> 8);
  m[63] = (unsigned char)(bits & 0xFF);
  uint32_t w[80];
  for (int i = 0; i < 16; ++i)
    w[i] = ((uint32_t)m[4 * i] << 24) | ((uint32_t)m[4 * i + 1] << 16) | ((uint32_t)m[4 * i + 2] << 8) | (uint32_t)m[4 * i + 3];
  for (int i = 16; i < 80; ++i) w[i] = rol(w[i - 3] ^ w[i - 8] ^ w[i - 14] ^ w[i - 16], 1);
  uint32_t a = 0x67452301u, b = 0xEFCDAB89u, c = 0x98BADCFEu, d = 0x10325476u, e = 0xC3D2E1F0u;
  for (int i = 0; i < 80; ++i) {
    uint32_t f, k;
    if (i < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
    else if (i < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
    else if (i < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
    else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
    const uint32_t t = rol(a, 5) + f + e + k + w[i];
    e = d; d = c; c = rol(b, 30); b = a; a = t;
  }
  const uint32_t h0 = 0x67452301u + a, h1 = 0xEFCDAB89u + b, h2 = 0x98BADCFEu + c;
  out10[0] = (uint8_t)(h0 >> 24); out10[1] = (uint8_t)(h0 >> 16); out10[2] = (uint8_t)(h0 >> 8); out10[3] = (uint8_t)h0;
  out10[4] = (uint8_t)(h1 >> 24); out10[5] = (uint8_t)(h1 >> 16); out10[6] = (uint8_t)(h1 >> 8); out10[7] = (uint8_t)h1;
  out10[8] = (uint8_t)(h2 >> 24); out10[9] = (uint8_t)(h2 >> 16);
}

// mask (F, T) uint8.  Peaks in (time, freq) order = the reference's stable sort by time of the row-major list.
// digests (cap, 10) uint8, t1 (cap) int32, counts[b] = number of hashes (-1 on overflow).
__global__ __launch_bounds__(HT) void dejavu_hashes_kernel(const uint8_t* __restrict__ mask, int F, int T, int cap,
                                                           int peak_cap, int fan, int min_dt, int max_dt,
                                                           uint8_t* __restrict__ digests, int32_t* __restrict__ t1,
                                                           int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  int* sh = reinterpret_cast<int*>(smem);          // [HT + 2]
  int* col_off = sh + HT + 2;                      // [T]
  short* pf = reinterpret_cast<short*>(col_off + T);   // [peak_cap] freq
  short* pt = pf + peak_cap;                       // [peak_cap] time
  const int tid = threadIdx.x, b = blockIdx.x;
  const uint8_t* M = mask + (size_t)b * F * T;
  const int per = (T + HT - 1) / HT;
  const int c0 = tid * per, c1 = min(T, c0 + per);
  int mine = 0;
  for (int c = c0; c < c1; ++c) {
    int n = 0;
    for (int r = 0; r < F; ++r) n += M[(size_t)r * T + c] != 0;
    col_off[c] = n;
    mine += n;
  }
  int off = tile_excl_scan(mine, sh, tid);
  const int npeaks = sh[HT];
  if (npeaks > peak_cap) {
    if (tid == 0) counts[b] = -1;
    return;
  }
  for (int c = c0; c < c1; ++c) {
    for (int r = 0; r < F; ++r)
      if (M[(size_t)r * T + c]) { pf[off] = (short)r; pt[off] = (short)c; ++off; }
  }
  __syncthreads();
  // hashes per peak i: j = 1 .. fan-1, kept when min_dt <= t2 - t1 <= max_dt
  const int pper = (npeaks + HT - 1) / HT;
  const int i0 = tid * pper, i1 = min(npeaks, i0 + pper);
  mine = 0;
  for (int i = i0; i < i1; ++i)
    for (int j = 1; j < fan; ++j)
      if (i + j < npeaks) { const int dt = pt[i + j] - pt[i]; mine += (dt >= min_dt && dt <= max_dt); }
  off = tile_excl_scan(mine, sh, tid);
  const int total = sh[HT];
  if (total > cap) {
    if (tid == 0) counts[b] = -1;
    return;
  }
  uint8_t* D = digests + (size_t)b * cap * 10;
  int32_t* TT = t1 + (size_t)b * cap;
  for (int i = i0; i < i1; ++i)
    for (int j = 1; j < fan; ++j)
      if (i + j < npeaks) {
        const int dt = pt[i + j] - pt[i];
        if (dt >= min_dt && dt <= max_dt) {
          sha1_trunc10(pf[i], pf[i + j], dt, D + (size_t)off * 10);
          TT[off] = pt[i];
          ++off;
        }
      }
  if (tid == 0) counts[b] = total;
}

}  // namespace

extern "C" {

int mfpa_audfprint_landmarks(const uint8_t* mask, int B, int R, int T, int cap, int mindt, int targetdt, int targetdf,
                             int maxpairs, int32_t* landmarks, int32_t* hashes, int32_t* uniq, int32_t* counts,
                             void* stream) {
  if (B == 0) return MFPA_OK;
  if (!mask || !landmarks || !hashes || !uniq || !counts || B < 0) return MFPA_EINVAL;
  if (R < 1 || R > 256 || T < 1 || T > 4096 || cap < 1 || cap > SORT_CAP || maxpairs < 1 || maxpairs > CLIP_MAX_PAIRS || mindt < 0) return MFPA_EINVAL;
  const size_t lds = aud_lds(T, pow2_at_least(cap)).total;
  if (lds > 150 * 1024) return MFPA_EINVAL;
  hipLaunchKernelGGL(audfprint_landmarks_kernel, dim3(B), dim3(HT), lds, mfpa_stream(stream), mask, R, T, cap,
                     PairRule{mindt, targetdt, targetdf, maxpairs}, landmarks, hashes, uniq, counts);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_audfprint_landmarks_track(const uint8_t* mask, int B, int R, int T, int cap, int mindt, int targetdt, int targetdf, int maxpairs,
                                   int32_t* tiles, int32_t* landmarks, int32_t* hashes, int32_t* uniq, int32_t* counts, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!mask || !tiles || !uniq || !counts || B < 0) return MFPA_EINVAL;
  if ((landmarks == nullptr) != (hashes == nullptr)) return MFPA_EINVAL;                  // both lists or neither
  if (R < 4 || R > 256 || (R % 4) != 0 || T < 1 || T > MFPA_TRACK_MAX_T || cap < 1) return MFPA_EINVAL;
  if (maxpairs < 1 || maxpairs > MAX_PAIRS || mindt < 0 || targetdt < 1 || targetdt > MAX_TARGETDT || targetdf < 0) return MFPA_EINVAL;
  const int ntiles = (T + TILE_W - 1) / TILE_W;
  const int tile_max = TILE_W * MAXPK * maxpairs;              // most landmarks of a tile
  const int cap_lds = pow2_at_least(cap < tile_max ? cap : tile_max);
  const size_t lds = tile_lds(TILE_W + targetdt - 1, cap_lds).total;   // <= 64 KB of keys + 9 KB of peak lists
  const PairRule q{mindt, targetdt, targetdf, maxpairs};
  hipStream_t s = mfpa_stream(stream);
  hipLaunchKernelGGL(landmarks_tile_kernel<false>, dim3(B, ntiles), dim3(HT), lds, s, mask, R, T, ntiles, cap_lds, q, cap, tiles,
                     (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(tile_scan_kernel, dim3((B + 63) / 64), dim3(64), 0, s, tiles, B, ntiles, cap, counts);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(landmarks_tile_kernel<true>, dim3(B, ntiles), dim3(HT), lds, s, mask, R, T, ntiles, cap_lds, q, cap, tiles,
                     landmarks, hashes, uniq, (const int32_t*)counts);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_dejavu_hashes(const uint8_t* mask, int B, int F, int T, int cap, int peak_cap, int fan, int min_dt, int max_dt,
                       uint8_t* digests, int32_t* t1, int32_t* counts, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!mask || !digests || !t1 || !counts || B < 0) return MFPA_EINVAL;
  if (F < 1 || F > 32767 || T < 1 || T > 32767 || cap < 1 || peak_cap < 1 || peak_cap > 16384 || fan < 1 || fan > 64) return MFPA_EINVAL;
  const size_t lds = sizeof(int) * ((size_t)HT + 2 + T) + sizeof(short) * 2 * (size_t)peak_cap;
  if (lds > 150 * 1024) return MFPA_EINVAL;
  hipLaunchKernelGGL(dejavu_hashes_kernel, dim3(B), dim3(HT), lds, mfpa_stream(stream), mask, F, T, cap, peak_cap, fan, min_dt,
                     max_dt, digests, t1, counts);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
