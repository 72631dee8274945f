// Audfprint on whole tracks for MI355X (gfx950): the peak picker and the landmark / hash kernel without the clip-sized limits of
// audfprint.hip (1500 frames: the pruner's event list in LDS) and hashes.hip (8192 landmarks: one LDS sort per clip).  Up to
// 16384 frames per track -- what the 14 time bits of the hash table hold without wrapping (afp/audfprint/hash_table.py:55 of
// the reference; its find_peaks and peaks2landmarks, peak_extractor.py:236-346, take a file of any length).
//
// Compiled with -ffp-contract=off like audfprint.hip: every float64 value that takes part in a comparison is produced by the same
// un-fused IEEE sequence, so the peak set equals that of mfpa_audfprint_pick / mfpa_audfprint_prepare + mfpa_audfprint_prune bit
// for bit wherever both apply.
//
//   pick_track      : launch 1 = prep_sum_kernel (this translation unit's copy from mfpa_prepsum.h; nothing in it depends on T):
//                     log values frame-major + the node sums of np.mean's pairwise tree, (B, 2 * nchunks) workgroups;
//                     launch 2 = prune_track_kernel: prune_kernel<true> of audfprint.hip with the event list and the frame table
//                     in a per-clip slice of a global workspace instead of LDS (LDS holds the Gaussian row only).
//   landmarks_track : tiles of 256 frames (+ a halo of targetdt - 1 frames of peak lists).  A tile holds <= 256 * 8 * maxpairs
//                     <= 8192 landmarks, so the LDS bitonic sort of hashes.hip holds any tile; the sort key is time << 32 | hash
//                     and a tile owns a contiguous time range, so tiles sorted on their own and written in tile order ARE the
//                     globally sorted list, and duplicates can only meet inside one tile.  Three launches: per-tile counts,
//                     an exclusive scan over the tiles of a clip, emission at those offsets (the tile is computed again).
//                     The launches are ordered by the stream: no workgroup reads what another wrote in the same launch.
#include "mfpa_common.h"
#include "mfpa_fastlog.h"
#include "mfpa_npsum.h"
#include "mfpa_prepsum.h"

namespace {

using namespace mfpa_np;
using namespace mfpa_prepsum;

constexpr int TRACK_MAX_T = 16384;   // frame times below 2^14 are stored in the hash table without wrapping
constexpr int MAXP = 8;

// ---------------------------------------------------------------------------------------------- prune
// best_of / readlane_f64 / dpp_f64 / wave_best: as in audfprint.hip (kept there untouched; ~40 lines repeated here)
struct Best {
  double v;
  int p;
};

// lexicographic max on (value, bin); p < 0 means "none"
__device__ __forceinline__ Best best_of(Best a, Best b) {
  const bool take_b = (a.p < 0) || (b.p >= 0 && (b.v > a.v || (b.v == a.v && b.p > a.p)));
  return Best{take_b ? b.v : a.v, take_b ? b.p : a.p};      // field by field: a struct select goes through scratch memory
}

// v of lane `src` (wave-uniform index) through v_readlane: a scalar-path broadcast
__device__ __forceinline__ double readlane_f64(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// One-lane wavefront shifts as DPP moves (GFX9 wave_shr:1 / wave_shl:1): no LDS crossbar round trip.
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false),
                          __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false));
}

// Wavefront arg-max on (value, bin): the candidates are visited one by one from the ballot mask.  The result is wave-uniform.
__device__ __forceinline__ Best wave_best(Best x) {
  unsigned long long m = __ballot(x.p >= 0);
  Best best{0.0, -1};
  while (m) {
    const int src = __ffsll((long long)m) - 1;
    m &= m - 1;
    best = best_of(best, Best{readlane_f64(x.v, src), __builtin_amdgcn_readlane(x.p, src)});
  }
  return best;
}

// One wavefront per clip, the frames walked one after the other, exactly as prune_kernel<true> (audfprint.hip; the comment there
// explains the frame step): `logs` holds the LOG values frame-major with pitch R + 1 (prep_sum_kernel, fm = 1) and the kernel applies
// "minus mean, 1-pole high-pass along the frames" itself while it walks the frames forward.  What differs:
//   * the mean is formed from the chunk sums at the stride the launcher passes (2 * nchunks doubles per clip, up to 514 chunks);
//   * the event list (ev: value, ep: frame << 8 | bin, sign bit = pruned) and the frame table fs (int: up to 81920 entries) live in
//     global memory: ev / ep [B][T * maxpks], fs [B][T + 2].  Only this wavefront touches its clip's slice.  The backward pass reads
//     what the forward pass wrote behind the workgroup barrier between the passes (which drains the wave's stores), the emission
//     what the backward pass wrote behind the second one; the same-frame read-modify-write of `ep` in the backward pass concerns
//     entries of frames c and c + 1 only, while the loads in flight are those of frame c - 1.
__global__ __launch_bounds__(64) void prune_track_kernel(const double* __restrict__ logs, int R, int T,
                                                         const double* __restrict__ gauss, double a_dec, int maxpks,
                                                         uint8_t* __restrict__ mask, int32_t* __restrict__ npeaks,
                                                         const double* __restrict__ node_sums, long long sum_stride,
                                                         const double* __restrict__ denom, double pole,
                                                         double* ev_all, int* ep_all, int* fs_all) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int cap = T * maxpks;                                  // most peaks a clip can record
  double* G = reinterpret_cast<double*>(smem);                 // [2R+2]

  const int lane = threadIdx.x, b = blockIdx.x;
  double* ev = ev_all + (size_t)b * cap;                       // [cap] peak values, in recording order (frame, then rank)
  int* ep = ep_all + (size_t)b * cap;                          // [cap] frame << 8 | bin; sign bit set = pruned
  int* fs = fs_all + (size_t)b * (T + 2);                      // [T + 2] first entry of every frame, fs[T] = number of entries
  const int P = R + 1;                                         // pitch of a frame
  const double* S = logs + (size_t)b * T * P;
  const int k0 = 4 * lane;
  double mean = 0.0, zf[4] = {0.0, 0.0, 0.0, 0.0}, lastcol[4] = {0.0, 0.0, 0.0, 0.0};
  const double npole = -pole;
  if (denom[b] > 0.0) {                                        // np.mean: acc = 0; acc += pairwise(chunk) for every chunk; / N
    const int N = (R + 1) * T, nchunks = (N + NPY_BUFSIZE - 1) / NPY_BUFSIZE;
    double total = 0.0;
    for (int c = 0; c < nchunks; ++c) {
      const int cn = min(NPY_BUFSIZE, N - c * NPY_BUFSIZE);
      const double* h = node_sums + (size_t)b * sum_stride + 2 * c;
      total = total + (cn > PW_BLOCK ? h[0] + h[1] : h[0]);
    }
    mean = total / (double)N;
  }
  // y[n] = x[n] + z; z = -x[n] - (-pole) * y[n] on this lane's four bins (scipy lfilter, DF-II transposed), x = log value - mean
  auto filt = [&](double (&v)[4], double (&z)[4]) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      const double xn = v[q4] - mean;
      const double yn = xn + z[q4];
      z[q4] = -xn - npole * yn;
      v[q4] = yn;
    }
  };
  const bool own = k0 < R;  // R % 4 == 0: a lane owns 4 bins or none

  for (int i = lane; i < 2 * R + 1; i += 64) G[i] = gauss[i];
  __syncthreads();

  // Unconditional loads from clamped addresses (frames past the end re-read frame T - 1, lanes without bins read bins 0..3; neither is
  // ever used), see prune_kernel
  const double* Sk = S + (own ? k0 : 0);
  auto load_col = [&](int c, double (&v)[4]) {
    const int cc = c < T ? c : T - 1;
    const double* q = Sk + (size_t)cc * P;                     // pitch R + 1 doubles: 8-byte aligned only
    v[0] = q[0]; v[1] = q[1]; v[2] = q[2]; v[3] = q[3];
  };
  // locmax flags of a column held 4 bins per lane (peak_extractor.py:61-73)
  auto locmax4 = [&](const double (&v)[4], bool (&pk)[4]) {
    const double left = dpp_f64<0x138>(v[3]);   // wave_shr:1 -> lane - 1's value: bin k0-1 (lane 0 keeps its own, unused)
    const double right = dpp_f64<0x130>(v[0]);  // wave_shl:1 -> lane + 1's value: bin k0+4 (lane 63: unused)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = k0 + s;
      const double lft = (s == 0) ? left : v[s - 1];
      const double rgt = (s == 3) ? right : v[s + 1];
      const bool ge_prev = (k == 0) || (v[s] >= lft);
      const bool nxt_ge = (k < R - 1) && (rgt >= v[s]);
      pk[s] = own && ge_prev && !nxt_ge;
    }
  };
  double th[4];
  // th[k] = max(th[k], val * G[k - p + R]) for this lane's bins
  auto raise = [&](double val, int p) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (own) {
        const double g = val * G[R - p + k0 + s];
        th[s] = g > th[s] ? g : th[s];
      }
    }
  };
  // spreadpeaksinvector(vec, f_sd): zeros raised by every local maximum of vec
  auto spread_init = [&](const double (&v)[4]) {
    bool pk[4];
    locmax4(v, pk);
#pragma unroll
    for (int s = 0; s < 4; ++s) th[s] = 0.0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      unsigned long long m = __ballot(pk[s]);
      while (m) {
        const int src = __ffsll((long long)m) - 1;
        m &= m - 1;
        const double val = readlane_f64(v[s], src);
        raise(val, 4 * src + s);
      }
    }
  };
  int ne = 0;                                                  // entries recorded so far (wave-uniform, <= cap: <= maxpks per frame)
  auto record = [&](int c, double val, int p) {
    ev[ne] = val;                                              // every lane stores the same (wave-uniform) value to the same address
    ep[ne] = (c << 8) | p;
    ++ne;
  };

  // ---- forward pass (peak_extractor.py:173-204)
  {
    double v10[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    const int n10 = T < 10 ? T : 10;
    double z10[4] = {0.0, 0.0, 0.0, 0.0};                      // the filter over the first frames, run again from zero by the main loop
    for (int c = 0; c < n10; ++c) {
      double v[4];
      load_col(c, v);
      filt(v, z10);
#pragma unroll
      for (int s = 0; s < 4; ++s) v10[s] = v[s] > v10[s] ? v[s] : v10[s];
    }
    spread_init(v10);
  }
  double cur[4][4], nxt[4][4];
#pragma unroll
  for (int q = 0; q < 4; ++q) load_col(q, cur[q]);
  for (int c0 = 0; c0 < T; c0 += 4) {
#pragma unroll
    for (int q = 0; q < 4; ++q) load_col(c0 + 4 + q, nxt[q]);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + q;
      if (c < T) {
        filt(cur[q], zf);
        if (c == T - 1) {
#pragma unroll
          for (int s = 0; s < 4; ++s) lastcol[s] = cur[q][s];
        }
        fs[c] = ne;                                              // (uniform store, as in record)
        bool ex[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) ex[s] = own && (cur[q][s] > th[s]);    // against the pre-update threshold
        if (__ballot(ex[0] || ex[1] || ex[2] || ex[3]) != 0ull) {           // else: no candidate in this frame, whatever locmax says
          bool cand[4];
          locmax4(cur[q], cand);
          unsigned long long m[4];
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            cand[s] = cand[s] && ex[s];
            m[s] = __ballot(cand[s]);
          }
          const int total = __popcll(m[0]) + __popcll(m[1]) + __popcll(m[2]) + __popcll(m[3]);
          if (total == 1) {                                                  // the common case: take it from the masks
            const int s1 = m[0] ? 0 : (m[1] ? 1 : (m[2] ? 2 : 3));
            const unsigned long long mm = m[0] | m[1] | m[2] | m[3];
            const int src = __ffsll((long long)mm) - 1;
            const double sel = s1 == 0 ? cur[q][0] : (s1 == 1 ? cur[q][1] : (s1 == 2 ? cur[q][2] : cur[q][3]));
            const double val = readlane_f64(sel, src);
            const int p = 4 * src + s1;
            raise(val, p);
            record(c, val, p);
          } else if (total > 1) {
            int cnt = 0;
            while (cnt < maxpks) {
              Best mine{0.0, -1};
#pragma unroll
              for (int s = 0; s < 4; ++s)
                if (cand[s]) mine = best_of(mine, Best{cur[q][s], k0 + s});
              if (__ballot(mine.p >= 0) == 0ull) break;
              const Best w = wave_best(mine);
              raise(w.v, w.p);
#pragma unroll
              for (int s = 0; s < 4; ++s)
                if (k0 + s == w.p) cand[s] = false;
              record(c, w.v, w.p);
              ++cnt;
            }
          }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) th[s] = th[s] * a_dec;
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int s = 0; s < 4; ++s) cur[q][s] = nxt[q][s];
  }
  fs[T] = ne;
  fs[T + 1] = ne;
  __syncthreads();                                             // the forward pass's stores to ev / ep / fs are complete

  // ---- backward pass (peak_extractor.py:206-234)
  spread_init(lastcol);
  // entries of a frame in lanes 0..7: (value, frame << 8 | bin, entry index); -1 bin = none / pruned
  auto fetch = [&](int start, int n, double& fv, int& fp) {
    fv = 0.0; fp = -1;
    if (lane < n) { fv = ev[start + lane]; fp = ep[start + lane]; }
  };
  auto ufs = [&](int i) { return __builtin_amdgcn_readfirstlane(fs[i]); };           // wave-uniform table cell
  int st_c = ufs(T - 1), st_c1 = ufs(T);                       // frame T-1: entries [st_c, st_c1)
  double cv; int cp;
  fetch(st_c, st_c1 - st_c, cv, cp);
  int st_n = T >= 2 ? ufs(T - 2) : 0;                          // frame T-2 starts here (its end is st_c)
  int prev_p = -1, prev_idx = 0;                               // frame c+1's entries in lanes 0..7 (bin, entry index), -1 = none
  for (int c = T - 1; c >= 0; --c) {
    const int n = st_c1 - st_c;
    // requests for the next iterations go out first: entries of frame c-1, the table cell of frame c-2
    double nv = 0.0; int np = -1;
    if (c >= 1) fetch(st_n, st_c - st_n, nv, np);
    const int st_nn_raw = c >= 2 ? fs[c - 2] : 0;              // consumed (made uniform) at the end of the iteration
    int my_p = (lane < n) ? (cp & 255) : -1;                   // this frame's bins (lane i = rank i), -1 once pruned
    for (int i = 0; i < n; ++i) {
      const double val = readlane_f64(cv, i);
      const int p = __builtin_amdgcn_readlane(cp, i) & 255;    // wave-uniform
      const int s_sel = p & 3;
      const double mine = s_sel == 0 ? th[0] : (s_sel == 1 ? th[1] : (s_sel == 2 ? th[2] : th[3]));
      const double thp = readlane_f64(mine, p >> 2);
      if (val >= thp) {
        raise(val, p);
        if (prev_p == p) {                                     // delete any following peak in the same bin (frame c+1)
          ep[prev_idx] |= (int)0x80000000;
          prev_p = -1;
        }
      } else if (lane == i) {
        ep[st_c + i] = cp | (int)0x80000000;
        my_p = -1;
      }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) th[s] = a_dec * th[s];
    prev_p = my_p; prev_idx = st_c + lane;
    st_c1 = st_c; st_c = st_n; st_n = __builtin_amdgcn_readfirstlane(st_nn_raw);
    cv = nv; cp = np;
  }
  __syncthreads();                                             // the backward pass's marks in ep are complete

  // ---- emit: mask (R, T) uint8 was zeroed by the launcher's memset on the same stream
  uint8_t* M = mask + (size_t)b * R * T;
  int count = 0;
  for (int e = lane; e < ne; e += 64) {
    const int pe = ep[e];
    if (pe >= 0) {
      M[(size_t)(pe & 255) * T + (pe >> 8)] = 1;
      ++count;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) count += __shfl_xor(count, o);
  if (lane == 0) npeaks[b] = count;
}

// ---------------------------------------------------------------------------------------------- landmarks
constexpr int HT = 256;            // threads = frames of a tile
constexpr int TILE_W = HT;
constexpr int MAXPK = 8;           // peaks per frame (the pruner keeps <= 8)
constexpr int MAX_PAIRS = 4;       // 256 * 8 * 4 = 8192 landmarks per tile at the most
constexpr int MAX_TARGETDT = 256;  // halo frames of peak lists per tile: targetdt - 1

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

// exclusive scan over HT threads; sh[HT + 1]; the total in sh[HT]
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

// One tile of one clip: frames [t0, t0 + 256) pair with frames < t0 + 256 + targetdt - 1 (peak_extractor.py:313-346; `scols` there is only
// a loop bound -- frames beyond the last peak hold no peaks -- so the clip's frame count serves).
// EMIT = false: tiles[b][tile] = {landmarks, unique rows} of the tile; landmarks = -1 when a frame of the tile holds more than 8 peaks.
// EMIT = true : tiles[b][tile] holds the tile's offsets {first landmark, first unique row} (tile_scan_kernel); the landmarks and
//               hashes go out in list order (skipped when the pointers are null), the unique rows sorted; a flagged clip (counts[2b] < 0)
//               writes nothing.
template <bool EMIT>
__global__ __launch_bounds__(HT) void landmarks_tile_kernel(const uint8_t* __restrict__ mask, int R, int T, int ntiles, int cap_lds,
                                                            int mindt, int targetdt, int targetdf, int maxpairs, int cap,
                                                            int32_t* __restrict__ tiles, int32_t* __restrict__ landmarks,
                                                            int32_t* __restrict__ hashes, int32_t* __restrict__ uniq,
                                                            const int32_t* __restrict__ counts) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nfr_max = TILE_W + targetdt - 1;
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
  const uint8_t* M = mask + (size_t)b * R * T + t0;
  if (tid == 0) sh[HT + 1] = 0;
  __syncthreads();

  // per-frame peak lists (bins ascending): thread = frame, consecutive threads read consecutive bytes of a bin row
  for (int c = tid; c < nfr; c += HT) {
    int n = 0;
    for (int r = 0; r < R; ++r) {
      if (M[(size_t)r * T + c]) {
        if (n < MAXPK) pk[c * MAXPK + n] = (short)r;
        ++n;
      }
    }
    if (n > MAXPK) {
      if (c < nown) atomicOr(&sh[HT + 1], 1);                    // (a halo frame is flagged by the tile that owns it)
      n = MAXPK;
    }
    npk[c] = (short)n;
  }
  __syncthreads();
  if (sh[HT + 1]) {
    if (!EMIT && tid == 0) { tc[0] = -1; tc[1] = 0; }
    return;                                                      // (EMIT: unreachable, the clip is flagged)
  }

  // landmarks of peak i of (tile-relative) frame c, scanning col2 then bin2 ascending
  auto pairs_of = [&](int c, int i, int32_t* out /* nullable */) {
    const int p = pk[c * MAXPK + i];
    int pairs = 0;
    const int c_end = min(nfr, c + targetdt);
    for (int c2 = c + mindt; c2 < c_end && pairs < maxpairs; ++c2) {
      const int n2 = npk[c2];
      for (int k = 0; k < n2 && pairs < maxpairs; ++k) {
        const int p2 = pk[c2 * MAXPK + k];
        const int d = p2 - p;
        if ((d < 0 ? -d : d) < targetdf) {
          if (out) { out[4 * pairs] = t0 + c; out[4 * pairs + 1] = p; out[4 * pairs + 2] = p2; out[4 * pairs + 3] = c2 - c; }
          ++pairs;
        }
      }
    }
    return pairs;
  };
  // thread = frame: the scan over the threads yields list order
  int mine = 0;
  if (tid < nown)
    for (int i = 0; i < npk[tid]; ++i) mine += pairs_of(tid, i, nullptr);
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
      const int n = pairs_of(tid, i, tmp);
      for (int k = 0; k < n; ++k) {
        const int e = off + k;
        const int32_t h = ((tmp[4 * k + 1] & 255) << 12) | (((tmp[4 * k + 2] - tmp[4 * k + 1]) & 63) << 6) | (tmp[4 * k + 3] & 63);
        if (lists) {
          int32_t* LM = landmarks + (lm0 + e) * 4;
          int32_t* HS = hashes + (lm0 + e) * 2;
          LM[0] = tmp[4 * k]; LM[1] = tmp[4 * k + 1]; LM[2] = tmp[4 * k + 2]; LM[3] = tmp[4 * k + 3];
          HS[0] = tmp[4 * k];
          HS[1] = h;
        }
        keys[e] = ((unsigned long long)(unsigned)tmp[4 * k] << 32) + (unsigned long long)(unsigned)h;
      }
      off += n;
    }
  }
  __syncthreads();
  // bitonic sort of npow keys in LDS
  for (int k = 2; k <= npow; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < npow; i += HT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a = keys[i], c = keys[ixj];
          const bool up = ((i & k) == 0);
          if ((a > c) == up) { keys[i] = c; keys[ixj] = a; }
        }
      }
      __syncthreads();
    }
  }
  // unique compaction (keys sorted ascending; padding = ~0 never equals a real key)
  {
    const int per = (total + HT - 1) / HT;
    const int i0 = min(total, tid * per), i1 = min(total, i0 + per);
    int cnt = 0;
    for (int i = i0; i < i1; ++i) cnt += (i == 0 || keys[i] != keys[i - 1]);
    int uoff = tile_excl_scan(cnt, sh, tid);
    if (EMIT) {
      int32_t* UQ = uniq + uq0 * 2;
      for (int i = i0; i < i1; ++i) {
        if (i == 0 || keys[i] != keys[i - 1]) {
          UQ[2 * uoff] = (int32_t)(keys[i] >> 32);
          UQ[2 * uoff + 1] = (int32_t)(keys[i] & 0xFFFFFFFFull);
          ++uoff;
        }
      }
    } else if (tid == 0) {
      tc[0] = total;
      tc[1] = sh[HT];
    }
  }
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

}  // namespace

extern "C" {

int mfpa_audfprint_pick_track(const double* spec, const double* clip_max, int B, int F, int T, double pole, const double* gauss,
                              double a_dec, int maxpks, double* logs, double* sums, void* events, uint8_t* mask, int32_t* npeaks,
                              void* stream) {
  if (B == 0) return MFPA_OK;
  if (!spec || !clip_max || !gauss || !logs || !sums || !events || !mask || !npeaks || B < 0) return MFPA_EINVAL;
  const int R = F - 1;
  if (F < 141 || F > 257 || (R % 4) != 0 || T < 1 || T > TRACK_MAX_T || maxpks < 1 || maxpks > MAXP) return MFPA_EINVAL;   // (F >= 141: a half-chunk node spans <= 32 frames)
  if ((reinterpret_cast<uintptr_t>(events) & 7) != 0) return MFPA_EINVAL;
  const long long N = (long long)F * T;                        // <= 257 * 16384: int arithmetic in the kernels holds
  const int nchunks = (int)((N + NPY_BUFSIZE - 1) / NPY_BUFSIZE);
  hipStream_t s = mfpa_stream(stream);
  MFPA_HIP(hipMemsetAsync(mask, 0, (size_t)B * R * T, s));
  const size_t lds1 = sizeof(double) * (NPY_BUFSIZE / 2 + 8 + HEAP + 128 * 3);
  hipLaunchKernelGGL(prep_sum_kernel, dim3(B, 2 * nchunks), dim3(SPLIT_THREADS), lds1, s, spec, F, T, clip_max, 1, logs, 1, sums,
                     (long long)(2 * nchunks), 1.0, F - 1);
  MFPA_CHECK_LAUNCH();
  const size_t cap = (size_t)T * maxpks;
  double* ev = reinterpret_cast<double*>(events);              // [B][cap]
  int* ep = reinterpret_cast<int*>(ev + (size_t)B * cap);      // [B][cap]
  int* fs = ep + (size_t)B * cap;                              // [B][T + 2]
  hipLaunchKernelGGL(prune_track_kernel, dim3(B), dim3(64), sizeof(double) * (2 * R + 2), s, (const double*)logs, R, T, gauss, a_dec, maxpks, mask,
                     npeaks, (const double*)sums, (long long)(2 * nchunks), clip_max, pole, ev, ep, fs);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

int mfpa_audfprint_landmarks_track(const uint8_t* mask, int B, int R, int T, int cap, int mindt, int targetdt, int targetdf, int maxpairs,
                                   int32_t* tiles, int32_t* landmarks, int32_t* hashes, int32_t* uniq, int32_t* counts, void* stream) {
  if (B == 0) return MFPA_OK;
  if (!mask || !tiles || !uniq || !counts || B < 0) return MFPA_EINVAL;
  if ((landmarks == nullptr) != (hashes == nullptr)) return MFPA_EINVAL;                  // both lists or neither
  if (R < 4 || R > 256 || (R % 4) != 0 || T < 1 || T > TRACK_MAX_T || cap < 1) return MFPA_EINVAL;
  if (maxpairs < 1 || maxpairs > MAX_PAIRS || mindt < 0 || targetdt < 1 || targetdt > MAX_TARGETDT || targetdf < 0) return MFPA_EINVAL;
  const int ntiles = (T + TILE_W - 1) / TILE_W;
  const int tile_max = TILE_W * MAXPK * maxpairs;              // most landmarks of a tile
  const int cap_lds = pow2_at_least(cap < tile_max ? cap : tile_max);
  const size_t lds = tile_lds(TILE_W + targetdt - 1, cap_lds).total;   // <= 64 KB of keys + 9 KB of peak lists
  hipStream_t s = mfpa_stream(stream);
  hipLaunchKernelGGL(landmarks_tile_kernel<false>, dim3(B, ntiles), dim3(HT), lds, s, mask, R, T, ntiles, cap_lds, mindt, targetdt, targetdf,
                     maxpairs, cap, tiles, (int32_t*)nullptr, (int32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(tile_scan_kernel, dim3((B + 63) / 64), dim3(64), 0, s, tiles, B, ntiles, cap, counts);
  MFPA_CHECK_LAUNCH();
  hipLaunchKernelGGL(landmarks_tile_kernel<true>, dim3(B, ntiles), dim3(HT), lds, s, mask, R, T, ntiles, cap_lds, mindt, targetdt, targetdf,
                     maxpairs, cap, tiles, landmarks, hashes, uniq, (const int32_t*)counts);
  MFPA_CHECK_LAUNCH();
  return MFPA_OK;
}

}  // extern "C"
