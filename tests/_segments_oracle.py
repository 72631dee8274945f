"""numpy restatement of the segment stage (csrc/segments.hip), written from the reference's semantics
(training/dataset.py:55-122): framing without end padding, exact sums of squares, the keep rule in float64, the
(key, index) selection and the float32 peak division; plus the reference's own float32 formula for comparison, and the input
generator the GPU tests share."""
import math

import numpy as np

DBS = -7.5
MAX_PER_TRACK = 8192


def frame_samples(dur, step_per_cent, sr):
    """(L, S) as dataset.py:75-82 forms them: int(float32(x) * float32(sr))."""
    L = int(np.float32(dur) * np.float32(sr))
    S = int(np.float32(dur * step_per_cent) * np.float32(sr))
    return L, S


def n_frames(N, L, S):
    return 1 + (N - L) // S if N >= L else 0


def geometry(lengths, L, S):
    """Exclusive prefix of the segments per track, or None where the C entry point refuses."""
    if L < 1 or S < 1 or any(n < 0 for n in lengths):
        return None
    nf = [n_frames(int(n), L, S) for n in lengths]
    if any(f > MAX_PER_TRACK for f in nf) or sum(nf) > 2 ** 31 - 1:
        return None
    return np.concatenate([[0], np.cumsum(nf)]).astype(np.int64)


def sumsq(x):
    """Exact (correctly rounded) sum of the float64 squares; the square of a float32 is exact in float64."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    return math.fsum((x * x).tolist())


def stats(x, L, S):
    """(seg_sumsq (nf,), trk_sumsq, trk_peak) of one track."""
    x = np.asarray(x, dtype=np.float32)
    nf = n_frames(len(x), L, S)
    seg = np.array([sumsq(x[j * S: j * S + L]) for j in range(nf)], dtype=np.float64)
    peak = np.float32(np.max(np.abs(x))) if len(x) else np.float32(0)
    return seg, sumsq(x), peak


def threshold(dbs=DBS):
    return float(np.exp(np.float64(dbs) / 5.0))


def keep(seg_sumsq, trk_sumsq, N, L, dbs=DBS):
    """seg * N > (thr * trk) * L in float64: 10 ln(rms_seg / rms_ref) > dbs without roots and logarithm."""
    seg = np.asarray(seg_sumsq, dtype=np.float64)
    rhs = np.float64(threshold(dbs)) * np.float64(trk_sumsq) * np.float64(L)
    return seg * np.float64(N) > rhs


def margin(seg_sumsq, trk_sumsq, N, L, dbs=DBS):
    """Relative distance of each segment from the threshold: |lhs - rhs| / rhs (inf for an all-zero track)."""
    seg = np.asarray(seg_sumsq, dtype=np.float64)
    rhs = threshold(dbs) * float(trk_sumsq) * L
    if rhs == 0:
        return np.full(seg.shape, np.inf)
    return np.abs(seg * N - rhs) / rhs


def keep_tf32(x, L, S, dbs=DBS):
    """The reference's formula in float32 (select_no_silence_frames): 10 * log(sqrt(mean(seg^2)) / sqrt(mean(x^2))) > dbs, with
    numpy's float32 reductions standing for TensorFlow's (for comparison only: their summation orders differ)."""
    x = np.asarray(x, dtype=np.float32)
    nf = n_frames(len(x), L, S)
    if nf == 0:
        return np.zeros(0, dtype=bool)
    segs = np.stack([x[j * S: j * S + L] for j in range(nf)])
    with np.errstate(divide="ignore", invalid="ignore"):
        rms_ref = np.sqrt(np.mean(np.power(x, np.float32(2)), dtype=np.float32))
        rms_seg = np.sqrt(np.mean(np.power(segs, np.float32(2)), axis=-1, dtype=np.float32))
        dbs_seg = np.float32(10) * np.log(rms_seg / rms_ref)
        return dbs_seg > np.float32(dbs)


def select(keep_mask, keys, n_keep):
    """Local indices of the winners: the kept segments in ascending (key, index) order, the first n_keep; -1 padded."""
    idx = [j for j in range(len(keep_mask)) if keep_mask[j]]
    idx.sort(key=lambda j: (int(keys[j]), j))
    out = np.full(n_keep, -1, dtype=np.int64)
    out[:min(n_keep, len(idx))] = idx[:n_keep]
    return out


def divide(x, peak, do_norm=True):
    x = np.asarray(x, dtype=np.float32)
    return x / np.float32(peak) if (do_norm and peak > 0) else x.copy()


def select_all(tracks, L, S, keys, n_keep, dbs=DBS, sums=None):
    """The whole selection for a list of tracks: (mask (NS,), kept (n,), sel (n * n_keep,) global indices or -1).  `sums`: use these
    (seg_sumsq (NS,), trk_sumsq (n,)) in place of the exact ones."""
    seg_off = geometry([len(t) for t in tracks], L, S)
    mask = np.zeros(int(seg_off[-1]), dtype=bool)
    kept = np.zeros(len(tracks), dtype=np.int64)
    sel = np.full(len(tracks) * n_keep, -1, dtype=np.int64)
    for i, t in enumerate(tracks):
        a, b = int(seg_off[i]), int(seg_off[i + 1])
        if sums is None:
            seg, trk, _ = stats(t, L, S)
        else:
            seg, trk = sums[0][a:b], sums[1][i]
        m = keep(seg, trk, len(t), L, dbs)
        mask[a:b] = m
        kept[i] = int(m.sum())
        loc = select(m, keys[a:b], n_keep)
        sel[i * n_keep:(i + 1) * n_keep] = np.where(loc >= 0, loc + a, -1)
    return mask, kept, sel


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
def make_track(rng, N, L, S):
    """A track of N samples whose segments sit on both sides of the silence threshold, none closer than 1 % to it as built: white
    noise with one gain per frame-sized piece, loud (1), quiet (0.05: -30 dB under a loud track's mean) or exactly silent."""
    x = rng.standard_normal(N).astype(np.float32) * np.float32(0.25)
    pieces = max(1, -(-N // max(L, 1)))
    gains = rng.choice(np.array([1.0, 0.05, 0.0], dtype=np.float32), size=pieces, p=[0.55, 0.3, 0.15])
    gains[rng.integers(pieces)] = 1.0                                     # at least one loud piece: the mean is a loud one's
    g = np.repeat(gains, L)[:N]
    return (x * g).astype(np.float32)


def track_lengths(L):
    return [0, L - 1, L, L + 1, 2 * L - 1, 5 * L + 7]


def make_tracks(seed, L, S, lengths=None):
    rng = np.random.default_rng([seed, L, S])
    return [make_track(rng, N, L, S) for N in (track_lengths(L) if lengths is None else lengths)]


GPU_SHAPES = [(24, 24), (23, 23), (24, 8), (24, 30), (24000, 24000)]
SEED = 4100


def gpu_tracks(L, S):
    """The tracks of tests/test_gpu_segments.py for one (L, S): the edge lengths, an all-zero track, and a track with a segment of
    exact zeros."""
    tracks = make_tracks(SEED, L, S)
    tracks.append(np.zeros(3 * L + 1, dtype=np.float32))
    t = make_tracks(SEED + 1, L, S, [4 * L + 3])[0]
    t[L:2 * L + S] = 0                                                    # segment 1 (S <= L) or the samples segment 1 reads
    t[:L] = np.where(t[:L] == 0, np.float32(0.25), t[:L])
    tracks.append(t)
    return tracks


def long_track():
    """One track of exactly MAX_PER_TRACK segments at (L, S) = (4, 1)."""
    return make_tracks(SEED + 2, 4, 1, [MAX_PER_TRACK + 3])[0]
