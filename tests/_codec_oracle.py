"""Oracle of the lossy-coding kernels (csrc/codec.hip), shared by tests/test_codec_oracle.py (CPU) and tests/test_gpu_codec.py.  The
definitions are those of include/mfpa.h (mfpa_transform_codec, mfpa_mulaw), restated in numpy:

  reference()  in float64, every product and sum in the order of the formula: the pinned reference;
  truth()      the same in numpy's long double (80-bit here): what the formula means.

Transform codec, per row and per frame f of 512 samples at hop M = 256 (the row stands behind M zeros, F = ceil(T / M) + 1 frames):
  X[k]   = sum_n w[n] x_f[n] cos(pi / M (n + 1/2 + M / 2)(k + 1/2)),  w[n] = sin(pi (n + 1/2) / 512); the cosine is taken from a table
           over the exactly reduced argument (2 n + 1 + M)(2 k + 1) mod 8 M, so its error is that of one rounding;
  var_b  = (sum_{k in b} X[k]^2) / W_b in ascending k;  m_b = max_b' var_b' 10^(-a(b, b') / 10);  L_b = log2 var_b - log2 m_b;
  for every band j with var_j > 0:  S_j, P_j = sum W_b, sum W_b L_b over {b : L_b >= L_j} in ascending b;  lam_j = (P_j - 2 R) / S_j,
  admissible if lam_j < L_j;  lam = lam_j of the admissible j with the smallest L_j;  band b is coded iff L_b > lam;
  D_b = m_b 2^lam, step_b = sqrt(12 D_b), t = |X| / step_b, q = floor(t + 1/2), Xq = sign(X) q step_b  (Xq = X where t >= 2^52);
  y_f[n] = (2 / M) w[n] sum_k Xq[k] cos(...), overlap-added, the earlier frame first.
R = +inf: Xq = X, lam = -inf and the count of coded coefficients is 0.

The error convention is the project's: E = max |reference - truth| over a case, D = max |device - truth|, and the bound is D <= 8 E
(BOUND); where E == 0 the device must give the reference's bits.  errors() returns (D, E).

The codec takes discrete decisions (a rounding per coefficient, a band in or out, a candidate admissible or not).  The device and
the oracle agree on them only where no decision hangs on a rounding error, so every case the GPU tests use must keep every decision
at least MARGIN away from its threshold in the reference (tests/test_codec_oracle.py holds the cases to that): a condition on the
inputs, not a tolerance."""
import functools
import math

import numpy as np

M = 256
N = 2 * M
BOUND = 8.0
MARGIN = 1e-9
SAMPLE_RATE = 8000
SIDE_BITS = 6
DEFAULT_EDGES = (0, 4, 8, 12, 16, 20, 24, 30, 36, 44, 52, 62, 74, 88, 104, 124, 148, 176, 208, 256)
UP_DB, DOWN_DB = 10.0, 25.0
RATES = (6.0, 8.0, 16.0, 32.0, 64.0)                 # kbit/s; one per row of the five-row case
PI_L = np.longdouble(4.0) * np.arctan(np.longdouble(1.0))


def lengths(G: int):
    """The shapes of the GPU tests; G = frames per workgroup (MFPA_CODEC_FRAMES)."""
    return (1, 255, 256, 257, 513, G * M - 1, G * M + 1, 2 * G * M + 1)


def n_frames(T: int) -> int:
    return (T + M - 1) // M + 1


def budget(kbps, sample_rate=SAMPLE_RATE, side_bits=SIDE_BITS, n_bands=len(DEFAULT_EDGES) - 1):
    """R = kbps 1000 M / sample_rate - side_bits n_bands, in float64 and in this order."""
    return np.asarray(kbps, dtype=np.float64) * 1000.0 * 256.0 / float(sample_rate) - float(side_bits * n_bands)


# ---------------------------------------------------------------------------------------------------------------------------------
# named cases
def two_tones(T: int, seed: int = 0, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """0.5 sin(2 pi 440 t) + 0.2 sin(2 pi 1234.5 t) + 0.05 N(0, 1)."""
    rng = np.random.default_rng(seed)
    t = np.arange(T) / sample_rate
    return 0.5 * np.sin(2.0 * np.pi * 440.0 * t) + 0.2 * np.sin(2.0 * np.pi * 1234.5 * t) + 0.05 * rng.standard_normal(T)


def impulse(T: int) -> np.ndarray:
    x = np.zeros(T)
    x[min(T - 1, 300)] = 0.75
    return x


def silence(T: int) -> np.ndarray:
    return np.zeros(T)


def five_rows(T: int, seed: int = 0) -> np.ndarray:
    """Five rows of two_tones with different seeds and amplitudes; coded at RATES, one per row."""
    return np.stack([(1.0 - 0.15 * r) * two_tones(T, seed=seed + 1 + r) for r in range(5)])


# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tables(dtype):
    """(w (512,), C (512, 256)).  The cosine table holds cos(2 pi j / 8 M), j < 8 M, from arguments inside [0, pi / 4] in long double
    (symmetries applied to the integer j), rounded once to dtype."""
    Q = 8 * M
    j = np.arange(Q)
    jq = j % (Q // 4)                                   # position inside the quadrant, quadrant = j // (Q / 4)
    quad = j // (Q // 4)
    first = np.where(jq <= Q // 8, np.cos(2 * PI_L * jq.astype(np.longdouble) / Q), np.sin(2 * PI_L * (Q // 4 - jq).astype(np.longdouble) / Q))
    sinq = np.where(jq <= Q // 8, np.sin(2 * PI_L * jq.astype(np.longdouble) / Q), np.cos(2 * PI_L * (Q // 4 - jq).astype(np.longdouble) / Q))
    table = np.select([quad == 0, quad == 1, quad == 2, quad == 3], [first, -sinq, -first, sinq]).astype(dtype)
    n = np.arange(N)
    k = np.arange(M)
    C = table[((2 * n[:, None] + 1 + M) * (2 * k[None, :] + 1)) % Q]
    if dtype is np.float64:
        w = np.sin(np.pi * (n + 0.5) / 512.0)
    else:
        w = np.sin(PI_L * (n.astype(dtype) + dtype(0.5)) / dtype(512.0))
    return w, C


def spread_factors(n_bands: int, up_db: float, down_db: float, dtype=np.float64) -> np.ndarray:
    """fac[b, b'] = 10^(-a(b, b') / 10): a = up_db (b - b') for b >= b', down_db (b' - b) otherwise.  The host makes them in float64
    (fac[b, b] is exactly 1); truth() takes the same doubles."""
    d = np.arange(n_bands)[:, None] - np.arange(n_bands)[None, :]
    a = np.where(d >= 0, float(up_db) * d, float(down_db) * -d).astype(np.float64)
    return np.power(10.0, -a / 10.0).astype(dtype)


def _frames(x, dtype):
    B, T = x.shape
    F = n_frames(T)
    pad = np.zeros((B, (F + 1) * M), dtype=dtype)
    pad[:, M:M + T] = x
    return np.stack([pad[:, f * M:f * M + N] for f in range(F)], axis=1)        # (B, F, 512)


def _allocate(X, R, edges, fac, dtype, margins):
    """One frame: X (256,), R a float.  Returns (Xq, lam, coded)."""
    nb = len(edges) - 1
    if math.isinf(R) and R > 0:
        return X.copy(), dtype(-np.inf), 0
    W = np.array([edges[b + 1] - edges[b] for b in range(nb)], dtype=dtype)
    var = np.zeros(nb, dtype=dtype)
    for b in range(nb):
        s = dtype(0.0)
        for k in range(edges[b], edges[b + 1]):
            s = s + X[k] * X[k]
        var[b] = s / W[b]
    m = np.max(var[None, :] * fac, axis=1)
    live = var > 0
    Xq = np.zeros_like(X)
    if not live.any():
        return Xq, dtype(np.nan), 0
    with np.errstate(divide="ignore", invalid="ignore"):
        L = np.log2(var) - np.log2(m)
    lam, best = None, None
    for j in range(nb):
        if not live[j]:
            continue
        S, P = dtype(0.0), dtype(0.0)
        for b in range(nb):
            if live[b] and L[b] >= L[j]:
                S = S + W[b]
                P = P + W[b] * L[b]
        lj = (P - dtype(2.0) * dtype(R)) / S
        if margins is not None:
            margins.append(abs(float(L[j] - lj)))
            margins.extend(abs(float(L[b] - L[j])) for b in range(nb) if live[b] and L[b] != L[j])
        if lj < L[j] and (best is None or L[j] < best):
            lam, best = lj, L[j]
    if lam is None:
        return Xq, dtype(np.nan), 0
    count = 0
    for b in range(nb):
        if not live[b]:
            continue
        if margins is not None:
            margins.append(abs(float(L[b] - lam)))
        if not L[b] > lam:
            continue
        step = np.sqrt(dtype(12.0) * (m[b] * np.exp2(lam)))
        seg = X[edges[b]:edges[b + 1]]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            t = np.abs(seg) / step
            q = np.floor(t + dtype(0.5))
            v = np.sign(seg) * q * step
        fine = ~(t < dtype(2.0 ** 52))
        v = np.where(fine, seg, v)
        q = np.where(fine, np.abs(seg), q)
        if margins is not None and (~fine).any():
            r = (t + dtype(0.5))[~fine]
            fr = r - np.floor(r)
            margins.append(float(np.min(np.minimum(fr, dtype(1.0) - fr))))
        Xq[edges[b]:edges[b + 1]] = v
        count += int(np.count_nonzero(q))
    return Xq, lam, count


def _run(x, R, edges, up_db, down_db, dtype, margins=None):
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x).astype(dtype)
    B, T = x.shape
    R = np.broadcast_to(np.asarray(R, dtype=np.float64), (B,))
    edges = tuple(int(e) for e in (DEFAULT_EDGES if edges is None else edges))
    fac = spread_factors(len(edges) - 1, up_db, down_db, dtype)
    w, C = _tables(dtype)
    fr = _frames(x, dtype)
    F = fr.shape[1]
    X = (fr * w) @ C                                                             # (B, F, 256)
    Xq = np.empty_like(X)
    lam = np.empty((B, F), dtype=dtype)
    coded = np.zeros((B, F), dtype=np.int32)
    for b in range(B):
        for f in range(F):
            Xq[b, f], lam[b, f], coded[b, f] = _allocate(X[b, f], float(R[b]), edges, fac, dtype, margins)
    yf = (dtype(2.0) / dtype(M)) * (w * (Xq @ C.T))                              # (B, F, 512)
    y = (yf[:, :-1, M:] + yf[:, 1:, :M]).reshape(B, -1)[:, :T]
    return (y[0], lam[0], coded[0]) if one else (y, lam, coded)


def reference(x, R, edges=None, up_db=UP_DB, down_db=DOWN_DB):
    """(y, lam, coded) in float64; x (T,) or (B, T), R a float or (B,) (bits per frame, +inf = lossless)."""
    return _run(x, R, edges, up_db, down_db, np.float64)


def truth(x, R, edges=None, up_db=UP_DB, down_db=DOWN_DB):
    """The same in long double, from the same float64 inputs."""
    return _run(x, R, edges, up_db, down_db, np.longdouble)


def decision_margin(x, R, edges=None, up_db=UP_DB, down_db=DOWN_DB) -> float:
    """The smallest distance of any discrete decision of reference(x, R) from its threshold: the rounding of every coded coefficient
    (distance of |X| / step + 1/2 from an integer), |L_b - lam| over the bands that are in, |L_j - lam_j| over the candidates and
    |L_b - L_j| between bands of different L (the membership of the candidate sets).  inf where nothing is decided."""
    margins = []
    _run(x, R, edges, up_db, down_db, np.float64, margins)
    return min(margins) if margins else math.inf


def errors(y, want):
    """(D, E) of an output: D = max |y - truth|, E = max |reference - truth|; want = (truth, reference) of the same shape."""
    t, r = want
    return float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - t))), float(np.max(np.abs(np.asarray(r, dtype=np.longdouble) - t)))


def snr_db(x, y) -> float:
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    return float(10.0 * np.log10(np.sum(x * x) / np.sum((x - y) ** 2)))


# ---------------------------------------------------------------------------------------------------------------------------------
# mu-law (torchaudio's mu_law_encoding / mu_law_decoding formulas)
def _mulaw_arg(x, channels, dtype):
    mu = dtype(channels - 1)
    x = np.clip(np.asarray(x, dtype=np.float64).astype(dtype), dtype(-1.0), dtype(1.0))
    c = np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu)
    return (c + dtype(1.0)) / dtype(2.0) * mu + dtype(0.5)


def mulaw_encode(x, channels=256, dtype=np.float64):
    return np.floor(_mulaw_arg(x, channels, dtype)).astype(np.int64)


def mulaw_decode(codes, channels=256, dtype=np.float64):
    mu = dtype(channels - 1)
    v = dtype(2.0) * np.asarray(codes).astype(dtype) / mu - dtype(1.0)
    return np.sign(v) * (np.exp(np.abs(v) * np.log1p(mu)) - dtype(1.0)) / mu


def mulaw_margin(x, channels=256) -> float:
    """The distance of the encoder's floor argument from an integer.  Exact zeros are left out: log1p(0) is exactly 0, so their
    argument is mu / 2 + 1 / 2 without a rounding on any machine."""
    x = np.asarray(x, dtype=np.float64)
    a = _mulaw_arg(x[x != 0.0], channels, np.float64)
    fr = a - np.floor(a)
    return float(np.min(np.minimum(fr, 1.0 - fr))) if a.size else math.inf


def mulaw_signal(T: int, seed: int = 3) -> np.ndarray:
    """Noise that crosses the clamp on both sides, with exact 0, 1 and -1 among the first samples."""
    x = 0.6 * np.random.default_rng(seed).standard_normal(T)
    x[:3] = (0.0, 1.0, -1.0)[:min(T, 3)]
    return x


# ---------------------------------------------------------------------------------------------------------------------------------
# what the GPU tests run; tests/test_codec_oracle.py holds every one of them to the margin condition
MULAW_CASES = tuple((T, ch) for T in (1, 255, 4097) for ch in (256, 2, 1024))


def coded_cases(T: int):
    """(name, x, kbps) of every coded comparison of tests/test_gpu_codec.py at length T: the two-tone signal at each rate, the
    five-row batch with one rate per row, the impulse at 16 kbit/s.  The budget is budget(kbps)."""
    for k in RATES:
        yield f"tones-T{T}-{k:g}k", two_tones(T), k
    yield f"five-T{T}", five_rows(T), np.array(RATES)
    yield f"impulse-T{T}", impulse(T), 16.0
