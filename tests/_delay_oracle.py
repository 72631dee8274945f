"""Oracle of the delay lines (csrc/delay.hip), shared by tests/test_delay_oracle.py (CPU) and tests/test_gpu_delay.py.  Both
definitions of include/mfpa.h (mfpa_varidelay, mfpa_comb) restated in numpy operation for operation:

  reference() / comb_reference()   in float64, every product and sum in the order of the formula: the pinned reference;
  truth() / comb_truth()           the same in numpy's long double (80-bit here), from the same float64 inputs.

The variable delay, per row x[0..T), voices v with gains g[v] and delays d[v][n], dry gain g0, half = (filter_len - 1) / 2:
  acc = g0 x[n];  per voice in order:  p = n - d[v][n];  if p > -(half + 1) and p < T + half:  whole = floor(p), frac = p - whole,
  s = sum over j = -half .. half + 1 in order, where |t| <= half with t = j - frac, of x[whole + j] (w sinc),
  w = 0.5 (1 + (cos(pi j / half) cos(pi frac / half) + sin(pi j / half) sin(pi frac / half))),
  sinc = 1 if t == 0 else (sin(pi frac) if j is odd else -sin(pi frac)) / (pi t);  acc += g[v] s  (s = 0 where the test on p fails).
The read position p, its floor and its fraction ARE float64 in both: the header defines p with one rounding, the subtraction
p - floor(p) is exact except for a tiny negative p (frac = 1), and a position is an input of the interpolator, not a result of it.
Everything behind frac (pi, the sines and cosines, the weights, the sums) is in the function's own dtype.

The comb:  y[n] = b0 x[n] + (bD x[n - D] + aD y[n - D]), zeros before the row's start, float64 state.

The error convention is the project's: E = max |reference - truth| over a case, D = max |device - truth|, and the bound is D <= 8 E
(BOUND); where E == 0 the device must give the reference's bits.  errors() returns (D, E)."""
import numpy as np

TILE = 256                 # MFPA_VARIDELAY_TILE
WINDOW = 1024              # MFPA_VARIDELAY_WINDOW
MAX_VOICES = 8             # MFPA_DELAY_MAX_VOICES
BOUND = 8.0
SAMPLE_RATE = 8000
PI_TEXT = "3.14159265358979323846264338327950288"
HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 2e-19)

# The largest |oracle in float64 - analytic sinusoid| over the interior of ramp_case(eps) (filter_len 81, T = 4099), measured by
# tests/test_delay_oracle.py on the CPU, which also holds these figures against a fresh measurement.  The device test allows twice
# this: the interpolator's own error, not the device's.
INTERP_ERR = {0.01: 4.154e-06, -0.03: 4.154e-06}
RAMP_T = 4099


def signal(T: int, seed: int = 0, B: int = None) -> np.ndarray:
    """Seeded white noise in [-1, 1) plus a 440 Hz tone at 8 kHz: every sample different, no exact zero."""
    rng = np.random.default_rng(seed)
    rows = 1 if B is None else B
    x = rng.uniform(-1.0, 1.0, (rows, T)) + 0.5 * np.sin(2.0 * np.pi * 440.0 * np.arange(T) / SAMPLE_RATE + np.arange(rows)[:, None])
    return x[0] if B is None else x


def impulse(T: int, at: int) -> np.ndarray:
    x = np.zeros(T)
    if 0 <= at < T:
        x[at] = 1.0
    return x


# ----------------------------------------------------------------------------- delay patterns, (B, V, T) float64
def constant(B, V, T, value, spread=0.0):
    """value + spread * (v + b / 4) for every sample."""
    return np.broadcast_to((value + spread * (np.arange(V)[None, :] + np.arange(B)[:, None] / 4.0))[:, :, None], (B, V, T)).copy()


def lfo(B, V, T, base=12.0, depth=5.0, period=97.0):
    n = np.arange(T)
    ph = 0.7 * np.arange(V)[None, :, None] + 0.3 * np.arange(B)[:, None, None]
    return base + depth * np.sin(2.0 * np.pi * n / period + ph)


def ramp(B, V, T, eps, offset=0.0):
    """d[n] = offset - eps n: the read position advances by 1 + eps per sample."""
    return np.broadcast_to(offset + 0.5 * np.arange(V)[None, :, None] - eps * np.arange(T), (B, V, T)).copy()


def random_delays(B, V, T, seed=0):
    return np.random.default_rng(seed).uniform(-float(T), float(T), (B, V, T))


def lfo_delay(B, T, sample_rate, base_ms, depth_ms, rate_hz, phase=0.0):
    """numpy twin of ops.lfo_delay."""
    base_ms, depth_ms, rate_hz, phase = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))[:, None] for v in (base_ms, depth_ms, rate_hz, phase))
    n = np.arange(T, dtype=np.float64)
    return (base_ms + depth_ms * np.sin(2.0 * np.pi * rate_hz * n / sample_rate + phase)) * (sample_rate / 1000.0)


def speed_drift_delay(B, T, sample_rate, components):
    """numpy twin of ops.speed_drift_delay: components = [(depth, hz, phase), ...], each a number or (B,)."""
    n = np.arange(T, dtype=np.float64)
    d = np.zeros((B, T))
    for depth, hz, phase in components:
        depth, hz, phase = (np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))[:, None] for v in (depth, hz, phase))
        with np.errstate(divide="ignore", invalid="ignore"):
            term = depth * sample_rate / (2.0 * np.pi * hz) * (np.cos(2.0 * np.pi * hz * n / sample_rate + phase) - np.cos(phase))
        d += np.where((hz > 0.0) & (depth != 0.0), term, 0.0)
    return d


# ----------------------------------------------------------------------------- the accuracy cases (test_gpu_delay.py, test_delay_oracle.py)
ROWS = 5
GAINS = np.array([0.5, -0.25, 0.75, 0.3, -0.6, 0.2, 0.9, -0.4])
DRY = np.array([0.7, 0.0, -0.5, 1.0, 0.25])
TINY = (2.0 ** -60, 2.0 ** -70, 1e-20, 2.0 ** -54, 2.0 ** -1000)


def rows(T: int) -> np.ndarray:
    """(5, T): two rows of the seeded signal, then a unit impulse at 0, TILE - 1 and TILE (a row of zeros where T is shorter)."""
    return np.stack(list(signal(T, seed=7, B=2)) + [impulse(T, 0), impulse(T, TILE - 1), impulse(T, TILE)])


def case_gains(V: int) -> np.ndarray:
    """(5, V): every row its own gains."""
    return np.broadcast_to(GAINS[:V], (ROWS, V)) * (1.0 + 0.1 * np.arange(ROWS))[:, None]


def edges(B, V, T, half):
    """Windows off the start, off the end, across each end, and on the comparison's own boundaries."""
    values = [half / 2 + 0.3, -(half / 2 + 0.3), T + half + 3.0, -(T + half + 3.0), T - 0.5, -(T - 0.5), half + 1.0, -(T - 1.0 + half)]
    return np.broadcast_to(np.array(values[:V])[None, :, None] + 0.25 * np.arange(B)[:, None, None], (B, V, T)).copy()


def near_one(B, V, T, half):
    """Constant delays k + 1 - 2^-50, k = v mod 7: all below 8, so the 2^-50 is in d for every row and voice (and in p = n - d while
    |p| < 8: the definition rounds p once).  At sample 0 the delay is a tiny positive number instead: p is a tiny negative number,
    whole = -1 and frac = p + 1 rounds to 1, the one case in which t reaches half at j = half + 1 and that tap is weighed."""
    d = np.broadcast_to((np.arange(V) % 7 + (1.0 - 2.0 ** -50))[None, :, None], (B, V, T)).copy()
    assert np.all(d < 8.0) and np.all(d != np.rint(d))
    for b in range(B):
        for v in range(V):
            d[b, v, 0] = TINY[(b + v) % len(TINY)]
    return d


FAMILIES = {
    "integer": lambda B, V, T, half: np.floor(constant(B, V, T, 3.0, 4.0)),
    "frac_0.25": lambda B, V, T, half: constant(B, V, T, 7.25, 4.0),
    "frac_0.5": lambda B, V, T, half: constant(B, V, T, 2.5, 4.0),
    "frac_1-2^-50": near_one,
    "lfo": lambda B, V, T, half: lfo(B, V, T),
    "ramp_0.01": lambda B, V, T, half: ramp(B, V, T, 0.01, 5.0),
    "ramp_-0.03": lambda B, V, T, half: ramp(B, V, T, -0.03, 5.0),
    "negative": lambda B, V, T, half: -lfo(B, V, T) - 0.5,
    "edges": edges,
    "random": lambda B, V, T, half: random_delays(B, V, T, seed=T),
}


# ----------------------------------------------------------------------------- the variable delay
def _shape(x, delay, gains, dry):
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    B, T = x.shape
    d = np.asarray(delay, dtype=np.float64)
    if d.ndim == 1:
        d = d[None, None, :]
    elif d.ndim == 2:
        d = d[:, None, :]
    V = d.shape[1]
    d = np.broadcast_to(d, (B, V, T))
    g = np.broadcast_to(np.asarray(gains, dtype=np.float64), (B, V))
    g0 = np.broadcast_to(np.asarray(dry, dtype=np.float64), (B,))
    return one, x, d, g, g0


def _varidelay(x, delay, gains, dry, filter_len, dtype, rounded_functions=False):
    """rounded_functions (float64 only): sin(pi u) and cos(pi u) are taken in long double and rounded once to float64, i.e. a sinpi
    and cospi that are correctly rounded up to the long double's own error, where plain numpy rounds pi u first."""
    one, x, d, g, g0 = _shape(x, delay, gains, dry)
    B, T = x.shape
    V = d.shape[1]
    half = (filter_len - 1) // 2
    assert filter_len == 2 * half + 1 and 3 <= filter_len <= 255 and 1 <= V <= MAX_VOICES
    with np.errstate(invalid="ignore"):
        p = np.arange(T, dtype=np.float64) - d                                   # float64: one rounding
        live = (p > -float(half + 1)) & (p < float(T) + float(half))
    pl = np.where(live, p, 0.0)
    whole = np.floor(pl)
    fr = (pl - whole).astype(dtype)
    first = whole.astype(np.int64)
    pi, dh = dtype(PI_TEXT), dtype(half)
    if rounded_functions:
        assert dtype is np.float64
        wide = np.longdouble(PI_TEXT)
        sinpi = lambda u: np.sin(wide * np.asarray(u, dtype=np.longdouble)).astype(np.float64)      # noqa: E731
        cospi = lambda u: np.cos(wide * np.asarray(u, dtype=np.longdouble)).astype(np.float64)      # noqa: E731
    else:
        sinpi, cospi = (lambda u: np.sin(pi * u)), (lambda u: np.cos(pi * u))
    sf = sinpi(fr)
    cw, sw = cospi(fr / dh), sinpi(fr / dh)
    pad = 2 * half + 2
    xp = np.zeros((B, T + 2 * pad), dtype=dtype)
    xp[:, pad:pad + T] = x
    xp = np.broadcast_to(xp[:, None, :], (B, V, T + 2 * pad))
    s = np.zeros((B, V, T), dtype=dtype)
    for j in range(-half, half + 2):
        t = dtype(j) - fr
        u = dtype(j) / dh
        w = dtype(0.5) * (dtype(1) + (cospi(u) * cw + sinpi(u) * sw))
        zero = t == 0
        sinc = np.where(zero, dtype(1), (sf if j & 1 else -sf) / (pi * np.where(zero, dtype(1), t)))
        xv = np.take_along_axis(xp, first + (j + pad), axis=2)
        s = np.where(live & (np.abs(t) <= dh), s + xv * (w * sinc), s)
    acc = g0.astype(dtype)[:, None] * x.astype(dtype)
    for v in range(V):
        acc = acc + g.astype(dtype)[:, v, None] * s[:, v, :]
    return acc[0] if one else acc


def reference(x, delay, gains=1.0, dry=0.0, filter_len=81):
    """x (T,) or (B, T); delay (T,), (B, T) or anything that broadcasts to (B, V, T); gains to (B, V); dry to (B,).  float64."""
    return _varidelay(x, delay, gains, dry, filter_len, np.float64)


def truth(x, delay, gains=1.0, dry=0.0, filter_len=81):
    return _varidelay(x, delay, gains, dry, filter_len, np.longdouble)


def reference_rounded_functions(x, delay, gains=1.0, dry=0.0, filter_len=81):
    """The float64 definition with correctly rounded sinpi / cospi in place of numpy's sin(pi u) / cos(pi u): every other operation
    as in reference().  What an implementation with exact elementary functions computes (the device library's are close to that)."""
    return _varidelay(x, delay, gains, dry, filter_len, np.float64, rounded_functions=True)


def live_mask(delay, T, filter_len):
    """Where a voice contributes at all: the comparison of the definition, (.., T)."""
    half = (filter_len - 1) // 2
    with np.errstate(invalid="ignore"):
        p = np.arange(T, dtype=np.float64) - np.asarray(delay, dtype=np.float64)
        return (p > -float(half + 1)) & (p < float(T) + float(half))


# ----------------------------------------------------------------------------- the comb
def _comb(x, D, b0, bD, aD, dtype):
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x).astype(dtype)
    B, T = x.shape
    D, b0, bD, aD = (np.broadcast_to(np.asarray(v), (B,)) for v in (D, b0, bD, aD))
    y = np.zeros((B, T), dtype=dtype)
    for b in range(B):
        d, c0, cD, cA = int(D[b]), dtype(np.float64(b0[b])), dtype(np.float64(bD[b])), dtype(np.float64(aD[b]))
        assert d >= 1
        xprev, yprev = np.zeros(d, dtype=dtype), np.zeros(d, dtype=dtype)
        for start in range(0, T, d):
            m = min(d, T - start)
            xs = x[b, start:start + m]
            ys = c0 * xs + (cD * xprev[:m] + cA * yprev[:m])
            y[b, start:start + m] = ys
            xprev, yprev = xs, ys                                                 # a short last block ends the walk
    return y[0] if one else y


def comb_reference(x, D, b0=1.0, bD=0.0, aD=0.0):
    """x (T,) or (B, T); D, b0, bD, aD numbers or (B,).  float64; a float32 device result is this rounded once."""
    return _comb(x, D, b0, bD, aD, np.float64)


def comb_truth(x, D, b0=1.0, bD=0.0, aD=0.0):
    return _comb(x, D, b0, bD, aD, np.longdouble)


def errors(y, want):
    """(D, E) of an output: D = max |y - truth|, E = max |reference - truth|; want = (truth, reference) of the same shape."""
    t, r = want
    return float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - t))), float(np.max(np.abs(np.asarray(r, dtype=np.longdouble) - t)))


# ----------------------------------------------------------------------------- the constant-speed ramp on a sinusoid
def ramp_case(eps: float, T: int = RAMP_T, filter_len: int = 81):
    """(x, delay, analytic, interior): a 1 kHz sinusoid at 8 kHz read at p = (1 + eps) n comes out at (1 + eps) kHz.  interior marks
    the outputs whose read position keeps half + 1 samples off both ends of the row."""
    half = (filter_len - 1) // 2
    n = np.arange(T, dtype=np.float64)
    x = np.sin(2.0 * np.pi * 1000.0 * n / SAMPLE_RATE)
    d = -eps * n
    p = n - d
    return x, d, np.sin(2.0 * np.pi * 1000.0 * p / SAMPLE_RATE), (p >= half + 1) & (p <= T - 1 - (half + 1))
