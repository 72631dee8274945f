"""Oracle of the dynamic range compressor (csrc/dynamics.hip), shared by tests/test_dynamics_oracle.py (CPU) and
tests/test_gpu_dynamics.py.  The definition (include/mfpa.h, mfpa_dynamics), serial over the samples and vectorised over the rows:

  reference()  in float64, every product and sum in the order of the formula: the pinned reference;
  truth()      the same in numpy's long double (80-bit here): what the formula means.

A row has six float64 parameters (threshold_db, slope = 1 - 1/ratio, knee_db, attack_coef, release_coef, makeup_db) and the state
(y1, yL); per sample
  xg = 20 log10(max(|x|, 1e-10));  o = xg - threshold
  xl = 0 if 2 o <= -W,  s (o + W/2)^2 / (2 W) if 2 |o| < W,  s o otherwise
  y1 = max(xl, aR y1 + (1 - aR) xl);  yL = aA yL + (1 - aA) y1;  y = x 10^((M - yL) / 20)
and in level-in mode the input is xl itself and the output yL.

The error convention is the project's: E = max |reference - truth| over a case, D = max |device - truth|, and the bound is D <= 8 E
(BOUND); where E == 0 the device must give the reference's bits.  errors() returns (D, E)."""
import numpy as np

P = 8                      # wavefronts per row in csrc/dynamics.hip
L = 16                     # samples per lane
SUPER = 64 * L             # samples per super-chunk
BOUND = 8.0
SAMPLE_RATE = 8000
LENGTHS = (1, L - 1, L, L + 1, SUPER - 1, SUPER, SUPER + 1, P * SUPER - 1, P * SUPER + 1, 2 * P * SUPER + 3)

# name: threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db
CASES = {
    "comp": (-20.0, 4.0, 6.0, 5.0, 100.0, 3.0),
    "hard": (-12.0, 8.0, 0.0, 1.0, 50.0, 0.0),
    "lim": (-6.0, float("inf"), 0.0, 0.0, 50.0, 0.0),
    "inst": (-20.0, 2.0, 10.0, 0.0, 0.0, 0.0),
}
FIFTH = (-30.0, 3.0, 12.0, 10.0, 200.0, 6.0)          # with the four above: five different rows for one launch
WITH_MEMORY = ("comp", "hard", "lim")


def time_coef(seconds: float, sample_rate: float) -> float:
    return float(np.exp(-1.0 / (seconds * sample_rate))) if seconds > 0.0 else 0.0


def params(threshold_db, ratio, knee_db, attack_ms, release_ms, makeup_db, sample_rate=SAMPLE_RATE) -> np.ndarray:
    """(6,) float64: what the device takes."""
    return np.array([threshold_db, 1.0 - 1.0 / ratio, knee_db, time_coef(attack_ms / 1000.0, sample_rate),
                     time_coef(release_ms / 1000.0, sample_rate), makeup_db], dtype=np.float64)


def case(name: str) -> np.ndarray:
    return params(*CASES[name])


def five_rows() -> np.ndarray:
    """(5, 6): comp, hard, lim, inst and a fifth set."""
    return np.stack([case(n) for n in CASES] + [params(*FIFTH)])


def signal(T: int, seed: int = 0, B: int = None, sample_rate: int = SAMPLE_RATE) -> np.ndarray:
    """A 220 Hz tone gated on and off at 3 Hz plus 0.05 of white noise, samples 300..419 exact zeros; with B, B rows of different
    amplitude (0.9, 0.75, 0.6, ...) and noise.  The tone crosses every threshold of CASES, the gaps let the release run."""
    rng = np.random.default_rng(seed)
    rows = 1 if B is None else B
    t = np.arange(T) / sample_rate
    gate = (np.sin(2.0 * np.pi * 3.0 * t + 0.4) >= 0.0).astype(np.float64)
    amp = np.maximum(0.9 - 0.15 * np.arange(rows), 0.2)[:, None]
    x = amp * gate * np.sin(2.0 * np.pi * 220.0 * t + 0.3 * np.arange(rows)[:, None]) + 0.05 * rng.standard_normal((rows, T))
    x[:, 300:420] = 0.0
    return x[0] if B is None else x


def levels(x, q, dtype=np.float64):
    """xl of the definition: the gain reduction wanted in dB, elementwise; x (..., T), q (6,) or (B, 6)."""
    x = np.asarray(x, dtype=dtype)
    q = np.asarray(q, dtype=np.float64).astype(dtype)
    th, s, W = (q[..., i, None] for i in range(3))
    xg = dtype(20.0) * np.log10(np.maximum(np.abs(x), dtype(1e-10)))
    o = xg - th
    t = o + W / dtype(2.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        knee = s * (t * t) / (dtype(2.0) * W)
    return np.where(dtype(2.0) * o <= -W, dtype(0.0), np.where(dtype(2.0) * np.abs(o) < W, knee, s * o))


def _run(x, q, zi, level_in, dtype):
    x = np.asarray(x, dtype=dtype)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    q = np.asarray(q, dtype=np.float64).astype(dtype)
    xl = x if level_in else levels(x, q, dtype)
    aA, aR, M = q[..., 3], q[..., 4], q[..., 5]
    bA, bR = dtype(1.0) - aA, dtype(1.0) - aR
    B, T = x.shape
    y1 = np.zeros(B, dtype=dtype) if zi is None else np.array(np.atleast_2d(zi)[:, 0], dtype=dtype)
    yL = np.zeros(B, dtype=dtype) if zi is None else np.array(np.atleast_2d(zi)[:, 1], dtype=dtype)
    gr = np.empty((B, T), dtype=dtype)
    for n in range(T):
        v = xl[:, n]
        y1 = np.maximum(v, aR * y1 + bR * v)
        yL = aA * yL + bA * y1
        gr[:, n] = yL
    zf = np.stack([y1, yL], axis=-1)
    y = gr if level_in else x * np.power(dtype(10.0), (np.reshape(M, (-1, 1)) - gr) / dtype(20.0))
    return (y[0], gr[0], zf[0]) if one else (y, gr, zf)


def reference(x, q, zi=None, level_in=False):
    """(y, gr, zf) in float64; x (T,) or (B, T), q (6,) or (B, 6), zi (2,) or (B, 2).  In level-in mode y is gr."""
    return _run(x, q, zi, level_in, np.float64)


def truth(x, q, zi=None, level_in=False):
    """The same in long double, from the same float64 inputs."""
    return _run(x, q, zi, level_in, np.longdouble)


def errors(y, want):
    """(D, E) of an output: D = max |y - truth|, E = max |reference - truth|; want = (truth, reference) of the same shape."""
    t, r = want
    return float(np.max(np.abs(np.asarray(y, dtype=np.longdouble) - t))), float(np.max(np.abs(np.asarray(r, dtype=np.longdouble) - t)))
