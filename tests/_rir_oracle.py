"""numpy restatement of mfpa_rir_shoebox (include/mfpa.h): the image-source response of a shoebox room (Allen and Berkley), every
image an 81-tap (filter_len) Hann-windowed sinc at its fractional delay, parametrised by the dtype of its arithmetic.

Per axis and signed reflection index i in [-N, N]: p = i mod 2, n = (i + p) / 2, image coordinate s + i L (even i) or -s + (i + 1) L
(odd i), X[i] = (image - mic)^2, G[i] = beta0^|n - p| beta1^|n| with beta = sqrt(1 - alpha) of the axis's two walls.  Per image
(ix, iy, iz), |ix| + |iy| + |iz| <= N:  d = sqrt((X + Y) + Z),  amp = Gx Gy Gz / (4 pi d),  tau = (d fs) / c, and
h[k] += amp w(k - tau) sinc(k - tau),  w(x) = 0.5 (1 + cos(pi x / half)) for |x| <= half, sinc(0) = 1; taps outside [0, length) are
dropped, and so is an image at distance 0.

Error unit of every RIR test: E(case) = max |oracle in float64 - oracle in np.longdouble|, both from the same float64 geometry, each
with pi, the tables, tau and the taps in its own dtype: the float64 rounding error of this formula on this case.  It is dominated by
the rounding of tau (an ulp of tau moves every tap of the image) and of pi (k - tau).  Bounds are 8 E, the convention of
tests/_istft_oracle.py.  Where np.longdouble is no wider than float64 (eps >= 2e-19) there is no unit: HAVE_LONGDOUBLE is False and
the callers skip."""
import math

import numpy as np

HAVE_LONGDOUBLE = bool(np.finfo(np.longdouble).eps < 2e-19)
BOUND = 8.0
PI_TEXT = "3.14159265358979323846264338327950288"
CHUNK = 16384                                                     # images per vectorised step

# the asymmetric case of the GPU tests: a swapped wall or axis changes the result
ROOM, SOURCE, MIC = (5.2, 4.1, 2.7), (1.3, 2.9, 1.1), (3.7, 0.8, 1.6)
ALPHA = (0.3, 0.25, 0.4, 0.15, 0.5, 0.2)


def image_count(N):
    return (2 * N + 1) * (2 * N * N + 2 * N + 3) // 3


def axis_tables(L, s, m, a0, a1, N, dtype=np.float64):
    """(X, G) of one axis, each (2N + 1,), index i + N."""
    L, s, m, a0, a1 = (dtype(np.float64(v)) for v in (L, s, m, a0, a1))
    i = np.arange(-N, N + 1)
    p = i % 2                                                  # 1 for odd i, negative ones too
    n = (i + p) // 2
    img = np.where(p == 1, -s + (i + 1).astype(dtype) * L, s + i.astype(dtype) * L)
    b0, b1 = np.sqrt(dtype(1) - a0), np.sqrt(dtype(1) - a1)
    return (img - m) ** 2, b0 ** np.abs(n - p).astype(dtype) * b1 ** np.abs(n).astype(dtype)


def images(room, source, mic, absorption, N, fs, c=343.0, dtype=np.float64):
    """(amp, tau) of the images with d > 0, in (ix, iy, iz) index order."""
    alpha = np.broadcast_to(np.asarray(absorption, dtype=np.float64), (6,))
    tabs = [axis_tables(room[a], source[a], mic[a], alpha[2 * a], alpha[2 * a + 1], N, dtype) for a in range(3)]
    i = np.arange(-N, N + 1)
    keep = (np.abs(i)[:, None, None] + np.abs(i)[None, :, None] + np.abs(i)[None, None, :]) <= N
    d = np.sqrt((tabs[0][0][:, None, None] + tabs[1][0][None, :, None]) + tabs[2][0][None, None, :])[keep]
    G = (tabs[0][1][:, None, None] * tabs[1][1][None, :, None] * tabs[2][1][None, None, :])[keep]
    pi = dtype(PI_TEXT)
    ok = d > 0
    d, G = d[ok], G[ok]
    return G / (dtype(4) * pi * d), (d * dtype(np.float64(fs))) / dtype(np.float64(c))


def rir(room, source, mic, absorption, N, length, fs, c=343.0, filter_len=81, dtype=np.float64):
    """(length,) of `dtype`."""
    assert filter_len % 2 == 1 and filter_len >= 3
    half = (filter_len - 1) // 2
    amp, tau = images(room, source, mic, absorption, N, fs, c, dtype)
    near = tau < length + half + 1                               # the others have no tap inside [0, length)
    amp, tau = amp[near], tau[near]
    pi = dtype(PI_TEXT)
    h = np.zeros(length, dtype=dtype)
    for lo in range(0, len(tau), CHUNK):                          # in index order, a chunk at a time: memory, not arithmetic
        a, t = amp[lo:lo + CHUNK], tau[lo:lo + CHUNK]
        k = np.floor(t).astype(np.int64)[:, None] + np.arange(-half, half + 2)[None, :]
        x = k.astype(dtype) - t[:, None]
        zero = x == 0
        px = pi * np.where(zero, dtype(1), x)
        sinc = np.where(zero, dtype(1), np.sin(px) / px)
        w = dtype(0.5) * (dtype(1) + np.cos(pi * x / dtype(half)))
        v = a[:, None] * w * sinc
        take = (np.abs(x) <= half) & (k >= 0) & (k < length)
        np.add.at(h, k[take], v[take])
    return h


def error_unit(case):
    """case: the keyword arguments of rir() without dtype."""
    assert HAVE_LONGDOUBLE
    return float(np.max(np.abs(rir(**case, dtype=np.float64).astype(np.longdouble) - rir(**case, dtype=np.longdouble))))


def case(N, length, fs=8000, filter_len=81, room=ROOM, source=SOURCE, mic=MIC, absorption=ALPHA, c=343.0):
    return dict(room=room, source=source, mic=mic, absorption=absorption, N=N, length=length, fs=fs, c=c, filter_len=filter_len)


def decay_time(h, fs):
    """3 x the -5 ... -25 dB span of the Schroeder curve (backward-integrated energy) of h, in seconds."""
    e = np.cumsum(np.asarray(h, dtype=np.float64)[::-1] ** 2)[::-1]
    db = 10.0 * np.log10(e / e[0])
    t5, t25 = int(np.argmax(db <= -5.0)), int(np.argmax(db <= -25.0))
    assert t25 > t5 > 0
    return 3.0 * (t25 - t5) / fs


def eyring_absorption(room, rt60):
    V = room[0] * room[1] * room[2]
    S = 2.0 * (room[0] * room[1] + room[1] * room[2] + room[0] * room[2])
    return 1.0 - math.exp(-0.161 * V / (S * rt60))
