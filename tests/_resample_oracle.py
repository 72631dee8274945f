"""float64 numpy restatement of torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults (sinc_interp_hann,
lowpass_filter_width 6, rolloff 0.99), as include/mfpa.h states it for mfpa_resample*.  torchaudio is not a dependency: the
restatement is compared with the real transform only where torchaudio is installed (tests/test_resample_oracle.py)."""
import math

import numpy as np

LOWPASS_FILTER_WIDTH = 6
ROLLOFF = 0.99

# (orig_freq, new_freq) -> (o, n, width, K): checked by hand / on the CPU when the feature was specified
TABLE = {
    (44100, 8000): (441, 80, 34, 509),
    (16000, 8000): (2, 1, 13, 28),
    (48000, 8000): (6, 1, 37, 80),
    (22050, 8000): (441, 160, 17, 475),
    (8000, 16000): (1, 2, 7, 15),
    (32000, 8000): (4, 1, 25, 54),
    (11025, 8000): (441, 320, 9, 459),
    (44100, 48000): (147, 160, 7, 161),
    (48000, 44100): (160, 147, 7, 174),
}
# (orig_freq, new_freq, L) -> Tout
LENGTHS = {(44100, 8000, 4411): 801, (44100, 8000, 1): 1, (16000, 8000, 1001): 501, (16000, 8000, 2): 1, (48000, 8000, 613): 103,
           (22050, 8000, 2000): 726, (8000, 16000, 257): 514, (32000, 8000, 5): 2, (11025, 8000, 443): 322}


def geometry(orig_freq, new_freq, lowpass_filter_width=LOWPASS_FILTER_WIDTH, rolloff=ROLLOFF):
    """(o, n, width, K)."""
    g = math.gcd(int(orig_freq), int(new_freq))
    o, n = int(orig_freq) // g, int(new_freq) // g
    base = min(o, n) * rolloff
    width = math.ceil(lowpass_filter_width * o / base)
    return o, n, width, 2 * width + o


def out_len(orig_freq, new_freq, L):
    o, n, _, _ = geometry(orig_freq, new_freq)
    return -((-n * int(L)) // o)


def taps64(orig_freq, new_freq, lowpass_filter_width=LOWPASS_FILTER_WIDTH, rolloff=ROLLOFF):
    """(n, K) float64 taps before their one rounding to float32."""
    o, n, width, K = geometry(orig_freq, new_freq, lowpass_filter_width, rolloff)
    base = min(o, n) * rolloff
    phase = (-np.arange(n)).astype(np.float32) / np.float32(n)           # torchaudio makes the phase offset in float32
    idx = np.arange(-width, width + o, dtype=np.float64) / o
    t = (phase.astype(np.float64)[:, None] + idx[None, :]) * base
    t = np.clip(t, -lowpass_filter_width, lowpass_filter_width)
    win = np.cos(t * math.pi / lowpass_filter_width / 2) ** 2
    t = t * math.pi
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.where(t == 0, 1.0, np.sin(t) / t)
    return sinc * win * (base / o)


def taps32(orig_freq, new_freq):
    return taps64(orig_freq, new_freq).astype(np.float32)


def _frames(x, o, n, width, K):
    """(B, J, K) windows xpad[j * o + k] of (B, L) clips, J = L // o + 1 frames (all torchaudio's strided convolution makes)."""
    B, L = x.shape
    J = L // o + 1
    xpad = np.zeros((B, (J - 1) * o + K), dtype=np.float64)
    m = min(L, xpad.shape[1] - width)
    xpad[:, width:width + m] = x[:, :m]
    s = xpad.strides
    return np.lib.stride_tricks.as_strided(xpad, (B, J, K), (s[0], o * s[1], s[1]), writeable=False)


def resample(x, orig_freq, new_freq, with_bound=False):
    """(B, L) -> (B, Tout) float64 with the float32 taps; with_bound: also bound = conv(|taps|, |x|) per output sample."""
    x = np.asarray(x, dtype=np.float64)
    if orig_freq == new_freq:
        return (x, np.abs(x)) if with_bound else x
    o, n, width, K = geometry(orig_freq, new_freq)
    tp = taps32(orig_freq, new_freq).astype(np.float64)
    B, L = x.shape
    Tout = out_len(orig_freq, new_freq, L)
    y = np.einsum("bjk,ik->bji", _frames(x, o, n, width, K), tp).reshape(B, -1)[:, :Tout]
    if not with_bound:
        return y
    bound = np.einsum("bjk,ik->bji", _frames(np.abs(x), o, n, width, K), np.abs(tp)).reshape(B, -1)[:, :Tout]
    return y, bound
