"""CPU: the numpy restatement of csrc/iir.hip (tests/_iir_oracle.py: restate) against the long-double truth with scipy's own error
as the yardstick (D <= 8 E), and the cookbook designs of functional.biquad_coefficients against scipy.signal.freqz.  The restatement
must hold here before the kernel is compared with it on the GPU (tests/test_gpu_iir.py)."""
import inspect

import numpy as np
import pytest
import scipy.signal

from tests import _iir_oracle as io

FILTERS = io.filters()


@pytest.fixture(scope="module")
def long_case():
    """Per filter: the longest signal, its truth and its reference, computed once."""
    out = {}
    for name, sos in FILTERS.items():
        x = io.signal(io.LENGTHS[-1], seed=3)
        out[name] = (x, io.truth(x, sos)[0], io.reference(x, sos)[0])
    return out


@pytest.mark.parametrize("name", sorted(FILTERS))
def test_restatement_is_within_eight_of_scipys_errors(name, long_case):
    sos = FILTERS[name]
    x, t, r = long_case[name]
    for T in io.LENGTHS:                                                       # a prefix of a causal filter's output is the shorter signal's output
        y, _ = io.restate(x[:T], sos)
        D, E = io.errors(y, x[:T], sos, want=(t[:T], r[:T]))
        print(f"{name} T={T}: D={D:.3e} E={E:.3e} D/E={D / E if E else float('nan'):.2f}")
        assert D <= io.BOUND * E if E > 0 else np.array_equal(y, r[:T]), (name, T, D, E)


@pytest.mark.parametrize("name", ["peak50_q8_8k", "lowpass30_8k"])
def test_squared_powers_are_the_trap(name, long_case):
    """The same restatement with the powers formed by products of A loses several times more than with the recurrence's powers on the
    low-frequency sections (8 E and 19 E against 0.8 E and 1.0 E here): the reason sos_powers_kernel exists.  Printed, and asserted
    only as an ordering."""
    sos = FILTERS[name]
    x, t, r = long_case[name]
    D_rec, E = io.errors(io.restate(x, sos)[0], x, sos, want=(t, r))
    D_sq, _ = io.errors(io.restate(x, sos, powers_fn=io.powers_by_squaring)[0], x, sos, want=(t, r))
    print(f"{name}: recurrence {D_rec / E:.2f} E, squaring {D_sq / E:.2f} E")
    assert D_rec <= D_sq


@pytest.mark.parametrize("T", [1, io.L, io.L + 1, io.SUPER, io.SUPER + 5, 2 * io.SUPER + 17])
@pytest.mark.parametrize("name", ["peak50_q8_8k", "seven_bands_44k"])
def test_states(name, T):
    sos = FILTERS[name]
    rng = np.random.default_rng(T)
    x, zi = io.signal(T, seed=T + 1), rng.uniform(-1.0, 1.0, (len(sos), 2))
    y, zf = io.restate(x, sos, zi)
    D, E = io.errors(y, x, sos, zi)
    Ds, Es = io.state_errors(zf, x, sos, zi)
    print(f"{name} T={T}: output D/E={D / E:.2f}, state D/E={Ds / Es:.2f}")
    assert D <= io.BOUND * E and Ds <= io.BOUND * Es
    n = T // 2                                                                 # two calls joined by the state: the one-shot result
    if n:
        y0, z0 = io.restate(x[:n], sos, zi)
        y1, z1 = io.restate(x[n:], sos, z0)
        D2, _ = io.errors(np.concatenate([y0, y1]), x, sos, zi)
        Ds2, _ = io.state_errors(z1, x, sos, zi)
        assert D2 <= io.BOUND * E and Ds2 <= io.BOUND * Es


@pytest.mark.parametrize("T", io.LENGTHS)
def test_exact_cases(T):
    """E == 0: the identity section returns the input, and FIR sections with exactly representable coefficients on integer-valued
    input give scipy's output exactly (the powers of a nilpotent A are zero, the carry is the lane's own end state)."""
    x = io.signal(T, seed=T)
    y, zf = io.restate(x, io.IDENTITY)
    assert np.array_equal(y, x) and not zf.any()
    xi = np.random.default_rng(T).integers(-1000, 1000, T).astype(np.float64)
    fir = np.array([[0.5, -2.0, 0.25, 1.0, 0.0, 0.0], [3.0, 1.0, -0.5, 1.0, 0.0, 0.0]])
    y, zf = io.restate(xi, fir)
    r, rz = io.reference(xi, fir)
    assert io.errors(y, xi, fir)[1] == 0.0 and np.array_equal(y, r) and np.array_equal(zf, rz)


def _h(c, sample_rate, freqs):
    return scipy.signal.freqz(c[:3], c[3:], worN=np.atleast_1d(np.asarray(freqs, dtype=np.float64)), fs=sample_rate)[1]


def _close(got, want):
    assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (got, want)


@pytest.mark.parametrize("sr,f0,Q,g", [(8000, 50.0, 8.0, 12.0), (8000, 1000.0, 0.707, -6.0), (44100, 20.0, 4.0, -12.0), (44100, 9000.0, 0.3, 18.0),
                                       (8000, 3900.0, 10.0, 24.0)])
def test_designs_meet_their_defining_gains(sr, f0, Q, g):
    from musicfpaugment_amd.functional import biquad_coefficients as bc
    A2 = 10.0 ** (g / 20.0)
    _close(abs(_h(bc("peaking", sr, f0, Q, g), sr, f0)[0]), A2)
    lo, hi = bc("lowshelf", sr, f0, Q, g), bc("highshelf", sr, f0, Q, g)
    _close(abs(_h(lo, sr, 0.0)[0]), A2), _close(abs(_h(lo, sr, sr / 2)[0]), 1.0)
    _close(abs(_h(hi, sr, 0.0)[0]), 1.0), _close(abs(_h(hi, sr, sr / 2)[0]), A2)
    lp, hp = bc("lowpass", sr, f0, Q), bc("highpass", sr, f0, Q)
    _close(abs(_h(lp, sr, 0.0)[0]), 1.0), _close(abs(_h(lp, sr, sr / 2)[0]), 0.0), _close(abs(_h(lp, sr, f0)[0]), Q)
    _close(abs(_h(hp, sr, 0.0)[0]), 0.0), _close(abs(_h(hp, sr, sr / 2)[0]), 1.0), _close(abs(_h(hp, sr, f0)[0]), Q)
    _close(abs(_h(bc("bandpass", sr, f0, Q), sr, f0)[0]), 1.0)
    _close(abs(_h(bc("bandpass_skirt", sr, f0, Q), sr, f0)[0]), Q)
    _close(abs(_h(bc("bandreject", sr, f0, Q), sr, f0)[0]), 0.0)
    for h in _h(bc("allpass", sr, f0, Q), sr, np.linspace(0.0, sr / 2, 16)):
        _close(abs(h), 1.0)


def test_bass_and_treble_are_the_shelves_at_their_default_centres(monkeypatch):
    from musicfpaugment_amd import functional as F
    seen = []
    monkeypatch.setattr(F, "_filter", lambda waveform, sos, clamp, who: seen.append((np.array(sos), clamp)))
    F.bass_biquad(None, 8000, 7.0)
    F.treble_biquad(None, 8000, -5.0)
    F.equalizer_biquad(None, 8000, 440.0, 3.0, 2.0)
    F.bandpass_biquad(None, 8000, 440.0, const_skirt_gain=True)
    want = [F.biquad_coefficients("lowshelf", 8000, 100.0, 0.707, 7.0), F.biquad_coefficients("highshelf", 8000, 3000.0, 0.707, -5.0),
            F.biquad_coefficients("peaking", 8000, 440.0, 2.0, 3.0), F.biquad_coefficients("bandpass_skirt", 8000, 440.0, 0.707)]
    assert len(seen) == 4 and all(np.array_equal(s[0], w[None]) and s[1] is True for s, w in zip(seen, want))
    assert [p.default for p in list(inspect.signature(F.lfilter).parameters.values())[3:]] == [True, True]
    assert list(inspect.signature(F.lfilter).parameters)[:3] == ["waveform", "a_coeffs", "b_coeffs"]              # torchaudio's a-before-b
