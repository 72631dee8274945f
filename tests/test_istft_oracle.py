"""CPU: tests/_istft_oracle.py (the numpy restatement of mfpa_istft) against torch.istft, in the error unit that module defines
(E = torch's own float64 round-trip error on the input; bounds are 8 E)."""
import numpy as np
import pytest
import torch

from tests import _istft_oracle as io
from tests._istft_oracle import error_unit, torch_istft, torch_stft

SIZES = (257, 300, 511, 512, 769, 1000, 8548)


def _clip(T, B=2, seed=0):
    g = torch.Generator().manual_seed(seed + T)
    return torch.rand(B, T, generator=g) * 2 - 1


@pytest.mark.parametrize("T", SIZES)
def test_round_trip_within_8E_of_the_input_and_of_torch(T):
    x = _clip(T)
    E = error_unit(x)
    Z = torch_stft(x)
    got = io.istft(Z.numpy(), T)
    ratio = np.abs(got - x.double().numpy()).max() / E
    ratio_t = np.abs(got - torch_istft(Z, T).numpy()).max() / E
    print(f"T={T} E={E:.3e} oracle-vs-x {ratio:.2f} E, oracle-vs-torch {ratio_t:.2f} E")
    assert ratio <= 8 and ratio_t <= 8


def test_imaginary_dc_and_nyquist_bins_are_ignored():
    x = _clip(1000, seed=5)
    E = error_unit(x)
    Z = torch_stft(x).clone()
    Z[:, 0] += 3.0j
    Z[:, 256] -= 2.0j
    want = torch_istft(Z, 1000).numpy()
    assert np.abs(io.istft(Z.numpy(), 1000) - want).max() <= 8 * E
    assert np.abs(want - x.double().numpy()).max() <= 8 * E                    # torch ignored them too


def test_magnitude_rule_zero_bins_and_clamp():
    x = _clip(769, seed=7)
    E = error_unit(x)
    S = torch_stft(x).numpy()
    d = np.array([3.0, 0.25])
    mag = np.abs(S) / d[:, None, None]
    assert np.abs(io.istft(S, 769, mag=mag, denom=d) - x.double().numpy()).max() <= 8 * E     # |spec| / d with denom d: the input
    assert np.abs(io.istft(S, 769, mag=np.abs(S).astype(np.float64)) - x.double().numpy()).max() <= 8 * E
    S0 = S.copy()
    S0[:, 40, 1] = 0
    Z = io.apply_magnitude(S0, np.full(S.shape, 2.0))
    assert Z[0, 40, 1] == 2.0 + 0j and np.allclose(np.abs(Z), 2.0)               # phase 0 where the spectrum is zero
    neg = -np.abs(S)
    assert np.array_equal(io.apply_magnitude(S, neg, clamp=True), np.zeros_like(S))
    flipped = io.apply_magnitude(S, neg)
    assert np.abs(flipped + S).max() <= 4 * np.spacing(np.abs(S).max())         # without the clamp a negative m flips the sign
    assert np.abs(io.istft(S, 769, mag=neg) + x.double().numpy()).max() <= 8 * E


def test_envelope_minimum_and_torchs_refusal():
    w = io.window()
    assert io.envelope_min(w, 251, 64000) == pytest.approx(0.5030853576634366, rel=1e-15)
    assert io.envelope_min(w, 2, 511) == pytest.approx(2.2501246633972162e-08, rel=1e-15)
    x = _clip(600, B=1)
    Z = torch_stft(x)
    zero = torch.zeros(512, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        torch.istft(Z, 512, 256, window=zero, center=True, length=600)
    with pytest.raises(RuntimeError, match="window overlap add min"):
        io.istft(Z.numpy(), 600, win=zero.numpy())
    assert io.length_ok(3, 600) and not io.length_ok(3, 768) and not io.length_ok(3, 511) and not io.length_ok(1, 100)
