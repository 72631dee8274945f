"""CPU: the extended matcher's C-ABI entry points reject bad arguments on the host, before any launch (no GPU here)."""
import ctypes
import os

import pytest


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


# table counts hashesperid n_ids hashbits timebits depth hashes nq B cap thresh search_depth window max_alignments | flags quantile
# p2mask hashesfor hf_cap hf_out hf_count | hcap scratch K out info stream
ARGS = [1, 1, 1, 10, 20, 14, 100, 1, 1, 4, 64, 5, 100, 2, 100, 0, 0.05, 0, -1, 0, None, None, 1 << 15, 1, 1, 1, 1, None]


def test_match_ex_argument_errors_do_not_touch_the_gpu(lib):
    h, E = lib.lib(), lib.EINVAL
    n = ctypes.c_longlong(0)
    assert h.mfpa_audfprint_match_ex_scratch_bytes(1 << 15, ctypes.addressof(n)) == 0 and n.value == 56 << 15
    assert h.mfpa_audfprint_match_ex_scratch_bytes(1000, ctypes.addressof(n)) == E          # not a power of two
    assert h.mfpa_audfprint_match_ex_scratch_bytes(32, ctypes.addressof(n)) == E
    assert h.mfpa_audfprint_match_ex_scratch_bytes(1 << 15, None) == E
    bad = {"exact with threshcount 0": {15: 1, 11: 0}, "exact and range with threshcount 0": {15: 3, 11: 0},
           "quantile 1": {16: 1.0}, "quantile < 0": {16: -0.01}, "quantile nan": {16: float("nan")}, "flags 4": {15: 4},
           "flags -1": {15: -1}, "hcap not a power of two": {22: 3000}, "hcap 32": {22: 32}, "hcap 2^27": {22: 1 << 27},
           "hashesfor -2": {18: -2}, "hashesfor without room": {18: 0, 19: 0, 20: 1, 21: 1},
           "hashesfor without a buffer": {18: 0, 19: 16, 20: None, 21: 1}, "hashesfor without a count": {18: 0, 19: 16, 20: 1, 21: None},
           "cap beyond the row field": {10: 32769}, "search_depth": {12: 257}, "window": {13: -1}, "K": {24: 0}, "depth": {6: 0},
           "threshcount -1": {11: -1}}
    for i in (0, 1, 2, 7, 8, 23, 25, 26):                                                    # null pointers
        bad["null argument %d" % i] = {i: None}
    for name, change in bad.items():
        a = list(ARGS)
        for i, v in change.items():
            a[i] = v
        assert h.mfpa_audfprint_match_ex(*a) == E, name
    a = list(ARGS)
    a[9] = 0                                                                                 # an empty batch is a no-op
    assert h.mfpa_audfprint_match_ex(*a) == 0
    a[11], a[15] = 0, 2                                                                      # threshcount 0 is allowed without exact
    assert h.mfpa_audfprint_match_ex(*a) == 0


def test_ops_reject_on_the_host():
    import torch
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    z = torch.zeros(4, dtype=torch.int32)
    with pytest.raises(MfpaError):                                                           # no CPU fallback
        ops.audfprint_match(z.reshape(4, 1), z, z, z.reshape(1, 2, 2), z[:1], exact_count=True)
