"""conv_ws64_kernel (csrc/unet_ws.hip) computes, bit for bit, what it computed before its fragment reads were shared: the products and the
order of every accumulator's additions are part of the kernel's contract, so a change of its read schedule, its pixel order or its staging
must leave every output byte alone -- the 64-channel rows, the fused max-pool, the fused OutConv, the split layouts, the scale-folded form
and the fused first layer's.  tests/golden/ws64_bits.json holds the sha256 of the output bytes (and the first 16 floats, for a readable
failure) of tools/record_ws64_bits.py's cases, recorded with the library of the commit BEFORE that change; a difference here is a bug,
not a tolerance question."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load_tool():
    spec = importlib.util.spec_from_file_location("record_ws64_bits", os.path.join(ROOT, "tools", "record_ws64_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _load_tool()
with open(os.path.join(ROOT, "tests", "golden", "ws64_bits.json")) as _fh:
    GOLDEN_BITS = json.load(_fh)


def test_the_golden_file_covers_exactly_the_recorded_cases():
    assert sorted(GOLDEN_BITS) == sorted(REC.case_id(c) for c in REC.CASES) and len(set(REC.CASES)) == len(REC.CASES)
    assert {c[:3] for c in REC.CASES} == {(1, 8, 32), (1, 9, 35), (2, 26, 98), (20, 26, 98)}
    assert {c[3] for c in REC.CASES} == {64, 96, 128} and {c[4] for c in REC.CASES} == {0, 32} and {c[5] for c in REC.CASES} == {64, 128}
    assert {c[6] for c in REC.CASES} == {"plain", "pool", "out1x1", "split", "folded"} and {c[7] for c in REC.CASES} == {"", "spec64", "x32"}
    # every small geometry meets every channel combination in every form, and the fused first layer from both sources
    for geo in [(1, 8, 32), (1, 9, 35), (2, 26, 98)]:
        for ch in REC.CHANNELS:
            for form in REC.FORMS:
                assert (geo + ch + (form, "") in REC.CASES) == (form != "out1x1" or ch[2] == 64)
        for src in ("spec64", "x32"):
            for form in REC.C1_FORMS:
                assert geo + (64, 0, 64, form, src) in REC.CASES


@pytest.mark.parametrize("case", REC.CASES, ids=REC.case_id)
def test_conv_ws64_output_bits_are_those_of_the_recorded_commit(case):
    got, want = REC.digest(REC.run(case)), GOLDEN_BITS[REC.case_id(case)]
    if got["sha256"] != want["sha256"]:
        print(f"[ws64 bits {case}] first 16 floats now {got['first16']}, recorded {want['first16']}")
    assert got["sha256"] == want["sha256"], case
