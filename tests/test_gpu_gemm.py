"""GPU: every kernel behind mfpa_gemm_mfma (csrc/demucs_gemm.hip) and every switch of their shared epilogue, element by element, at the
tile edges -- against the float64 reference and the bf16x3 arithmetic model of tests/_gemm_oracle.py, with the derived bounds
stated there (none of them measured).  Outputs are pre-filled with a NaN sentinel whose bit pattern must survive everywhere the
kernel has no business writing; the gaps between the clips of A hold NaN, which a correct kernel never lets reach an output.

Each test prints the worst (error / bound) it saw: a record for NOTES.md, not a threshold."""
import ctypes
from dataclasses import replace

import pytest
import torch

from tests import _gemm_oracle as go

pytestmark = pytest.mark.gpu


def _sentinel(n):
    return torch.full((n,), go.SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)


def _device_case(c):
    """A walk case gets its batch from the device: more 256 x 128 tiles than workgroups of the persistent launch."""
    if not c.walk:
        return c
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    c = go.fixed(c, cus)
    tiles = (c.npad // 128) * ((c.M + 255) // 256) * c.batch
    assert tiles > (cus + 7) // 8 * 8 and tiles % 8
    return c


def _upload(c, inp):
    from musicfpaugment_amd import ops_demucs as D
    dev = {k: (v.cuda() if v is not None else None) for k, v in inp.items()}
    dev["Wsplit"] = D.split_rows(dev["W"]) if c.K % 32 == 0 and c.K >= 128 else None
    return dev


def _launch(c, dev, geom=None):
    """One mfpa_gemm_mfma call of case `c` on uploaded operands; buffer strides from `geom` (default c).  -> (C, C2) flat, on the host."""
    from musicfpaugment_amd import ops_demucs as D
    from musicfpaugment_amd._lib import lib
    geom = geom or c
    k = ctypes.c_int(-7)
    d = go.descriptor(c)
    assert lib().mfpa_gemm_mfma_route(ctypes.byref(d), ctypes.byref(k)) == 0 and k.value == c.kid, (c.name, k.value)
    C = _sentinel(c.batch * geom.stride_c)
    C2 = _sentinel(c.batch * geom.stride_c2) if c.c2 else None
    W = dev["Wsplit"] if c.precision == 2 else dev["W"]
    assert tuple(W.shape) == (c.npad, c.K)
    D.gemm(0 if c.c1 else D._p(dev["A"]), c.ld_a, 0 if c.c1 else geom.stride_a, c.batch, c.M, W, dev["bias"] if c.bias else None, c.N,
           D._p(C), c.ldc, geom.stride_c, mode=c.mode, relu=c.relu, addend=D._p(dev["addend"]) if c.mode >= 2 else 0, ldadd=c.ldadd,
           strideAdd=geom.stride_add, precision=c.precision, c1=(dev["x"], dev["c1_w"], dev["c1_b"]) if c.c1 else None,
           C2=D._p(C2) if c.c2 else 0, ldc2=c.ldc2, strideC2=geom.stride_c2)
    torch.cuda.synchronize()
    return C.cpu(), (C2.cpu() if c.c2 else None)


def _take(c, flat, ld, stride, cols, geom=None):
    """The written block (batch, M, cols) of a flat output, after checking that every other element still holds the sentinel."""
    rows = stride // ld
    v = flat.view(c.batch, rows, ld)
    bits = v.view(torch.int32).clone()
    bits[:, :c.M, :cols] = go.SENTINEL_BITS
    assert bool((bits == go.SENTINEL_BITS).all()), f"{c.name}: wrote outside (rows < {c.M}, columns < {cols}) of a pitch-{ld} output"
    return v[:, :c.M, :cols].contiguous()


def _check(c, C, C2, ref, X, against):
    """Element-wise assertions of one case against X (the reference or the model); returns the worst error / bound seen."""
    worst = 0.0

    def within(err, bound, what):
        nonlocal worst
        r = go.ratio(err, bound)
        worst = max(worst, r)
        assert r <= 1.0, f"{c.name}: {what} against {against}: error / bound = {r:.3g}"

    pb = go.pre_bound(c, ref, against)
    if c.mode == 1 and c.c2:
        within((C2.double() - X["pre"]).abs(), pb, "C2 (packed pre-activations)")
        v, g = go.glu_unpack(C2.double())                       # C from the device's OWN pre-activations
        within((C.double() - (v * torch.sigmoid(g))[..., :c.N]).abs(), go.glu_from_c2_bound(v, g)[..., :c.N], "C = v sigmoid(g) of C2")
    else:
        within((C.double() - X["C"]).abs(), go.out_bound(c, ref, against), "C")
        if c.c2:
            within((C2.double() - X["C2"]).abs(), pb[..., :c.N], "C2")
    return worst


@pytest.mark.parametrize("case", go.CASES, ids=lambda c: c.name)
def test_case_against_reference_and_model(case):
    c = _device_case(case)
    inp = go.inputs_for(c)
    ref = go.reference(c, inp)
    flatC, flatC2 = _launch(c, _upload(c, inp))
    C = _take(c, flatC, c.ldc, c.stride_c, c.N)
    C2 = _take(c, flatC2, c.ldc2, c.stride_c2, c.c2_cols) if c.c2 else None
    if c.mode == 3:                                             # masked-out elements are exactly +0.0
        off = go._addend(c, inp) <= 0
        assert int(off.sum()) > 0
        assert bool((C.view(torch.int32)[off] == 0).all()), f"{c.name}: a masked-out element is not +0.0"
    if c.kid in go.FP32_IDS:
        w = {"fp32": _check(c, C, C2, ref, ref, "fp32")}
    else:
        w = {"model": _check(c, C, C2, ref, go.model_bf16x3(c, inp), "model"), "reference": _check(c, C, C2, ref, ref, "reference")}
    print(f"\nGEMM-RATIO {c.name} " + " ".join(f"{k}={v:.4f}" for k, v in w.items()))


def test_all_twelve_kernels_are_reached():
    assert {c.kid for c in go.CASES} == set(range(12))


def _same_bits(a, b):
    return (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))


_PRESPLIT = [c for c in go.CASES if c.kid in go.WSPLIT_IDS and (c.walk and c.mode == 2 or not c.walk and (
    (c.mode, c.relu, c.c2) in ((2, 2, True), (1, 0, True), (3, 0, True)) or (c.mode == 0 and c.M in (192, 257, 129, 300))))]


@pytest.mark.parametrize("case", _PRESPLIT, ids=lambda c: c.name)
def test_presplit_weights_give_the_same_bits_as_the_split_on_the_fly(case):
    """precision 2 (W split once by ops_demucs.split_rows) and precision 1 reach the same kernel family with the same bf16 values in the
    same order: the whole output buffers are identical, bit for bit -- the pipelined kernel in mode 2 with a tail tile among them."""
    c2_ = _device_case(case)
    c1_ = replace(c2_, precision=1, kid=c2_.kid - 1)
    dev = _upload(c2_, go.inputs_for(c2_))
    a, b = _launch(c2_, dev), _launch(c1_, dev)
    assert _same_bits(a[0], b[0]) and _same_bits(a[1], b[1])


def test_the_three_chunked_bf16x3_kernels_give_the_same_bits():
    """gemm_bf16x3_kernel (npad 192), the wide kernel (npad 256, 191 of the rows) and the pipelined kernel (npad 256, all 200 rows) on the
    same A, W and bias: their per-element product order is the same (per 16-wide k-step: al bh, ah bl, ah bh, chunks in order), so the
    common rows and columns are identical, bit for bit."""
    base = go.Case(go.BF16X3, 1, 128, 192, 161, 200, 2, mode=0, relu=0)
    inp = go.inputs_for(base)
    dev = _upload(base, inp)
    flat, _ = _launch(base, dev)
    want = _take(base, flat, base.ldc, base.stride_c, base.N)
    assert go.ratio((want.double() - go.reference(base, inp)["C"]).abs(), go.out_bound(base, go.reference(base, inp), "reference")) <= 1.0
    dev256 = dict(dev)
    dev256["W"] = torch.zeros(256, base.K, device="cuda")
    dev256["W"][:192] = dev["W"]
    dev256["bias"] = torch.zeros(256, device="cuda")
    dev256["bias"][:192] = dev["bias"]
    for other in (replace(base, kid=go.PIPE, npad=256), replace(base, kid=go.WIDE, npad=256, M=191)):
        flat, _ = _launch(other, dev256, geom=base)
        got = flat.view(base.batch, base.M + go.GAP_ROWS, base.ldc)[:, :other.M, :base.N]
        assert torch.equal(got.view(torch.int32) if got.is_contiguous() else got.contiguous().view(torch.int32),
                           want[:, :other.M].contiguous().view(torch.int32)), go.KERNEL_NAMES[other.kid]
