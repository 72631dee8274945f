"""GPU: every instantiation of the LSTM recurrence kernels (csrc/lstm.hip) launched once at a small shape -- 22 cases:
lstm_seq_kernel<KS, MS> x 8, lstm_step_kernel<MT> x 2, lstm_bwd_seq_kernel<KS, MTB> x 9, lstm_step_bwd_kernel<MT, BUT> x 3.

Which kernel a case launches follows from the plan rules, on a part with 256 CUs and an explicit workgroup budget of at most 128:
  forward persistent   ms = 1 iff ceil(B / 32) H / 16 <= min(budget, CUs / 2); KS = H / 128
  forward per step     MT = 1 iff H / 16 ceil(B / 32) <= 256
  backward persistent  mtb = the smallest c in {1, 2, 4} with ceil(B / 16 c) H / 16 <= budget; KS = H / 64
  backward per step    MT = 1 iff H / 32 ceil(B / 32) <= 256; BUT = 16 iff MT = 1 and H / 16 ceil(B / 32) <= 128
and the persistent cases assert that mfpa_lstm_seq_workgroups / mfpa_lstm_bwd_seq_workgroups report nslab x H / 16 for the slab size the
case names (another slab size gives another slab count at every B used here).  B is ragged in its last slab, Tn is 3 .. 5.

References: the float64 recurrences of tests/_lstm_reference.py.  Bounds, as in tests/test_gpu_demucs.py / test_gpu_demucs_train.py:
2e-4 absolute on the forward outputs (h, h + skip; and on the saved gate activations and cell states, which come out of the same
sums through functions of slope <= 1), 2e-4 x max |reference| on the backward gate gradients, 2e-4 x max(1, max |dc|) on dcstate,
1e-4 (x that scale) between the persistent and the per-step path.  Every case prints its worst error / bound ratio (pytest -s).
Every output buffer has three rows past B that must stay NaN, as must cstate in training mode and cseq in inference mode; the
error word is zero after every persistent launch; a case run twice on fresh buffers gives the same bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests._lstm_reference import lstm_layer_backward, lstm_layer_forward

pytestmark = pytest.mark.gpu

PAD = 3                      # rows past B in every buffer the kernels write
NAN = float("nan")

# (kernel, H, B, Tn, workgroup budget)
FWD_SEQ = [(f"lstm_seq_kernel<{H // 128}, {ms}>", H, B, Tn, H // 8) for H, Tn in [(256, 5), (512, 4), (768, 4), (1024, 3)] for ms, B in [(1, 50), (2, 65)]]
FWD_STEP = [("lstm_step_kernel<1>", 1024, 100, 3, 0), ("lstm_step_kernel<2>", 1024, 129, 3, 0)]
BWD_SEQ = [(f"lstm_bwd_seq_kernel<{H // 64}, {mtb}>", H, B, Tn, H // 8) for H, Tn in [(256, 5), (512, 4), (768, 3)]
           for mtb, B in [(1, 31), (2, 50), (4, 100)]]
BWD_STEP = [("lstm_step_bwd_kernel<1, 16>", 768, 50, 3, 0), ("lstm_step_bwd_kernel<1, 32>", 768, 100, 3, 0),
            ("lstm_step_bwd_kernel<2, 32>", 768, 321, 3, 0)]
KERNELS = [c[0] for c in FWD_SEQ + FWD_STEP + BWD_SEQ + BWD_STEP]
assert len(set(KERNELS)) == 22


def _slab(kernel):
    """Clips per slab of a persistent kernel, from its name: 32 MS forward, 16 MTB backward."""
    last = int(kernel.rstrip(">").split(",")[-1])
    return (16 if "bwd" in kernel else 32) * last


def _lib():
    from musicfpaugment_amd._lib import lib
    return lib()


def _workgroups(backward, B, H, budget):
    n = ctypes.c_int(-1)
    fn = _lib().mfpa_lstm_bwd_seq_workgroups if backward else _lib().mfpa_lstm_seq_workgroups
    assert fn(B, H, budget, ctypes.addressof(n)) == 0
    return n.value


def _work(backward, B, H):
    n = ctypes.c_longlong(0)
    fn = _lib().mfpa_lstm_bwd_seq_work_bytes if backward else _lib().mfpa_lstm_seq_work_bytes
    assert fn(B, H, ctypes.addressof(n)) == 0
    return torch.zeros(n.value // 4, dtype=torch.int32, device="cuda")


def _sync_words(work, nslab):
    """(error word, the counters of slabs 0 .. nslab-1) of a work buffer: the counter of slab s is word 16 s."""
    torch.cuda.synchronize()
    return int(work[_lib().mfpa_lstm_seq_error_offset() // 4]), [int(work[16 * s]) for s in range(nslab)]


def _padded(t):
    """t (B, ...) on the device with PAD rows of NaN behind it."""
    out = torch.full((t.shape[0] + PAD,) + tuple(t.shape[1:]), NAN, device="cuda")
    out[:t.shape[0]] = t
    return out


def _nan_rows(shape):
    return torch.full(shape, NAN, device="cuda")


_INPUTS = {}


def forward_inputs(H, B, Tn):
    """Operands and float64 reference of a forward case, made once per shape and never written."""
    key = ("fwd", H, B, Tn)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * H + 10 * B + Tn)
        xp = torch.randn(B, Tn, 4 * H, generator=g) * 0.5
        skip = torch.randn(B, Tn, H, generator=g)
        whh = torch.randn(4 * H, H, generator=g) / np.sqrt(H)
        grouped = whh.reshape(4, H // 16, 16, H).permute(1, 0, 2, 3).reshape(4 * H, H).contiguous().cuda()
        h, c, gates = lstm_layer_forward(xp, whh)
        _INPUTS[key] = dict(xp=xp, skip=skip.cuda(), grouped=grouped, h=h, c=c, gates=gates, xsum=h + skip.double())
    return _INPUTS[key]


def backward_inputs(H, B, Tn):
    key = ("bwd", H, B, Tn)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 * H + 10 * B + Tn + 1)
        gates = torch.cat([torch.rand(B, Tn, H, generator=g), torch.rand(B, Tn, H, generator=g), torch.rand(B, Tn, H, generator=g) * 2 - 1,
                           torch.rand(B, Tn, H, generator=g)], dim=2).contiguous()                # [sig i | sig f | tanh g | sig o]
        cseq = (torch.randn(B, Tn, H, generator=g) * 0.7).contiguous()
        dhout = (torch.randn(B, Tn, H, generator=g) * 0.1).contiguous()
        whh = torch.randn(4 * H, H, generator=g) / np.sqrt(H)
        want, dc = lstm_layer_backward(gates, cseq, dhout, whh)
        _INPUTS[key] = dict(gates=gates, cseq=_padded(cseq), dhout=_padded(dhout), whhT=whh.t().contiguous().cuda(), want=want, dc=dc)
    return _INPUTS[key]


def run_forward(H, B, Tn, train, ranges, budget, persistent, work=None):
    """One layer over `ranges` through mfpa_lstm_layer_seq (persistent) or mfpa_lstm_layer_range on fresh NaN-padded buffers
    -> the buffers on the CPU (whole, pad rows included)."""
    from musicfpaugment_amd._lib import check, ptr, stream
    L, inp = _lib(), forward_inputs(H, B, Tn)
    xp = _padded(inp["xp"])
    hseq, xsum, cseq = _nan_rows((B + PAD, Tn, H)), _nan_rows((B + PAD, Tn, H)), _nan_rows((B + PAD, Tn, H))
    cstate = _nan_rows((B + PAD, H))
    # the strides are those of a (B, Tn, .) tensor, so the pad rows lie behind row B - 1 of each buffer
    for (a, b) in ranges:
        if persistent:
            check(L.mfpa_lstm_layer_seq(ptr(inp["grouped"]), ptr(xp), ptr(hseq), ptr(cseq), ptr(cstate), B, Tn, H, ptr(xsum), ptr(inp["skip"]),
                                        int(train), a, b, budget, ptr(work), stream()), "mfpa_lstm_layer_seq")
        else:
            check(L.mfpa_lstm_layer_range(ptr(inp["grouped"]), ptr(xp), ptr(hseq), ptr(cseq), ptr(cstate), B, Tn, H, ptr(xsum), ptr(inp["skip"]),
                                          int(train), a, b, stream()), "mfpa_lstm_layer_range")
    torch.cuda.synchronize()
    return dict(xp=xp.cpu(), hseq=hseq.cpu(), xsum=xsum.cpu(), cseq=cseq.cpu(), cstate=cstate.cpu())


def run_backward(H, B, Tn, ranges, budget, persistent, work=None):
    from musicfpaugment_amd._lib import check, ptr, stream
    L, inp = _lib(), backward_inputs(H, B, Tn)
    gates, dcs = _padded(inp["gates"]), _nan_rows((B + PAD, H))
    for (a, b) in ranges:
        if persistent:
            check(L.mfpa_lstm_layer_bwd_seq(ptr(inp["whhT"]), ptr(gates), ptr(inp["cseq"]), ptr(inp["dhout"]), ptr(dcs), B, Tn, H, a, b, budget,
                                            ptr(work), stream()), "mfpa_lstm_layer_bwd_seq")
        else:
            check(L.mfpa_lstm_layer_bwd_range(ptr(inp["whhT"]), ptr(gates), ptr(inp["cseq"]), ptr(inp["dhout"]), ptr(dcs), B, Tn, H, a, b, stream()),
                  "mfpa_lstm_layer_bwd_range")
    torch.cuda.synchronize()
    return dict(gates=gates.cpu(), dcstate=dcs.cpu())


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _err(got, want):
    return float((got.double() - want.double()).abs().max())


def check_forward(out, H, B, Tn, train, ratios):
    """The sentinels and the float64 bounds of one forward run; appends (name, error / bound) to `ratios`."""
    inp = forward_inputs(H, B, Tn)
    for name in ("hseq", "xsum", "cseq", "cstate", "xp"):
        assert _all_nan(out[name][B:]), name                                   # rows past B: never written
    assert _all_nan(out["cstate"] if train else out["cseq"])                   # the other mode's state buffer: never written
    ratios.append(("h", _err(out["hseq"][:B], inp["h"]) / 2e-4))
    ratios.append(("xsum", _err(out["xsum"][:B], inp["xsum"]) / 2e-4))
    if train:
        ratios.append(("cseq", _err(out["cseq"][:B], inp["c"]) / 2e-4))
        ratios.append(("gates", _err(out["xp"][:B], inp["gates"]) / 2e-4))
    else:
        ratios.append(("cstate", _err(out["cstate"][:B], inp["c"][:, Tn - 1]) / 2e-4))
        assert torch.equal(out["xp"][:B], inp["xp"])                           # inference leaves the projections alone


def check_backward(out, H, B, Tn, ratios):
    inp = backward_inputs(H, B, Tn)
    assert _all_nan(out["gates"][B:]) and _all_nan(out["dcstate"][B:])
    scale = float(inp["want"].abs().max())
    ratios.append(("dgates", _err(out["gates"][:B], inp["want"]) / (2e-4 * scale)))
    ratios.append(("dcstate", _err(out["dcstate"][:B], inp["dc"]) / (2e-4 * max(1.0, float(inp["dc"].abs().max())))))
    return scale


def _same(a, b):
    """Bit identity of two runs' buffers (NaN pad rows included: compared as bit patterns)."""
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def _report(kernel, ratios):
    worst = max(r for _, r in ratios)
    print(f"LSTM-RATIO {kernel:34s} worst {worst:.4f}  " + "  ".join(f"{n} {r:.4f}" for n, r in ratios))
    for n, r in ratios:
        assert r < 1.0, (kernel, n, r)


def forward_case(kernel, H, B, Tn, budget):
    """All runs of one forward case -> {run name: buffers}: inference and training, the per-step path beside a persistent one."""
    persistent = "seq" in kernel
    outs = {}
    for train in (False, True):
        work = _work(False, B, H) if persistent else None
        outs["train" if train else "infer"] = run_forward(H, B, Tn, train, [(0, Tn)], budget, persistent, work)
        if persistent:
            assert _sync_words(work, 1)[0] == 0, "a wait gave up"
    return outs


def backward_case(kernel, H, B, Tn, budget):
    persistent = "seq" in kernel
    work = _work(True, B, H) if persistent else None
    out = run_backward(H, B, Tn, [(0, Tn)], budget, persistent, work)
    if persistent:
        assert _sync_words(work, 1)[0] == 0, "a wait gave up"
    return {"bwd": out}


def run_case(kernel, H, B, Tn, budget):
    """The buffers a case leaves, for a comparison between two builds of the library: {run name: {buffer name: CPU tensor}}."""
    return (backward_case if "bwd" in kernel else forward_case)(kernel, H, B, Tn, budget)


@pytest.mark.parametrize("kernel,H,B,Tn,budget", FWD_SEQ + FWD_STEP, ids=[c[0] for c in FWD_SEQ + FWD_STEP])
def test_forward_instantiation(kernel, H, B, Tn, budget):
    persistent = "seq" in kernel
    if persistent:
        slab = _slab(kernel)
        assert _workgroups(False, B, H, budget) == ((B + slab - 1) // slab) * (H // 16) and B % slab
    else:
        assert (int(kernel[-2]) == 1) == ((H // 16) * ((B + 31) // 32) <= 256)
    outs = forward_case(kernel, H, B, Tn, budget)
    ratios = []
    for train in (False, True):
        check_forward(outs["train" if train else "infer"], H, B, Tn, train, ratios)
    if persistent:                                                                # ... against the per-step kernels on the same operands
        for train in (False, True):
            steps, seq = run_forward(H, B, Tn, train, [(0, Tn)], 0, False), outs["train" if train else "infer"]
            for name in ("hseq", "xsum") + (("cseq", "xp") if train else ("cstate",)):
                ratios.append((name + "~steps", _err(seq[name][:B], steps[name][:B]) / 1e-4))
    _report(kernel, ratios)
    assert all(_same(outs[k], v) for k, v in forward_case(kernel, H, B, Tn, budget).items())      # the same bits on fresh buffers


@pytest.mark.parametrize("kernel,H,B,Tn,budget", BWD_SEQ + BWD_STEP, ids=[c[0] for c in BWD_SEQ + BWD_STEP])
def test_backward_instantiation(kernel, H, B, Tn, budget):
    persistent = "seq" in kernel
    if persistent:
        slab = _slab(kernel)
        assert _workgroups(True, B, H, budget) == ((B + slab - 1) // slab) * (H // 16) and B % slab
    else:
        mt = 1 if (H // 32) * ((B + 31) // 32) <= 256 else 2
        but = 16 if mt == 1 and (H // 16) * ((B + 31) // 32) <= 128 else 32
        assert kernel == f"lstm_step_bwd_kernel<{mt}, {but}>"
    outs = backward_case(kernel, H, B, Tn, budget)
    ratios = []
    scale = check_backward(outs["bwd"], H, B, Tn, ratios)
    if persistent:
        steps = run_backward(H, B, Tn, [(0, Tn)], 0, False)
        ratios.append(("dgates~steps", _err(outs["bwd"]["gates"][:B], steps["gates"][:B]) / (1e-4 * scale)))
    _report(kernel, ratios)
    assert _same(outs["bwd"], backward_case(kernel, H, B, Tn, budget)["bwd"])


@pytest.mark.parametrize("train", [False, True])
def test_forward_two_chained_ranges(train):
    """Steps [0, 2) and [2, Tn) as two persistent launches on one work buffer (the second starts at t0 > 0 from hseq and cstate /
    cseq), and the second launch counted its barrier rounds from zero.  Against the single launch the bound between two paths
    holds, not bit identity: a range's first step takes h[t0 - 1] from memory and splits that float, a later step splits the
    value in the cell's registers, where the compiler may form the lo half from a fused product."""
    kernel, H, B, Tn, budget = FWD_SEQ[5]                                         # lstm_seq_kernel<6, 2>: H 768, B 65, Tn 4
    ranges = [(0, 2), (2, Tn)]
    work = _work(False, B, H)
    two = run_forward(H, B, Tn, train, ranges, budget, True, work)
    err, counters = _sync_words(work, 2)
    assert err == 0 and counters == [(Tn - 2) * (H // 16)] * 2                    # one arrival per workgroup and step of the LAST range
    ratios = []
    check_forward(two, H, B, Tn, train, ratios)
    one = run_forward(H, B, Tn, train, [(0, Tn)], budget, True, _work(False, B, H))
    for name in ("hseq", "xsum") + (("cseq", "xp") if train else ("cstate",)):
        ratios.append((name + "~one", _err(two[name][:B], one[name][:B]) / 1e-4))
    _report(kernel + " two ranges", ratios)
    assert _same(two, run_forward(H, B, Tn, train, ranges, budget, True, _work(False, B, H)))


def test_backward_two_chained_ranges():
    """Steps [2, Tn) and then [0, 2) (t1 < Tn: dgates[t1] and dcstate come from the first launch) on one work buffer; against the
    single launch as in the forward test."""
    kernel, H, B, Tn, budget = BWD_SEQ[4]                                         # lstm_bwd_seq_kernel<8, 2>: H 512, B 50, Tn 4
    ranges = [(2, Tn), (0, 2)]
    work = _work(True, B, H)
    two = run_backward(H, B, Tn, ranges, budget, True, work)
    err, counters = _sync_words(work, 2)
    assert err == 0 and counters == [2 * (H // 16)] * 2
    ratios = []
    scale = check_backward(two, H, B, Tn, ratios)
    one = run_backward(H, B, Tn, [(0, Tn)], budget, True, _work(True, B, H))
    ratios.append(("dgates~one", _err(two["gates"][:B], one["gates"][:B]) / (1e-4 * scale)))
    _report(kernel + " two ranges", ratios)
    assert _same(two, run_backward(H, B, Tn, ranges, budget, True, _work(True, B, H)))


def test_backward_falls_back_to_the_per_step_kernels_where_no_persistent_kernel_exists():
    """H = 1024 would need KS = 16: mfpa_lstm_layer_bwd_seq plans no workgroups and runs mfpa_lstm_layer_bwd_range's launches."""
    H, B, Tn = 1024, 37, 3
    assert _workgroups(True, B, H, 128) == 0
    work = _work(True, B, H)
    seq = run_backward(H, B, Tn, [(0, Tn)], 128, True, work)
    assert not bool(work.any())                                                   # the work buffer was not touched
    ratios = []
    check_backward(seq, H, B, Tn, ratios)
    _report("mfpa_lstm_layer_bwd_seq fallback", ratios)
    assert _same(seq, run_backward(H, B, Tn, [(0, Tn)], 0, False))
