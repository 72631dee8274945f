"""GPU: the forward convolution family behind mfpa_conv_mfma (conv_ws64_kernel, the 29 forms of conv_wd16_kernel, conv_mfma_kernel,
convT_mfma_kernel: 66 instantiations), pinned element by element on exact operands.  Every case is launched from a descriptor of the
second table of tests/_conv_route_cases.py, must route to the instantiation its row names, and every element of every output and side
output is compared with a float64 CPU reference by torch.equal -- no tolerance anywhere.

Why that is legitimate: sources and weights are integers in [-3, 3]; the on-load affine is scale 1 and an integer shift in [-2, 2] (the
activated source is an integer in [0, 5]); the fused first layer takes an integer input in [-2, 2], integer weights in [-1, 1], scale 1
and an integer shift (its output is at most 20; with c1_spec64 the input arrives as integer * denom[b], denom a power of two that differs
per clip).  Such values are exact in bfloat16 -- the bf16x3 low halves are zero and plain bf16 loses nothing -- and every product and
partial sum is an integer below 2^24, so the float32 accumulators are exact whatever the accumulation order, at precisions 0, 1 and 2
alike.  The epilogue scales by 0.5, 1 or 2 per channel and adds an integer shift: dyadic, exact.  Statistics cases narrow sources and
weights to [-1, 1] so that each wave's float32 partial sums stay below 2^24 as well.  _reference() asserts all of these conditions on
the float64 reference itself before anything is compared with it.

Groups (tests/_conv_route_cases.py, exact_cases): `inst` -- every row of cases() with two different clips and extents ragged against the
row's patch in both directions, reaching all 66 instantiations (asserted below); `pair` -- two sources, the second smaller and centred;
`epi` -- scale / shift / ReLU (and the folded form wherever mfpa_conv_scale_folds says 1), the cropped output, the fused MaxPool2d and
OutConv, the split layout, c1_spec64, the BatchNorm backward's sums; `walk` -- the persistent kernels on a periodic batch with
2 G < tiles < 3 G, so that every workgroup prefetches, hands over and drains at least once.  NaN guards sit in front of and behind every
output and side output; bfloat16 tensors are compared as int16 bit patterns.  Dropout is not covered here (tests/test_gpu_train.py)."""
import ctypes
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from tests import _conv_route_cases as rc

pytestmark = pytest.mark.gpu
GUARD = 1024
LIMIT = float(2 ** 24)
GROUPS = rc.exact_cases()


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    return _lib


def _ints(g, lo, hi, *shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _tile_sums(t, ph, pw):
    """Largest sum of a non-negative (n, C, H, W) tensor over one ph x pw tile, per clip and channel."""
    n, C, H, W = t.shape
    t = F.pad(t, [0, -W % pw, 0, -H % ph])
    return float(t.reshape(n, C, t.shape[2] // ph, ph, t.shape[3] // pw, pw).sum(dim=(3, 5)).max())


@functools.lru_cache(maxsize=None)
def _reference(key):
    """Operands and expected outputs of one case in float64 (NCHW), shared by every precision and bfloat16 / split form of its shape.  The
    exactness conditions are asserted here, on the CPU, before any GPU result is compared."""
    s = dict(key)
    g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    n, H, W, C0, C1, Cout, mode = (s[k] for k in ("clips", "H", "W", "C0", "C1", "Cout", "mode"))
    if s["walk"]:
        G, per_clip, P = s["walk"]
        # the period condition: a workgroup's consecutive tiles (G apart) must not be copies of one another
        assert n == P and G % (per_clip * P) != 0 and 2 * G < s["B"] * per_clip < 3 * G and s["B"] % P == 0, s["walk"]
    a = 1 if s["stats"] else 3
    ref = {}
    if s["c1"]:
        ref["c1_x"], ref["c1_w"], ref["c1_shift"] = _ints(g, -2, 2, n, H, W), _ints(g, -1, 1, 9, 64), _ints(g, -2, 2, 64)
        src = F.relu(F.conv2d(ref["c1_x"][:, None], ref["c1_w"].t().reshape(64, 1, 3, 3), padding=1) + ref["c1_shift"][None, :, None, None])
        assert float(src.max()) <= 20
        if s["c1"] == 2:
            ref["c1_denom"] = 2.0 ** (1 + torch.arange(n, dtype=torch.float64))             # differs per clip; integer * 2^k / 2^k is exact
            ref["c1_spec"] = ref["c1_x"] * ref["c1_denom"][:, None, None]
    else:
        ref["x0"] = _ints(g, -a, a, n, C0, 2 * H if mode == 2 else H, 2 * W if mode == 2 else W)
        src = ref["x0"]
        if s["affine"]:
            ref["in_shift"] = _ints(g, -2, 2, C0)
            src = F.relu(src + ref["in_shift"][None, :, None, None])
            assert float(src.max()) <= 5
    ref["a0"] = src                                                        # source 0 as the convolution sees it
    if C1:
        ref["x1"] = _ints(g, -a, a, n, C1, s["H1"], s["W1"])
        dy, dx = H - s["H1"], W - s["W1"]
        src = torch.cat([src, F.pad(ref["x1"], [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])], dim=1)
    cin, taps = C0 + C1, 9 if mode == 0 else 4
    ref["w"] = w = _ints(g, -a, a, taps, Cout, cin)                        # kernel layout [tap][Cout][Cin]
    if s["scale"]:
        ref["out_scale"] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (Cout,), generator=g)]
    if s["shift"]:
        ref["out_shift"] = _ints(g, -3, 3, Cout)
    if mode == 0:
        z = F.conv2d(src, w.view(3, 3, Cout, cin).permute(2, 3, 0, 1), padding=1)
    elif mode == 1:
        z = F.conv_transpose2d(src, w.view(2, 2, Cout, cin).permute(3, 2, 0, 1), stride=2)
    else:
        z = F.conv2d(src, w.view(2, 2, Cout, cin).permute(2, 3, 0, 1), stride=2)
    # exact accumulators: an integer-valued reference, and no partial sum of any order can reach 2^24
    assert z.dtype == torch.float64 and torch.equal(z, z.round())
    assert float(src.abs().max()) * float(w.abs().max()) * taps * cin < LIMIT and float(z.abs().max()) < LIMIT
    if mode != 1:
        z = z[:, :, :s["yH"], :s["yW"]]
    e = z
    if s["scale"]:
        e = e * ref["out_scale"][None, :, None, None]
    if s["shift"]:
        e = e + ref["out_shift"][None, :, None, None]
    if s["relu"]:
        e = F.relu(e)
    assert torch.equal(2 * e, (2 * e).round()) and float(e.abs().max()) < LIMIT / 2           # dyadic: exact in float32
    ref["y"] = e.contiguous()
    if s["pool"]:
        ref["y_pool"] = F.max_pool2d(e, 2)
    if s["w1x1"]:
        ref["w1x1"], ref["b1x1"] = _ints(g, -2, 2, 64), float(_ints(g, -2, 2, 1))
        assert float((e.abs() * ref["w1x1"].abs()[None, :, None, None]).sum(dim=1).max()) + abs(ref["b1x1"]) < LIMIT
        ref["y1x1"] = (e * ref["w1x1"][None, :, None, None]).sum(dim=1) + ref["b1x1"]
    if s["stats"]:
        ph, pw = s["stats"]
        # the header does not say which of a tile's pixels a wave owns: a whole tile's sums below 2^24 bound every wave's row partial
        assert _tile_sums(e * e, ph, pw) < LIMIT and _tile_sums(e.abs(), ph, pw) < LIMIT
        if s["bwd"]:
            ref["bwd_z"] = _ints(g, -3, 3, *e.shape)
            ref["bwd_scale"] = torch.tensor([1.0, 2.0], dtype=torch.float64)[torch.randint(0, 2, (Cout,), generator=g)]
            ref["bwd_invstd"] = torch.tensor([0.5, 1.0, 2.0], dtype=torch.float64)[torch.randint(0, 3, (Cout,), generator=g)]
            ref["bwd_shift"], ref["bwd_mean"] = _ints(g, -2, 2, Cout), _ints(g, -1, 1, Cout)
            c = lambda k: ref[k][None, :, None, None]
            gg = torch.where(ref["bwd_z"] * c("bwd_scale") + c("bwd_shift") > 0, e, torch.zeros_like(e))
            second = gg * ((ref["bwd_z"] - c("bwd_mean")) * c("bwd_invstd"))                  # g * xhat: dyadic however xhat is formed
            assert torch.equal(2 * second, (2 * second).round())
            assert _tile_sums(gg.abs(), ph, pw) < LIMIT and _tile_sums(second.abs(), ph, pw) < LIMIT
            ref["sums"] = torch.stack([gg.sum(dim=(0, 2, 3)), second.sum(dim=(0, 2, 3))], dim=1)
        else:
            ref["sums"] = torch.stack([e.sum(dim=(0, 2, 3)), (e * e).sum(dim=(0, 2, 3))], dim=1)     # [C][sum, sum of squares]
    return ref


def _split(x):
    """float32 (..., C) -> the bf16 halves (..., C / 32, 32) of the split layout: hi = bf16(x), lo = bf16(x - hi)."""
    x4 = x.reshape(*x.shape[:-1], x.shape[-1] // 32, 32)
    hi = x4.bfloat16()
    return hi, (x4 - hi.float()).bfloat16()


def _to_split(x):
    """float32 NHWC -> the split layout ([32 bf16 hi | 32 bf16 lo] per 32-channel chunk) as a float32 tensor of the same shape and bytes."""
    hi, lo = _split(x)
    return torch.cat([hi, lo], dim=-1).contiguous().view(torch.float32).reshape(x.shape)


def _bits(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t


def _same(what, got, want):
    """torch.equal, with the count of bad elements, the largest difference and the first bad indices on a mismatch."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if torch.equal(_bits(got), _bits(want)):
        return
    bad = (_bits(got) != _bits(want)) | torch.isnan(got)
    diff = (got.double() - want.double()).abs()
    raise AssertionError((what, f"{int(bad.sum())} of {bad.numel()} elements differ", "largest difference",
                          float(torch.nan_to_num(diff, nan=float("inf")).max()), "first bad indices", bad.nonzero()[:6].tolist()))


def _plan(lib, name, fields, want, walk, cus):
    """Host side of a case: the full descriptor fields, the route (asserted), the batch of a walk case, and the reference's key."""
    f = dict(C0=64, C1=0, H1=0, W1=0, B=1, H=8, W=33, Cout=64, mode=0, precision=0, w_layout=0, relu=0, yH=0, yW=0)
    f.update(fields)
    code, got, r = rc.route(lib, rc.desc(lib, **f))
    assert code == 0 and got == want, (name, code, got, want)
    H, W, mode = f["H"], f["W"], f["mode"]
    period = None
    if walk:                                                               # the batch from the launcher's own rule and this device's CUs
        assert rc.walks(want), (name, want)
        G = cus // (f["Cout"] // r.bn)
        per_clip = -(-H // r.ph) * -(-W // r.pw)
        f["B"], P = rc.walk_batch(G, per_clip)
        period = (G, per_clip, P)
    yH, yW = (2 * H, 2 * W) if mode == 1 else (f["yH"] or H, f["yW"] or W)
    c1 = 2 if f.get("c1_spec64") else 1 if f.get("c1_x32") else 0
    key = dict(clips=period[2] if walk else f["B"], B=f["B"], H=H, W=W, C0=f["C0"], C1=f["C1"], H1=f["H1"], W1=f["W1"], Cout=f["Cout"],
               mode=mode, walk=period, c1=c1, affine=bool(f.get("in_scale0")), scale=bool(f.get("out_scale")),
               shift=bool(f.get("out_shift")), relu=bool(f["relu"]), yH=yH, yW=yW, pool=bool(f.get("y_pool")), w1x1=bool(f.get("w1x1")),
               stats=(r.ph, r.pw) if f.get("stats_part") else None, bwd=bool(f.get("bwd_z")))
    return f, r, tuple(sorted(key.items()))


def _run(lib, name, fields, want, walk=False, fold=False):
    from musicfpaugment_amd import ops_unet as K
    h = lib.lib()
    f, r, key = _plan(lib, name, fields, want, walk, torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
    ref = _reference(key)
    B, H, W, C0, C1, Cout, mode, prec, lay = (f[k] for k in ("B", "H", "W", "C0", "C1", "Cout", "mode", "precision", "w_layout"))
    n, yH, yW = dict(key)["clips"], dict(key)["yH"], dict(key)["yW"]
    c1 = dict(key)["c1"]
    clip = torch.arange(B) % n                                             # clip b holds the data of clip b % P
    in16 = bool(f.get("x0_is_bf16"))
    keep, guarded, p = [], [], {}

    def dev(t, field, dtype=torch.float32):
        t = t.to(dtype).contiguous().cuda()
        keep.append(t)
        p[field] = lib.ptr(t)
        return t

    def nhwc(t, dtype=torch.float32):                                      # (n, C, H, W) float64 -> (B, H, W, C) on the CPU
        return t.permute(0, 2, 3, 1).to(dtype)[clip].contiguous()

    def out(field, shape, dtype=torch.float32):
        numel = 1
        for k in shape:
            numel *= k
        buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        guarded.append((field, buf, numel))
        p[field] = buf.data_ptr() + GUARD * buf.element_size()
        return buf[GUARD:GUARD + numel].view(shape)

    # ---- operands
    w = ref["w"].float()
    if fold:                                                               # the scale already in the weights (a power of two: still exact in bf16)
        w = w * ref["out_scale"].float()[None, :, None]
    wdev = w.cuda()
    dev(wdev if prec == 0 else K.split_bf16x3_frag(wdev, 2) if lay == 2 else K.split_bf16x3(wdev), "w")
    src16 = torch.bfloat16 if in16 else torch.float32
    if c1:
        p["x0"] = 0
        dev(ref["c1_w"], "c1_w"); dev(torch.ones(64), "c1_scale"); dev(ref["c1_shift"], "c1_shift")
        if c1 == 2:
            dev(ref["c1_spec"][clip], "c1_spec64", torch.float64); dev(ref["c1_denom"][clip], "c1_denom", torch.float64)
        else:
            dev(ref["c1_x"][clip], "c1_x32")
    else:
        x0 = nhwc(ref["x0"], src16)
        assert not in16 or torch.equal(x0[:n].double(), nhwc(ref["x0"], torch.float64)[:n])      # bfloat16 sources lose nothing
        dev(_to_split(x0) if f.get("x0_split") else x0, "x0", x0.dtype)
        if f.get("in_scale0"):
            dev(torch.ones(C0), "in_scale0"); dev(ref["in_shift"], "in_shift0")
    if C1:
        x1 = nhwc(ref["x1"], src16)
        dev(_to_split(x1) if f.get("x1_split") else x1, "x1", x1.dtype)
    if f.get("out_scale") and not fold:
        dev(ref["out_scale"], "out_scale")
    if fold:
        p["out_scale"] = 0
    if f.get("out_shift"):
        dev(ref["out_shift"], "out_shift")
    # ---- outputs, each between NaN guards
    got_y = out("y", (B, yH, yW, Cout)) if f.get("y", 1) else None
    if not f.get("y", 1):
        p["y"] = 0
    got_y16 = out("y_bf16", (B, yH, yW, Cout), torch.bfloat16) if f.get("y_bf16") else None
    got_x0 = out("x0_bf16", (B, H, W, C0), torch.bfloat16) if f.get("x0_bf16") else None
    got_x1 = out("x1_bf16", (B, f["H1"], f["W1"], C1), torch.bfloat16) if f.get("x1_bf16") else None
    got_pool = out("y_pool", (B, H // 2, W // 2, Cout)) if f.get("y_pool") else None
    got_1x1 = None
    if f.get("w1x1"):
        dev(ref["w1x1"], "w1x1")
        p["b1x1"] = ref["b1x1"]
        got_1x1 = out("y1x1", (B, H, W))
    rows = 0
    if f.get("stats_part"):
        rows = h.mfpa_conv_stats_rows(B, H, W, C0 + C1, Cout)
        assert rows == B * -(-H // r.ph) * -(-W // r.pw) * r.stats_rows and rows > 0, (name, rows)
        got_part = out("stats_part", (rows, 2, Cout))
    if f.get("bwd_z"):
        dev(nhwc(ref["bwd_z"]), "bwd_z")
        for k in ("bwd_scale", "bwd_shift", "bwd_mean", "bwd_invstd"):
            dev(ref[k], k)
    d = rc.desc(lib, **{**f, **p})
    code, got, _ = rc.route(lib, d)                                        # the same route with the real pointers
    assert code == 0 and got == want, (name, code, got, want)
    lib.check(h.mfpa_conv_mfma(ctypes.byref(d), lib.stream()), name)
    if rows:
        sums = torch.full((2 * Cout,), float("nan"), dtype=torch.float64, device="cuda")
        work = torch.empty(h.mfpa_red_blocks() * 2 * 1024, dtype=torch.float64, device="cuda")
        lib.check(h.mfpa_conv_stats_reduce(lib.ptr(got_part), rows, Cout, lib.ptr(sums), lib.ptr(work), lib.stream()), name + ": stats_reduce")
    torch.cuda.synchronize()
    for field, buf, numel in guarded:
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + numel:]).all()), (name, field, "written outside the tensor")
    # ---- every element of every output
    y32 = nhwc(ref["y"])
    tag = name + (" (scale folded into the weights)" if fold else "")
    if got_y is not None and f.get("y_split"):
        hi, lo = _split(y32)
        got2 = got_y.cpu().view(torch.bfloat16).reshape(B, yH, yW, Cout // 32, 64)
        _same(tag + ": y, split hi", got2[..., :32].contiguous(), hi)
        _same(tag + ": y, split lo", got2[..., 32:].contiguous(), lo)
    elif got_y is not None:
        _same(tag + ": y", got_y.cpu(), y32)
    if got_y16 is not None:
        _same(tag + ": y_bf16", got_y16.cpu(), y32.bfloat16())
    if got_x0 is not None:
        _same(tag + ": x0_bf16", got_x0.cpu(), nhwc(ref["a0"]).bfloat16())
    if got_x1 is not None:
        _same(tag + ": x1_bf16", got_x1.cpu(), nhwc(ref["x1"]).bfloat16())
    if got_pool is not None and f.get("y_pool_split"):
        hi, lo = _split(nhwc(ref["y_pool"]))
        got2 = got_pool.cpu().view(torch.bfloat16).reshape(B, H // 2, W // 2, Cout // 32, 64)
        _same(tag + ": y_pool, split hi", got2[..., :32].contiguous(), hi)
        _same(tag + ": y_pool, split lo", got2[..., 32:].contiguous(), lo)
    elif got_pool is not None:
        _same(tag + ": y_pool", got_pool.cpu(), nhwc(ref["y_pool"]))
    if got_1x1 is not None:
        _same(tag + ": y1x1", got_1x1.cpu(), ref["y1x1"].float()[clip].contiguous())
    if rows:
        _same(tag + ": reduced stats_part", sums.cpu().view(Cout, 2), ref["sums"] * (B // n))
    return got


def _params(group):
    return pytest.mark.parametrize("name,fields,want", GROUPS[group], ids=[c[0] for c in GROUPS[group]])


def _folds(lib, f):
    """The launches whose folded form (out_scale = NULL, the scale in the weights) is run as well: where mfpa_conv_scale_folds says 1."""
    return bool(f.get("out_scale")) and f.get("w_layout") == 2 and \
        lib.lib().mfpa_conv_scale_folds(f.get("H", 8), f.get("W", 33), f.get("C0", 64) + f.get("C1", 0), f.get("Cout", 64)) == 1


@_params("inst")
def test_every_instantiation_two_clips_ragged_extents(lib, name, fields, want):
    _run(lib, name, fields, want)


def test_the_instantiation_cases_reach_all_66_kernels(lib):
    """Each case above asserts that its launch is routed to the instantiation its row names; together the rows name the whole family."""
    reached = {rc.route(lib, rc.desc(lib, **fields))[1] for _, fields, _ in GROUPS["inst"]}
    assert reached == {want for _, _, want in GROUPS["inst"]} == rc.KERNELS and len(rc.KERNELS) == 66, sorted(rc.KERNELS - reached)


@_params("pair")
def test_two_sources(lib, name, fields, want):
    _run(lib, name, fields, want)


@_params("epi")
def test_epilogue_features(lib, name, fields, want):
    _run(lib, name, fields, want)
    if _folds(lib, fields):
        _run(lib, name, fields, want, fold=True)


def test_some_epilogue_cases_fold():
    """The folded form is exercised on conv_ws64_kernel (with and without the fused first layer, pool, 1x1, split) and on conv_wd16_kernel."""
    from musicfpaugment_amd import _lib
    folded = {want[0] for _, f, want in GROUPS["epi"] if _folds(_lib, f)}
    assert folded == {"ws64", "wd16"}, folded


@_params("walk")
def test_tile_walk_on_a_periodic_batch(lib, name, fields, want):
    _run(lib, name, fields, want, walk=True)
