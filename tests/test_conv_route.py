"""mfpa_conv_mfma_route (include/mfpa.h): the routing of the UNet convolution family, host arithmetic only -- no GPU.  The case table
(tests/_conv_route_cases.py) pins which template instantiation serves a descriptor, the threshold edges pin each constant of the "Tile
choice" block of csrc/unet.hip (the row-image kernels it names live in csrc/unet_mfma.hip), the rejects pin that the route and the launcher refuse the same descriptors, and the query sweep pins
that mfpa_conv_scale_folds / mfpa_conv_c1_layout / mfpa_conv_stats_rows say what the route says."""
import ctypes
import os

import pytest

from tests import _conv_route_cases as rc

LEVELS = [(257, 251), (128, 125), (64, 62), (32, 31), (16, 15), (8, 17), (7, 17), (16, 16), (15, 16)]
CHANNELS = (32, 64, 96, 128, 192, 256, 512, 1024)


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def test_case_table_names_every_instantiation(lib):
    seen = set()
    for name, fields, want in rc.cases():
        code, got, r = rc.route(lib, rc.desc(lib, **fields))
        assert code == 0 and got == want, (name, code, got, want)
        seen.add(got)
    assert seen == rc.KERNELS, (sorted(rc.KERNELS - seen), sorted(seen - rc.KERNELS))
    assert len(rc.KERNELS) == 66


def test_exact_case_table_routes(lib):
    """The table of tests/test_gpu_conv_exact.py: every row gets the instantiation it names (a routing change that moves a case to another
    kernel fails here, without a GPU), the per-instantiation group alone reaches all 66, every walk case is a persistent kernel with
    2 G < tiles < 3 G and a period that does not divide G, and the walk group holds every persistent form."""
    groups = rc.exact_cases(cus=256)
    assert sorted(groups) == ["epi", "inst", "pair", "walk"]
    seen = {g: set() for g in groups}
    names = set()
    for group, rows in groups.items():
        for name, fields, want in rows:
            assert (group, name) not in names, (group, name)
            names.add((group, name))
            code, got, r = rc.route(lib, rc.desc(lib, **fields))
            assert code == 0 and got == want, (group, name, code, got, want)
            seen[group].add(got)
            if group != "walk":
                assert fields["B"] == 2, (group, name)
    assert seen["inst"] == rc.KERNELS and len(rc.KERNELS) == 66, (sorted(rc.KERNELS - seen["inst"]), sorted(seen["inst"] - rc.KERNELS))
    assert set().union(*seen.values()) == rc.KERNELS
    # the per-instantiation rows are ragged against their patch in both directions, and cover two clips
    for name, fields, want in groups["inst"]:
        ph, pw = rc.patch(want)
        assert fields["H"] % ph and fields["W"] % pw and fields.get("C1", 0) == 0, name
    # two sources everywhere in `pair`, with a smaller second source
    for name, fields, want in groups["pair"]:
        assert fields["C1"] > 0 and fields["H1"] < fields["H"] and fields["W1"] < fields["W"], name
    assert {(f["H"] - f["H1"], f["W"] - f["W1"]) for _, f, _ in groups["pair"]} == {(1, 1), (3, 2), (5, 2)}
    persistent = {k for k in rc.KERNELS if rc.walks(k)}
    assert len(persistent) == 25                                           # 2 ws64 + 7 WMW 4 + 14 PLAIN at WMW 2 + the 2 plain-loop taps forms
    assert seen["walk"] == persistent, sorted(persistent - seen["walk"])
    for name, fields, want in groups["walk"]:
        assert want[0] == "ws64" or rc.wd16_persist(want[3], want[4], want[5], want[6]), name
        _, _, r = rc.route(lib, rc.desc(lib, **fields))
        G = 256 // (fields.get("Cout", 64) // r.bn)
        per_clip = -(-fields["H"] // r.ph) * -(-fields["W"] // r.pw)
        B, P = rc.walk_batch(G, per_clip)
        assert B == fields["B"] and B % P == 0 and 2 * G < B * per_clip < 3 * G and G % (per_clip * P) != 0, (name, G, B, P)
    assert rc.walk_batch(256, 4) == (162, 3) and rc.walk_batch(256, 2) == (321, 3)
    assert rc.walk_batch(240, 4) == (154, 7)                                # 240 % 12 == 0 and 240 % 20 == 0: the period after those


def test_route_fields(lib):
    """The fields that name no template parameter: channels per workgroup, rows of stats_part per tile, the no-op, the optional out."""
    h = lib.lib()
    _, _, r = rc.route(lib, rc.desc(lib, Cout=128, C0=256, stats_part=1, **rc.FRAG))
    assert (r.bn, r.wmw, r.stats_rows, r.mode, r.prec) == (128, 2, 2, 0, 1)
    _, _, r = rc.route(lib, rc.desc(lib, stats_part=1, **rc.FRAG))
    assert (r.bn, r.wmw, r.stats_rows) == (64, 4, 4)
    _, _, r = rc.route(lib, rc.desc(lib, Cout=128, C0=256, **rc.FRAG))
    assert r.stats_rows == 0                                               # nothing asked for, nothing written
    _, _, r = rc.route(lib, rc.desc(lib, **rc.FRAG))
    assert (r.family, r.bn, r.ph, r.pw, r.stats_rows) == (rc.WS64, 64, 8, 32, 0)
    r = lib.ConvRoute(family=7)
    assert h.mfpa_conv_mfma_route(None, ctypes.byref(r)) == lib.EINVAL and r.family == rc.NONE
    assert h.mfpa_conv_mfma_route(None, None) == lib.EINVAL
    d = rc.desc(lib, B=0, C0=48)                                           # the no-op comes before every other check
    r = lib.ConvRoute(family=7)
    assert h.mfpa_conv_mfma_route(ctypes.byref(d), ctypes.byref(r)) == 0 and r.family == rc.NONE
    assert h.mfpa_conv_mfma(ctypes.byref(d), None) == 0
    assert h.mfpa_conv_mfma_route(ctypes.byref(rc.desc(lib)), None) == 0   # out is optional


def test_threshold_edges(lib):
    def k(**f):
        code, got, _ = rc.route(lib, rc.desc(lib, **f))
        return got if code == 0 else code

    E = lib.EINVAL
    # CONV_BIG_MIN_CIN = 64: the 8-wave tile of the bf16x3 row-image loop, and the fragment image, from 64 input channels on
    assert k(precision=1, Cout=128, C0=32) == ("mfma", 128, 4, 32, 0, 1, 0) and k(precision=1, Cout=128, C0=64) == ("mfma", 128, 8, 32, 0, 1, 0)
    assert k(Cout=128, C0=32, **rc.FRAG) == E and k(Cout=128, C0=64, **rc.FRAG) == ("ws64", 0)
    # CONV_WS_ALL = 128: conv_ws64_kernel takes 128-channel-multiple outputs up to 128 input channels
    assert k(Cout=128, C0=128, **rc.FRAG) == ("ws64", 0) and k(Cout=128, C0=160, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0)
    assert k(Cout=256, C0=96, C1=32, x1=1, H1=8, W1=33, **rc.FRAG) == ("ws64", 0)
    # CONV_WD16_ROWS = 512 (and Cin % 64 == 0)
    assert k(Cout=128, C0=480, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0) and k(Cout=128, C0=512, **rc.FRAG) == ("wd16", 8, 32, 1, 2, 0, 0, 0, 0)
    assert k(Cout=128, C0=544, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0) and k(Cout=128, C0=448, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0)
    # the fp32 family (and mode 2) keeps 256
    for f in (dict(precision=0), dict(precision=0, mode=2), dict(precision=1, mode=2)):
        m, p = f.get("mode", 0), f["precision"]
        assert k(Cout=128, C0=224, **f) == ("mfma", 128, 4, 32, m, p, 0) and k(Cout=128, C0=256, **f) == ("mfma", 128, 8, 32, m, p, 0)
    # W 16 / 17
    assert k(precision=1, Cout=128, H=16, W=16) == ("mfma", 128, 16, 16, 0, 1, 0) and k(precision=1, Cout=128, H=16, W=17) == ("mfma", 128, 8, 32, 0, 1, 0)
    assert k(Cout=128, C0=256, H=16, W=16, **rc.FRAG) == ("wd16", 16, 16, 0, 2, 0, 0, 0, 0)
    assert k(Cout=128, C0=256, H=16, W=17, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0)
    assert k(mode=1, H=16, W=16) == ("convT", 8, 16, 0, 0, 0) and k(mode=1, H=16, W=17) == ("convT", 4, 32, 0, 0, 0)
    # H 7 / 8 at W > 16
    assert k(precision=1, Cout=128, H=7, W=17) == ("mfma", 128, 4, 32, 0, 1, 0) and k(precision=1, Cout=128, H=8, W=17) == ("mfma", 128, 8, 32, 0, 1, 0)
    assert k(Cout=128, H=7, W=17, **rc.FRAG) == E and k(Cout=128, H=8, W=17, **rc.FRAG) == ("ws64", 0)
    assert k(H=7, W=17, **rc.FRAG) == E and k(H=8, W=17, **rc.FRAG) == ("ws64", 0)
    # H 15 / 16 at W <= 16
    assert k(precision=1, Cout=128, H=15, W=16) == ("mfma", 128, 8, 16, 0, 1, 0) and k(precision=1, Cout=128, H=16, W=16) == ("mfma", 128, 16, 16, 0, 1, 0)
    assert k(Cout=128, H=15, W=16, **rc.FRAG) == E and k(Cout=128, H=16, W=16, **rc.FRAG) == ("wd16", 16, 16, 0, 2, 0, 0, 0, 0)
    assert k(H=16, W=16, **rc.FRAG) == E                                  # 64-channel tiles have no 16 x 16 patch
    # Cout 64 / 128 / 192 at 256 input channels
    assert k(Cout=64, C0=256, **rc.FRAG) == ("ws64", 0) and k(Cout=128, C0=256, **rc.FRAG) == ("wd16", 8, 32, 0, 2, 0, 0, 0, 0)
    assert k(Cout=192, C0=256, **rc.FRAG) == ("ws64", 0) and k(Cout=192, C0=96, **rc.FRAG) == E       # 64-channel tiles: Cin % 64
    assert k(Cout=192, C0=256, stats_part=1, **rc.FRAG) == ("wd16", 8, 32, 0, 4, 1, 0, 0, 0)
    assert k(precision=1, Cout=192, C0=256) == ("mfma", 64, 8, 32, 0, 1, 0)


# (base descriptor, one change) -- every condition that rejects a launch of the family
TRAIN = dict(Cout=128, C0=256, stats_part=1, **rc.FRAG)                # the training forward's launch
PAIR = dict(Cout=128, C0=64, C1=64, x1=1, H1=8, W1=33, **rc.FRAG)      # a decoder launch: two sources (conv_ws64_kernel)
BWD = dict(bwd_z=1, bwd_scale=1, bwd_shift=1, bwd_mean=1, bwd_invstd=1)
REJECTS = [
    ({}, dict(x0=0)), ({}, dict(w=0)), ({}, dict(y=0)), ({}, dict(B=-1)), ({}, dict(H=0)), ({}, dict(W=0)),
    ({}, dict(C0=0)), ({}, dict(C0=48)), ({}, dict(C1=-32)), ({}, dict(C1=48, x1=1, H1=8, W1=33)), ({}, dict(Cout=0)), ({}, dict(Cout=96)),
    ({}, dict(mode=-1)), ({}, dict(mode=3)),
    (PAIR, dict(x1=0)), (PAIR, dict(H1=0)), (PAIR, dict(W1=0)), (PAIR, dict(H1=9)), (PAIR, dict(W1=34)), (PAIR, dict(mode=2, precision=1, w_layout=0)),
    ({}, dict(in_scale0=1)), ({}, dict(in_shift0=1)),
    ({}, dict(H=4096, W=4096, Cout=64)),                                     # a clip's output beyond 32-bit byte offsets
    ({}, dict(yH=9)), ({}, dict(yW=34)),
    ({}, dict(drop_thresh=1)), (dict(mode=2, **rc.AFF), dict(drop_thresh=1)),
    (dict(mode=2), dict(y_pool=1)), (dict(mode=1), dict(w1x1=1, y1x1=1)),
    ({}, dict(y_pool=1, H=1)), ({}, dict(y_pool=1, yH=7)), ({}, dict(y_pool=1, W=1)),
    ({}, dict(w1x1=1)), (dict(Cout=128), dict(w1x1=1, y1x1=1)),
    (rc.C1, dict(mode=2)), (rc.C1, dict(C0=128)), (rc.C1, dict(C1=32, x1=1, H1=8, W1=33)), (rc.C1, dict(Cout=128)), (rc.C1, dict(W=16)),
    (rc.C1, dict(H=7)), (rc.C1, dict(c1_w=0)), (rc.C1, dict(c1_scale=0)), (rc.C1, dict(c1_shift=0)), (rc.C1, dict(rc.AFF)),
    (rc.C1, dict(c1_spec64=1)), (rc.C1, dict(x0_is_bf16=1, mode=0, precision=2, w_layout=2)),
    ({}, dict(precision=-1)), ({}, dict(precision=3)),
    (TRAIN, dict(w_layout=1)), (TRAIN, dict(w_layout=3)), (TRAIN, dict(w_layout=-1)), (TRAIN, dict(mode=2)), (TRAIN, dict(precision=0)),
    ({}, dict(precision=2)),                                                 # plain bf16 3x3: the fragment image only
    (dict(mode=1), dict(precision=2)),                                       # plain bf16 transposed conv: bfloat16 I/O only
    (rc.IN16, dict(precision=1)), (dict(rc.IN16, Cout=128, C0=128), dict(C0=96)), (dict(rc.IN16, Cout=128, C0=64, C1=64, x1=1, H1=8, W1=33), dict(x1_bf16=1)),
    (dict(mode=1, precision=1, x0_is_bf16=1), dict(precision=0)),            # fp32 transposed convolution with a bfloat16 source
    (dict(mode=1, precision=1, y=0, y_bf16=1), dict(precision=0)),           # ... with a bfloat16-only output
    (dict(mode=2), dict(x0_is_bf16=1, precision=1)),
    (PAIR, dict(x0_split=1, mode=2, w_layout=0)), (PAIR, dict(x0_split=1, precision=2)), (PAIR, dict(x0_split=1, w_layout=0)),
    (dict(rc.FRAG), dict(x1_split=1)), (dict(rc.FRAG, w1x1=1, y1x1=1, y=0), dict(y_split=1)), (dict(rc.FRAG), dict(y_pool_split=1)),
    (dict(rc.C1, **rc.FRAG), dict(x0_split=1, x0=1)),
    (dict(rc.FRAG, Cout=128, C0=256), dict(x0_split=1)),                     # a split tensor where conv_ws64_kernel does not serve: too many input channels,
    (dict(rc.FRAG), dict(y_split=1, yH=7)),                                  # ... a cropped output,
    (dict(rc.FRAG, **rc.AFF), dict(x0_split=1)),                             # ... an on-load affine
    ({}, dict(x0_bf16=1)), (dict(rc.C1, **rc.FRAG), dict(x0_bf16=1)), (dict(mode=1, precision=1), dict(x0_bf16=1, precision=0)),
    (dict(Cout=128, C0=64, C1=64, x1=1, H1=8, W1=33), dict(x1_bf16=1)), (dict(rc.FRAG), dict(x1_bf16=1)),
    ({}, dict(y_bf16=1)), (dict(mode=1, precision=1), dict(y_bf16=1)), (dict(mode=1), dict(y=0, y_bf16=1)),
    (dict(rc.FRAG, y=0, y_bf16=1), dict(y_pool=1)), (dict(rc.FRAG, y=0, y_bf16=1), dict(w1x1=1, y1x1=1)),
    ({}, dict(stats_part=1)), (dict(rc.FRAG, w1x1=1, y1x1=1, y=0), dict(stats_part=1)),
    (TRAIN, dict(bwd_z=1)), (TRAIN, dict(BWD, bwd_mean=0)), (dict(rc.FRAG, Cout=128, C0=256), dict(BWD)),
    (dict(rc.IN16, stats_part=1, **BWD), dict(rc.AFF)), (dict(rc.IN16, stats_part=1, **BWD), dict(x0_bf16=1)),
    ({}, dict(H=32768, W=1, C0=32)), ({}, dict(H=1, W=32768, C0=32)),         # 16-bit coordinates
    (dict(Cout=64), dict(H=8192, W=8192, C0=32)),                            # a clip's input beyond 32-bit byte offsets (the output is checked first)
    (dict(mode=2, Cout=64), dict(H=4096, W=4096, C0=32)),                    # mode 2 reads (2H, 2W)
    (TRAIN, dict(C0=32)), (TRAIN, dict(H=7)), (TRAIN, dict(W=16)), (dict(rc.FRAG, stats_part=1), dict(C0=96)),     # the weight layout
    (dict(rc.FRAG, **rc.AFF), dict(C0=96, Cout=192)),                        # cin % 64 on 64-channel tiles (WMW 4)
]


def test_rejects_are_the_launchers_rejects(lib):
    """One change to a routable descriptor: the route and the launcher both answer MFPA_EINVAL (the launcher before it touches a device --
    there is none here)."""
    h = lib.lib()
    for base, change in REJECTS:
        code, got, _ = rc.route(lib, rc.desc(lib, **base))
        assert code == 0 and got is not None, ("base", base, code)
        d = rc.desc(lib, **{**base, **change})
        r = lib.ConvRoute(family=7)
        assert h.mfpa_conv_mfma_route(ctypes.byref(d), ctypes.byref(r)) == lib.EINVAL, (base, change)
        assert r.family == rc.NONE, (base, change)
        assert h.mfpa_conv_mfma(ctypes.byref(d), None) == lib.EINVAL, (base, change)
    # the tile count is a 32-bit grid extent: 2^31 tiles of one 8 x 16 patch
    d = rc.desc(lib, H=8, W=16, B=(1 << 31) - 1)
    assert rc.route(lib, d)[0] == 0
    d = rc.desc(lib, H=9, W=16, B=(1 << 31) - 1)
    assert rc.route(lib, d)[0] == lib.EINVAL and h.mfpa_conv_mfma(ctypes.byref(d), None) == lib.EINVAL
    # the two older entry points keep their own argument checks and route through the same function
    assert h.mfpa_conv3x3_bn_relu(1, 32, None, 0, 0, 0, 1, 32768, 1, 1, 64, None, None, 1, 0, 1, None) == lib.EINVAL
    assert h.mfpa_conv3x3_bn_relu(1, 32, None, 0, 0, 0, (1 << 31) - 1, 9, 16, 1, 64, None, None, 1, 0, 1, None) == lib.EINVAL
    assert h.mfpa_convT2x2(1, 1, 32768, 1, 32, 1, 1, 64, 0, 1, None) == lib.EINVAL


def layout_by_the_header(H, W, cin, cout):
    """mfpa_conv_weight_layout(.., mode 0, precision 1) as csrc/unet.hip's comment states it: the fragment image from 64 input channels on,
    on the 8 x 32 patches of the wide levels (W > 16, H >= 8) or, for 128-channel tiles, the 16 x 16 patches of W <= 16, H >= 16;
    64-channel tiles need Cin % 64 == 0."""
    if cin < 64:
        return 0
    wide = W > 16 and H >= 8
    if cout % 128:
        return 2 if wide and cout % 64 == 0 and cin % 64 == 0 else 0
    return 2 if wide or (W <= 16 and H >= 16) else 0


def check_raw_queries(h):
    """The four host queries over the sweep, against the rules as the header and the tile-choice comment state them.  Uses only entry points
    that exist since ABI 44 (it was run once against a library built from the commit before the route existed)."""
    n = 0
    for H, W in LEVELS:
        wide = W > 16 and H >= 8
        for cin in CHANNELS:
            for cout in CHANNELS:
                lay = layout_by_the_header(H, W, cin, cout)
                assert h.mfpa_conv_weight_layout(H, W, cin, cout, 0, 1) == lay, (H, W, cin, cout)
                for mode, prec in ((0, 0), (0, 2), (1, 1), (2, 1)):
                    assert h.mfpa_conv_weight_layout(H, W, cin, cout, mode, prec) == 0
                # conv_ws64_kernel: the wide levels' fragment-image launches with 64-channel tiles, or up to 128 input channels
                folds = 1 if lay == 2 and wide and cout % 64 == 0 and (cout % 128 != 0 or cin <= 128) else 0
                assert h.mfpa_conv_scale_folds(H, W, cin, cout) == folds, (H, W, cin, cout)
                # conv_wd16_kernel: 256-pixel patches (8 x 32, 16 x 16 at W <= 16), one row per wave row: 2 at 128-channel tiles, else 4
                for B in (1, 3):
                    pw = 32 if W > 16 else 16
                    ph = 256 // pw
                    rows = -(-W // pw) * -(-H // ph) * B * (2 if cout % 128 == 0 else 4) if lay == 2 else 0
                    assert h.mfpa_conv_stats_rows(B, H, W, cin, cout) == rows, (B, H, W, cin, cout)
                n += 1
        assert h.mfpa_conv_c1_layout(H, W) == (2 if wide else 0), (H, W)
    return n


def test_queries_say_what_the_route_says(lib):
    h = lib.lib()
    assert check_raw_queries(h) == len(LEVELS) * len(CHANNELS) ** 2
    for H, W in LEVELS:
        for cin in CHANNELS:
            for cout in CHANNELS:
                at = (H, W, cin, cout)
                shape = dict(H=H, W=W, C0=cin, Cout=cout)
                code, got, _ = rc.route(lib, rc.desc(lib, **shape, **rc.FRAG))                  # the plain inference launch
                assert (h.mfpa_conv_scale_folds(*at) == 1) == (code == 0 and got is not None and got[0] == "ws64"), at
                for B in (1, 3):
                    code, got, r = rc.route(lib, rc.desc(lib, B=B, stats_part=1, **shape, **rc.FRAG))      # the training forward's launch
                    rows = -(-W // r.pw) * -(-H // r.ph) * B * r.stats_rows if code == 0 else 0
                    assert h.mfpa_conv_stats_rows(B, *at) == rows, (B,) + at
                    assert code != 0 or (got[0] == "wd16" and r.stats_rows == r.wmw), at
        code, got, _ = rc.route(lib, rc.desc(lib, H=H, W=W, **rc.C1, **rc.FRAG))                 # the fused first layer
        assert (h.mfpa_conv_c1_layout(H, W) == 2) == (code == 0 and got == ("ws64", 1)), (H, W)


def test_queries_keep_their_answers_where_no_launch_exists(lib):
    """The queries answer from the shape rules alone (include/mfpa.h says so at each): beyond the limits a launch must also meet they say
    what they said before the route existed, while the route rejects the launch or sends it to conv_wd16_kernel."""
    h = lib.lib()
    assert h.mfpa_conv_stats_rows(1, 128, 125, 65, 128) == 128                       # Cin % 32: no launch
    assert rc.route(lib, rc.desc(lib, H=128, W=125, C0=65, Cout=128, stats_part=1, **rc.FRAG))[0] == lib.EINVAL
    assert h.mfpa_conv_scale_folds(40000, 64, 64, 64) == 1 and h.mfpa_conv_c1_layout(40000, 64) == 2      # 16-bit coordinates
    assert rc.route(lib, rc.desc(lib, H=40000, W=64, **rc.FRAG))[0] == lib.EINVAL
    assert h.mfpa_conv_scale_folds(2048, 2047, 256, 64) == 1                          # past conv_ws64_kernel's byte-offset limit: conv_wd16_kernel
    assert rc.route(lib, rc.desc(lib, H=2048, W=2047, C0=256, Cout=64, **rc.FRAG))[1] == ("wd16", 8, 32, 0, 4, 0, 0, 0, 0)
    assert h.mfpa_conv_stats_rows((1 << 31) - 1, 16, 32, 64, 128) == lib.EINVAL        # 2 x 2 rows per clip: beyond 2^31 - 1
    assert h.mfpa_conv_stats_rows(0, 16, 32, 64, 128) == 0
