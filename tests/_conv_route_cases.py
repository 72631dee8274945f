"""Case table of mfpa_conv_mfma_route (include/mfpa.h): descriptors and the template instantiation each must get, written from the header
text and the "Tile choice" comment of csrc/unet.hip -- not from the function under test.  Shared by tests/test_conv_route.py (CPU),
tests/test_gpu_conv_route.py (one launch per row) and tests/test_gpu_conv_exact.py (the second table, exact_cases(): every element).

An instantiation is named by a tuple:
    ("ws64", C1SRC)                                              conv_ws64_kernel<C1SRC>
    ("wd16", PH, PW, ROWS, WMW, SIDE, PLAIN, IN16, AFF16)        conv_wd16_kernel<...>
    ("mfma", BN, PH, PW, MODE, PREC, C1SRC)                      conv_mfma_kernel<BN, PH, PW, PH * PW / 64, BN / 64, MODE, PREC, C1SRC>
    ("convT", PH, PW, PREC, IO16, PLAIN)                         convT_mfma_kernel<...>
"""
import ctypes

NONE, WS64, WD16, MFMA, CONVT = -1, 0, 1, 2, 3       # MFPA_CONV_*

MFMA_TILES = [(64, 8, 32), (128, 8, 32), (128, 4, 32), (64, 4, 32), (128, 8, 16), (64, 8, 16)]
# (ROWS, SIDE, PLAIN, IN16, AFF16) of conv_wd16_kernel at WMW 2 (both patches) and at WMW 4 (the 8 x 32 patch)
WD16_FORMS_WMW2 = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (1, 0, 0, 0, 0), (1, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 1, 1, 0, 0), (1, 0, 1, 0, 0),
                   (1, 1, 1, 0, 0), (1, 0, 1, 1, 0), (1, 1, 1, 1, 0), (1, 1, 1, 1, 1)]
WD16_FORMS_WMW4 = [(0, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0), (0, 1, 1, 0, 0), (0, 0, 1, 1, 0), (0, 1, 1, 1, 0), (0, 1, 1, 1, 1)]

# every instantiation the launcher's table (CONV_KERNELS, csrc/unet.hip; the 29 wd16, 27 mfma and 8 convT forms from MFPA_WD16_FORMS / MFPA_MFMA_FORMS / MFPA_CONVT_FORMS,
# csrc/mfpa_unet_args.h; the row-image kernels themselves: csrc/unet_mfma.hip) names:
# 2 + 29 + 27 + 8 = 66 kernels
KERNELS = (
    {("ws64", 0), ("ws64", 1)}
    | {("wd16", ph, pw, r, 2, s, p, i, a) for ph, pw in ((8, 32), (16, 16)) for r, s, p, i, a in WD16_FORMS_WMW2}
    | {("wd16", 8, 32, r, 4, s, p, i, a) for r, s, p, i, a in WD16_FORMS_WMW4}
    | {("mfma", bn, ph, pw, mode, prec, 0) for bn, ph, pw in MFMA_TILES for mode in (0, 2) for prec in (0, 1)}
    | {("mfma", 128, 16, 16, 0, 1, 0), ("mfma", 64, 8, 32, 0, 0, 1), ("mfma", 64, 8, 32, 0, 1, 1)}
    | {("convT", ph, pw, prec, io16, plain) for ph, pw in ((4, 32), (8, 16)) for prec, io16, plain in ((0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1))}
)


def desc(lib, **kw):
    """mfpa_conv_desc with x0 / w / y given, one clip, a 3x3 convolution unless told otherwise.  Pointers are arbitrary non-null integers:
    the route looks at no memory."""
    d = dict(x0=1, w=1, y=1, C0=64, C1=0, B=1, H=8, W=33, Cout=64, mode=0)
    d.update(kw)
    return lib.ConvDesc(**d)


def route(lib, d):
    """(rc, instantiation tuple or None, the raw mfpa_conv_route)."""
    r = lib.ConvRoute()
    rc = lib.lib().mfpa_conv_mfma_route(ctypes.byref(d), ctypes.byref(r))
    if r.family == WS64:
        k = ("ws64", r.c1src)
    elif r.family == WD16:
        k = ("wd16", r.ph, r.pw, r.rows, r.wmw, r.side, r.plain, r.in16, r.aff16)
    elif r.family == MFMA:
        k = ("mfma", r.bn, r.ph, r.pw, r.mode, r.prec, r.c1src)
    elif r.family == CONVT:
        k = ("convT", r.ph, r.pw, r.prec, r.io16, r.plain)
    else:
        k = None
    return rc, k, r


C1 = dict(x0=0, c1_x32=1, c1_w=1, c1_scale=1, c1_shift=1)          # the fused first layer (64 -> 64)
AFF = dict(in_scale0=1, in_shift0=1)                                # the previous layer's BatchNorm + ReLU on load
FRAG = dict(precision=1, w_layout=2)                                # bf16x3 on the fragment image
PLAIN = dict(precision=2, w_layout=2)                               # plain bf16 (the training step)
IN16 = dict(precision=2, w_layout=2, x0_is_bf16=1)                  # ... with bfloat16 sources


def cases():
    """[(name, descriptor fields, instantiation)].  Shapes: 8 x 33 (two 8 x 32 patches), 16 x 16, 15 x 16, 7 x 17."""
    rows = []
    # conv_mfma_kernel, the row image: "Cout % 128 == 0: 128-channel tiles; 8 waves on 8x32 patches when K is long enough [Cin >= 64 for the
    # bf16x3 3x3 convolution, 256 for the others], else 4 waves on 4x32; otherwise 64-channel tiles on 8x32; W <= 16: 16x16 patches for the
    # bf16x3 3x3 convolution's 128-channel tiles [H >= 16], else 8x16"; H < 8 at W > 16: 4x32
    for mode in (0, 2):
        for prec in (0, 1):
            f = dict(mode=mode, precision=prec)
            n = f"mfma m{mode} p{prec} "
            rows += [(n + "64ch 8x32", dict(f, Cout=64), ("mfma", 64, 8, 32, mode, prec, 0)),
                     (n + "128ch long K", dict(f, Cout=128, C0=256), ("mfma", 128, 8, 32, mode, prec, 0)),
                     (n + "128ch short K", dict(f, Cout=128, C0=32), ("mfma", 128, 4, 32, mode, prec, 0)),
                     (n + "64ch H<8", dict(f, Cout=64, H=7, W=17), ("mfma", 64, 4, 32, mode, prec, 0)),
                     (n + "128ch W<=16", dict(f, Cout=128, H=15, W=16), ("mfma", 128, 8, 16, mode, prec, 0)),
                     (n + "64ch W<=16", dict(f, Cout=64, H=16, W=16), ("mfma", 64, 8, 16, mode, prec, 0))]
    rows += [("mfma 16x16", dict(precision=1, Cout=128, H=16, W=16), ("mfma", 128, 16, 16, 0, 1, 0)),
             ("mfma plain bf16 input gradient of the transposed conv", dict(mode=2, precision=2, Cout=64), ("mfma", 64, 8, 32, 2, 1, 0)),
             ("mfma c1 fp32", dict(C1, precision=0), ("mfma", 64, 8, 32, 0, 0, 1)),
             ("mfma c1 bf16x3 row image", dict(C1, precision=1), ("mfma", 64, 8, 32, 0, 1, 1))]
    # conv_ws64_kernel: "the fused first layer, the 64-channel outputs and the wider ones up to CONV_WS_ALL input channels"
    rows += [("ws64 64ch", dict(FRAG), ("ws64", 0)), ("ws64 c1", dict(C1, **FRAG), ("ws64", 1)),
             ("ws64 128ch, 128 in", dict(FRAG, Cout=128, C0=128), ("ws64", 0))]
    # conv_wd16_kernel: "the shapes it does not serve and the training step's launches".  SIDE: a bf16 copy / the partial statistics;
    # ROWS: 128-channel tiles, Cin % 64 == 0 and Cin >= 512 (plain bf16: any Cin % 64 == 0); bf16 sources: ROWS wherever WMW == 2,
    # AFF16 with an on-load affine (the training forward)
    for ph, pw, H, W in ((8, 32, 8, 33), (16, 16, 16, 16)):
        s = dict(Cout=128, H=H, W=W)
        n = f"wd16 {ph}x{pw} "
        rows += [(n + "taps", dict(s, C0=256, **FRAG), ("wd16", ph, pw, 0, 2, 0, 0, 0, 0)),
                 (n + "taps side", dict(s, C0=256, stats_part=1, **FRAG), ("wd16", ph, pw, 0, 2, 1, 0, 0, 0)),
                 (n + "rows", dict(s, C0=512, **FRAG), ("wd16", ph, pw, 1, 2, 0, 0, 0, 0)),
                 (n + "rows side", dict(s, C0=512, stats_part=1, **FRAG), ("wd16", ph, pw, 1, 2, 1, 0, 0, 0)),
                 (n + "plain taps", dict(s, C0=96, **PLAIN), ("wd16", ph, pw, 0, 2, 0, 1, 0, 0)),
                 (n + "plain taps side", dict(s, C0=96, y_bf16=1, **PLAIN), ("wd16", ph, pw, 0, 2, 1, 1, 0, 0)),
                 (n + "plain rows", dict(s, C0=128, **PLAIN), ("wd16", ph, pw, 1, 2, 0, 1, 0, 0)),
                 (n + "plain rows side", dict(s, C0=128, stats_part=1, **PLAIN), ("wd16", ph, pw, 1, 2, 1, 1, 0, 0)),
                 (n + "in16", dict(s, C0=128, **IN16), ("wd16", ph, pw, 1, 2, 0, 1, 1, 0)),
                 (n + "in16 side", dict(s, C0=128, stats_part=1, **IN16), ("wd16", ph, pw, 1, 2, 1, 1, 1, 0)),
                 (n + "in16 forward", dict(s, C0=128, stats_part=1, **IN16, **AFF), ("wd16", ph, pw, 1, 2, 1, 1, 1, 1))]
    rows += [("wd16 64ch", dict(FRAG, **AFF), ("wd16", 8, 32, 0, 4, 0, 0, 0, 0)),
             ("wd16 64ch side", dict(FRAG, stats_part=1), ("wd16", 8, 32, 0, 4, 1, 0, 0, 0)),
             ("wd16 64ch plain", dict(PLAIN), ("wd16", 8, 32, 0, 4, 0, 1, 0, 0)),
             ("wd16 64ch plain side", dict(PLAIN, x0_bf16=1), ("wd16", 8, 32, 0, 4, 1, 1, 0, 0)),
             ("wd16 64ch in16", dict(IN16), ("wd16", 8, 32, 0, 4, 0, 1, 1, 0)),
             ("wd16 64ch in16 side", dict(IN16, y=0, y_bf16=1, stats_part=1, bwd_z=1, bwd_scale=1, bwd_shift=1, bwd_mean=1, bwd_invstd=1),
              ("wd16", 8, 32, 0, 4, 1, 1, 1, 0)),
             ("wd16 64ch in16 forward", dict(IN16, y=0, y_bf16=1), ("wd16", 8, 32, 0, 4, 1, 1, 1, 1))]
    # convT_mfma_kernel (mode 1): 4x32 patches, 8x16 at W <= 16; bfloat16 I/O is a bf16x3 instantiation and carries the plain form
    for ph, pw, H, W in ((4, 32, 8, 33), (8, 16, 16, 16)):
        s = dict(mode=1, H=H, W=W)
        n = f"convT {ph}x{pw} "
        rows += [(n + "fp32", dict(s, precision=0), ("convT", ph, pw, 0, 0, 0)), (n + "bf16x3", dict(s, precision=1), ("convT", ph, pw, 1, 0, 0)),
                 (n + "bf16 I/O", dict(s, precision=1, y=0, y_bf16=1), ("convT", ph, pw, 1, 1, 0)),
                 (n + "plain", dict(s, precision=2, x0_is_bf16=1), ("convT", ph, pw, 1, 1, 1))]
    return rows


# ---------------------------------------------------------------------------------------------------------------------------------
# The second table: the descriptors of tests/test_gpu_conv_exact.py (every output element against a float64 reference on exact integer
# operands).  Same row form as cases(); a field that is a pointer is 1 here ("give this buffer") and a real address in the GPU test.

def wd16_persist(rows, wmw, side, plain):
    """The forms of conv_wd16_kernel whose grid is clamped to the CUs (one workgroup walks several tiles): every WMW == 4 form, every PLAIN
    form, and the non-ROWS non-SIDE ones."""
    return wmw == 4 or bool(plain) or (not rows and not side)


def patch(want):
    """(PH, PW) of an instantiation tuple."""
    return (8, 32) if want[0] == "ws64" else (want[2], want[3]) if want[0] == "mfma" else (want[1], want[2])


def walks(want):
    return want[0] == "ws64" or (want[0] == "wd16" and wd16_persist(want[3], want[4], want[5], want[6]))


def ragged(fields, want):
    """The extents of a row of cases() made ragged in both directions against the row's patch (modes 1 / 2: the matching input extents
    follow from H, W as everywhere in the descriptor)."""
    ph, pw = patch(want)
    return dict(H=7 if fields.get("H", 8) < 8 else 17 if ph == 16 else 9, W=33 if pw == 32 else 15)


def walk_batch(G, tiles_per_clip):
    """(B, P) of a tile-walk case: a batch of period P (clip b holds the data of clip b % P) with 2 G < tiles < 3 G, so that each of the G
    workgroups of a persistent kernel owns two tiles and some own three; B is a multiple of P (the statistics are then B / P times one
    period's) and G % (tiles_per_clip * P) != 0 -- else a workgroup's consecutive tiles, G apart, would be copies of one another."""
    for P in (3, 5, 7):
        if G % (tiles_per_clip * P):
            B = P * -(-5 * G // (2 * tiles_per_clip * P))
            if 2 * G < B * tiles_per_clip < 3 * G:
                return B, P
    raise ValueError(f"no periodic batch for {G} workgroups of {tiles_per_clip} tiles per clip")


EPI = dict(out_scale=1, out_shift=1, relu=1)
BWD = dict(bwd_z=1, bwd_scale=1, bwd_shift=1, bwd_mean=1, bwd_invstd=1)
C1S = dict(x0=0, c1_spec64=1, c1_denom=1, c1_w=1, c1_scale=1, c1_shift=1)     # the fused first layer from the float64 spectrogram
OUT1 = dict(w1x1=1, y1x1=1)


def _x1(C1=64, H=9, W=33, dh=1, dw=1):
    return dict(x1=1, C1=C1, B=2, H=H, W=W, H1=H - dh, W1=W - dw)


def exact_cases(cus=256):
    """{group: [(name, descriptor fields, instantiation)]}.  `inst`: every row of cases() with two clips and ragged extents; `pair`: two
    sources; `epi`: the epilogue's features, the split layout, c1_spec64; `walk`: the persistent kernels with more tiles than twice their
    grid (`cus`: the device's compute units -- the launcher clamps the grid to cus // grid.y)."""
    inst, walk = [], []
    for name, f, want in cases():
        # (every row keeps its route at the ragged shape -- tests/test_conv_route.py asserts it -- so none keeps its own)
        inst.append((name, dict(f, B=2, **ragged(f, want)), want))
        if walks(want) and name != "ws64 128ch, 128 in":
            s = ragged(f, want)
            ph, pw = patch(want)
            grid_y = f.get("Cout", 64) // (64 if want[0] == "ws64" or want[4] == 4 else 128)
            B, _ = walk_batch(cus // grid_y, -(-s["H"] // ph) * -(-s["W"] // pw))
            walk.append((name + " walk", dict(f, B=B, **s), want))
    wd = lambda ph, pw, *form: ("wd16", ph, pw) + form
    # An odd number of 32-channel chunks (C_in % 64 == 32, the tap-by-tap WMW = 2 forms only): a halo stage is chosen by the chunk's parity,
    # so these launches keep one tile per workgroup -- the batch is the same, more tiles than twice the CUs.  The plain taps rows above
    # (96 channels: their only shapes) are of this kind; here the bf16x3 taps form beside its 256-channel (walking) row above.
    for ph, pw, H, W in ((8, 32, 9, 33), (16, 16, 17, 15)):
        B, _ = walk_batch(cus, -(-H // ph) * -(-W // pw))
        walk.append((f"wd16 {ph}x{pw} taps, odd chunks walk", dict(FRAG, B=B, H=H, W=W, Cout=128, C0=160), wd(ph, pw, 0, 2, 0, 0, 0, 0)))
    mf = lambda bn, ph, pw, mode, prec, c1=0: ("mfma", bn, ph, pw, mode, prec, c1)
    P1 = dict(precision=1)
    # ---- two sources: source 1 one pixel smaller (zero-padded at the bottom / right), centred with offsets, the on-load affine on source 0 only
    pair = [("ws64", dict(FRAG, **_x1()), ("ws64", 0)),
            ("ws64 128ch", dict(FRAG, Cout=128, **_x1()), ("ws64", 0)),
            ("ws64 offsets", dict(FRAG, **_x1(dh=3, dw=2)), ("ws64", 0)),
            ("ws64 offsets 2 / 1", dict(FRAG, **_x1(dh=5, dw=2)), ("ws64", 0)),
            ("wd16 taps", dict(FRAG, Cout=128, C0=128, **_x1(128)), wd(8, 32, 0, 2, 0, 0, 0, 0)),
            ("wd16 taps offsets", dict(FRAG, Cout=128, C0=128, **_x1(128, dh=3, dw=2)), wd(8, 32, 0, 2, 0, 0, 0, 0)),
            ("wd16 taps offsets 2 / 1", dict(FRAG, Cout=128, C0=128, x1_bf16=1, **_x1(128, dh=5, dw=2)), wd(8, 32, 0, 2, 1, 0, 0, 0)),
            ("wd16 taps x1 copy", dict(FRAG, Cout=128, C0=128, x1_bf16=1, **_x1(128)), wd(8, 32, 0, 2, 1, 0, 0, 0)),
            ("wd16 16x16 taps x1 copy", dict(FRAG, Cout=128, C0=128, x1_bf16=1, **_x1(128, 17, 15)), wd(16, 16, 0, 2, 1, 0, 0, 0)),
            ("wd16 rows", dict(FRAG, Cout=128, C0=256, **_x1(256)), wd(8, 32, 1, 2, 0, 0, 0, 0)),
            ("wd16 rows copies", dict(FRAG, Cout=128, C0=256, x0_bf16=1, x1_bf16=1, **_x1(256)), wd(8, 32, 1, 2, 1, 0, 0, 0)),
            ("wd16 16x16 rows", dict(FRAG, Cout=128, C0=256, **_x1(256, 17, 15)), wd(16, 16, 1, 2, 0, 0, 0, 0)),
            ("wd16 plain taps", dict(PLAIN, Cout=128, **_x1(32)), wd(8, 32, 0, 2, 0, 1, 0, 0)),
            ("wd16 plain rows", dict(PLAIN, Cout=128, **_x1()), wd(8, 32, 1, 2, 0, 1, 0, 0)),
            ("wd16 plain rows copies", dict(PLAIN, Cout=128, x0_bf16=1, x1_bf16=1, **_x1()), wd(8, 32, 1, 2, 1, 1, 0, 0)),
            ("wd16 in16", dict(IN16, Cout=128, **_x1()), wd(8, 32, 1, 2, 0, 1, 1, 0)),
            ("wd16 in16 forward", dict(IN16, Cout=128, x0_bf16=1, **AFF, **_x1()), wd(8, 32, 1, 2, 1, 1, 1, 1)),
            ("wd16 64ch in16", dict(IN16, **_x1()), wd(8, 32, 0, 4, 0, 1, 1, 0)),
            ("wd16 64ch x1 copy", dict(FRAG, x1_bf16=1, **_x1()), wd(8, 32, 0, 4, 1, 0, 0, 0)),
            ("wd16 64ch affine on source 0", dict(FRAG, **AFF, **_x1()), wd(8, 32, 0, 4, 0, 0, 0, 0)),
            ("wd16 64ch affine, offsets, copies", dict(FRAG, x0_bf16=1, x1_bf16=1, **AFF, **_x1(dh=3, dw=2)), wd(8, 32, 0, 4, 1, 0, 0, 0)),
            ("mfma p0", dict(_x1()), mf(64, 8, 32, 0, 0)),
            ("mfma p1", dict(P1, **_x1()), mf(64, 8, 32, 0, 1)),
            ("mfma p0 offsets", dict(_x1(dh=3, dw=2)), mf(64, 8, 32, 0, 0)),
            ("mfma p1 offsets, 128ch", dict(P1, Cout=128, **_x1(dh=3, dw=2)), mf(128, 8, 32, 0, 1)),
            ("mfma p0 affine on source 0", dict(AFF, **_x1()), mf(64, 8, 32, 0, 0)),
            ("mfma p1 8x16", dict(P1, **_x1(64, 9, 15)), mf(64, 8, 16, 0, 1))]
    # ---- the epilogue: scale / shift / ReLU on every family
    epi = [("ws64 epilogue", dict(FRAG, B=2, H=9, **EPI), ("ws64", 0)),
           ("ws64 c1 epilogue", dict(C1, B=2, H=9, **FRAG, **EPI), ("ws64", 1)),
           ("ws64 128ch epilogue", dict(FRAG, B=2, H=9, Cout=128, C0=128, **EPI), ("ws64", 0)),
           ("wd16 taps epilogue", dict(FRAG, B=2, H=9, Cout=128, C0=256, **EPI), wd(8, 32, 0, 2, 0, 0, 0, 0)),
           ("wd16 rows epilogue, y copy", dict(FRAG, B=2, H=9, Cout=128, C0=512, y_bf16=1, **EPI), wd(8, 32, 1, 2, 1, 0, 0, 0)),
           ("wd16 16x16 taps epilogue", dict(FRAG, B=2, H=17, W=15, Cout=128, C0=256, **EPI), wd(16, 16, 0, 2, 0, 0, 0, 0)),
           ("wd16 64ch epilogue", dict(FRAG, B=2, H=9, **AFF, **EPI), wd(8, 32, 0, 4, 0, 0, 0, 0)),
           ("wd16 plain rows epilogue", dict(PLAIN, B=2, H=9, Cout=128, C0=128, **EPI), wd(8, 32, 1, 2, 0, 1, 0, 0)),
           ("wd16 in16 forward epilogue, bf16 only", dict(IN16, B=2, H=9, Cout=128, C0=128, y=0, y_bf16=1, **AFF, **EPI), wd(8, 32, 1, 2, 1, 1, 1, 1)),
           ("mfma m0 p0 epilogue", dict(B=2, H=9, **EPI), mf(64, 8, 32, 0, 0)),
           ("mfma m0 p1 epilogue", dict(P1, B=2, H=9, **EPI), mf(64, 8, 32, 0, 1)),
           ("mfma m0 p1 128ch epilogue", dict(P1, B=2, H=9, Cout=128, **EPI), mf(128, 8, 32, 0, 1)),
           ("mfma 16x16 epilogue", dict(P1, B=2, H=17, W=15, Cout=128, **EPI), mf(128, 16, 16, 0, 1)),
           ("mfma c1 p0 epilogue", dict(C1, B=2, H=9, **EPI), mf(64, 8, 32, 0, 0, 1)),
           ("mfma m2 p0 epilogue", dict(B=2, H=9, mode=2, **EPI), mf(64, 8, 32, 2, 0)),
           ("mfma m2 p1 epilogue", dict(P1, B=2, H=9, mode=2, **EPI), mf(64, 8, 32, 2, 1)),
           ("convT fp32 bias", dict(B=2, H=9, mode=1, out_shift=1), ("convT", 4, 32, 0, 0, 0)),
           ("convT bf16x3 epilogue", dict(P1, B=2, H=9, mode=1, **EPI), ("convT", 4, 32, 1, 0, 0)),
           ("convT 8x16 bf16 I/O bias", dict(P1, B=2, H=9, W=15, mode=1, y=0, y_bf16=1, out_shift=1), ("convT", 8, 16, 1, 1, 0))]
    # ---- the cropped output (modes 0 and 2): by one row and column, and by a full patch row
    for yH, yW in ((16, 32), (8, 33)):
        s = dict(B=2, H=17, W=33, yH=yH, yW=yW)
        n = f" crop {yH}x{yW}"
        epi += [("wd16 64ch" + n, dict(FRAG, **s), wd(8, 32, 0, 4, 0, 0, 0, 0)),
                ("wd16 taps side" + n, dict(FRAG, Cout=128, C0=256, stats_part=1, y_bf16=1, **s), wd(8, 32, 0, 2, 1, 0, 0, 0)),
                ("wd16 plain rows" + n, dict(PLAIN, Cout=128, C0=128, **s, **EPI), wd(8, 32, 1, 2, 0, 1, 0, 0)),
                ("mfma m0 p0" + n, dict(s, **EPI), mf(64, 8, 32, 0, 0)),
                ("mfma m0 p1 128ch" + n, dict(P1, Cout=128, **s), mf(128, 8, 32, 0, 1)),
                ("mfma m2 p0" + n, dict(s, mode=2), mf(64, 8, 32, 2, 0)),
                ("mfma m2 p1" + n, dict(P1, mode=2, **s, **EPI), mf(64, 8, 32, 2, 1))]
    # ---- the fused MaxPool2d(2) at odd extents, the fused OutConv with and without the output itself
    s = dict(B=2, H=9, W=33)
    epi += [("ws64 pool", dict(FRAG, y_pool=1, **s, **EPI), ("ws64", 0)),
            ("ws64 c1 pool", dict(C1, y_pool=1, **s, **FRAG), ("ws64", 1)),
            ("wd16 taps pool", dict(FRAG, Cout=128, C0=256, y_pool=1, **s, **EPI), wd(8, 32, 0, 2, 0, 0, 0, 0)),
            ("wd16 16x16 rows pool", dict(FRAG, B=2, H=17, W=15, Cout=128, C0=512, y_pool=1), wd(16, 16, 1, 2, 0, 0, 0, 0)),
            ("wd16 64ch pool", dict(FRAG, y_pool=1, **s, **AFF), wd(8, 32, 0, 4, 0, 0, 0, 0)),
            ("wd16 plain rows pool", dict(PLAIN, Cout=128, C0=128, y_pool=1, **s), wd(8, 32, 1, 2, 0, 1, 0, 0)),
            ("mfma p0 pool", dict(s, y_pool=1, **EPI), mf(64, 8, 32, 0, 0)),
            ("mfma p1 128ch pool", dict(P1, Cout=128, y_pool=1, **s), mf(128, 8, 32, 0, 1)),
            ("mfma p1 8x16 pool", dict(P1, B=2, H=9, W=15, y_pool=1), mf(64, 8, 16, 0, 1)),
            ("ws64 1x1", dict(FRAG, **s, **OUT1, **EPI), ("ws64", 0)),
            ("ws64 1x1 only", dict(FRAG, y=0, **s, **OUT1, **EPI), ("ws64", 0)),
            ("wd16 64ch 1x1", dict(FRAG, **s, **OUT1, **AFF, **EPI), wd(8, 32, 0, 4, 0, 0, 0, 0)),
            ("wd16 64ch 1x1 only", dict(FRAG, y=0, **s, **OUT1, **AFF), wd(8, 32, 0, 4, 0, 0, 0, 0)),
            ("wd16 64ch plain 1x1", dict(PLAIN, **s, **OUT1), wd(8, 32, 0, 4, 0, 1, 0, 0)),
            ("mfma p0 1x1", dict(s, **OUT1, **EPI), mf(64, 8, 32, 0, 0)),
            ("mfma p0 1x1 only", dict(s, y=0, **OUT1), mf(64, 8, 32, 0, 0)),
            ("mfma p1 1x1", dict(P1, **s, **OUT1, **EPI), mf(64, 8, 32, 0, 1))]
    # ---- the split layout of conv_ws64_kernel, one flag at a time and all together; the first layer from the float64 spectrogram
    sp = dict(FRAG, y_pool=1, **_x1(), **EPI)
    epi += [("ws64 x0_split", dict(sp, x0_split=1), ("ws64", 0)), ("ws64 x1_split", dict(sp, x1_split=1), ("ws64", 0)),
            ("ws64 y_split", dict(sp, y_split=1), ("ws64", 0)), ("ws64 y_pool_split", dict(sp, y_pool_split=1), ("ws64", 0)),
            ("ws64 all split", dict(sp, x0_split=1, x1_split=1, y_split=1, y_pool_split=1), ("ws64", 0)),
            ("ws64 c1_spec64", dict(C1S, **s, **FRAG, **EPI), ("ws64", 1)),
            ("mfma p0 c1_spec64", dict(C1S, **s), mf(64, 8, 32, 0, 0, 1)),
            ("mfma p1 c1_spec64", dict(C1S, **s, **P1, **EPI), mf(64, 8, 32, 0, 1, 1))]
    # ---- the BatchNorm backward's sums (bwd_z) beside the forward's statistics of the inst rows
    epi += [("wd16 taps side bwd_z", dict(FRAG, Cout=128, C0=256, stats_part=1, **s, **BWD), wd(8, 32, 0, 2, 1, 0, 0, 0)),
            ("wd16 16x16 plain rows side bwd_z", dict(PLAIN, B=2, H=17, W=15, Cout=128, C0=128, stats_part=1, **BWD), wd(16, 16, 1, 2, 1, 1, 0, 0)),
            ("wd16 64ch side bwd_z", dict(FRAG, stats_part=1, **s, **BWD), wd(8, 32, 0, 4, 1, 0, 0, 0))]
    return dict(inst=inst, pair=pair, epi=epi, walk=walk)
