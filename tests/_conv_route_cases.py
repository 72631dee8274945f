"""Case table of mfpa_conv_mfma_route (include/mfpa.h): descriptors and the template instantiation each must get, written from the header
text and the "Tile choice" comment of csrc/unet.hip -- not from the function under test.  Shared by tests/test_conv_route.py (CPU) and
tests/test_gpu_conv_route.py (one launch per row).

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

# every instantiation the launcher's table (CONV_KERNELS, csrc/unet.hip; the 29 wd16 forms from MFPA_WD16_FORMS, csrc/mfpa_unet_args.h) names:
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
