"""UNet building blocks over the C ABI (csrc/unet.hip and the kernels' own files unet_mfma.hip, unet_wd16.hip, unet_ws.hip, unet_up.hip): weight packing and the eval forward.

Activations are NHWC float32 tensors (B, H, W, C) -- H = frequency bins, W = frames.
"""
from __future__ import annotations

import ctypes
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from ._lib import ConvDesc, KernelTimer, UpconvDesc, check, lib, ptr, set_timer, stream, timed  # noqa: F401  (KernelTimer, set_timer: bench.py)

BN_EPS = 1e-5  # nn.BatchNorm2d default (training/unet.py:17,20)

ENC = ["inc.double_conv", "down1.maxpool_conv.1.double_conv", "down2.maxpool_conv.1.double_conv",
       "down3.maxpool_conv.1.double_conv", "down4.maxpool_conv.1.double_conv"]
DEC = ["up1", "up2", "up3", "up4"]


def _fold_bn(sd, prefix):
    scale = sd[prefix + ".weight"].float() / torch.sqrt(sd[prefix + ".running_var"].float() + BN_EPS)
    shift = sd[prefix + ".bias"].float() - sd[prefix + ".running_mean"].float() * scale
    return scale.contiguous(), shift.contiguous()


def pack_conv3x3(w: torch.Tensor) -> torch.Tensor:
    """(Cout, Cin, 3, 3) -> [tap = ky*3+kx][Cout][Cin] (Cin contiguous: both MFMA operands K-contiguous)."""
    co, ci = w.shape[:2]
    return w.detach().float().permute(2, 3, 0, 1).reshape(9, co, ci).contiguous()


def pack_convT2x2(w: torch.Tensor) -> torch.Tensor:
    """(Cin, Cout, 2, 2) -> [tap = dy*2+dx][Cout][Cin]."""
    ci, co = w.shape[:2]
    return w.detach().float().permute(2, 3, 1, 0).reshape(4, co, ci).contiguous()


def split_bf16x3(w: torch.Tensor) -> torch.Tensor:
    """Kernel-layout fp32 weights [taps][Cout][Cin] -> the bf16x3 operand image of the convolution kernels (csrc/unet_mfma.hip, PREC 1):
    [tap][chunk = Cin / 32][Cout][128 bytes], a row = the 32 channels of a chunk split w = hi + lo (+ O(2^-17 w)) into 8 slots
    of 16 bytes, logical slots 0-3 = 32 bf16 hi, 4-7 = 32 bf16 lo, stored at physical slot (logical ^ ((row >> 1) & 7)) -- a
    (tap, chunk, 128-row) tile is 16 KB contiguous and goes into LDS verbatim by LDS-DMA, the XOR keeps the fragment reads
    bank-conflict-free.  Returned as an opaque float32 tensor of the input's shape (same byte count)."""
    t, co, ci = w.shape
    w4 = w.reshape(t, co, ci // 32, 32)
    hi = w4.to(torch.bfloat16)
    lo = (w4 - hi.float()).to(torch.bfloat16)
    rows = torch.cat([hi, lo], dim=-1).reshape(t, co, ci // 32, 8, 8)             # [t][row][chunk][logical slot][8 bf16]
    swz = (torch.arange(co, device=w.device) >> 1) & 7
    phys = torch.arange(8, device=w.device)[None, :] ^ swz[:, None]                # physical slot p of row r holds logical p ^ swz(r)
    idx = phys[None, :, None, :, None].expand(t, co, ci // 32, 8, 8)
    img = torch.gather(rows, 3, idx).permute(0, 2, 1, 3, 4).contiguous()           # [t][chunk][row][slot][8]
    return img.view(torch.float32).reshape(t, co, ci)


def frag_layout() -> int:
    """Which fragment-ordered image the library's weights-direct kernels read (mfpa_conv_weight_layout on a representative shape):
    2 = the 16 x 16 x 32 form (conv_ws64_kernel, conv_wd16_kernel), 0 = none."""
    return int(lib().mfpa_conv_weight_layout(128, 125, 128, 128, 0, 1))


def split_bf16x3_frag(w: torch.Tensor, layout: int = 2) -> torch.Tensor:
    """Kernel-layout fp32 weights [taps][Cout][Cin] (Cout % 16 == 0, Cin % 32 == 0) -> the FRAGMENT-ORDERED bf16x3 image of the
    "weights direct" convolution kernels (mfpa_conv_desc.w_layout 2; v_mfma_f32_16x16x32_bf16 in conv_ws64_kernel, csrc/unet_ws.hip, and conv_wd16_kernel, csrc/unet_wd16.hip): a
    wave reads the MFMA weight operand of a column tile as 1 KB contiguous pieces, one 16-byte fragment per lane.  Same split w = hi + lo
    as split_bf16x3.  [tap][chunk = Cin / 32][Cout / 16][hi | lo][lane 64][8 bf16], lane (g = l >> 4, c = l & 15) = output channel
    16 t + c, input channels 32 chunk + 8 g .. + 7.  Opaque float32 tensor of w's shape.  `layout` must be 2."""
    if layout != 2:
        raise ValueError(f"no fragment-ordered weight image in layout {layout} (only 2)")
    t, co, ci = w.shape
    w6 = w.reshape(t, co // 16, 16, ci // 32, 4, 8)                                # [t][ct16][c][chunk][g][j]
    hi = w6.to(torch.bfloat16)
    lo = (w6 - hi.float()).to(torch.bfloat16)
    img = torch.stack([hi, lo], dim=0).permute(1, 4, 2, 0, 5, 3, 6).contiguous()    # [t][chunk][ct16][hl][g][c][j]
    return img.view(torch.float32).reshape(t, co, ci)


def frag_f32(w: torch.Tensor) -> torch.Tensor:
    """Kernel-layout fp32 weights [taps][Cout][Cin] (Cout % 16 == 0, Cin % 32 == 0) -> the FP32 fragment image of mfpa_upconv_fused(precision 0)
    (v_mfma_f32_16x16x4_f32): [tap][chunk = Cin / 32][Cout / 16][piece 2][lane 64][4 floats], lane (g = l >> 4, c = l & 15) = output channel
    16 t + c, input channels 32 chunk + 8 g + 4 piece .. + 3.  Same shape and bytes as w."""
    t, co, ci = w.shape
    w7 = w.reshape(t, co // 16, 16, ci // 32, 4, 2, 4)                                # [t][ct16][c][chunk][g][piece][j]
    return w7.permute(0, 3, 1, 5, 4, 2, 6).contiguous().reshape(t, co, ci)            # [t][chunk][ct16][piece][g][c][j]


class WeightImage(NamedTuple):
    """A weight operand as a kernel reads it: the tensor alone (opaque float32, the fp32 weights' shape) cannot say which image it is."""
    t: torch.Tensor
    precision: int               # 0 fp32 products, 1 bf16x3 (pre-split)
    layout: int                  # 0 the row image [tap][Cout][Cin]; 2 the fragment image (mfpa_conv_desc.w_layout; precision 0: frag_f32)
    scale_folded: bool = False   # the folded BatchNorm scale is multiplied in: the launch passes out_scale = None


def weight_image(w: torch.Tensor, precision: int, layout: int = 0, scale: Optional[torch.Tensor] = None) -> WeightImage:
    """Kernel-layout fp32 weights [taps][Cout][Cin] (times `scale` (Cout) if given) -> their image; the fp32 row image is `w` itself."""
    if scale is not None:
        w = w * scale[None, :, None]
    if layout not in (0, 2) or (layout and precision not in (0, 1)):
        raise ValueError(f"no weight image of precision {precision} in layout {layout}")
    t = (split_bf16x3(w) if precision == 1 else w) if layout == 0 else (split_bf16x3_frag(w, layout) if precision == 1 else frag_f32(w))
    return WeightImage(t, precision, layout, scale is not None)


def _operand(img, what: str, precision: int, layouts, scale_folded=(False, True)) -> WeightImage:
    """`img` as the WeightImage launch `what` reads; ValueError if it is one and does not match.  The untyped forms -- a bare tensor, a
    (layout, tensor) pair -- carry nothing to check: they are taken to be that image, as callers outside the UNet's eval path pass them."""
    if not isinstance(img, WeightImage):
        layout, t = img if isinstance(img, tuple) else (layouts[0], img)
        return WeightImage(t, precision, layout, scale_folded[0])
    if not (img.precision == precision and img.layout in layouts and img.scale_folded in scale_folded):
        raise ValueError(f"{what} at precision {precision} reads a weight image in layout {tuple(layouts)}, scale folded {scale_folded}; "
                         f"got (precision, layout, scale_folded) = {tuple(img[1:])}")
    return img


def image(pw: Dict, key: str, layout: int = 0, scale_folded: bool = False) -> WeightImage:
    """Layer `key`'s weight image at pw's precision: made from '<key>.w' (and '.scale') when first asked for, then kept in pw['images']."""
    images = pw.setdefault("images", {})
    if (key, layout, scale_folded) not in images:
        w = pw[key + ".w"]
        images[key, layout, scale_folded] = weight_image(w, pw["precision"], layout, pw[key + ".scale"] if scale_folded else None)
        if w.is_cuda:
            torch.cuda.current_stream(w.device).synchronize()    # made on this stream, may be read from another (UNet.two_streams)
    return images[key, layout, scale_folded]


def pack_unet_weights(sd: Dict[str, torch.Tensor], precision: int = 0) -> Dict:
    """Every layer's fp32 kernel-layout weights '<layer>.w' and folded BatchNorm '.scale' / '.shift', and the images unet_plan() may pick
    at `precision` (see image()): row images, at bf16x3 also the fragment images of the "weights direct" kernels, plain and scale-folded.
    A folding decoder level (level_folds) gets its mfpa_upconv_fused operands '<up>.upc.*' instead of its two launches' images."""
    pw: Dict = {"precision": precision, "images": {}}

    def dconv(prefix, first_layer=False):
        w0 = sd[prefix + ".0.weight"]
        if first_layer:   # (Cout, 1, 3, 3) -> [tap][Cout]
            pw[prefix + ".0.w"] = w0.detach().float().permute(2, 3, 1, 0).reshape(9, w0.shape[0]).contiguous()
        else:
            pw[prefix + ".0.w"] = pack_conv3x3(w0)
        pw[prefix + ".0.scale"], pw[prefix + ".0.shift"] = _fold_bn(sd, prefix + ".1")
        pw[prefix + ".3.w"] = pack_conv3x3(sd[prefix + ".3.weight"])
        pw[prefix + ".3.scale"], pw[prefix + ".3.shift"] = _fold_bn(sd, prefix + ".4")

    for i, p in enumerate(ENC):
        dconv(p, first_layer=(i == 0))
    for name in DEC:
        pw[name + ".up.w"] = pack_convT2x2(sd[name + ".up.weight"])
        pw[name + ".up.b"] = sd[name + ".up.bias"].detach().float().contiguous()
        dconv(name + ".conv.double_conv")
    pw["outc.w"] = sd["outc.conv.weight"].detach().float().reshape(-1).contiguous()
    pw["outc.b"] = sd["outc.conv.bias"].detach().float().reshape(-1).contiguous()
    pw["outc.b_host"] = float(sd["outc.conv.bias"].detach().float().reshape(-1)[0].item())
    lay, folding = (frag_layout() if precision == 1 else 0), [n for n in DEC if level_folds(n, precision)]
    for name in folding:
        pw.update(pack_upconv(pw, name, precision))
    kinds = [(0, False)] + [(lay, False)] * bool(lay) + [(2, True)] * (lay == 2)       # (layout, scale_folded)
    for key in [p + i for p in ENC + [n + ".conv.double_conv" for n in DEC] for i in (".0", ".3")][1:] + [n + ".up" for n in DEC]:
        if key.split(".")[0] not in folding or key.endswith(".3"):   # (a folding level's two-launch images: made if a shape needs them)
            for layout, folded in kinds[:1] if key.endswith(".up") else kinds:
                image(pw, key, layout, folded)
    return pw


FOLD_UP = True                # False: never fold a level's transposed convolution into its consumer (A/B runs)
FOLD_UP_LEVELS = ("up1", "up2", "up3", "up4")   # the decoder levels whose Up block runs as ONE launch (mfpa_upconv_fused); same-call pairs against
                                                # the two launches it replaces, 64 clips: +10.0 / +19.2 / +29.4 / +40.1 % (profiles/r06_upconv_levels.txt)
FOLD_UP_FP32 = True           # the fp32 MFMA path (precision 0) folds too (mfpa_upconv_fused(precision 0)); False: A/B runs


def level_folds(name: str, precision: int) -> bool:
    """Does decoder level `name` run as one mfpa_upconv_fused launch at `precision`, wherever mfpa_upconv_serves takes the shape?"""
    return FOLD_UP and name in FOLD_UP_LEVELS and (frag_layout() == 2 if precision == 1 else FOLD_UP_FP32)


def pack_upconv(pw: Dict, name: str, precision: int = 1) -> Dict:
    """Operands of mfpa_upconv_fused for decoder level `name` from the fp32 kernel-layout weights already in `pw`: the skip half of the
    level's first 3x3 convolution with the folded BatchNorm scale multiplied in (fragment image), the composite weights of its up half
    (ConvTranspose2d folded in: mfpa_upconv_pack on the device, float64 accumulation; fragment image as a 16-tap kernel) and the
    border-class bias table.  Reference: training/unet.py:41-65."""
    w3 = pw[name + ".conv.double_conv.0.w"]                        # [9][Cout][Cs + Cu]
    wt = pw[name + ".up.w"]                                        # [4][Cu][Cl]
    bt = pw[name + ".up.b"]
    scale = pw[name + ".conv.double_conv.0.scale"]
    Cout, Cu, Cl = w3.shape[1], wt.shape[1], wt.shape[2]
    Cs = w3.shape[2] - Cu
    if not w3.is_cuda:
        return {}                                                  # (CPU-side packing: the fused launch is simply not offered)
    wc, tab = upconv_pack_raw(w3, wt, bt, scale)
    return {name + ".upc.wsk": weight_image(w3[:, :, :Cs], precision, 2, scale),
            name + ".upc.wup": weight_image(wc, precision, 2)._replace(scale_folded=True),      # (mfpa_upconv_pack multiplied it in)
            name + ".upc.bias": tab, name + ".upc.shape": (Cs, Cl, Cout)}


def upconv_pack_raw(w3: torch.Tensor, wt: torch.Tensor, bt: torch.Tensor, scale: Optional[torch.Tensor]):
    """mfpa_upconv_pack: kernel-layout w3 [9][Cout][Cs + Cu], wt [4][Cu][Cl], bt (Cu), scale (Cout) or None -> (composite weights (16, Cout, Cl),
    border-class bias table (4, 4, Cout)), float32 (float64 accumulation on the device)."""
    Cout, Cu, Cl = w3.shape[1], wt.shape[1], wt.shape[2]
    Cs = w3.shape[2] - Cu
    wc = torch.empty((16, Cout, Cl), dtype=torch.float32, device=w3.device)
    tab = torch.empty((4, 4, Cout), dtype=torch.float32, device=w3.device)
    check(lib().mfpa_upconv_pack(ptr(w3), ptr(wt), ptr(bt), ptr(scale), Cout, Cs, Cu, Cl, ptr(wc), ptr(tab), stream()), "mfpa_upconv_pack")
    return wc, tab


def upconv_fused(skip, low, w_skip: WeightImage, w_up: WeightImage, shift, bias_tab, Cout, relu=True, precision=1):
    """One decoder level's up -> pad -> cat -> conv3x3 + BN + ReLU (training/unet.py:58-65) as one launch; see include/mfpa.h.
    `w_skip` / `w_up`: the scale-folded fragment images of pack_upconv at `precision`."""
    w_skip, w_up = (_operand(img, "mfpa_upconv_fused", precision, (2,), (True,)) for img in (w_skip, w_up))
    B, H, W, Cs = skip.shape
    _, Hl, Wl, Cl = low.shape
    y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=skip.device)
    d = UpconvDesc(skip=ptr(skip), low=ptr(low), w_skip=ptr(w_skip.t), w_up=ptr(w_up.t), shift=ptr(shift), bias_tab=ptr(bias_tab), y=ptr(y),
                   B=B, H=H, W=W, Cs=Cs, Hl=Hl, Wl=Wl, Cl=Cl, Cout=Cout, relu=int(relu), precision=int(precision))
    with timed():
        check(lib().mfpa_upconv_fused(ctypes.byref(d), stream()), "mfpa_upconv_fused")
    return y


# ----------------------------------------------------------------------------- kernels
_SIDE = {}


def side_stream(dev):
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if idx not in _SIDE:
        _SIDE[idx] = torch.cuda.Stream(device=dev)
    return _SIDE[idx]


def conv3x3_bn_relu(x0, w, scale, shift, x1=None, relu=True, precision=0):
    B, H, W, C0 = x0.shape
    Cout = w.shape[1]
    _, H1, W1, C1 = x1.shape if x1 is not None else (0, 0, 0, 0)
    if w.shape != (9, Cout, C0 + C1):
        raise ValueError(f"weight shape {tuple(w.shape)} does not match input channels {C0}+{C1}")
    y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=x0.device)
    with timed():
        check(lib().mfpa_conv3x3_bn_relu(ptr(x0), C0, ptr(x1), C1, H1, W1, B, H, W, ptr(w), Cout, ptr(scale), ptr(shift),
                                         int(relu), precision, ptr(y), stream()), "mfpa_conv3x3_bn_relu")
    return y


USE_WEIGHTS_DIRECT = True     # False: always the row image / LDS-staged weight tiles (A/B runs)
FOLD_SCALE = True             # False: never pass scale-folded weights (A/B runs)
C1_ON_MFMA = True             # False: the fused first layer stays on conv_mfma_kernel<C1SRC> (exact fp32 FMAs in its loader; A/B runs)
SPLIT_EDGES = True            # False: every tensor between two convolutions stays float32 (A/B runs)


def conv3x3_fused(x0, w, scale, shift, *, x1=None, precision=0, pool=False, out1x1=None, store=True, c1=None, wf=None, wff=None,
                  x0_split=False, x1_split=False, y_split=False, pool_split=False):
    """3x3 conv + folded BN + ReLU through mfpa_conv_mfma with optional fused epilogues: `pool` also writes
    MaxPool2d(2) of the output, `out1x1 = (w (64,), bias)` also writes the OutConv result (B,H,W); `store=False`
    skips the full-resolution output.  `w`: the weight image the launch reads (row or fragment image; a scale-folded one passes
    out_scale = None).  `wf` / `wff` (bf16x3): fragment images of the same weights, plain / scale-folded, taken where conv_route() says.
    `c1 = dict(x32= | spec64=, denom=, w, scale, shift)` (x0 None): the 64 input channels are the UNet's first layer, computed
    from the 1-channel input while the tile is staged (mfpa_conv_desc.c1_*).
    `x0_split` / `x1_split` / `y_split` / `pool_split` (mfpa_conv_desc.*_split): that tensor is / leaves in the SPLIT layout -- same shape
    and bytes, [32 bf16 hi | 32 bf16 lo] per 32-channel chunk of a pixel -- which only conv_ws64_kernel launches read and write.
    Returns (y | None, y_pool | None, y1x1 | None)."""
    w = _operand(w, "mfpa_conv_mfma", precision, (0, 1, 2) if precision == 1 else (0,))
    wf = None if wf is None else _operand(wf, "mfpa_conv_mfma (wf)", 1, (1, 2), (False,))
    wff = None if wff is None else _operand(wff, "mfpa_conv_mfma (wff)", 1, (1, 2), (True,))
    src = None if c1 is None else (c1.get("x32") if c1.get("x32") is not None else c1["spec64"])
    B, H, W, C0 = x0.shape if c1 is None else (*src.shape, 64)
    Cout, C1, dev = w.t.shape[1], 0 if x1 is None else x1.shape[3], w.t.device
    if wf is not None and precision == 1:
        layout, folded, _ = conv_route(H, W, C0 + C1, Cout, wf.layout, c1=c1 is not None, out1x1=out1x1 is not None)
        if layout:
            w = wff if folded and wff is not None and wff.layout == layout else wf
    scale = None if w.scale_folded else scale
    y = torch.empty((B, H, W, Cout), dtype=torch.float32, device=dev) if store else None
    yp = torch.empty((B, H // 2, W // 2, Cout), dtype=torch.float32, device=dev) if pool else None
    y1 = torch.empty((B, H, W), dtype=torch.float32, device=dev) if out1x1 is not None else None
    d = ConvDesc(x0=ptr(x0), in_scale0=0, in_shift0=0, x1=ptr(x1), w=ptr(w.t), out_scale=ptr(scale), out_shift=ptr(shift),
                 y=ptr(y), C0=C0, C1=C1, H1=0 if x1 is None else x1.shape[1], W1=0 if x1 is None else x1.shape[2],
                 B=B, H=H, W=W, Cout=Cout, relu=1, yH=H, yW=W, mode=0, drop_seed=0, drop_thresh=0, drop_scale=1.0,
                 precision=precision, y_pool=ptr(yp), w1x1=ptr(out1x1[0]) if out1x1 is not None else 0,
                 b1x1=float(out1x1[1]) if out1x1 is not None else 0.0, y1x1=ptr(y1), w_layout=w.layout,
                 x0_split=int(x0_split), x1_split=int(x1_split), y_split=int(y_split), y_pool_split=int(pool_split))
    if c1 is not None:
        d.c1_x32, d.c1_spec64, d.c1_denom = ptr(c1.get("x32")), ptr(c1.get("spec64")), ptr(c1.get("denom"))
        d.c1_w, d.c1_scale, d.c1_shift = ptr(c1["w"]), ptr(c1["scale"]), ptr(c1["shift"])
    with timed():
        check(lib().mfpa_conv_mfma(ctypes.byref(d), stream()), "mfpa_conv_mfma")
    return y, yp, y1


def conv3x3_c1_bn_relu(w, scale, shift, x32=None, spec64=None, denom=None, per_clip=True, relu=True, out_dtype=torch.float32, stats_out=None):
    """`stats_out` (a list, training forward): the kernel's per-row partial BatchNorm statistics of the output, (B * H, 2, Cout) float32, are appended."""
    src = x32 if x32 is not None else spec64
    B, H, W = src.shape
    Cout = w.shape[1]
    y = torch.empty((B, H, W, Cout), dtype=out_dtype, device=src.device)
    part = None
    if stats_out is not None and (Cout <= 256 and 256 % Cout == 0):
        part = torch.empty((B * H, 2, Cout), dtype=torch.float32, device=src.device)
        stats_out.append(part)
    check(lib().mfpa_conv3x3_c1_bn_relu(ptr(x32), ptr(spec64), ptr(denom), int(per_clip), B, H, W, ptr(w), Cout,
                                        ptr(scale), ptr(shift), int(relu), ptr(y), int(out_dtype == torch.bfloat16), ptr(part), stream()), "mfpa_conv3x3_c1_bn_relu")
    return y


def maxpool2(x):
    B, H, W, C = x.shape
    y = torch.empty((B, H // 2, W // 2, C), dtype=torch.float32, device=x.device)
    check(lib().mfpa_maxpool2(ptr(x), B, H, W, C, ptr(y), stream()), "mfpa_maxpool2")
    return y


def convT2x2(x, w: WeightImage, bias, precision=0):
    """ConvTranspose2d(k 2, stride 2) of NHWC `x`; `w` the row image [tap][Cout][Cin] at `precision`."""
    w = _operand(w, "mfpa_convT2x2", precision, (0,), (False,))
    B, H, W, Cin = x.shape
    Cout = w.t.shape[1]
    if w.t.shape != (4, Cout, Cin):
        raise ValueError("transposed-conv weight shape mismatch")
    y = torch.empty((B, 2 * H, 2 * W, Cout), dtype=torch.float32, device=x.device)
    with timed():
        check(lib().mfpa_convT2x2(ptr(x), B, H, W, Cin, ptr(w.t), ptr(bias), Cout, precision, ptr(y), stream()), "mfpa_convT2x2")
    return y


def conv1x1_out(x, w, bias: float):
    B, H, W, C = x.shape
    y = torch.empty((B, H, W), dtype=torch.float32, device=x.device)
    check(lib().mfpa_conv1x1_out(ptr(x), B * H * W, C, ptr(w), float(bias), ptr(y), stream()), "mfpa_conv1x1_out")
    return y


FUSE_FIRST_LAYER = True    # False: run mfpa_conv3x3_c1_bn_relu as its own launch (timing experiments, tiny images)


# ----------------------------------------------------------------------------- routing of the eval forward
class ConvStep(NamedTuple):
    """One mfpa_conv_mfma launch of the eval forward."""
    layout: int                  # the weight image it reads: 0 the row image, else that fragment layout ...
    scale_folded: bool           # ... with the scale folded in (out_scale = None)
    c1: bool = False             # the UNet's first layer runs in its loader (else mfpa_conv3x3_c1_bn_relu before it)
    x0_split: bool = False       # its source / output / pooled output in the SPLIT layout (mfpa_conv_desc.*_split)
    y_split: bool = False
    pool_split: bool = False


def conv_route(H: int, W: int, cin: int, cout: int, frag: int, c1=False, out1x1=False) -> Tuple[int, bool, bool]:
    """(layout, scale_folded, on conv_ws64_kernel) of the image a bf16x3 3x3 launch reads under the module switches, offered fragment layout
    `frag` (0: none): that image where the "weights direct" kernel reading it serves the shape, scale-folded on conv_ws64_kernel."""
    L = lib()
    layout = frag if (frag and USE_WEIGHTS_DIRECT and L.mfpa_conv_weight_layout(H, W, cin, cout, 0, 1) == frag
                      and (not c1 or (C1_ON_MFMA and cout == 64 and not out1x1 and L.mfpa_conv_c1_layout(H, W) == frag))
                      and (not out1x1 or (frag == 2 and cout == 64))) else 0
    on_ws = layout == 2 and L.mfpa_conv_scale_folds(H, W, cin, cout) == 1
    return layout, on_ws and FOLD_SCALE, on_ws


_PLANS: Dict[tuple, Dict[str, ConvStep]] = {}


def unet_plan(H0: int, W0: int, precision: int) -> Dict[str, ConvStep]:
    """The convolutions unet_forward_eval launches on (H0, W0) inputs at `precision` under the module switches as they are now, by layer
    (resolved once, then cached).  A decoder level without its '.conv.double_conv.0' runs as ONE mfpa_upconv_fused launch."""
    key = (H0, W0, precision, USE_WEIGHTS_DIRECT, FOLD_SCALE, C1_ON_MFMA, SPLIT_EDGES, FUSE_FIRST_LAYER, FOLD_UP, tuple(FOLD_UP_LEVELS), FOLD_UP_FP32)
    if key in _PLANS:
        return _PLANS[key]
    plan, ws, frag = {}, set(), (frag_layout() if precision == 1 else 0)     # ws: the launches on conv_ws64_kernel

    def conv(key, H, W, cin, cout, src=None, out="y_split", c1=False, out1x1=False):
        # launch `key`, its x0 = output `out` of launch `src`.  The split layout has one reader and writer, conv_ws64_kernel: a tensor
        # between two of its launches travels split (round 5: the producer splits each value once, the consumer's loader waves only copy)
        layout, scale_folded, on_ws = conv_route(H, W, cin, cout, frag, c1=c1, out1x1=out1x1)
        ws.update([key] if on_ws else [])
        plan[key] = {"layout": layout, "scale_folded": scale_folded, "c1": c1}
        if SPLIT_EDGES and src in ws and key in ws:
            plan[src][out] = plan[key]["x0_split"] = True
        return key

    fused_inc = FUSE_FIRST_LAYER and W0 > 16 and H0 >= 8
    skips = [conv(ENC[0] + ".3", H0, W0, 64, 64, c1=fused_inc)]
    if not fused_inc:
        ws.clear()              # (after the separate first-layer launch, inc's outputs stay float32)
    for k, name in enumerate(ENC[1:], 1):
        conv(name + ".0", H0 >> k, W0 >> k, 32 << k, 64 << k, src=skips[-1], out="pool_split")
        skips.append(conv(name + ".3", H0 >> k, W0 >> k, 64 << k, 64 << k, src=name + ".0"))
    for k, name in zip(range(len(DEC) - 1, -1, -1), DEC):
        H, W, C, p = H0 >> k, W0 >> k, 64 << k, name + ".conv.double_conv"
        if not (level_folds(name, precision) and lib().mfpa_upconv_serves(H, W, H >> 1, W >> 1, C, 2 * C, C) == 1):
            conv(p + ".0", H, W, 2 * C, C, src=skips[k])
        conv(p + ".3", H, W, C, C, src=p + ".0", out1x1=name == DEC[-1])
    _PLANS[key] = {k: ConvStep(**v) for k, v in plan.items()}
    return _PLANS[key]


def unet_forward_eval(pw: Dict, x32: Optional[torch.Tensor] = None,
                      spec64: Optional[torch.Tensor] = None, denom: Optional[torch.Tensor] = None) -> torch.Tensor:
    """UNet.forward in eval mode (training/unet.py:97-108) on (B, F, T) -> (B, F, T) float32, launch by launch as unet_plan() says.
    The max-pools (unet.py:34) and the final OutConv (unet.py:71) run inside the epilogues of the convolutions that
    produce their inputs, so neither the pooled tensors' sources are re-read nor is up4's 64-channel output stored."""
    prec = int(pw.get("precision", 0))
    plan = unet_plan(*(x32 if x32 is not None else spec64).shape[1:], prec)

    def c(x, key, **kw):
        st = plan[key]
        return conv3x3_fused(x, image(pw, key, st.layout, st.scale_folded), pw[key + ".scale"], pw[key + ".shift"], precision=prec,
                             x0_split=st.x0_split, y_split=st.y_split, pool_split=st.pool_split, **kw)

    p = ENC[0] + ".0"
    c1 = dict(x32=x32, spec64=spec64, denom=denom, w=pw[p + ".w"], scale=pw[p + ".scale"], shift=pw[p + ".shift"])
    if plan[ENC[0] + ".3"].c1:  # inc.double_conv: the 1 -> 64 layer is evaluated inside the loader of the 64 -> 64 layer (no 64-channel intermediate)
        x, xp, _ = c(None, ENC[0] + ".3", pool=True, c1=c1)
    else:
        m = conv3x3_c1_bn_relu(c1.pop("w"), c1.pop("scale"), c1.pop("shift"), **c1)
        x, xp, _ = c(m, ENC[0] + ".3", pool=True)
        del m
    skips = [x]
    for name in ENC[1:]:
        m, _, _ = c(xp, name + ".0")
        x, xp, _ = c(m, name + ".3", pool=name != ENC[-1])
        del m
        skips.append(x)
    y = skips.pop()                                         # x5
    for name in DEC:
        skip, p = skips.pop(), name + ".conv.double_conv"
        if p + ".0" not in plan:
            # round 6: the level's transposed convolution folded into its first 3x3 convolution -- one launch, `up` never exists
            if name + ".upc.wup" not in pw:
                pw.update(pack_upconv(pw, name, prec))
            m = upconv_fused(skip, y, pw[name + ".upc.wsk"], pw[name + ".upc.wup"], pw[p + ".0.shift"], pw[name + ".upc.bias"],
                             pw[name + ".upc.shape"][2], precision=prec)
        else:
            u = convT2x2(y, image(pw, name + ".up"), pw[name + ".up.b"], precision=prec)
            m, _, _ = c(skip, p + ".0", x1=u)
            del u
        del skip
        # (up4: OutConv fused, the 64-channel tensor is never written)
        y = c(m, p + ".3")[0] if name != DEC[-1] else c(m, p + ".3", out1x1=(pw["outc.w"], pw["outc.b_host"]), store=False)[2]
        del m
    return y
