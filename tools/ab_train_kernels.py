#!/usr/bin/env python3
"""Output bytes of every entry point of csrc/unet_train.hip, one library per process.  usage: ab_train_kernels.py [--lib PATH] --out FILE
       ab_train_kernels.py --summarize FILE      (no GPU: per entry point, the number of FILE's lines and their SHA-256 -- the short form kept in profiles/)

Seeded inputs (CPU generator: the same in every process), every extern "C" function of the file over its shapes and flags, and for each
(entry, case, output buffer) one line `entry case buffer sha256` in FILE.  To compare two builds, run this once per library, a fresh
process each, and compare the two files: they must be identical.  Cases: C in {4, 8, 64, 256, 1024, 2048} where the entry accepts it (2048
walks chan_reduce_kernel's quad loop twice), npix in {1, 3*37*29} and 3*61*47 at C = 1024 (the capped grid's stride loop), the four pool
shapes (odd / even both ways), z and dy as float32 and bfloat16, dz_bf16 given and null, dropout off and on, row partials of 1, 7 and
9000 rows, and the packing / cast / loss / Adam entries at one small shape each."""
import argparse, ctypes, hashlib, os, sys
ap = argparse.ArgumentParser(); ap.add_argument("--lib", default=None); ap.add_argument("--out"); ap.add_argument("--summarize")
args = ap.parse_args()
if args.summarize:
    per = {}
    for line in open(args.summarize):
        per.setdefault(line.split()[0], []).append(line)
    for entry in sorted(per):
        print(f"{entry:32s} {len(per[entry]):5d} lines  {hashlib.sha256(''.join(per[entry]).encode()).hexdigest()}")
    print(f"{'all':32s} {sum(map(len, per.values())):5d} lines  {hashlib.sha256(open(args.summarize, 'rb').read()).hexdigest()}")
    sys.exit(0)
assert args.out, "--out FILE"
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from musicfpaugment_amd import _lib
if args.lib:
    _lib.set_library_path(args.lib)
from musicfpaugment_amd._lib import PackJob, lib, ptr, stream

dev = torch.device("cuda:0")
out = open(args.out, "w")
EPS, MOM = 1e-5, 0.1
DROPS = {"nodrop": (0, 0, 1.0), "drop": (7, int(0.3 * 2 ** 32), 1.0 / 0.7)}
CS = (4, 8, 64, 256, 1024, 2048)
POOLS = ((1, 2, 2), (3, 17, 13), (2, 9, 8), (2, 8, 11))
ws = torch.zeros(1024 * (2 * 2048 + 2), dtype=torch.float64, device=dev)        # RED_BLOCKS x the widest partial row


def rnd(seed, *shape, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=dtype).to(dev)


def call(name, *a):
    rc = getattr(lib(), name)(*[ptr(x) if isinstance(x, torch.Tensor) else (0 if x is None else x) for x in a], stream())
    assert rc == 0, (name, rc)


def emit(entry, case, **bufs):
    torch.cuda.synchronize()
    for k, t in bufs.items():
        if t is not None:
            h = hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()
            out.write(f"{entry} {case} {k} {h}\n")
    out.flush()


def zeros(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=dev)


def layer(seed, npix, C):
    """z (npix, C), its BatchNorm constants (computed on the host: any consistent set serves) and an incoming gradient."""
    z = rnd(seed, npix, C)
    gamma, beta = 1 + 0.1 * rnd(seed + 1, C), 0.1 * rnd(seed + 2, C)
    mean = z.mean(0)
    invstd = 1 / torch.sqrt(z.var(0, unbiased=False) + EPS)
    scale = gamma * invstd
    return dict(z=z, z16=z.bfloat16(), gamma=gamma, beta=beta, mean=mean, invstd=invstd, scale=scale, shift=beta - mean * scale,
                dy=rnd(seed + 3, npix, C))


def stats_out(C):
    return dict(mean=zeros(C), invstd=zeros(C), scale=zeros(C), shift=zeros(C), rm=zeros(C), rv=torch.ones(C, device=dev))


def bwd_out(C):
    return dict(dgamma=zeros(C), dbeta=zeros(C), coef=zeros(3, C))


# the (dy dtype, write_f32, dz_bf16 given) forms of the backward's apply pass
FORMS = (("dy32_f32+bf16", False, 1, True), ("dy32_f32", False, 1, False), ("dy32_bf16", False, 0, True), ("dy16_bf16", True, 0, True))

emit("mfpa_red_blocks", "-", value=torch.tensor([lib().mfpa_red_blocks()], dtype=torch.int32))

for C in CS:
    for npix in (1, 3 * 37 * 29) + ((3 * 61 * 47,) if C == 1024 else ()):
        L = layer(1000 + C + npix, npix, C)
        sums_st, sums_bw = zeros(C, 2, dtype=torch.float64), zeros(C, 2, dtype=torch.float64)
        for zk in ("z", "z16"):
            z, z16 = L[zk], int(zk == "z16")
            case = f"C{C}_n{npix}_{zk}"
            o = stats_out(C)
            call("mfpa_bn_stats", z, npix, C, L["gamma"], L["beta"], EPS, MOM, o["mean"], o["invstd"], o["scale"], o["shift"], o["rm"], o["rv"], ws, z16)
            emit("mfpa_bn_stats", case, **o)
            call("mfpa_bn_stats_sums", z, npix, C, sums_st, ws, z16)
            emit("mfpa_bn_stats_sums", case, sums=sums_st)
            o = stats_out(C)
            call("mfpa_bn_stats_finish", sums_st, float(npix), C, L["gamma"], L["beta"], EPS, MOM, o["mean"], o["invstd"], o["scale"], o["shift"], o["rm"], o["rv"])
            emit("mfpa_bn_stats_finish", case, **o)
            part = rnd(77 + C, 7, 2, C)
            for dk, (seed, thr, dsc) in DROPS.items():
                call("mfpa_bn_relu_bwd_sums", L["dy"], z, npix, C, L["scale"], L["shift"], L["mean"], L["invstd"], sums_bw, ws, seed, thr, dsc, z16)
                emit("mfpa_bn_relu_bwd_sums", f"{case}_{dk}", sums=sums_bw)
                for fk, dy16, wf, has16 in FORMS:
                    c2 = f"{case}_{dk}_{fk}"
                    dz16 = zeros(npix, C, dtype=torch.bfloat16) if has16 else None
                    if not dy16:
                        dy, o = L["dy"].clone(), bwd_out(C)
                        call("mfpa_bn_relu_bwd", dy, z, npix, C, L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"], o["dgamma"], o["dbeta"],
                             o["coef"], ws, seed, thr, dsc, dz16, wf, z16)
                        emit("mfpa_bn_relu_bwd", c2, dy=dy, dz16=dz16, **o)
                    dy, o = (L["dy"].bfloat16() if dy16 else L["dy"].clone()), bwd_out(C)
                    call("mfpa_bn_relu_bwd_from_part", dy, z, npix, C, L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"], part, 7, o["dgamma"],
                         o["dbeta"], o["coef"], ws, seed, thr, dsc, dz16, wf, z16, int(dy16))
                    emit("mfpa_bn_relu_bwd_from_part", c2, dy=dy, dz16=dz16, **o)
                    dy, o = (L["dy"].bfloat16() if dy16 else L["dy"].clone()), bwd_out(C)
                    call("mfpa_bn_relu_bwd_finish", dy, z, npix, C, L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"], sums_bw, sums_st,
                         2.0 * npix, o["dgamma"], o["dbeta"], o["coef"], seed, thr, dsc, dz16, wf, z16, int(dy16))
                    emit("mfpa_bn_relu_bwd_finish", c2, dy=dy, dz16=dz16, **o)
            dpred, w1 = rnd(5 + C, npix), rnd(6 + C, C)
            for fk, f32, b16 in (("f32+bf16", True, True), ("f32", True, False), ("bf16", False, True)):
                dz, dz16, o = (zeros(npix, C) if f32 else None), (zeros(npix, C, dtype=torch.bfloat16) if b16 else None), bwd_out(C)
                call("mfpa_bn_relu_bwd_finish_rank1", dpred, w1, z, npix, C, L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"], sums_bw, sums_st,
                     2.0 * npix, o["dgamma"], o["dbeta"], o["coef"], dz, dz16, z16)
                emit("mfpa_bn_relu_bwd_finish_rank1", f"{case}_{fk}", dz=dz, dz16=dz16, **o)
        colsum = zeros(C)
        call("mfpa_colsum", L["dy"], npix, C, colsum, ws)
        emit("mfpa_colsum", f"C{C}_n{npix}", out=colsum)
        if C in (4, 64, 256):
            wb = rnd(9 + C, C + 1)
            rows = ctypes.c_int(0)
            assert lib().mfpa_outconv_bwd_rows(npix, C, ctypes.byref(rows)) == 0
            emit("mfpa_outconv_bwd_rows", f"C{C}_n{npix}", value=torch.tensor([rows.value], dtype=torch.int32))
            for zk in ("z", "z16"):
                z, z16, case = L[zk], int(zk == "z16"), f"C{C}_n{npix}_{zk}"
                pred = zeros(npix)
                call("mfpa_outconv_fwd", z, npix, C, L["scale"], L["shift"], wb, wb[C:], pred, z16)
                emit("mfpa_outconv_fwd", case, pred=pred)
                dy, dwb = zeros(npix, C), zeros(C + 1)
                call("mfpa_outconv_bwd", z, dpred, npix, C, L["scale"], L["shift"], wb, dy, dwb, ws, z16)
                emit("mfpa_outconv_bwd", case, dy=dy, dwb=dwb)
                dwb, part = zeros(C + 1), zeros(rows.value, 2, C)
                call("mfpa_outconv_bwd_sums", z, dpred, npix, C, L["scale"], L["shift"], L["mean"], L["invstd"], wb, dwb, ws, part, z16)
                emit("mfpa_outconv_bwd_sums", case, dwb=dwb, part=part)
        del L

    # row partials -> float64 sums / finished statistics
    for rows in (1, 7, 9000):
        part, sums, o = rnd(300 + C + rows, rows, 2, C), zeros(C, 2, dtype=torch.float64), stats_out(C)
        call("mfpa_conv_stats_reduce", part, rows, C, sums, ws)
        emit("mfpa_conv_stats_reduce", f"C{C}_r{rows}", sums=sums)
        part[:, 1] = part[:, 1] ** 2 + part[:, 0] ** 2                                         # (a plausible sum of squares)
        call("mfpa_conv_stats_bn_finish", part, rows, C, 64.0 * rows, 1 + 0.1 * rnd(1, C), 0.1 * rnd(2, C), EPS, MOM, o["mean"], o["invstd"], o["scale"],
             o["shift"], o["rm"], o["rv"], ws)
        emit("mfpa_conv_stats_bn_finish", f"C{C}_r{rows}", **o)

    # pool forward / backward
    for (B, H, W) in POOLS:
        npix = B * H * W
        L = layer(2000 + C + npix, npix, C)
        dp = rnd(8 + C, B, H // 2, W // 2, C)
        for zk in ("z", "z16"):
            z, z16 = L[zk], int(zk == "z16")
            for dk, (seed, thr, dsc) in DROPS.items():
                case = f"C{C}_{B}x{H}x{W}_{zk}_{dk}"
                for p16 in (0, 1):
                    p = zeros(B, H // 2, W // 2, C, dtype=torch.bfloat16 if p16 else torch.float32)
                    call("mfpa_bn_relu_pool", z, B, H, W, C, L["scale"], L["shift"], p, seed, thr, dsc, z16, p16)
                    emit("mfpa_bn_relu_pool", f"{case}_p{16 if p16 else 32}", p=p)
                dy = L["dy"].clone()
                call("mfpa_maxpool2_bwd_add", z, B, H, W, C, L["scale"], L["shift"], dp, dy, seed, thr, dsc, z16)
                emit("mfpa_maxpool2_bwd_add", case, dy=dy)
                if C > 1024:
                    continue                                                                   # (a thread keeps ONE channel quad's sums)
                dy, part = L["dy"].clone(), zeros(B * (H // 2), 2, C)
                call("mfpa_maxpool2_bwd_add_sums", z, B, H, W, C, L["scale"], L["shift"], L["mean"], L["invstd"], dp, dy, seed, thr, dsc, part, z16)
                emit("mfpa_maxpool2_bwd_add_sums", case, dy=dy, part=part)
                for dy16 in (0, 1):
                    dy = L["dy"].bfloat16() if dy16 else L["dy"].clone()
                    part, o, dz16 = zeros(B * (H // 2), 2, C), bwd_out(C), zeros(npix, C, dtype=torch.bfloat16)
                    call("mfpa_maxpool2_bwd_bn_relu_bwd", z, B, H, W, C, L["gamma"], L["scale"], L["shift"], L["mean"], L["invstd"], dp, dy, dy16, seed, thr,
                         dsc, part, o["dgamma"], o["dbeta"], o["coef"], ws, dz16, z16)
                    emit("mfpa_maxpool2_bwd_bn_relu_bwd", f"{case}_dy{16 if dy16 else 32}", dy=dy, part=part, dz16=dz16, **o)
        del L

# packing, cast, loss, Adam: one small shape each
Co, Ci = 64, 96
for taps in (4, 9):
    w = rnd(40 + taps, taps, Co, Ci)
    jobs, images, tile0 = [], [], 0
    for code in (0, 1, 3):
        for tr in (0, 1):
            nrows, K = (Ci if tr else Co) - 32, (Co if tr else Ci)
            img = zeros(taps * nrows * K)              # [tap][row][K] floats, or as many bytes of bf16 hi | lo pairs
            call("mfpa_pack_conv_weights", w, taps, Co, Ci, tr, 32, nrows, code, img)
            emit("mfpa_pack_conv_weights", f"taps{taps}_code{code}_tr{tr}", image=img)
            images.append(zeros(img.numel()))
            jobs.append(PackJob(ptr(w), ptr(images[-1]), taps, Co, Ci, tr, 32, nrows, code, 0, tile0))
            tile0 += (K // 32) * (nrows // 32) * taps
    raw = b"".join(bytes(j) for j in jobs)
    jobs_dev = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(dev)
    call("mfpa_pack_conv_weights_batch", jobs_dev, len(jobs), tile0)
    emit("mfpa_pack_conv_weights_batch", f"taps{taps}", **{f"image{k}": t for k, t in enumerate(images)})
L = layer(50, 3 * 7 * 5, 64)
for dk, (seed, thr, dsc) in DROPS.items():
    o16 = zeros(105, 64, dtype=torch.bfloat16)
    call("mfpa_act_to_bf16", L["z"], 105 * 64, 64, L["scale"], L["shift"], seed, thr, dsc, o16)
    emit("mfpa_act_to_bf16", f"affine_{dk}", out=o16)
o16 = zeros(105, 64, dtype=torch.bfloat16)
call("mfpa_act_to_bf16", L["z"], 105 * 64, 64, None, None, 0, 0, 1.0, o16)
emit("mfpa_act_to_bf16", "identity", out=o16)
n = 3 * 257 * 33
pred, target, dpred, loss = rnd(60, n), rnd(61, n, dtype=torch.float64), zeros(n), zeros(1, dtype=torch.float64)
call("mfpa_l1_loss", pred, target, n, dpred, loss, ws)
emit("mfpa_l1_loss", f"n{n}", dpred=dpred, loss=loss)
p, g, m, v = rnd(62, n), rnd(63, n), 0.1 * rnd(64, n), 0.01 * rnd(65, n) ** 2
call("mfpa_adam_step", p, g, m, v, n, 1e-3, 0.9, 0.999, 1e-8, 3, 0.5)
emit("mfpa_adam_step", f"n{n}_step3", p=p, m=m, v=v)
out.close()
print("wrote", args.out, sum(1 for _ in open(args.out)), "lines", flush=True)
