"""Host oracle of the Demucs VALU kernels (csrc/demucs.hip) and of the training step's small kernels and TN weight-gradient GEMM
(csrc/demucs_train.hip): float64 restatements of the formulas in the two files' header comments, the operand makers with their
exactness argument, two error models for the kernels that cannot be exact, the case tables that tests/test_demucs_small_oracle.py (CPU)
and tests/test_gpu_demucs_small.py (GPU) both walk, and deliberately FAULTY variants of every restatement.  No GPU, no libmfpa here.

Exactness.  Operands are integers in [-3, 3] (the resampler taps too, and ASYMMETRIC: the real sinc taps are symmetric to 1.5e-8, which
hides a flipped tap walk); every `scale` is a power of two.  Every product and partial sum is then an integer, or a dyadic of one fixed
scale, below 2^24 in units of that scale: the float32 result is exact under any summation or atomic order and the comparison is
torch.equal.  Every maker asserts that before anything is compared (_exact()).

gemm_tn at precision 1 / 2 draws v = a + b 2^-10 (a, b integers in [-3, 3]; b carries a's sign and is 0 where a is), so that
hi = bf16(v) = a and lo = bf16(v - hi) = b 2^-10 split exactly with lo != 0 for 36/49 of the values.  Products ah bh are integers, ah bl
and al bh multiples of 2^-10 (al bl is what bf16x3 drops): the three references
    precision 0: sum a_A a_B (plain integers)      precision 1: sum ah bh + ah bl + al bh      precision 2: sum ah bh
are exact while 9.1 * 2^10 * (total rows) < 2^24, i.e. up to 1800 rows; such cases keep batch * R <= 1500.  The two conditions on b are
what makes hi an integer: with a = 0, hi would be b 2^-10 and two such operands multiply to b_A b_B 2^-20; with a = -1, b = 3 the value
-1 + 3 2^-10 lies in the binade below 1, where bf16's half ulp is 2 2^-10, and rounds to hi = -1 + 2^-8.  tn_build asserts hi == a.

Every buffer is a flat float32 tensor in the layout the C call addresses.  Positions of an output that must not be written hold
SENTINEL_BITS (a quiet NaN with a payload), positions of an input that must not be read (row pads, the gaps between clips) hold NaN."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

SENTINEL_BITS = 0x7FC0BEEF
GUARD = 4                                  # sentinel floats behind every output buffer
GAP = 8                                    # NaN floats between the clips of an input (a multiple of 4)
U24, U23 = 2.0 ** -24, 2.0 ** -23
LIMIT = 2.0 ** 24
NAN = float("nan")


def sentinel(n: int) -> torch.Tensor:
    return torch.full((n,), SENTINEL_BITS, dtype=torch.int32).view(torch.float32)


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def ints(g: torch.Generator, *shape, lo: int = -3, hi: int = 3) -> torch.Tensor:
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _exact(ref: torch.Tensor, unit: float, worst_partial: float) -> torch.Tensor:
    """The reference is a whole number of `unit`s and the largest partial sum any order can meet stays below 2^24 units."""
    assert ref.dtype == torch.float64
    q = ref / unit
    assert torch.equal(q, q.round()), "the reference is not integer-valued in its unit"
    assert worst_partial / unit < LIMIT and float(ref.abs().max()) <= worst_partial, (worst_partial, unit)
    return ref


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def mismatch(got: torch.Tensor, want: torch.Tensor) -> Optional[str]:
    """Flat float32 buffers: sentinel positions of `want` must hold the sentinel bits, every other position the same value.  None if so."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32
    keep = want.view(torch.int32) == SENTINEL_BITS
    if not bool((got.view(torch.int32)[keep] == SENTINEL_BITS).all()):
        bad = (keep & (got.view(torch.int32) != SENTINEL_BITS)).nonzero().flatten()
        return f"{bad.numel()} sentinel positions were written, first at {bad[:4].tolist()}"
    g, w = got[~keep], want[~keep]
    if not torch.equal(g, w):
        bad = (~keep & ~(got == want)).nonzero().flatten()
        i = int(bad[0])
        return f"{bad.numel()} elements differ, first at {bad[:4].tolist()}: got {float(got[i])!r}, want {float(want[i])!r}"
    return None


@dataclass
class Built:
    """One case on the host: `inp` flat float32 inputs, `out` name -> (initial contents, expected contents) of the flat outputs."""
    inp: Dict[str, torch.Tensor]
    out: Dict[str, Tuple[torch.Tensor, torch.Tensor]]
    aux: dict


def _out(shape_rows: int, ld: int, cols: int, block: torch.Tensor, init_block: Optional[torch.Tensor] = None, batch: int = 1,
         stride: Optional[int] = None):
    """(init, want) of an output of `batch` clips of `shape_rows` rows at pitch `ld`, `cols` written columns, clip stride `stride`."""
    stride = shape_rows * ld if stride is None else stride
    init, want = sentinel(batch * stride + GUARD), sentinel(batch * stride + GUARD)
    v = want.as_strided((batch, shape_rows, cols), (stride, ld, 1))
    v.copy_(block.reshape(batch, shape_rows, cols).float())
    held = lambda t: torch.nan_to_num(t, nan=2.0 ** 30)             # a faulty variant may expect NaN (it read a gap)
    assert torch.equal(held(v.double()), held(block.reshape(batch, shape_rows, cols))), "the expected block is not exact in float32"
    if init_block is not None:
        init.as_strided((batch, shape_rows, cols), (stride, ld, 1)).copy_(init_block.reshape(batch, shape_rows, cols).float())
    return init, want


def _clips(blocks: torch.Tensor, rows: int, ld: int, cols: int, stride: int) -> torch.Tensor:
    """An input of blocks.shape[0] clips, (rows, cols) values each at pitch ld, NaN in the row pads and between the clips."""
    b = blocks.shape[0]
    flat = torch.full((b * stride,), NAN)
    flat.as_strided((b, rows, cols), (stride, ld, 1)).copy_(blocks.reshape(b, rows, cols).float())
    return flat


# ====================================================================================================== sinc x2 resamplers
TAPS_N, ZEROS = 112, 56


def int_taps() -> torch.Tensor:
    """112 asymmetric integer taps in [-3, 3]; the ends and the two centre taps are non-zero and differ from their mirror images."""
    k = ints(_gen("taps"), TAPS_N)
    k[0], k[111], k[55], k[56], k[1], k[110] = 3, -2, 1, -3, -1, 2
    assert not torch.equal(k, k.flip(0)) and int((k != k.flip(0)).sum()) > 60
    return k


def upsample2(x: torch.Tensor, ker: torch.Tensor, fault: Optional[str] = None) -> torch.Tensor:
    """y[2i] = x[i], y[2i+1] = sum_k x[i + k - 55] ker[k] (zero beyond the ends).  x (B, T) float64."""
    if fault == "taps_flipped":
        ker = ker.flip(0)
    off = 56 if fault == "tap_offset" else 55
    B, T = x.shape
    xp = torch.nn.functional.pad(x, (off, TAPS_N - 1 - off + 1))                 # xp[j] = x[j - off]
    odd = xp.unfold(1, TAPS_N, 1)[:, :T] @ ker                                   # window i, tap k: xp[i + k]
    return torch.stack([x, odd], dim=-1).reshape(B, 2 * T)


def downsample2(x: torch.Tensor, ker: torch.Tensor, scale: Optional[torch.Tensor] = None, nout: Optional[int] = None,
                fault: Optional[str] = None) -> torch.Tensor:
    """out[i] = sc 0.5 (x[2i] + sum_k xodd[i + k - 56] ker[k]), i < nout, xodd[j] = x[2j+1] or 0.  x (B, T) float64 -> (B, nout)."""
    if fault == "taps_flipped":
        ker = ker.flip(0)
    off = 55 if fault == "tap_offset" else 56
    B, T = x.shape
    th = (T + 1) // 2
    xz = torch.nn.functional.pad(x, (0, 2 * th - T))
    xe, xo = xz[:, 0::2], (xz[:, 0::2] if fault == "xodd_even" else xz[:, 1::2])
    xp = torch.nn.functional.pad(xo, (off, TAPS_N - off))                        # xp[j] = xodd[j - off]
    out = 0.5 * (xe + xp.unfold(1, TAPS_N, 1)[:, :th] @ ker)
    if scale is not None:
        out = out * scale[:, None]
    return out[:, :th if nout is None else nout]


def downsample2_adjoint(dy: torch.Tensor, ker: torch.Tensor, T: int, scale: Optional[torch.Tensor] = None,
                        fault: Optional[str] = None) -> torch.Tensor:
    """dx[2i] = g[i], dx[2j+1] = sum_k g[j + 56 - k] ker[k], g[i] = 0.5 sc dy[i] (0 for i >= nout).  dy (B, nout) float64 -> (B, T)."""
    B, nout = dy.shape
    th = (T + 1) // 2
    g = 0.5 * dy * (scale[:, None] if scale is not None else 1.0)
    g = torch.nn.functional.pad(g, (0, th - nout))
    if fault == "adjoint_sign":                                                  # g[j + k - 56]
        gp = torch.nn.functional.pad(g, (56, 56))                                # gp[m] = g[m - 56]
        odd = gp.unfold(1, TAPS_N, 1)[:, :th] @ ker
    else:
        gp = torch.nn.functional.pad(g, (55, 57))                                # gp[m] = g[m - 55]; j + 56 - k = (j + (111 - k)) - 55
        odd = gp.unfold(1, TAPS_N, 1)[:, :th] @ ker.flip(0)
    return torch.stack([g, odd], dim=-1).reshape(B, 2 * th)[:, :T]


RS_T = (2, 3, 5, 56, 57, 113, 1023, 1024, 1025, 2049, 2052)                      # upsample2 adds T = 1
RS_SCALES = (0.5, 2.0, 4.0)                                                      # one power of two per clip


@dataclass(frozen=True)
class RsCase:
    kind: str                    # "up", "down", "adj"
    B: int
    T: int
    keep: int = 0                # down: the Tkeep argument; adj: nout
    pad: int = 0                 # down: To - nout; adj: ldy - nout
    scale: bool = False

    @property
    def name(self):
        return f"{self.kind}-B{self.B}-T{self.T}-keep{self.keep}+{self.pad}" + ("-scale" if self.scale else "")

    @property
    def th(self): return (self.T + 1) // 2
    @property
    def nout(self): return self.keep if self.keep > 0 else self.th


def _rs_cases() -> List[RsCase]:
    out = [RsCase("up", 3, T) for T in (1,) + RS_T]
    for T in RS_T:
        th = (T + 1) // 2
        keeps = {0, 1, th - 1, th} | ({1023, 1024, 1025} if T >= 2049 else set())
        for keep in sorted(k for k in keeps if k >= 0):
            for sc in (False, True):
                out.append(RsCase("down", 3, T, keep, 3, sc))
        for nout in sorted({th, th - 1} - {0}):
            for sc in (False, True):
                out.append(RsCase("adj", 3, T, nout, 3 if nout < th or sc else 0, sc))
    out.append(RsCase("adj", 1, 262147, 131074, 0, True))                         # ceil(T / 256) = 1025 > 1024 blocks: the grid-stride loop
    return out


RS_CASES = _rs_cases()


@functools.lru_cache(maxsize=None)
def _rs_x(B: int, T: int) -> torch.Tensor:
    return ints(_gen("rs-x", B, T), B, T)


def rs_build(c: RsCase, fault: Optional[str] = None, ker: Optional[torch.Tensor] = None) -> Built:
    ker = int_taps() if ker is None else ker
    sc = torch.tensor(RS_SCALES[:c.B], dtype=torch.float64) if c.scale else None
    inp = {"ker": ker.float(), "scale": sc.float() if c.scale else None}
    tap_sum = float(ker.abs().sum()) * 3                                          # |sum_k x ker| <= 3 sum |ker|
    if c.kind == "up":
        x = _rs_x(c.B, c.T)
        y = _exact(upsample2(x, ker, fault), 1.0, tap_sum)
        inp["x"] = x.float().reshape(-1)
        return Built(inp, {"y": _out(1, 2 * c.T, 2 * c.T, y, batch=c.B)}, {})
    if c.kind == "down":
        x = _rs_x(c.B, c.T)
        y = _exact(downsample2(x, ker, sc, c.nout, fault), 0.25, 4.0 * (3 + tap_sum))     # 0.5 * sc, sc >= 0.5: quarters
        inp["x"] = x.float().reshape(-1)
        to = c.nout + c.pad
        return Built(inp, {"y": _out(1, to, c.nout, y, batch=c.B)}, {"To": to})
    dy = ints(_gen("rs-dy", c.B, c.T, c.keep), c.B, c.keep)
    dx = _exact(downsample2_adjoint(dy, ker, c.T, sc, fault), 0.25, 2.0 * tap_sum)
    ldy = c.keep + c.pad
    inp["dy"] = _clips(dy, 1, ldy, c.keep, ldy)
    return Built(inp, {"dx": _out(1, c.T, c.T, dx, batch=c.B)}, {"ldy": ldy, "dy64": dy})


# ====================================================================================================== 1-channel convolutions
def conv1d_c1(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], lout: int, relu: bool) -> torch.Tensor:
    """y[b][t][c] = act(bias[c] + sum_j x[b][4t + j] w[j][c]), t < lout.  x (B, Lin), w (8, C) -> (B, lout, C)."""
    win = x.as_strided((x.shape[0], lout, 8), (x.stride(0), 4, 1))
    y = win @ w + (bias if bias is not None else 0.0)
    return torch.relu(y) if relu else y


def convT1d_c1(P: torch.Tensor, w: torch.Tensor, bias: float) -> torch.Tensor:
    """out[b][4t + j] = bias + sum_c P[b][t+1][c] w[j][c] + P[b][t][c] w[j+4][c], t = 0..L, j < 4.  P (B, L + 2, C), w (8, C)."""
    out = bias + P[:, 1:] @ w[:4].t() + P[:, :-1] @ w[4:].t()                     # (B, L + 1, 4)
    return out.reshape(P.shape[0], -1)


def c1_wgrad(x: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """dw[j][c] = sum_{b, t} x[b][4t + j] g[b][t][c].  x (B, >= 4 (L - 1) + 8), g (B, L, C) -> (8, C)."""
    L = g.shape[1]
    win = x.as_strided((x.shape[0], L, 8), (x.stride(0), 4, 1))
    return torch.einsum("btj,btc->jc", win, g)


@dataclass(frozen=True)
class ConvCase:
    B: int
    C: int
    L: int                       # Lout
    extra: int = 0               # Lin - (4 (Lout - 1) + 8)
    relu: int = 0
    bias: bool = True

    @property
    def name(self): return f"B{self.B}-C{self.C}-L{self.L}+{self.extra}-relu{self.relu}" + ("" if self.bias else "-nobias")
    @property
    def lin(self): return 4 * (self.L - 1) + 8 + self.extra


def _conv_cases() -> List[ConvCase]:
    out = [ConvCase(3, C, L, e, r) for C in (4, 48, 52, 256) for L in (1, 2, 333) for e in (0, 3) for r in (0, 1)]
    out += [ConvCase(3, C, 2, 3, r, bias=False) for C, r in ((4, 1), (48, 0), (52, 1), (256, 0))]
    out.append(ConvCase(2, 256, 8200, 0, 1))          # 8200 * 64 = 524800 quads > 2048 * 256 = 524288 threads: the grid-stride loop
    return out


CONV_CASES = _conv_cases()


def conv_build(c: ConvCase) -> Built:
    g = _gen("conv", c.B, c.C, c.L)
    x, w, bias = ints(g, c.B, c.lin), ints(g, 8, c.C), ints(g, c.C)
    y = _exact(conv1d_c1(x, w, bias if c.bias else None, c.L, bool(c.relu)), 1.0, 3 + 8 * 9)
    xin = x.float().clone()
    if c.extra:
        xin[:, c.lin - c.extra:] = NAN                 # behind the last window: never read
    return Built({"x": xin.reshape(-1), "w": w.float().reshape(-1), "bias": bias.float() if c.bias else None},
                 {"y": _out(c.L, c.C, c.C, y, batch=c.B)}, {})


@dataclass(frozen=True)
class ConvTCase:
    B: int
    C: int
    L: int

    @property
    def name(self): return f"B{self.B}-C{self.C}-L{self.L}"


CONVT_CASES = [ConvTCase(3, C, L) for C in (4, 48, 256) for L in (1, 2, 333)] + [
    ConvTCase(1, 4, 131075)]                            # 4 (L + 1) = 524304 outputs > 2048 * 256: the grid-stride loop


def convT_build(c: ConvTCase) -> Built:
    g = _gen("convT", c.B, c.C, c.L)
    P, w, bias = ints(g, c.B, c.L + 2, c.C), ints(g, 8, c.C), 2.0
    y = _exact(convT1d_c1(P, w, bias), 1.0, 2 + 2 * c.C * 9)
    return Built({"P": P.float().reshape(-1), "w": w.float().reshape(-1), "bias": torch.tensor([bias])},
                 {"y": _out(1, 4 * (c.L + 1), 4 * (c.L + 1), y, batch=c.B)}, {"bias": bias})


@dataclass(frozen=True)
class C1wCase:
    B: int
    C: int
    L: int
    trainer: bool                # g one row into a (L + 2, C) buffer with strideG = (L + 2) C, as the trainer calls it

    @property
    def name(self): return f"B{self.B}-C{self.C}-L{self.L}" + ("-trainer" if self.trainer else "-padded")
    @property
    def ldx(self): return 4 * (self.L - 1) + 8 + 4
    @property
    def ldg(self): return self.C if self.trainer else self.C + 4
    @property
    def stride_g(self): return (self.L + 2) * self.C if self.trainer else self.L * self.ldg + GAP
    @property
    def g_offset(self): return self.C if self.trainer else 0


# C = 48: Q = 12 column quads, 256 // 12 = 21 row lanes, threads 252..255 idle.  L = 2049: gx = 2, 1025 rows per block, 1024 in the last;
# L = 4100: gx = 3, 1367 rows per block, 1366 in the last
C1W_CASES = [C1wCase(3, C, L, tr) for C in (4, 48, 256) for L in (1, 20, 2049, 4100) for tr in (False, True)]


def c1w_build(c: C1wCase) -> Built:
    g = _gen("c1w", c.B, c.C, c.L)
    x, gr, dw0 = ints(g, c.B, c.ldx - 4), ints(g, c.B, c.L, c.C), ints(g, 8, c.C)
    dw = _exact(dw0 + c1_wgrad(x, gr), 1.0, 3 + 9 * c.B * c.L)
    if c.trainer:                                       # NaN in the zero rows at both ends: the kernel has no business there
        gin = torch.full((c.B, c.L + 2, c.C), NAN)
        gin[:, 1:-1] = gr.float()
        gin = gin.reshape(-1)
    else:
        gin = _clips(gr, c.L, c.ldg, c.C, c.stride_g)
    return Built({"x": _clips(x, 1, c.ldx, c.ldx - 4, c.ldx), "g": gin}, {"dw": _out(8, c.C, c.C, dw, dw0)}, {})


# ====================================================================================================== column sums
@dataclass(frozen=True)
class ColsumCase:
    C: int
    rows: int

    @property
    def name(self): return f"C{self.C}-rows{self.rows}"
    @property
    def ld(self): return self.C + 4


def colsum_blocks(C: int, rows: int) -> Tuple[int, int]:
    """(blocks, rows per block) of mfpa_colsum_any's host code."""
    blocks = max(1, min(2048, (rows * (C // 4) + 256 * 32 - 1) // (256 * 32)))
    rpb = (rows + blocks - 1) // blocks
    return (rows + rpb - 1) // rpb, rpb


# C <= 1024: one column quad per thread (NQ = 1), C = 1024 with a single row lane; C > 1024: NQ = 4 (1028: the second quad of thread 0 only).
# rows = 1000 at C = 1028: (1000 * 257 + 8191) // 8192 = 32 blocks of ceil(1000 / 32) = 32 rows, the last with 1000 - 31 * 32 = 8
COLSUM_CASES = [ColsumCase(C, r) for C in (4, 48, 1024, 1028, 1100, 4096) for r in (1, 3, 257, 1000)]
assert colsum_blocks(1028, 1000) == (32, 32) and 1000 - 31 * 32 == 8


def colsum_build(c: ColsumCase) -> Built:
    g = _gen("colsum", c.C, c.rows)
    x, o0 = ints(g, c.rows, c.C), ints(g, c.C)
    o = _exact(o0 + x.sum(0), 1.0, 3 + 3 * c.rows)
    return Built({"x": _clips(x[None], c.rows, c.ld, c.C, c.rows * c.ld)}, {"out": _out(1, c.C, c.C, o, o0)}, {})


# ====================================================================================================== TN weight-gradient GEMM
def tn_plan(M: int, N: int, R: int, batch: int):
    """mfpa_gemm_tn's host rule -> (big, tiles, rs, spb, ntn): 128 x 128 tiles when M > 64 and N > 64, else 64 x 64; about 2048 workgroups,
    at least 64 rows per K split, a multiple of 32, never across clips."""
    big = M > 64 and N > 64
    bt = 128 if big else 64
    ntn = (N + bt - 1) // bt
    tiles = ((M + bt - 1) // bt) * ntn
    want = max(1, 2048 // tiles)
    rs = max(64, (batch * R + want - 1) // want)
    rs = (rs + 31) // 32 * 32
    return big, tiles, rs, (R + rs - 1) // rs, ntn


@dataclass(frozen=True)
class TnCase:
    M: int
    N: int
    R: int
    batch: int
    precision: int
    colsum: bool
    lda_pad: int = 0             # lda = M + lda_pad; ldb = N + 4 - lda_pad (one of the two is padded)
    cin: int = 0                 # > 0: overlapping windows, N = 8 cin, ldb = 4 cin over (4 (R - 1) + 8) rows of cin floats
    split_ints: bool = True      # False: plain integers at every precision (the long case)

    @property
    def name(self):
        s = f"M{self.M}-N{self.N}-R{self.R}-b{self.batch}-p{self.precision}" + ("-colsum" if self.colsum else "")
        return s + (f"-win{self.cin}" if self.cin else f"-lda+{self.lda_pad}")

    @property
    def lda(self): return self.M + self.lda_pad
    @property
    def stride_a(self): return self.R * self.lda + GAP
    @property
    def ldb(self): return 4 * self.cin if self.cin else self.N + 4 - self.lda_pad
    @property
    def region_b(self): return (4 * (self.R - 1) + 8) * self.cin if self.cin else self.R * self.ldb
    @property
    def stride_b(self): return self.region_b + GAP
    @property
    def ldc(self): return self.N + 4
    @property
    def plan(self): return tn_plan(self.M, self.N, self.R, self.batch)
    @property
    def workgroups(self): return self.plan[1] * self.plan[3] * self.batch
    @property
    def kernel(self): return (self.plan[0], self.precision)
    @property
    def operand_key(self): return (self.M, self.N, self.R, self.batch, self.lda_pad, self.cin, self.precision > 0 and self.split_ints)


TN_MN = ((4, 4), (48, 68), (68, 48), (64, 64), (68, 68), (128, 128), (132, 260))
TN_R = (1, 15, 17, 31, 33, 65, 130)          # rs = 64 throughout: 65 -> splits of 64 + 1 rows, 130 -> 64 + 64 + 2


def _tn_cases() -> List[TnCase]:
    """Workgroup totals (tiles x splits x batch; tn_tile spreads them over 8 XCD ranges and idles the rest of the last 8):
    tiles are 1 for (4, 4), (64, 64), (68, 68), (128, 128); 2 for (48, 68) and (68, 48); 6 for (132, 260).  With batch 1 / 3 and 1, 2
    or 3 splits per clip the table's totals are 1, 2, 3, 4, 6, 9, 12, 18, 36, 54 -- none a multiple of 8 -- so four batch-4 cases add
    2 * 4 * 1 = 8, 2 * 4 * 2 = 16 (small tiles) and 6 * 4 * 1 = 24, 6 * 4 * 2 = 48 (large tiles); the long case has 6 * 94 * 3 = 1692."""
    out: List[TnCase] = []
    for p in (0, 1, 2):
        for i, (M, N) in enumerate(TN_MN):
            for j, R in enumerate(TN_R):
                for batch in (1, 3):
                    out.append(TnCase(M, N, R, batch, p, colsum=(i + j + batch) % 2 == 0, lda_pad=4 * ((i + j) % 2)))
        out.append(TnCase(48, 96, 33, 3, p, True, cin=12))       # the Conv1d(k8, s4) weight gradient's overlapping windows, 64 x 64 tiles
        out.append(TnCase(68, 96, 33, 3, p, True, cin=12))       # ... on the 128 x 128 tile, N = 96 ragged (the GLU layers' N)
        for (M, N), R in (((48, 68), 33), ((48, 68), 65), ((132, 260), 33), ((132, 260), 65)):
            out.append(TnCase(M, N, R, 4, p, True, lda_pad=4))
        out.append(TnCase(132, 260, 9000, 3, p, True, lda_pad=4, split_ints=False))
    return out


TN_CASES = _tn_cases()
assert len({c.name for c in TN_CASES}) == len(TN_CASES)
assert {c.kernel for c in TN_CASES} == {(big, p) for big in (False, True) for p in (0, 1, 2)}      # all six kernels, by big = M > 64 && N > 64
# the long case by the host rule: 6 tiles, want = 341, rs = ceil(27000 / 341) = 80 -> 96, 94 splits per clip, the last of 9000 - 93 * 96 = 72
# rows: three 32-row bf16 chunks per split (the two-ahead prefetch, kc + 2 < nk, needs nk >= 3), six 16-row fp32 chunks
assert tn_plan(132, 260, 9000, 3) == (True, 6, 96, 94, 3) and 9000 - 93 * 96 == 72
assert all(tn_plan(M, N, R, b)[2] == 64 for M, N in TN_MN for R in TN_R for b in (1, 3, 4))


def bf16_split(t64: torch.Tensor):
    """hi = bf16(v), lo = bf16(v - hi) as the kernels compute them (float32 in, round to nearest even); asserts hi + lo == v."""
    v = t64.float()
    assert torch.equal(v.double(), t64)
    hi = v.to(torch.bfloat16).float()
    lo = (v - hi).to(torch.bfloat16).float()
    assert torch.equal((hi + lo).double(), t64), "the bf16 hi / lo split is not exact"
    return hi.double(), lo.double()


@functools.lru_cache(maxsize=8)
def _tn_operands(key):
    M, N, R, batch, lda_pad, cin, frac = key
    g = _gen("tn", M, N, R, batch, cin)

    def draw(*shape):
        a = ints(g, *shape)
        b = ints(g, *shape)
        return a + torch.sign(a) * b.abs() * 2.0 ** -10 if frac else a            # b takes a's sign, and is 0 where a is

    A = draw(batch, R, M)
    Bv = draw(batch, 4 * (R - 1) + 8, cin) if cin else draw(batch, R, N)
    return A, Bv, ints(g, M, N), ints(g, M)


def tn_build(c: TnCase, fault: Optional[str] = None) -> Built:
    A, Bv, C0, cs0 = _tn_operands(c.operand_key)
    a_flat = _clips(A, c.R, c.lda, c.M, c.stride_a)
    b_flat = _clips(Bv, 1, c.region_b, c.region_b, c.stride_b) if c.cin else _clips(Bv, c.R, c.ldb, c.N, c.stride_b)
    big, tiles, rs, spb, ntn = c.plan
    rows = c.R
    if fault == "split_straddles_clip":                 # the last split of a clip runs its full rs rows, into the gap and the next clip
        rows = spb * rs
    tail = torch.full((rows * max(c.lda, c.ldb) + c.N + c.M,), NAN)
    Aw = torch.cat([a_flat, tail]).as_strided((c.batch, rows, c.M), (c.stride_a, c.lda, 1)).double()
    Bw = torch.cat([b_flat, tail]).as_strided((c.batch, rows, c.N), (c.stride_b, c.ldb, 1)).double()
    if fault is None:                                    # the windows hold what was drawn and nothing else
        assert torch.equal(Aw, A) and not bool(torch.isnan(Bw).any())
    if fault == "last_split_dropped":                   # the last K split of the last clip never runs
        Aw = Aw.clone()
        Aw[-1, (spb - 1) * rs:] = 0
    total_rows = c.batch * c.R
    if c.precision == 0 or not c.split_ints:
        prod, unit = torch.einsum("brm,brn->mn", Aw, Bw), 1.0
        assert total_rows * 9 + 3 < LIMIT
    else:
        if fault == "split_straddles_clip":
            ah, al, bh, bl = Aw, torch.zeros_like(Aw), Bw, torch.zeros_like(Bw)     # NaN rows: the value is NaN whatever the split
        else:
            (ah, al), (bh, bl) = bf16_split(Aw), bf16_split(Bw)
            assert total_rows <= 1500 and 9.1 * 2 ** 10 * total_rows < LIMIT
            assert torch.equal(ah, ah.round()) and torch.equal(bh, bh.round())       # hi = a: the products' unit is 2^-10, not 2^-20
            if fault is None and al.numel() >= 1000:
                assert 0.6 < float((al != 0).double().mean()) < 0.85                 # the low halves are really there (36 / 49 expected)
        e = lambda x, y: torch.einsum("brm,brn->mn", x, y)
        prod, unit = (e(ah, bh) + e(ah, bl) + e(al, bh) if c.precision == 1 else e(ah, bh)), 2.0 ** -10
    want_c = C0 + prod
    csum = cs0 + Aw.sum((0, 1)) * (ntn if fault == "colsum_every_tile" else 1)
    if fault is None:
        _exact(want_c, unit, 3 + 9.1 * total_rows)
        _exact(csum, unit, 3 + 3.1 * total_rows)
    else:
        want_c, csum = want_c.float().double(), csum.float().double()
    out = {"C": _out(c.M, c.ldc, c.N, want_c, C0)}
    if c.colsum:
        out["colsum"] = _out(1, c.M, c.M, csum, cs0)
    return Built({"A": a_flat, "Bm": b_flat}, out, {})


# ====================================================================================================== the two error models
PREP_FLOOR = 1e-3


@dataclass(frozen=True)
class PrepCase:
    B: int
    T: int
    VL: int

    @property
    def name(self): return f"B{self.B}-T{self.T}-VL{self.VL}"


PREP_CASES = [PrepCase(3, T, T + e) for T in (2, 3, 255, 256, 257, 1000) for e in (0, 1, 37)]


def prep(x: torch.Tensor, VL: int, floor_: float, fault: Optional[str] = None):
    """out = x / (std + floor) zero-padded to VL, std the unbiased standard deviation over time.  x (B, T) float64 -> (out (B, VL), std (B,))."""
    std = x.std(dim=1, unbiased=fault != "biased_std")
    return torch.nn.functional.pad(x / (std[:, None] + floor_), (0, VL - x.shape[1])), std


def prep_inputs(c: PrepCase) -> torch.Tensor:
    g = _gen("prep", c.B, c.T)
    gain = torch.tensor([0.01, 1.0, 30.0])[:c.B, None]
    return ((torch.randn(c.B, c.T, generator=g) + 0.25) * gain).float()


def prep_bounds(ref_out: torch.Tensor, ref_std: torch.Tensor):
    """|out - ref| <= 4 2^-23 |ref| (std rounded to float, the add of the floor, one float division allowed 2.5 ulp); std within 2^-23."""
    return 4 * U23 * ref_out.abs(), U23 * ref_std.abs()


@dataclass(frozen=True)
class GluCase:
    npad: int
    N: int
    rows: int
    ld_pad: int                  # ldg = N + ld_pad

    @property
    def name(self): return f"npad{self.npad}-N{self.N}-rows{self.rows}-ldg+{self.ld_pad}"
    @property
    def ldg(self): return self.N + self.ld_pad


GLU_CASES = [GluCase(npad, N, rows, p) for npad, N in ((64, 4), (64, 32), (128, 48), (192, 96)) for rows in (1, 37) for p in (0, 4)]
GLU_SMAX = 8.0


def glu_inputs(c: GluCase):
    """u (rows, npad) packed [32 values | 32 gates] per tile with gates in [-8, 8] (the ends and 0 included), finite values in the pad
    columns too; dg flat (rows, ldg) with NaN pads."""
    g = _gen("glu", c.npad, c.N, c.rows)
    u = torch.randn(c.rows, c.npad // 64, 2, 32, generator=g) * 2.0
    s = (torch.rand(c.rows, c.npad // 64, 32, generator=g) * 2 - 1) * GLU_SMAX
    s.reshape(-1)[:3] = torch.tensor([GLU_SMAX, -GLU_SMAX, 0.0])
    u[:, :, 1] = s
    dg = torch.randn(c.rows, c.N, generator=g)
    return u.reshape(c.rows, c.npad).float().contiguous(), _clips(dg[None].double(), c.rows, c.ldg, c.N, c.rows * c.ldg), dg.float()


def glu_bwd(u: torch.Tensor, dg: torch.Tensor, N: int, fault: Optional[str] = None):
    """In the packed layout: dv = d sigmoid(s), ds = d v sigmoid(s) (1 - sigmoid(s)) for output column n = 32 t + i < N, 0 in the pad
    columns.  u (rows, npad), dg (rows, N) float64 -> (du (rows, npad), |d| and |d v| in the same layout for the bounds)."""
    rows, npad = u.shape
    t = u.reshape(rows, npad // 64, 2, 32)
    v, s = (t[:, :, 1], t[:, :, 0]) if fault == "halves_swapped" else (t[:, :, 0], t[:, :, 1])
    d = torch.zeros(rows, npad // 2, dtype=torch.float64)
    d[:, :N] = dg
    d = d.reshape(rows, npad // 64, 32)
    sg = torch.sigmoid(s)
    dv, ds = d * sg, d * v * sg * (1.0 if fault == "one_minus_dropped" else (1 - sg))
    pack = lambda a, b: torch.stack([a, b], dim=2).reshape(rows, npad)
    return pack(dv, ds), pack(d.abs(), (d * v).abs())


def glu_bound(scale: torch.Tensor) -> torch.Tensor:
    """|dv - ref| <= 16 2^-24 |d|, |ds - ref| <= 16 2^-24 |d v| for |s| <= 8: the derivation (__expf's argument scaling |s| 2^-24, one ulp of
    the exponential, sg (1 - sg) <= 1/4, the add, the reciprocal and three multiplies) gives about 6.5 2^-24; 16 is a 2.5x margin."""
    return 16 * U24 * scale


def ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of err / bound; an error where the bound is 0 counts as infinite, and so does a NaN."""
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(torch.where(torch.isnan(r), inf, r).max()) if r.numel() else 0.0
