"""Host oracle of mfpa_gemm_mfma (csrc/demucs_gemm.hip): a float64 restatement of the formula in include/mfpa.h, an arithmetic model of the
bf16x3 kernels, the error bounds of tests/test_gpu_gemm.py and the case table both the CPU and the GPU tests walk.  No GPU here.

    C[b][m][n] = epi( sum_k A[b*strideA + m*lda + k] * W[n*K + k] + bias[n] ),  m < M

Everything is written from the header comment, not from the kernels: tests/test_gemm_oracle.py pins it against torch's own
convolutions, and shows that the bounds are satisfiable by correct arithmetic and miss faulty arithmetic tenfold."""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace
from typing import Dict, List, Optional

import numpy as np
import torch

# kernel ids of include/mfpa.h (MFPA_GEMM_*)
NONE, PIPE, PIPE_WSPLIT, WIDE, WIDE_WSPLIT, BF16X3, SHORTK48_C1, SHORTK48, SHORTK96, SMALLK48_C1, SMALLK48, MFMA_C1, MFMA = range(-1, 12)
KERNEL_NAMES = {PIPE: "pipe", PIPE_WSPLIT: "pipe_wsplit", WIDE: "wide", WIDE_WSPLIT: "wide_wsplit", BF16X3: "bf16x3",
                SHORTK48_C1: "shortk48_c1", SHORTK48: "shortk48", SHORTK96: "shortk96", SMALLK48_C1: "smallk48_c1",
                SMALLK48: "smallk48", MFMA_C1: "mfma_c1", MFMA: "mfma"}
FP32_IDS = (SMALLK48_C1, SMALLK48, MFMA_C1, MFMA)
WSPLIT_IDS = (PIPE_WSPLIT, WIDE_WSPLIT)
C1SRC_IDS = (SHORTK48_C1, SMALLK48_C1, MFMA_C1)

U24, U23, U15 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -15
SENTINEL_BITS = 0x7FC0BEEF            # a quiet NaN with a payload: outputs are pre-filled with it, A's gaps too
GAP_ROWS = 2                          # sentinel rows between the clips of C / C2
GAP_A = 12                            # NaN floats between the clips of A (a multiple of 4: strideA % 4)


@dataclass(frozen=True)
class Case:
    kid: int                 # the kernel this descriptor must route to
    precision: int
    K: int
    npad: int
    N: int
    M: int
    batch: int
    lda: int = 0             # 0: K (disjoint rows); K / 2: overlapping windows.  Unused with c1
    mode: int = 0
    relu: int = 0
    c2: bool = False
    bias: bool = True
    c1: bool = False         # A is the fused Conv1d(1 -> K, k8, s4) + ReLU of c1_x
    c1_extra: int = 0        # c1_lin = 4 (M - 1) + 8 + c1_extra
    walk: bool = False       # batch is chosen on the device: more tiles than ceil8(CUs) (the persistent tile walk)

    @property
    def name(self) -> str:
        s = f"{KERNEL_NAMES[self.kid]}-p{self.precision}-K{self.K}-n{self.npad}_{self.N}-M{self.M}-b{self.batch}"
        s += f"-lda{self.lda or self.K}" if not self.c1 else f"-c1+{self.c1_extra}"
        s += f"-m{self.mode}r{self.relu}" + ("+C2" if self.c2 else "") + ("" if self.bias else "-nobias") + ("-walk" if self.walk else "")
        return s

    # ---- buffer geometry (floats), shared by the host oracle and the device runner
    @property
    def ld_a(self): return self.lda or self.K
    @property
    def region_a(self): return (self.M - 1) * self.ld_a + self.K          # floats of A one clip's windows cover
    @property
    def stride_a(self): return self.region_a + GAP_A
    @property
    def ldc(self): return self.N + 8
    @property
    def stride_c(self): return (self.M + GAP_ROWS) * self.ldc
    @property
    def ldc2(self): return self.npad + 64
    @property
    def stride_c2(self): return (self.M + GAP_ROWS) * self.ldc2
    @property
    def ldadd(self): return self.N + 4
    @property
    def stride_add(self): return self.M * self.ldadd + 8
    @property
    def c1_lin(self): return 4 * (self.M - 1) + 8 + self.c1_extra
    @property
    def c2_cols(self): return self.npad if self.mode == 1 else self.N       # columns of a C2 row the kernel writes
    @property
    def operand_key(self):
        """Cases equal here draw the same operands (precision 2 against 1, the same rows on another kernel)."""
        return (self.K, self.npad, self.N, self.M, self.batch, self.ld_a, self.mode, self.bias, self.c1, self.c1_extra)


def pack_glu(w: torch.Tensor, b: Optional[torch.Tensor], npad: int):
    """(2N, K) value | gate rows -> npad rows in tiles of 64: [32 value rows | their 32 gate rows], zero padded (ops_demucs._pack_glu's order,
    restated)."""
    n = w.shape[0] // 2
    wp = torch.zeros(npad, w.shape[1], dtype=w.dtype)
    bp = torch.zeros(npad, dtype=w.dtype)
    for t in range((n + 31) // 32):
        c = min(32, n - 32 * t)
        wp[64 * t:64 * t + c] = w[32 * t:32 * t + c]
        wp[64 * t + 32:64 * t + 32 + c] = w[n + 32 * t:n + 32 * t + c]
        if b is not None:
            bp[64 * t:64 * t + c] = b[32 * t:32 * t + c]
            bp[64 * t + 32:64 * t + 32 + c] = b[n + 32 * t:n + 32 * t + c]
    return wp, (bp if b is not None else None)


def make_inputs(c: Case) -> Dict[str, Optional[torch.Tensor]]:
    """Seeded float32 operands of a case, on the host, in the layout the descriptor addresses."""
    g = torch.Generator().manual_seed(zlib.crc32(repr(c.operand_key).encode()))
    nan = float("nan")
    out: Dict[str, Optional[torch.Tensor]] = {"A": None, "x": None, "c1_w": None, "c1_b": None, "addend": None}
    if c.c1:
        out["x"] = torch.randn(c.batch, c.c1_lin, generator=g)
        out["c1_w"] = torch.randn(8, c.K, generator=g) / np.sqrt(8.0)
        out["c1_b"] = 0.5 * torch.randn(c.K, generator=g)
    else:
        A = torch.full((c.batch * c.stride_a,), nan)
        for b in range(c.batch):
            A[b * c.stride_a:b * c.stride_a + c.region_a] = torch.randn(c.region_a, generator=g)
        out["A"] = A
    if c.mode == 1:
        w = torch.randn(2 * c.N, c.K, generator=g) / np.sqrt(c.K)
        bias = torch.randn(2 * c.N, generator=g) if c.bias else None
        out["W"], out["bias"] = pack_glu(w, bias, c.npad)
    else:
        W = torch.zeros(c.npad, c.K)
        W[:c.N] = torch.randn(c.N, c.K, generator=g) / np.sqrt(c.K)
        out["W"] = W
        out["bias"] = None
        if c.bias:
            out["bias"] = torch.zeros(c.npad)
            out["bias"][:c.N] = torch.randn(c.N, generator=g)
    if c.mode >= 2:
        ad = torch.full((c.batch * c.stride_add,), nan)
        for b in range(c.batch):
            v = torch.randn(c.M, c.N, generator=g)
            if c.mode == 3:                      # away from 0 so that the mask is unambiguous, with exact zeros of both signs placed on purpose
                v = torch.where(v >= 0, v + 0.1, v - 0.1)
                flat = v.reshape(-1)
                flat[::7] = 0.0
                flat[3::11] = -0.0
            rows = ad[b * c.stride_add:b * c.stride_add + c.M * c.ldadd].view(c.M, c.ldadd)
            rows[:, :c.N] = v
        out["addend"] = ad
    return out


def _windows(c: Case, inp, dtype=torch.float64) -> torch.Tensor:
    """A as (batch, M, K) in `dtype`: the row windows, or the fused first layer evaluated exactly."""
    if not c.c1:
        return inp["A"].as_strided((c.batch, c.M, c.K), (c.stride_a, c.ld_a, 1)).to(dtype)
    xw = inp["x"].as_strided((c.batch, c.M, 8), (c.c1_lin, 4, 1)).double()
    return torch.relu(inp["c1_b"].double() + xw @ inp["c1_w"].double()).to(dtype)


def _c1_windows_f32(c: Case, inp) -> torch.Tensor:
    """The fused first layer as the device evaluates it: float32, bias first, then taps 0..7, one fused multiply-add each (the float64
    product of two float32 values is exact, so rounding the float64 sum to float32 is the FMA up to a double rounding)."""
    xw = inp["x"].as_strided((c.batch, c.M, 8), (c.c1_lin, 4, 1)).double()
    v = inp["c1_b"].double().expand(c.batch, c.M, c.K)
    for j in range(8):
        v = (v + xw[..., j:j + 1] * inp["c1_w"][j].double()).float().double()
    return torch.relu(v).float()


def _c1_abs(c: Case, inp) -> torch.Tensor:
    """S_A = |c1_b| + sum_j |c1_w| |x| (batch, M, K)."""
    xw = inp["x"].as_strided((c.batch, c.M, 8), (c.c1_lin, 4, 1)).double().abs()
    return inp["c1_b"].double().abs() + xw @ inp["c1_w"].double().abs()


def _addend(c: Case, inp) -> torch.Tensor:
    return inp["addend"].as_strided((c.batch, c.M, c.N), (c.stride_add, c.ldadd, 1)).double()


def glu_unpack(pre: torch.Tensor):
    """(..., npad) packed pre-activations -> values and gates (..., npad / 2): output column 32 t + i <- tile t, lanes i and 32 + i."""
    t = pre.reshape(*pre.shape[:-1], pre.shape[-1] // 64, 2, 32)
    return t[..., 0, :].reshape(*pre.shape[:-1], -1), t[..., 1, :].reshape(*pre.shape[:-1], -1)


def epilogue(c: Case, inp, pre: torch.Tensor, swap_glu_tile: Optional[int] = None):
    """float64 epilogue on (batch, M, npad) pre-activations (bias included) -> (C (batch, M, N), C2 (batch, M, c2_cols) or None)."""
    if c.mode == 1:
        v, g = glu_unpack(pre)
        if swap_glu_tile is not None:
            s = slice(32 * swap_glu_tile, 32 * swap_glu_tile + 32)
            v, g = v.clone(), g.clone()
            v[..., s], g[..., s] = g[..., s].clone(), v[..., s].clone()
        return (v * torch.sigmoid(g))[..., :c.N], (pre if c.c2 else None)
    y, c2 = pre[..., :c.N], None
    if c.relu == 2:
        y = torch.relu(y)
        c2 = y
    if c.mode == 2:
        y = y + _addend(c, inp)
    elif c.mode == 3:
        c2 = y
        y = torch.where(_addend(c, inp) > 0, y, torch.zeros_like(y))
    if c.relu == 1:
        y = torch.relu(y)
    return y, (c2 if c.c2 else None)


def reference(c: Case, inp) -> Dict[str, torch.Tensor]:
    """The header's formula in float64.  pre (batch, M, npad) = A W^T + bias; S = sum_k |a||w| + |bias| in the same layout; C, C2 the
    outputs; c1 (c1 cases) = sum_k S_A |w|, the weight of the fused first layer's own float32 error."""
    A, W = _windows(c, inp), inp["W"].double()
    bias = inp["bias"].double() if inp["bias"] is not None else torch.zeros(c.npad, dtype=torch.float64)
    pre = A @ W.t() + bias
    S = A.abs() @ W.abs().t() + bias.abs()
    C, C2 = epilogue(c, inp, pre)
    out = {"pre": pre, "S": S, "C": C, "C2": C2}
    if c.c1:
        out["c1"] = _c1_abs(c, inp) @ W.abs().t()
    return out


def _split(t32: torch.Tensor):
    hi = t32.to(torch.bfloat16).float()
    return hi.double(), (t32 - hi).to(torch.bfloat16).double()


def model_bf16x3(c: Case, inp, *, drop: Optional[str] = None, skip_chunk: Optional[int] = None, dup_last_row: bool = False,
                 swap_glu_tile: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The bf16x3 kernels' arithmetic in float64: x = hi + lo with hi = bf16(x), lo = bf16(x - hi), a product is al bh + ah bl + ah bh
    (al bl is dropped), accumulated exactly.  The keyword arguments build FAULTY variants (tests/test_gemm_oracle.py: the bounds must
    miss them): drop = "ah_bl" / "al_bh", skip_chunk = a 32-wide K chunk left out, dup_last_row = output row M - 1 taken from row
    M - 2, swap_glu_tile = value and gate exchanged in one 32-column output tile."""
    A32 = _c1_windows_f32(c, inp) if c.c1 else _windows(c, inp, torch.float32)
    return _products(c, inp, _split(A32), _split(inp["W"]), drop, skip_chunk, dup_last_row, swap_glu_tile)


def model_fp32_exact(c: Case, inp, *, skip_chunk: Optional[int] = None, dup_last_row: bool = False,
                     swap_glu_tile: Optional[int] = None) -> Dict[str, torch.Tensor]:
    """The fp32 kernels with exact accumulation (= reference on the float32 A), with the same fault switches."""
    A32 = _c1_windows_f32(c, inp) if c.c1 else _windows(c, inp, torch.float32)
    return _products(c, inp, (A32.double(), None), (inp["W"].double(), None), None, skip_chunk, dup_last_row, swap_glu_tile)


def _products(c, inp, a, w, drop, skip_chunk, dup_last_row, swap_glu_tile):
    (ah, al), (wh, wl) = a, w
    if skip_chunk is not None:
        keep = torch.ones(c.K, dtype=torch.float64)
        keep[32 * skip_chunk:32 * skip_chunk + 32] = 0
        ah, al = ah * keep, (al * keep if al is not None else None)
    pre = ah @ wh.t()
    if drop != "al_bh" and al is not None:
        pre = pre + al @ wh.t()
    if drop != "ah_bl" and wl is not None:
        pre = pre + ah @ wl.t()
    if inp["bias"] is not None:
        pre = pre + inp["bias"].double()
    if dup_last_row:
        pre = pre.clone()
        pre[:, c.M - 1] = pre[:, c.M - 2]
    C, C2 = epilogue(c, inp, pre, swap_glu_tile)
    return {"pre": pre, "C": C, "C2": C2}


# ------------------------------------------------------------------------------------------------------------------ bounds
def pre_bound(c: Case, ref, against: str) -> torch.Tensor:
    """Element-wise bound on |device pre-activation - X| in the (batch, M, npad) layout.
    against = "fp32":      X = reference, fp32 kernels:   (K + 4) 2^-24 S   (one fp32 rounding per accumulation step, bias, store)
    against = "model":     X = model_bf16x3:              (K + 4) 2^-24 S   (the accumulation alone)
    against = "reference": X = reference, bf16x3 kernels: (2^-15 + (K + 4) 2^-24) S   (lo rounding <= 2^-18 per operand, the dropped
                           al bl <= 2^-18: together ~ 2^-16.4, times a margin of 2.6)
    c1 cases add 9 2^-24 sum_k S_A |w| (the fp32 FMA chain of the fused first layer; ReLU is 1-Lipschitz)."""
    acc = (c.K + 4) * U24
    b = {"fp32": acc, "model": acc, "reference": U15 + acc}[against] * ref["S"]
    if c.c1:
        b = b + 9 * U24 * ref["c1"]
    return b


def out_bound(c: Case, ref, against: str) -> torch.Tensor:
    """Bound on |device C - X's C| (batch, M, N).  Modes 0, 2, 3: the pre-activation's (ReLU, the addition and the mask do not amplify).
    Mode 1 (no C2 to read the device's own pre-activations from): dv sigma + |v| (dg / 4 + sigma (|g| + 4) 2^-23), sigma' <= 1/4."""
    pb = pre_bound(c, ref, against)
    if c.mode != 1:
        return pb[..., :c.N]
    (dv, dg), (v, g) = glu_unpack(pb), glu_unpack(ref["pre"])
    s = torch.sigmoid(g)
    return (dv * s + v.abs() * (0.25 * dg + s * (g.abs() + 4) * U23))[..., :c.N]


def ratio(err: torch.Tensor, bound: torch.Tensor) -> float:
    """max over elements of err / bound; an error where the bound is 0 counts as infinite, and so does a NaN."""
    inf = torch.full_like(err, float("inf"))
    r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err == 0, torch.zeros_like(err), inf))
    return float(torch.where(torch.isnan(r), inf, r).max()) if r.numel() else 0.0


def glu_from_c2_bound(v: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
    """|C - v sigma(g)| for v, g the device's OWN stored pre-activations: relative (|g| + 4) 2^-23 (v_exp_f32 and v_rcp_f32 at 1 ulp each,
    the rounding of g log2(e), 1 + e, the product)."""
    return (g.abs() + 4) * U23 * (v * torch.sigmoid(g)).abs()


# ------------------------------------------------------------------------------------------------------------------ case table
def walk_batch(cus: int) -> int:
    """Pipe-walk cases (5 column tiles x 1 row tile per clip): the smallest batch with more tiles than ceil8(CUs) and a tile count that is
    no multiple of 8 (both ends of gemm_tile_at's range are then met)."""
    cus8 = (cus + 7) // 8 * 8
    b = cus8 // 5 + 1
    while (5 * b) % 8 == 0:
        b += 1
    return b


def _cases() -> List[Case]:
    out: List[Case] = []
    add = out.append
    # the eight epilogue forms: (mode, relu, C2)
    E = {"0/1": (0, 1, False), "2/2+C2": (2, 2, True), "2/1": (2, 1, False), "2/0": (2, 0, False), "3+C2": (3, 0, True), "3": (3, 0, False),
         "1": (1, 0, False), "1+C2": (1, 0, True)}

    def epi(base: Case, key: str, n_glu: int) -> Case:
        m, r, c2 = E[key]
        return replace(base, mode=m, relu=r, c2=c2, N=(n_glu if m == 1 else base.N))

    # ---- pipelined 256 x 128 kernel: K = 128 (4 chunks: the main loop is empty) / 192 (one trip); row tiles 192 .. 257 of 256
    for prec, kid in ((1, PIPE), (2, PIPE_WSPLIT)):
        for i, M in enumerate((192, 193, 255, 256, 257)):                   # every M edge in mode 0
            K = (128, 192)[i % 2]
            add(Case(kid, prec, K, 256, 225, M, 3, lda=(0, K // 2)[(i // 2) % 2], mode=0, relu=1))
        for i, key in enumerate(("2/2+C2", "2/1", "2/0", "3+C2", "3", "1", "1+C2")):    # every epilogue on a tail tile
            K = (192, 128)[i % 2]
            add(epi(Case(kid, prec, K, 256, 225, (257, 193)[i % 2], 3, lda=(K // 2, 0)[(i // 2) % 2]), key, 100))
        for key in ("0/0", "2/2"):                                           # the persistent tile walk (batch from the device's CU count)
            add(Case(kid, prec, 128, 640, 600, 193, 0, mode=int(key[0]), relu=int(key[2]), walk=True))
    # ---- wide 128 x 128 kernel: K = 160 (K % 64 != 0) keeps rows >= 192 here
    for prec, kid in ((1, WIDE), (2, WIDE_WSPLIT)):
        for i, M in enumerate((1, 127, 128, 129, 191, 300)):
            K = 160 if M == 300 else (128, 160)[i % 2]
            npad, N = ((128, 97), (256, 256))[i % 2]
            add(Case(kid, prec, K, npad, N, M, 2, lda=(0, K // 2)[(i // 2) % 2], mode=0, relu=1))
        for i, key in enumerate(("2/2+C2", "2/1", "2/0", "3+C2", "3", "1", "1+C2")):
            K = (160, 128)[i % 2]
            npad, N = ((128, 97), (256, 256))[(i // 2) % 2]
            add(epi(Case(kid, prec, K, npad, N, (300 if K == 160 else 129), 2, lda=(K // 2, 0)[i % 2]), key, 50 if npad == 128 else 100))
    # ---- 128 x 64 bf16x3 kernel (npad no multiple of 128)
    for M, K, (npad, N) in ((1, 128, (64, 31)), (129, 160, (192, 161)), (200, 128, (192, 161))):
        add(Case(BF16X3, 1, K, npad, N, M, 2, lda=K // 2, mode=0, relu=1))
    add(Case(BF16X3, 1, 128, 64, 17, 129, 2, lda=64, mode=1))
    add(Case(BF16X3, 1, 160, 192, 96, 200, 2, lda=80, mode=1))
    add(Case(BF16X3, 1, 128, 192, 161, 129, 2, lda=64, mode=2, relu=2, c2=True))
    add(Case(BF16X3, 1, 160, 64, 31, 200, 2, lda=80, mode=3))
    # ---- short-K bf16x3 kernels, K = 48 and 96
    for K, kid in ((48, SHORTK48), (96, SHORTK96)):
        half = K // 2 if K == 96 else 0
        add(Case(kid, 1, K, 64, 40, 127, 2, mode=0, relu=1))
        add(Case(kid, 1, K, 64, 40, 129, 2, lda=half, mode=0, relu=1))
        add(Case(kid, 1, K, 128, 48, 129, 2, mode=1))
        add(Case(kid, 1, K, 128, 48, 127, 2, lda=half, mode=1, c2=True))
        add(Case(kid, 1, K, 64, 40, 129, 2, lda=half, mode=3, c2=True))
    add(Case(SHORTK48_C1, 1, 48, 128, 48, 129, 2, mode=1, c1=True))
    add(Case(SHORTK48_C1, 1, 48, 128, 48, 1, 2, mode=1, c1=True, c1_extra=4))
    # ---- fp32 kernels (precision 0, and precision 1 where no bf16x3 kernel serves the K)
    add(Case(SMALLK48, 0, 48, 64, 40, 129, 2, mode=0, relu=1))
    add(Case(SMALLK48, 0, 48, 128, 48, 129, 2, mode=1))
    add(Case(SMALLK48_C1, 0, 48, 128, 48, 129, 2, mode=1, c1=True))
    add(Case(MFMA, 0, 16, 64, 33, 1, 2, lda=8, mode=0, relu=0, bias=False))
    add(Case(MFMA, 0, 64, 128, 128, 128, 2, mode=0, relu=0, bias=False))
    add(Case(MFMA, 0, 64, 64, 33, 130, 2, lda=32, mode=0, relu=0, bias=False))
    add(Case(MFMA, 0, 144, 64, 33, 130, 2, lda=72, mode=2, relu=1))
    add(Case(MFMA, 0, 192, 128, 128, 130, 2, lda=96, mode=3))
    add(Case(MFMA, 0, 192, 128, 64, 128, 2, mode=1))
    add(Case(MFMA, 1, 144, 128, 128, 130, 2, mode=0, relu=0, bias=False))        # precision 1: K = 144 has no bf16x3 kernel
    add(Case(MFMA, 1, 16, 64, 33, 130, 2, lda=8, mode=2, relu=1))
    add(Case(MFMA_C1, 1, 96, 128, 64, 130, 2, mode=1, c1=True))                   # the short-K kernel for 96 has no c1 form
    add(Case(MFMA_C1, 0, 256, 64, 33, 128, 2, mode=3, c1=True))
    add(Case(MFMA_C1, 0, 256, 128, 128, 1, 2, mode=0, relu=0, bias=False, c1=True, c1_extra=4))
    return out


CASES: List[Case] = _cases()
assert len({c.name for c in CASES}) == len(CASES)


def fixed(c: Case, cus: int = 256) -> Case:
    """A walk case with its batch filled in for a device of `cus` compute units (other cases unchanged)."""
    return replace(c, batch=walk_batch(cus)) if c.walk else c


@functools.lru_cache(maxsize=4)
def _inputs_cached(key_case: Case):
    return make_inputs(key_case)


def inputs_for(c: Case):
    """make_inputs(c), shared between the cases that draw the same operands (the case is reduced to what the draw depends on)."""
    return _inputs_cached(replace(c, kid=NONE, precision=0, relu=0, c2=False, walk=False))


def descriptor(c: Case, **ptrs):
    """The mfpa_gemm_desc of a case.  Pointers default to 1 (any non-null value: mfpa_gemm_mfma_route looks at no memory)."""
    from musicfpaugment_amd._lib import GemmDesc
    p = lambda k, used=True: (ptrs.get(k, 1) if used else 0)
    return GemmDesc(A=p("A", not c.c1), lda=c.ld_a, strideA=0 if c.c1 else c.stride_a, W=p("W"), bias=p("bias", c.bias),
                    addend=p("addend", c.mode >= 2), ldadd=c.ldadd, strideAdd=c.stride_add, C=p("C"), ldc=c.ldc, strideC=c.stride_c,
                    batch=c.batch, M=c.M, N=c.N, K=c.K, npad=c.npad, mode=c.mode, relu=c.relu, precision=c.precision,
                    c1_x=p("c1_x", c.c1), c1_lin=c.c1_lin if c.c1 else 0, c1_w=p("c1_w", c.c1), c1_b=p("c1_b", c.c1),
                    C2=p("C2", c.c2), ldc2=c.ldc2, strideC2=c.stride_c2)
