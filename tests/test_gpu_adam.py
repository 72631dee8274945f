"""The fused Adam step (csrc/unet_train.hip: adam_kernel behind mfpa_adam_step) past step one.

Adam's FIRST update is lr * g / (|g| + eps) whatever the code does with the betas, the bias corrections or a constant gradient
scale, and the parameter update is invariant to that scale at every step.  So this file compares parameters AND both moments,
after EVERY step of a longer run, with plain float64 Adam written out below (torch's form: p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2)
+ eps); no weight decay, no amsgrad):

  * the kernel over the C ABI: 40-step trajectories, a step entered mid-run (step 1000 / 100000), sizes around the launch's
    block and grid limits with guard regions behind every buffer, and the argument contract;
  * UNetTrainEngine / DemucsTrainEngine against torch.optim.Adam on the engines' own gradients, name by name, and a
    last_epoch.pt handed to a real torch.optim.Adam and to a fresh Trainer;
  * on the host (no GPU): five faulty variants of the float64 reference must miss the bound by 10x, so the inputs keep their
    discriminating power.

Bounds are measured, not chosen.  The yardstick is torch.optim.Adam in float32 on the CPU over the same gradients and the same
float32-rounded hyper-parameters (what the ABI receives: float32(0.999) moves 1 - beta2 by 1.3e-5 relative, which is the ABI's
doing, not the kernel's): its distance to the float64 reference, per step and per quantity -- max |dp| for the parameters,
max |dm| / max |m| and max |dv| / max |v| for the moments (plain relative error of m is useless: cancellation).  The kernel may
be FACTOR = 4 times as far (device sqrt / divide, another operation order).  A yardstick is taken over at least POP entries: the
maximum over a handful of entries is not an estimate of a rounding error.

The values measured on the MI355X are in the comment below the imports.
"""
import copy
import math

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

# Measured on the MI355X (every test prints its line with -s).  Yardstick = float32 torch.optim.Adam's distance to the float64
# reference (largest over the steps); ratio = kernel (or engine) distance / yardstick, worst over the steps; the bound is 4.
#
#   case                                      yardstick p / m / v               ratio p / m / v
#   40 steps, (1e-3, .9, .999, 1e-8, 1)       2.47e-6 / 1.31e-7 / 3.16e-7       1.00 / 2.43 / 1.23
#   40 steps, (2e-3, .8, .99, 1e-8, 1/2)      1.95e-6 / 1.09e-7 / 3.53e-7       1.00 / 1.90 / 1.17
#   40 steps, (1e-3, .5, .9, 1e-6, 1/4)       1.77e-6 / 6.51e-8 / 2.48e-7       1.00 / 1.00 / 1.29
#   entered at step 1000 / 100000, 3 sets     1.8..2.4e-7 / 3.6..7.4e-8 / 4.8..7.2e-8   1.00 / 0.67..1.70 / 1.00
#   sizes 1 .. 4099, 3 steps                  (over 65536 entries)              0.07..0.90 / 0.93..1.27 / 0.55..0.91
#   sizes 1048577, 4194561, 31036481          (over the n entries)              1.00 / 1.24..1.46 / 1.00..1.29
#   UNet engine, 6 steps                      3.03e-7 / 1.57e-7 / 2.40e-7       1.00 / 1.78 / 1.00
#   Demucs engine, 6 steps                    3.66e-8 / 1.13e-7 / 1.75e-7       1.00 / 1.18 / 1.00
#   checkpoint hand-over, step 4              5.97e-8 / 6.07e-8 / 8.06e-8       1.01 / 1.68 / 4.75 (*)
#
# A ratio of exactly 1.00 on p: the worst entry is the same one on both sides and the kernel's float32 result there is torch's.
# (*) torch holds the file's unrounded 0.99 there while the ABI holds float32(0.99), which moves 1 - beta2 by 9.5e-7 relative:
# that is the allowance of _anchor_extra (5.9e-6 on v), not kernel error -- on rounded betas the same step sits at 1.0 (engine rows).
# The five faulty variants of the reference land 158x .. 3e8x outside the bound (host self-check, printed with -s).

HYPER = [(1e-3, 0.9, 0.999, 1e-8, 1.0),
         (2e-3, 0.8, 0.99, 1e-8, 0.5),            # the betas Trainer.from_reference is tested with
         (1e-3, 0.5, 0.9, 1e-6, 0.25)]
HYPER_IDS = ["default", "from_reference_betas_half", "short_memory_big_eps_quarter"]
K_STEPS = 40
N_TRAJ = 200_000
FACTOR = 4.0
POP = 65536
GUARD = 1024
SENTINEL = 0x5A5A5A5A
# mfpa_adam_step launches grid_for(n, 256 * 4, 256 * 16) blocks of 256 threads (csrc/unet_train.hip)
THREADS, PER_BLOCK, GRID_CAP = 256, 256 * 4, 256 * 16
UNET_PARAMS = 31_036_481
EINVAL = -22
FAULTS = {"beta1_for_v": ("v", "p"), "bias_step_plus_1": ("p",), "eps_inside_sqrt": ("p",), "eps_before_bias": ("p",),
          "scale_dropped": ("m", "v", "p")}


def _f32(x) -> float:
    return float(np.float32(x))


def _hp32(hp):
    return tuple(_f32(x) for x in hp)


def _draw_grad(rng, base, step):
    """|g| = the entry's own scale (log-uniform over 1e-12 .. 1, fixed over the run, so entries within a few decades of eps STAY
    in the eps regime) times a fresh factor in 1/2 .. 2, fresh random sign; a moving 17th of the entries is exactly zero, and the
    entries i % 101 == 100 are zero at every step."""
    N = base.shape[0]
    mag = np.clip(base * 2.0 ** rng.uniform(-1.0, 1.0, N), 1e-12, 1.0)
    g = (mag * rng.choice(np.array([-1.0, 1.0]), N)).astype(np.float32)
    idx = np.arange(N)
    g[(idx + step) % 17 == 0] = 0.0
    g[idx % 101 == 100] = 0.0
    return g


def _always_zero(n):
    return np.arange(n) % 101 == 100


def ref_adam_step(p, g, m, v, step, hp, fault=None):
    """One float64 Adam step on numpy arrays; hp = (lr, beta1, beta2, eps, grad_scale) as the ABI holds them.  `fault`: one of
    FAULTS, the deliberately wrong variants of the host self-check."""
    lr, b1, b2, eps, scale = hp
    gs = g if fault == "scale_dropped" else g * scale
    m = b1 * m + (1.0 - b1) * gs
    bv = b1 if fault == "beta1_for_v" else b2
    v = bv * v + (1.0 - bv) * gs * gs
    t = step + 1 if fault == "bias_step_plus_1" else step
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if fault == "eps_inside_sqrt":
        den = np.sqrt(v + eps) / math.sqrt(bc2)
    elif fault == "eps_before_bias":
        den = (np.sqrt(v) + eps) / math.sqrt(bc2)
    else:
        den = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - lr / bc1 * m / den, m, v


class _TorchAdam:
    """torch.optim.Adam on ONE flat CPU tensor, entered at any step with given moments."""

    def __init__(self, p0, m0, v0, start_step, hp, dtype):
        lr, b1, b2, eps, self.scale = hp
        self.dtype = dtype
        self.p = torch.from_numpy(np.asarray(p0)).to(dtype).clone().requires_grad_(True)
        self.opt = torch.optim.Adam([self.p], lr=lr, betas=(b1, b2), eps=eps)
        self.opt.state[self.p] = {"step": torch.tensor(float(start_step - 1)),
                                  "exp_avg": torch.from_numpy(np.asarray(m0)).to(dtype).clone(),
                                  "exp_avg_sq": torch.from_numpy(np.asarray(v0)).to(dtype).clone()}

    def step(self, g32):
        g = torch.from_numpy(g32).to(self.dtype)
        self.p.grad = g * self.scale                  # scale 1, 1/2, 1/4: exact in either type
        self.opt.step()
        st = self.opt.state[self.p]
        return self.p.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


def _norm_dist(got, want):
    d = float(np.max(np.abs(got.astype(np.float64) - want)))
    den = float(np.max(np.abs(want)))
    if den == 0.0:
        return 0.0 if d == 0.0 else float("inf")
    return d / den


def _dist(got, want, n=None):
    """(max |dp|, max |dm| / max |m|, max |dv| / max |v|) of (p, m, v) triples, over the first n entries."""
    s = slice(None) if n is None else slice(0, n)
    return {"p": float(np.max(np.abs(got[0][s].astype(np.float64) - want[0][s]))),
            "m": _norm_dist(got[1][s], want[1][s]), "v": _norm_dist(got[2][s], want[2][s])}


class _Trajectory:
    """Inputs and yardsticks of one run: N = max(n, POP) entries, of which the kernel gets the first n."""

    def __init__(self, n, seed, hp, start_step=1, warm=False, anchor=False):
        self.n, self.N, self.hp, self.start = n, max(n, POP), hp, start_step
        self.rng = np.random.default_rng(seed)
        N = self.N
        self.base = 10.0 ** self.rng.uniform(-12.0, 0.0, N)
        self.p0 = self.rng.standard_normal(N).astype(np.float32)
        if warm:                                   # a run in progress: m of the gradients' size, v between m^2 and 4 m^2
            self.m0 = (self.base * self.rng.uniform(0.1, 1.0, N) * self.rng.choice(np.array([-1.0, 1.0]), N)).astype(np.float32)
            self.v0 = (self.m0.astype(np.float64) ** 2 * self.rng.uniform(1.0, 4.0, N)).astype(np.float32)
        else:
            self.m0, self.v0 = np.zeros(N, np.float32), np.zeros(N, np.float32)
        self.hp32 = _hp32(hp)
        self.ref = (self.p0.astype(np.float64), self.m0.astype(np.float64), self.v0.astype(np.float64))
        self.yard = _TorchAdam(self.p0, self.m0, self.v0, start_step, self.hp32, torch.float32)
        self.anchor = _TorchAdam(self.p0, self.m0, self.v0, start_step, hp, torch.float64) if anchor else None

    def steps(self, count):
        """Yields (step, g float32, float64 reference (p, m, v), yardstick distances, anchor (p, m, v) or None)."""
        for k in range(count):
            step = self.start + k
            g = _draw_grad(self.rng, self.base, step)
            self.ref = ref_adam_step(self.ref[0], g.astype(np.float64), self.ref[1], self.ref[2], step, self.hp32)
            yard = _dist(self.yard.step(g), self.ref)
            anchor = self.anchor.step(g) if self.anchor is not None else None
            yield step, g, self.ref, yard, anchor


def _anchor_extra(hp, steps_done):
    """What the unrounded Python betas of the outside anchor may add.  A float32 beta is off by at most half an ulp, 2^-25 for
    beta in [0.5, 1); that moves the weights (1 - beta) beta^k of a moment by at most 2^-24 * beta / (1 - beta) relative in sum,
    so m and v by that much of their largest entry.  One update is lr * mhat / (sqrt(vhat) + eps), at most lr * max(1, (1 - beta1)
    / sqrt(1 - beta2)) in size; its relative change is at most d1 + d2 / 2 from the moments and as much again from the bias
    corrections, and the parameters add that up over the steps taken."""
    lr, b1, b2, _, _ = hp
    d1, d2 = 2.0 ** -24 * b1 / (1.0 - b1), 2.0 ** -24 * b2 / (1.0 - b2)
    cap = max(1.0, (1.0 - b1) / math.sqrt(1.0 - b2))
    return {"p": steps_done * lr * cap * 2.0 * (d1 + d2 / 2.0), "m": d1, "v": d2}


# ----------------------------------------------------------------------------- host self-check (no GPU)
@pytest.mark.parametrize("hp", HYPER, ids=HYPER_IDS)
def test_faulty_variants_of_the_reference_miss_the_bound_tenfold_on_the_host(hp):
    """A condition on the INPUTS: with these gradients and hyper-parameters each of five plausible faults lands at least 10x
    outside the bound the kernel is held to (FACTOR x the float32-torch yardstick) on the quantity it should show in, at some
    step.  Needs no GPU."""
    traj = _Trajectory(N_TRAJ, 1234, hp)
    faults = {f: q for f, q in FAULTS.items() if not (f == "scale_dropped" and hp[4] == 1.0)}
    state = {f: traj.ref for f in faults}
    worst = {f: {q: 0.0 for q in qs} for f, qs in faults.items()}
    yard_max = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step, g, ref, yard, _ in traj.steps(K_STEPS):
        yard_max = {q: max(yard_max[q], yard[q]) for q in yard}
        for f, qs in faults.items():
            state[f] = ref_adam_step(state[f][0], g.astype(np.float64), state[f][1], state[f][2], step, traj.hp32, fault=f)
            d = _dist(state[f], ref)
            for q in qs:
                if yard[q] > 0.0:              # (step 1 at beta1 = 1/2 is exact in float32: yardstick 0, nothing to divide by)
                    worst[f][q] = max(worst[f][q], d[q] / (FACTOR * yard[q]))
    print(f"hp {hp}: largest yardsticks {yard_max}; fault distance / bound {worst}")
    for f, qs in faults.items():
        for q in qs:
            assert worst[f][q] >= 10.0, f"fault {f} is only {worst[f][q]:.2f}x the bound on {q} (yardsticks {yard_max})"


# ----------------------------------------------------------------------------- the kernel over the C ABI
def _L():
    from musicfpaugment_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


class _DeviceAdam:
    """p, g, m, v on the device, each followed by a guard region, stepped by mfpa_adam_step."""

    def __init__(self, p0, m0, v0, n):
        self.n = n
        self.buf = {}
        for k, a in (("p", p0), ("g", None), ("m", m0), ("v", v0)):
            t = torch.empty(n + GUARD, dtype=torch.float32, device="cuda")
            t.view(torch.int32).fill_(SENTINEL)
            if a is not None:
                t[:n].copy_(torch.from_numpy(np.ascontiguousarray(a[:n])))
            self.buf[k] = t

    def step(self, g, step, hp):
        L, ptr, stream = _L()
        b, n = self.buf, self.n
        b["g"][:n].copy_(torch.from_numpy(np.ascontiguousarray(g[:n])))
        lr, b1, b2, eps, scale = hp                                   # Python floats: ctypes rounds them to float32, as for the engines
        rc = L.mfpa_adam_step(ptr(b["p"]), ptr(b["g"]), ptr(b["m"]), ptr(b["v"]), n, lr, b1, b2, eps, step, scale, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert np.array_equal(b["g"][:n].cpu().numpy(), g[:n])         # the gradient is read only
        return tuple(b[k][:n].cpu().numpy() for k in ("p", "m", "v"))

    def guards_intact(self):
        return {k: bool((t.view(torch.int32)[self.n:] == SENTINEL).all()) for k, t in self.buf.items()}


def _check(case, step, got, ref, yard, n, extra=None, against="float64 reference"):
    d = _dist(got, ref, n)
    ratios = {}
    for q in ("p", "m", "v"):
        bound = FACTOR * yard[q] + (extra[q] if extra else 0.0)
        ratios[q] = d[q] / yard[q] if yard[q] > 0 else (0.0 if d[q] == 0 else float("inf"))
        assert d[q] <= bound, (f"{case}, step {step}, {q} against the {against}: kernel distance {d[q]:.3e}, float32-torch yardstick "
                               f"{yard[q]:.3e}, bound {bound:.3e} (= {FACTOR} x yardstick" + (f" + {extra[q]:.3e}" if extra else "") + ")")
    return ratios


def _worse(a, b):
    return {q: max(a[q], b[q]) for q in a}


@gpu
@pytest.mark.parametrize("hp", HYPER, ids=HYPER_IDS)
def test_kernel_trajectory_matches_float64_adam_at_every_step(hp):
    n = N_TRAJ
    traj = _Trajectory(n, 1234, hp, anchor=True)
    dev = _DeviceAdam(traj.p0, traj.m0, traj.v0, n)
    zero = _always_zero(n)
    worst, yard_max, done = {"p": 0.0, "m": 0.0, "v": 0.0}, {"p": 0.0, "m": 0.0, "v": 0.0}, 0
    for step, g, ref, yard, anchor in traj.steps(K_STEPS):
        got = dev.step(g, step, hp)
        done += 1
        worst = _worse(worst, _check(f"hp {hp}", step, got, ref, yard, n))
        yard_max = _worse(yard_max, yard)
        _check(f"hp {hp}", step, got, anchor, yard, n, extra=_anchor_extra(hp, done), against="float64 torch.optim.Adam (unrounded betas)")
        # an entry whose gradient is zero at every step is never touched: the Demucs engine's padding columns rely on it
        assert np.array_equal(got[0][zero].view(np.int32), traj.p0[:n][zero].view(np.int32)), step
        assert not got[1][zero].any() and not got[2][zero].any(), step
    assert all(dev.guards_intact().values()), dev.guards_intact()
    print(f"MEASURED trajectory hp {hp}: worst kernel distance / yardstick {worst}; largest yardsticks {yard_max}")


@gpu
@pytest.mark.parametrize("start", [1000, 100000])
@pytest.mark.parametrize("hp", HYPER, ids=HYPER_IDS)
def test_kernel_step_entered_mid_run(hp, start):
    """The resume path: given non-zero moments, one step at a large step number -- pow(0.5, 100000) underflows to 0."""
    n = N_TRAJ
    traj = _Trajectory(n, 77 + start, hp, start_step=start, warm=True, anchor=True)
    dev = _DeviceAdam(traj.p0, traj.m0, traj.v0, n)
    for step, g, ref, yard, anchor in traj.steps(1):
        assert step == start
        got = dev.step(g, step, hp)
        r = _check(f"hp {hp} entered at {start}", step, got, ref, yard, n)
        _check(f"hp {hp} entered at {start}", step, got, anchor, yard, n, extra=_anchor_extra(hp, 1), against="float64 torch.optim.Adam (unrounded betas)")
        print(f"MEASURED mid-run hp {hp} step {start}: kernel distance / yardstick {r}; yardsticks {yard}")
    assert all(dev.guards_intact().values()), dev.guards_intact()


SIZES = [1, 255, 256, 257, 1024 * 4 + 3, GRID_CAP * THREADS + 1, GRID_CAP * PER_BLOCK + 257, UNET_PARAMS]


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_kernel_sizes_and_guard_regions(n):
    """One thread, a partial block, exact blocks, more elements than the capped grid has threads (every thread takes several
    trips of the grid-stride loop, the last one partial), and the UNet's parameter count; nothing is written past n."""
    hp = HYPER[1]
    steps = 2 if n >= UNET_PARAMS else 3
    traj = _Trajectory(n, 4242 + n % 1000, hp)
    dev = _DeviceAdam(traj.p0, traj.m0, traj.v0, n)
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for step, g, ref, yard, _ in traj.steps(steps):
        got = dev.step(g, step, hp)
        worst = _worse(worst, _check(f"n {n}", step, got, ref, yard, n))
    assert all(dev.guards_intact().values()), dev.guards_intact()
    print(f"MEASURED size n {n}: worst kernel distance / yardstick {worst}")


@gpu
def test_kernel_argument_contract():
    """Return codes only: every refused call returns before anything is launched."""
    L, ptr, stream = _L()
    n = 64
    dev = _DeviceAdam(np.ones(n, np.float32), np.ones(n, np.float32), np.ones(n, np.float32), n)
    dev.buf["g"][:n].fill_(1.0)
    before = {k: t.clone() for k, t in dev.buf.items()}
    P = {k: ptr(t) for k, t in dev.buf.items()}
    hp = (1e-3, 0.9, 0.999, 1e-8)
    call = lambda p, g, m, v, cnt, step: L.mfpa_adam_step(p, g, m, v, cnt, *hp, step, 1.0, stream())
    assert call(P["p"], P["g"], P["m"], P["v"], 0, 1) == 0                   # n == 0: nothing to do
    assert call(0, 0, 0, 0, 0, 1) == 0
    for step in (0, -1):
        assert call(P["p"], P["g"], P["m"], P["v"], n, step) == EINVAL
    assert call(P["p"], P["g"], P["m"], P["v"], -1, 1) == EINVAL
    for missing in ("p", "g", "m", "v"):
        args = [0 if k == missing else P[k] for k in ("p", "g", "m", "v")]
        assert call(*args, n, 1) == EINVAL, missing
    torch.cuda.synchronize()
    for k, t in dev.buf.items():
        assert torch.equal(t.view(torch.int32), before[k].view(torch.int32)), k


# ----------------------------------------------------------------------------- the engines against torch.optim.Adam
ENGINE_LR, ENGINE_BETAS, ENGINE_EPS = 2e-3, (0.8, 0.99), 1e-8


class _NamedAdams:
    """torch.optim.Adam over named CPU copies of the parameters, twice: float64 (the reference) and float32 (the yardstick)."""

    def __init__(self, names, params, opts):
        self.names, self.params, self.opts = names, params, opts       # params / opts: {dtype: ...}
        self.last_yard = {}                                            # the yardsticks of the last check()

    @classmethod
    def fresh(cls, named, lr, betas, eps):
        """Both on the hyper-parameters as the ABI holds them (rounded to float32): the comparison is about the arithmetic."""
        names = list(named)
        params, opts = {}, {}
        for dt in (torch.float64, torch.float32):
            params[dt] = {k: named[k].detach().cpu().to(dt).clone().requires_grad_(True) for k in names}
            opts[dt] = torch.optim.Adam(list(params[dt].values()), lr=_f32(lr), betas=(_f32(betas[0]), _f32(betas[1])), eps=_f32(eps))
        return cls(names, params, opts)

    def step(self, grads):
        for dt in self.params:
            for k in self.names:
                self.params[dt][k].grad = grads[k].detach().cpu().to(dt).clone()
            self.opts[dt].step()

    def state(self, dt, key):
        return {k: self.opts[dt].state[self.params[dt][k]][key] for k in self.names}

    def torch_step(self):
        steps = {int(float(s)) for dt in self.params for s in self.state(dt, "step").values()}
        assert len(steps) == 1, steps
        return steps.pop()

    def check(self, case, got_p, got_m, got_v, extra=None):
        """Name by name: max |dp|, and max |dm| / max |m|, max |dv| / max |v| within the tensor; the yardstick is the float32
        torch run's worst tensor."""
        f64, f32 = torch.float64, torch.float32
        want = {"p": {k: self.params[f64][k].detach() for k in self.names}, "m": self.state(f64, "exp_avg"), "v": self.state(f64, "exp_avg_sq")}
        yard_src = {"p": {k: self.params[f32][k].detach() for k in self.names}, "m": self.state(f32, "exp_avg"), "v": self.state(f32, "exp_avg_sq")}
        got = {"p": got_p, "m": got_m, "v": got_v}
        ratios = {}
        for q in ("p", "m", "v"):
            def dist(src, k):
                a, w = src[k].detach().cpu().double().numpy(), want[q][k].numpy()
                assert a.shape == w.shape, (k, a.shape, w.shape)
                return float(np.max(np.abs(a - w))) if q == "p" else _norm_dist(a, w)
            yards = {k: dist(yard_src[q], k) for k in self.names}
            yard = max(yards.values())
            self.last_yard[q + " at"] = max(yards, key=yards.get)
            ds = {k: dist(got[q], k) for k in self.names}
            name = max(ds, key=ds.get)
            bound = FACTOR * yard + (extra[q] if extra else 0.0)
            assert ds[name] <= bound, (f"{case}, {q}: engine distance {ds[name]:.3e} at {name}, float32-torch yardstick {yard:.3e}, "
                                       f"bound {bound:.3e}")
            ratios[q] = ds[name] / yard if yard > 0 else 0.0
            self.last_yard[q] = yard
        return ratios


def _unet_inputs():
    from musicfpaugment_amd import ops, synth
    clean = synth.batch(2, seed=500, n=8000)
    aug = (0.7 * clean + 0.3 * synth.batch(2, seed=600, n=8000, tonal=False)).astype(np.float32)
    cm, cmax = ops.stft_mag(torch.from_numpy(clean).cuda(), torch.float64)
    am, amax = ops.stft_mag(torch.from_numpy(aug).cuda(), torch.float64)
    clean_spec = ops.normalize_(cm, cmax, per_clip=False)
    return am, amax.max().expand(2).contiguous(), clean_spec


@gpu
def test_unet_engine_steps_match_torch_adam_on_the_same_gradients():
    """Six optimiser steps of UNetTrainEngine with lr 2e-3, betas (0.8, 0.99); torch.optim.Adam is handed the ENGINE's gradients
    each step, so the comparison isolates the optimiser and the flat-buffer <-> named-tensor mapping (no float-atomic noise)."""
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    net = UNet(1, 1, rate=0.0)
    net.load_state_dict(formula_state_dict(0))
    net = net.cuda().train()
    eng = UNetTrainEngine(net, lr=ENGINE_LR, betas=ENGINE_BETAS, eps=ENGINE_EPS, precision=0)
    ref = _NamedAdams.fresh(dict(net.named_parameters()), ENGINE_LR, ENGINE_BETAS, ENGINE_EPS)
    am, aug_den, clean_spec = _unet_inputs()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k in range(6):
        pred = eng.forward(spec64=am, denom=aug_den)
        _, dpred = eng.l1_loss(pred, clean_spec)
        eng.backward(dpred)
        ref.step({n: g.clone() for n, g in eng.named_grads().items()})
        eng.optimizer_step()
        eng.sync_to_module()
        m, v = eng.named_moments()
        worst = _worse(worst, ref.check(f"UNet engine step {k + 1}", dict(net.named_parameters()), m, v))
        assert eng.step_count == ref.torch_step() == k + 1
    print(f"MEASURED UNet engine, 6 steps: worst engine distance / yardstick {worst}; yardsticks at step 6 {ref.last_yard}")


def _demucs_inputs():
    from musicfpaugment_amd import synth
    clean = torch.from_numpy(synth.batch(2, seed=31, n=4000))
    aug = (clean + 0.05 * torch.from_numpy(synth.batch(2, seed=77, n=4000))).float()
    return clean, aug


@gpu
def test_demucs_engine_steps_match_torch_adam_on_the_same_gradients():
    from musicfpaugment_amd.ops_demucs_train import DemucsTrainEngine
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict
    sd = formula_state_dict(0)
    eng = DemucsTrainEngine(sd, "cuda", lr=ENGINE_LR, betas=ENGINE_BETAS, eps=ENGINE_EPS, precision=0)
    ref = _NamedAdams.fresh(eng.state_dict(), ENGINE_LR, ENGINE_BETAS, ENGINE_EPS)
    assert set(ref.names) == set(sd)
    clean, aug = _demucs_inputs()
    clean, aug = clean.cuda(), aug.cuda()
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for k in range(6):
        pred = eng.forward(aug)
        _, _, _, dpred = eng.loss_and_grad(pred, clean)
        eng.backward(dpred)
        ref.step(eng.grad_dict())
        eng.adam_step()
        m, v = eng.named_moments()
        worst = _worse(worst, ref.check(f"Demucs engine step {k + 1}", eng.state_dict(), m, v))
        assert eng.step_count == ref.torch_step() == k + 1
    # the padding of the master layouts (rows / columns no reference parameter maps to) has zero gradients and stays zero
    mask = torch.empty_like(eng.flat_p)
    eng.load_state_dict({k: torch.ones_like(t) for k, t in sd.items()}, mask)
    pad = mask == 0
    assert 0 < int(pad.sum()) < pad.numel() and int((~pad).sum()) == sum(t.numel() for t in sd.values())
    for name in ("flat_p", "flat_m", "flat_v"):
        assert not bool(getattr(eng, name)[pad].any()), name
    print(f"MEASURED Demucs engine, 6 steps: worst engine distance / yardstick {worst}; yardsticks at step 6 {ref.last_yard}")


@gpu
def test_checkpoint_hands_betas_and_eps_over_to_torch_adam_and_to_a_fresh_trainer(tmp_path):
    """last_epoch.pt of a Trainer built through from_reference with betas (0.8, 0.99): torch.optim.Adam.load_state_dict restores
    the whole param group, so a fresh default-constructed Trainer that loads the same file must continue with the same betas and
    eps -- one more identical gradient, same update on both sides."""
    from musicfpaugment_amd import synth
    from musicfpaugment_amd.training.train import EarlyStopping, Trainer, _RefEarlyStopping
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict

    def loader(seed):
        k = 0
        while True:
            clean = synth.batch(2, seed=seed + 2 * (k % 2), n=8000)
            noise = synth.batch(2, seed=seed + 100 + 2 * (k % 2), n=8000, tonal=False)
            yield torch.from_numpy(clean)[:, :, None], torch.from_numpy((0.7 * clean + 0.3 * noise).astype(np.float32))[:, :, None]
            k += 1

    net = UNet(1, 1, rate=0.0)
    net.load_state_dict(formula_state_dict(3))
    opt = torch.optim.Adam(net.parameters(), lr=ENGINE_LR, betas=ENGINE_BETAS)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", factor=0.5, patience=3)
    a = Trainer.from_reference(net, loader(10), 4, loader(10), 2, {"l1": torch.nn.L1Loss(reduction="mean")}, opt, sched,
                               EarlyStopping(patience=7, min_delta=0.01), 2, "cuda", {"name": "t", "model": "unet"},
                               monitoring=False, save=True, checkpoint=str(tmp_path), input_type="spec")
    a.train_epoch(1)                                                     # train_steps - 1 = 3 optimiser steps
    a.epoch = 1
    assert a.engine.step_count == 3
    a.save_checkpoint(1.0)
    with torch.serialization.safe_globals([_RefEarlyStopping]):
        ck = torch.load(tmp_path / "last_epoch.pt", map_location="cpu", weights_only=True)
    group = ck["optimizer_state_dict"]["param_groups"][0]
    assert tuple(group["betas"]) == ENGINE_BETAS and group["eps"] == ENGINE_EPS and group["lr"] == ENGINE_LR
    # torch's side: a real Adam built with its defaults, then handed the file's state (float64 reference, float32 yardstick)
    names, params, opts = None, {}, {}
    for dt in (torch.float64, torch.float32):
        rn = UNet(1, 1, rate=0.0).to(dt)
        rn.load_state_dict(ck["model_state_dict"])
        o = torch.optim.Adam(rn.parameters())
        o.load_state_dict(copy.deepcopy(ck["optimizer_state_dict"]))      # (load_state_dict keeps the file's `step` tensors: one set each)
        assert tuple(o.param_groups[0]["betas"]) == ENGINE_BETAS
        names = [n for n, _ in rn.named_parameters()]
        params[dt], opts[dt] = dict(rn.named_parameters()), o
    ref = _NamedAdams(names, params, opts)
    # this package's side: a fresh default-constructed Trainer
    b = Trainer(UNet(1, 1, rate=0.0), loader(10), None, ckpt_path=str(tmp_path))
    assert b.load_checkpoint() and b.engine.step_count == 3
    m, v = b.engine.named_moments()
    for n in names:
        assert torch.equal(m[n].cpu().double(), ref.state(torch.float64, "exp_avg")[n]), n
        assert torch.equal(v[n].cpu().double(), ref.state(torch.float64, "exp_avg_sq")[n]), n
    am, aug_den, clean_spec = _unet_inputs()
    pred = b.engine.forward(spec64=am, denom=aug_den)
    _, dpred = b.engine.l1_loss(pred, clean_spec)
    b.engine.backward(dpred)
    ref.step({n: g.clone() for n, g in b.engine.named_grads().items()})
    b.engine.optimizer_step()
    b.engine.sync_to_module()
    m, v = b.engine.named_moments()
    # the torch side holds the file's unrounded Python betas: the derived allowance of the outside anchor, one step
    extra = _anchor_extra((ENGINE_LR, *ENGINE_BETAS, ENGINE_EPS, 1.0), 1)
    r = ref.check("step 4 after the hand-over", dict(b.model.named_parameters()), m, v, extra=extra)
    assert b.engine.step_count == ref.torch_step() == 4
    assert tuple(b.engine.betas) == ENGINE_BETAS and b.engine.eps == ENGINE_EPS and b.engine.lr == ENGINE_LR
    print(f"MEASURED checkpoint hand-over, step 4: engine distance / yardstick {r}; yardsticks {ref.last_yard}")
