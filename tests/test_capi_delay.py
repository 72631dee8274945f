"""CPU: the delay lines' entry points (mfpa_varidelay, mfpa_comb) through ctypes.  They check their arguments before any launch and
never dereference a pointer on the host, so all of this runs without a GPU (the style of tests/test_capi_dynamics.py).  The Python
refusals of ops.variable_delay / comb / lfo_delay / speed_drift_delay, of the functional fronts and of the Echo / WowFlutter /
Chorus transforms need none either."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 1 << 12          # a non-null, 16-byte aligned value for pointers that are never dereferenced


@pytest.fixture(scope="module")
def lib():
    from musicfpaugment_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from musicfpaugment_amd.csrc.build import build
        build(verbose=False)
    return _lib


def _varidelay(h, **kw):
    a = dict(x=P, x_f64=0, ldx=100, B=2, T=100, delay=P, row=300, voice=100, time=1, V=3, gains=P, dry=P, apply=None, filter_len=81, y=P,
             y_f64=0, stream=None)
    a.update(kw)
    return h.mfpa_varidelay(a["x"], a["x_f64"], a["ldx"], a["B"], a["T"], a["delay"], a["row"], a["voice"], a["time"], a["V"], a["gains"],
                            a["dry"], a["apply"], a["filter_len"], a["y"], a["y_f64"], a["stream"])


def _comb(h, **kw):
    a = dict(x=P, x_f64=0, ldx=100, B=2, T=100, params=P, per_row=0, max_delay=7, apply=None, y=P, y_f64=0, stream=None)
    a.update(kw)
    return h.mfpa_comb(a["x"], a["x_f64"], a["ldx"], a["B"], a["T"], a["params"], a["per_row"], a["max_delay"], a["apply"], a["y"],
                       a["y_f64"], a["stream"])


def test_symbols_header_constants_and_abi_version(lib):
    from musicfpaugment_amd import ops
    h = lib.lib()
    header = open(os.path.join(ROOT, "include", "mfpa.h")).read()
    declared = set(re.findall(r"^int\s+(mfpa_\w+)\s*\(", header, flags=re.M))
    for name, nargs in (("mfpa_varidelay", 17), ("mfpa_comb", 12)):
        assert name in lib.exported_symbols() and name in declared and hasattr(h, name)
        assert name in lib._SIGNATURES and len(lib._SIGNATURES[name][0]) == nargs
    assert int(re.search(r"#define MFPA_DELAY_MAX_VOICES (\d+)", header).group(1)) == ops.DELAY_MAX_VOICES == 8
    assert int(re.search(r"#define MFPA_VARIDELAY_TILE (\d+)", header).group(1)) == ops.VARIDELAY_TILE
    assert int(re.search(r"#define MFPA_VARIDELAY_WINDOW (\d+)", header).group(1)) == ops.VARIDELAY_WINDOW
    assert ops.VARIDELAY_TILE % 64 == 0 and ops.VARIDELAY_WINDOW >= ops.VARIDELAY_TILE + 256     # a tile of constant delay is always staged
    assert lib.ABI_VERSION == 47 and h.mfpa_version() == 47              # the new symbols are additive


@pytest.mark.parametrize("change", [dict(x=None), dict(y=None), dict(delay=None), dict(gains=None), dict(dry=None), dict(x=P + 2), dict(y=P + 2),
                                    dict(x=P + 4, x_f64=1), dict(y=P + 4, y_f64=1), dict(delay=P + 4), dict(gains=P + 4), dict(dry=P + 4),
                                    dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-5), dict(T=(1 << 30) + 1, ldx=1 << 31),
                                    dict(ldx=99), dict(filter_len=80), dict(filter_len=2), dict(filter_len=1), dict(filter_len=257),
                                    dict(filter_len=-81), dict(V=0), dict(V=9), dict(V=-1), dict(time=2), dict(time=-1), dict(time=100),
                                    dict(row=-1), dict(voice=-1), dict(x_f64=2), dict(y_f64=-1)], ids=str)
def test_varidelay_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _varidelay(lib.lib(), **change) == lib.EINVAL


@pytest.mark.parametrize("change", [dict(x=None), dict(y=None), dict(params=None), dict(x=P + 2), dict(y=P + 4, y_f64=1), dict(params=P + 4),
                                    dict(B=0), dict(B=-1), dict(B=65536), dict(T=0), dict(T=-1), dict(T=(1 << 30) + 1, ldx=1 << 31),
                                    dict(ldx=99), dict(max_delay=0), dict(max_delay=-3), dict(max_delay=(1 << 24) + 1), dict(per_row=2),
                                    dict(per_row=-1), dict(x_f64=2), dict(y_f64=2)], ids=str)
def test_comb_argument_errors_do_not_touch_the_gpu(lib, change):
    assert _comb(lib.lib(), **change) == lib.EINVAL


def test_python_refusals_need_no_gpu():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    x = torch.zeros(2, 100)
    d = torch.zeros(2, 3, 100, dtype=torch.float64)
    nan, inf = float("nan"), float("inf")
    for wav in (torch.zeros(100), torch.zeros(1, 2, 100), x.to(torch.float16), x.to(torch.int32), np.zeros((2, 100))):
        with pytest.raises(ValueError):
            ops.variable_delay(wav, d)
        with pytest.raises(ValueError):
            ops.comb(wav, 5, aD=0.5)
    for bad in (torch.zeros(3, 100, dtype=torch.float64), torch.zeros(2, 3, 50, dtype=torch.float64), torch.zeros(100, dtype=torch.float64),
                torch.zeros(2, 9, 100, dtype=torch.float64), torch.zeros(2, 0, 100, dtype=torch.float64), torch.zeros(2, 9, dtype=torch.float64),
                torch.zeros(2, 3, 100, 1, dtype=torch.float64), d.to(torch.float16), d.to(torch.int64)):
        with pytest.raises(ValueError):
            ops.variable_delay(x, bad)
    for kw in (dict(filter_len=80), dict(filter_len=1), dict(filter_len=257), dict(filter_len=81.5), dict(gains=nan), dict(gains=[1.0, inf, 1.0]),
               dict(gains=[1.0, 1.0]), dict(gains=np.ones((3, 3))), dict(dry=inf), dict(dry=[1.0, 1.0, 1.0]), dict(apply=torch.ones(3, dtype=torch.bool)),
               dict(out_dtype=torch.float16)):
        with pytest.raises(ValueError):
            ops.variable_delay(x, d, **kw)
    for kw in (dict(delay=0), dict(delay=-1), dict(delay=2.5), dict(delay=(1 << 24) + 1), dict(delay=nan), dict(delay=5, aD=1.0),
               dict(delay=5, aD=-1.0), dict(delay=5, aD=nan), dict(delay=5, b0=inf), dict(delay=5, bD=nan), dict(delay=[1, 2, 3]),
               dict(delay=[1, 2], aD=[0.1, 0.2, 0.3]), dict(delay=[[1, 2]]), dict(delay=5, apply=[True]), dict(delay=5, out_dtype=torch.int32)):
        with pytest.raises(ValueError):
            ops.comb(x, **kw)
    for kw in (dict(base_ms=nan, depth_ms=1.0, rate_hz=1.0), dict(base_ms=1.0, depth_ms=[1.0, 2.0, 3.0], rate_hz=1.0),
               dict(base_ms=1.0, depth_ms=1.0, rate_hz=inf)):
        with pytest.raises(ValueError):
            ops.lfo_delay(2, 100, 8000, **kw)
    with pytest.raises(ValueError):
        ops.lfo_delay(2, 100, 0, base_ms=1.0, depth_ms=1.0, rate_hz=1.0)
    for comps in ([(0.002, 0.8)], [(0.002, -0.8, 0.0)], [(nan, 0.8, 0.0)], [([0.1, 0.2, 0.3], 0.8, 0.0)]):
        with pytest.raises(ValueError):
            ops.speed_drift_delay(2, 100, 8000, comps)
    calls = [lambda: F.echo(x, 8000, [10.0, 20.0], [0.5]), lambda: F.echo(x, 8000, [10.0] * 9, [0.5] * 9), lambda: F.echo(x, 8000, [], []),
             lambda: F.echo(x, 8000, [-1.0], [0.5]), lambda: F.echo(x, 8000, [10.0], [nan]), lambda: F.echo(x, 0, [10.0], [0.5]),
             lambda: F.echo(x.to(torch.float16), 8000, [10.0], [0.5]), lambda: F.echo(x, 8000, [10.0], [0.5], gain_in=inf),
             lambda: F.feedback_echo(x, 8000, 10.0, 1.0), lambda: F.feedback_echo(x, 8000, -10.0, 0.5), lambda: F.feedback_echo(x, 8000, 10.0, nan),
             lambda: F.comb(x, 8000, 10.0, aD=-1.5), lambda: F.comb(x, 8000, 1e9), lambda: F.comb(x, 8000, 10.0, b0=[1.0, 2.0]),
             lambda: F.allpass_comb(x, 8000, 10.0, 1.0), lambda: F.allpass_comb(x.to(torch.int16), 8000, 10.0, 0.5),
             lambda: F.vibrato(x, 8000, rate_hz=-1.0), lambda: F.vibrato(x, 8000, depth_ms=nan), lambda: F.chorus(x, 8000, voices=0),
             lambda: F.chorus(x, 8000, voices=9), lambda: F.chorus(x, 8000, voices=2.5), lambda: F.chorus(x, 8000, base_ms=1.0, depth_ms=2.0),
             lambda: F.flanger(x, 8000, base_ms=-1.0), lambda: F.flanger(x, 8000, mix=inf), lambda: F.wow_flutter(x, 8000, wow_hz=-1.0),
             lambda: F.wow_flutter(x, 8000, wow_depth=0.7, flutter_depth=0.4), lambda: F.wow_flutter(x, 8000, phase=(0.0,)),
             lambda: F.wow_flutter(x, -8000)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"call {i} did not raise")
    assert F.comb_delay_samples(8000, 10.0) == 80 and F.comb_delay_samples(8000, 0.0) == 1 and F.comb_delay_samples(44100, 1.0) == 44
    assert np.allclose(F.chorus_phases(4), [0.0, np.pi / 2, np.pi, 3 * np.pi / 2])
    assert np.array_equal(ops.comb_params(5, 1.0, 0.0, 0.5), [5.0, 1.0, 0.0, 0.5]) and ops.comb_params([1, 2], aD=[0.1, 0.2]).shape == (2, 4)


def test_no_cpu_fallback():
    from musicfpaugment_amd import functional as F
    from musicfpaugment_amd import ops
    from musicfpaugment_amd._lib import MfpaError
    from musicfpaugment_amd.augmentation.transformations.delay_effects import Chorus, Echo, WowFlutter
    x = torch.zeros(2, 100)
    for d in (torch.zeros(2, 100, dtype=torch.float64), torch.zeros(2, 3, 100), torch.zeros(2, 3, 1, dtype=torch.float64), np.zeros((2, 8))):
        with pytest.raises(MfpaError):
            ops.variable_delay(x, d, dry=[0.5, 0.25], filter_len=33, apply=[True, False], out_dtype=torch.float64)
    with pytest.raises(MfpaError):
        ops.comb(x.double(), [5, 7], 1.0, [0.0, 0.5], 0.5, apply=[True, False], out_dtype=torch.float32)
    for t in (Echo(p=1.0, sample_rate=8000), Echo(feedback=True, p=1.0, sample_rate=8000), WowFlutter(p=1.0, sample_rate=8000),
              Chorus(p=1.0, sample_rate=8000)):
        with pytest.raises(MfpaError):
            t(torch.zeros(2, 1, 8000))
    if not torch.cuda.is_available():
        with pytest.raises(MfpaError):
            ops.lfo_delay(2, 100, 8000, base_ms=1.0, depth_ms=1.0, rate_hz=[1.0, 2.0])
        with pytest.raises(MfpaError):
            ops.speed_drift_delay(2, 100, 8000, [(0.002, 0.8, 0.0), ([0.001, 0.002], 8.0, 0.0)])
        x3 = torch.zeros(3, 1, 100)
        for call in (lambda: F.echo(x3, 8000, [10.0, 20.5], [0.5, 0.25]), lambda: F.feedback_echo(x3, 8000, 5.0, 0.5, mix=0.5),
                     lambda: F.comb(x3, 8000, 5.0, 0.5, 0.5, 0.0), lambda: F.allpass_comb(x3[0, 0], 8000, 5.0, 0.7), lambda: F.vibrato(x3, 8000),
                     lambda: F.chorus(x3, 8000), lambda: F.flanger(x3.double(), 8000), lambda: F.wow_flutter(x3, 8000)):
            with pytest.raises(MfpaError):
                call()


def test_transforms_construct_name_their_parameters_and_compose():
    from musicfpaugment_amd.augmentation.composition import Compose, OneOf, SomeOf
    from musicfpaugment_amd.augmentation.transformations.delay_effects import Chorus, Echo, WowFlutter
    e, w, c = Echo(), WowFlutter(), Chorus()
    assert (e.min_delay_ms, e.max_delay_ms, e.min_decay, e.max_decay, e.feedback, e.p) == (50.0, 400.0, 0.2, 0.6, False, 0.5)
    assert (w.min_wow_hz, w.max_wow_hz, w.min_wow_depth, w.max_wow_depth) == (0.3, 2.0, 0.0005, 0.004)
    assert (w.min_flutter_hz, w.max_flutter_hz, w.min_flutter_depth, w.max_flutter_depth) == (5.0, 12.0, 0.0002, 0.0015)
    assert (c.min_voices, c.max_voices, c.min_depth_ms, c.max_depth_ms, c.min_rate_hz, c.max_rate_hz, c.mix) == (2, 4, 1.0, 4.0, 0.3, 2.0, 0.5)
    x = torch.zeros(6, 2000)
    for t, names in ((e, ["decay", "delay_ms"]), (w, ["flutter_depth", "flutter_hz", "flutter_phase", "wow_depth", "wow_hz", "wow_phase"]),
                     (c, ["depth_ms", "rate_hz", "voices"])):
        torch.manual_seed(5)
        t.transform_parameters = {"should_apply": torch.tensor([True, False, True, True, False, True])}
        t.randomize_parameters(x, 8000)                                   # the draws are host work
        assert sorted(k for k in t.transform_parameters if k != "should_apply") == names
        assert all(len(v) == 4 for k, v in t.transform_parameters.items() if k != "should_apply")
    assert e.delay_samples(8000).shape == (6,) and np.all(e.delay_samples(8000) >= 400.0) and np.all(e.delay_samples(8000) <= 3200.0)
    e2 = Echo(feedback=True)
    e2.transform_parameters = {"should_apply": torch.ones(6, dtype=torch.bool)}
    e2.randomize_parameters(x, 8000)
    assert np.array_equal(e2.delay_samples(8000), np.rint(e2.delay_samples(8000)))
    g = c.voice_gains()
    assert g.shape == (6, 4) and np.allclose(g.sum(1), 0.5) and np.array_equal((g > 0).sum(1), c.voices.numpy())
    assert torch.all((c.voices >= 2) & (c.voices <= 4))
    for bad in (dict(min_delay_ms=-1.0), dict(min_delay_ms=500.0), dict(min_decay=-0.1), dict(max_decay=1.0), dict(min_decay=0.7)):
        with pytest.raises(ValueError):
            Echo(**bad)
    for bad in (dict(min_wow_hz=-1.0), dict(min_wow_hz=3.0), dict(min_flutter_depth=0.01), dict(max_wow_depth=0.9, max_flutter_depth=0.2)):
        with pytest.raises(ValueError):
            WowFlutter(**bad)
    for bad in (dict(min_voices=0), dict(max_voices=9), dict(min_voices=5), dict(min_voices=2.5), dict(min_depth_ms=-1.0), dict(mix=1.5),
                dict(max_depth_ms=30.0), dict(min_rate_hz=3.0)):
        with pytest.raises(ValueError):
            Chorus(**bad)
    chain = Compose([Echo(p=1.0), SomeOf((1, 2), [WowFlutter(p=1.0), Chorus(p=1.0)]), OneOf([Echo(feedback=True), Chorus()])])
    assert len(chain.transforms) == 3
