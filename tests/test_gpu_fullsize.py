"""GPU parity at BASELINE.json's FULL sizes (configs[1]: 256 clips STFT + peak-pick, configs[2]: 512 clips UNet forward,
configs[3]: the 64-clip train step), where the oracle cannot run the whole batch in seconds: a sampled subset goes through
the oracle, the rest is covered by size-independent properties -- determinism, invariance to batch composition / order /
sub-batching, the per-frame peak bound, and a digest over the whole batch."""
import hashlib

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from musicfpaugment_amd.training.weights import formula_state_dict

pytestmark = pytest.mark.gpu


def _digest(t: torch.Tensor) -> str:
    return hashlib.sha1(t.contiguous().cpu().numpy().tobytes()).hexdigest()


@pytest.fixture(scope="module")
def net():
    from musicfpaugment_amd.training.unet import UNet
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(formula_state_dict(0))
    return m.cuda().eval()


def test_config1_stft_peakpick_256_clips_bit_exact_and_batch_invariant():
    from musicfpaugment_amd.pipeline import HotPath
    from oracle import audfprint as oa
    B = 256
    wav = np.stack([synth.clip(3000 + i, tonal=(i % 3 != 0)) for i in range(B)])
    wav[17] = 0.0                                                      # a silent clip inside the batch
    wav[200, :32000] = 0.0                                             # half-silent
    x = torch.from_numpy(wav).cuda()
    hp = HotPath(None)
    mask, npk = hp(x)
    assert mask.shape == (B, 256, 251) and mask.dtype == torch.uint8
    # sampled clips through the oracle: bit-exact index sets
    for i in (0, 17, 100, 200, 255):
        want = oa.find_peaks(wav[i])[1]
        np.testing.assert_array_equal(mask[i].cpu().numpy(), np.asarray(want).reshape(256, 251).astype(np.uint8) if np.size(want) else 0)
    assert int(npk[17]) == 0 and not mask[17].any()                    # find_peaks of silence: no peaks (peak_extractor.py:262)
    np.testing.assert_array_equal(npk.cpu().numpy(), mask.reshape(B, -1).sum(dim=1).cpu().numpy())
    assert int(mask.sum(dim=1).max()) <= 2 * 5                         # <= maxpksperframe per column and pruning direction
    # determinism and invariance to order / sub-batching (clips are independent units)
    mask2, _ = hp(x)
    assert _digest(mask2) == _digest(mask)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(0)).cuda()
    maskp, _ = hp(x[perm].contiguous())
    assert torch.equal(maskp, mask[perm])
    parts = torch.cat([hp(x[s:s + 37].contiguous())[0] for s in range(0, B, 37)])      # ragged shards
    assert torch.equal(parts, mask)


def test_config1_consecutive_batches_on_two_streams_equal_the_serial_path():
    """HotPath(streams=2): batch k + 1's STFT runs beside batch k's pruner (bench.py --batch-streams; configs.
    config2_stft_peakpick_audfprint_2streams).  Six DIFFERENT batches produced on the caller's stream right before each call (the side
    streams must wait for them), results read behind join(): identical to the serial path's, with the allocator free to recycle."""
    from musicfpaugment_amd.pipeline import HotPath
    B = 256
    base = torch.from_numpy(np.stack([synth.clip(5000 + i, tonal=(i % 4 != 0)) for i in range(B)])).cuda()
    gains = [1.0, 0.5, -1.0, 0.25, 0.75, -0.3]                           # (a gain alone leaves a clip's mask as it is: the roll is what differs)
    batch = lambda k: torch.roll(base, 37 * k, dims=0) * gains[k]
    serial = HotPath(None)
    want = []
    for k in range(len(gains)):
        m, n = serial(batch(k))
        want.append((m.clone(), n.clone()))
    torch.cuda.synchronize()
    assert len({_digest(m) for m, _ in want}) > 1                        # the batches do differ
    for streams in (2, 3):
        hp = HotPath(None, streams=streams)
        got = []
        for k in range(len(gains)):
            x = batch(k)                                               # queued on the current stream; freed (for the allocator) right after the call
            got.append(hp(x))
            del x
        hp.join()
        for (m, n), (wm, wn) in zip(got, want):
            assert torch.equal(m, wm) and torch.equal(n, wn)
    with pytest.raises(ValueError):
        HotPath(None, streams=0)


def test_config2_unet_forward_512_clips_within_tolerance_and_batch_invariant(net):
    from oracle import stft as ostft
    from oracle import unet as ou
    B = 512
    wav = np.stack([synth.clip(4000 + i, tonal=(i % 2 == 0)) for i in range(B)])
    from musicfpaugment_amd import ops
    mag, cmax = ops.stft_mag(torch.from_numpy(wav).cuda(), torch.float64)
    sd = formula_state_dict(0)
    picks = [0, 63, 64, 127, 255, 256, 383, 511]                         # both ends of several 64-clip passes
    x = torch.from_numpy(np.stack([ostft.spectrogram(wav[i:i + 1])[0] for i in picks])).float().unsqueeze(1)
    with torch.no_grad():
        torch.set_num_threads(8)
        want = torch.cat([ou.forward(x[i:i + 2], sd) for i in range(0, len(picks), 2)])
    for prec, tol in ((0, 1e-5), (1, 1e-4)):                            # fp32 MFMA, bf16x3 (the bench default)
        net.precision = prec
        out = net.denoise_spectrogram(mag, cmax, per_clip=True)        # (512, 257, 251) float32
        assert out.shape == (B, 257, 251) and torch.isfinite(out).all()
        got = out[picks].cpu().unsqueeze(1)
        assert ou.relative_l1(got, want) <= tol, (prec, ou.relative_l1(got, want))
        # the same clips in a different batch composition: bit-identical (no cross-clip arithmetic, no atomics)
        sub = net.denoise_spectrogram(mag[picks].contiguous(), cmax[picks].contiguous(), per_clip=True)
        assert torch.equal(sub, out[picks])
        assert _digest(net.denoise_spectrogram(mag, cmax, per_clip=True)) == _digest(out)
    net.precision = 0


def test_config3_train_step_64_clips_precisions_agree_and_loss_falls():
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    B = 64
    clean = synth.batch(B, seed=5000, n=24000)                         # the reference's 3 s training windows
    aug = (0.7 * clean + 0.3 * synth.batch(B, seed=6000, n=24000, tonal=False)).astype(np.float32)
    cm, cmax = ops.stft_mag(torch.from_numpy(clean).cuda(), torch.float64)
    am, amax = ops.stft_mag(torch.from_numpy(aug).cuda(), torch.float64)
    target = ops.normalize_(cm, cmax.max().expand(B).contiguous(), per_clip=True)
    den = amax.max().expand(B).contiguous()
    losses = {}
    for prec in (0, 1):
        torch.manual_seed(0)
        net = UNet(1, 1, rate=0.05)
        net.load_state_dict(formula_state_dict(0))
        eng = UNetTrainEngine(net.cuda().train(), lr=1e-3, precision=prec)
        losses[prec] = [float(eng.train_step(am, den, target)) for _ in range(4)]
        assert all(np.isfinite(losses[prec])) and losses[prec][-1] < losses[prec][0]
    # the first step sees identical weights and dropout masks: the two arithmetic paths give the same loss to 1e-4
    assert abs(losses[0][0] - losses[1][0]) <= 1e-4 * abs(losses[0][0]), losses
    assert abs(losses[0][-1] - losses[1][-1]) <= 2e-2 * abs(losses[0][-1]), losses


def test_config4_train_step_64_clips_of_8_seconds():
    """BASELINE configs[3] at the size bench.py --mode train runs: 64 clips x 8 s (257 x 251 spectrograms), Dropout 0.05.  The exact-fp32
    and the bf16x3 engines see identical weights and dropout masks in step 1: same loss to 1e-4; the loss falls under both."""
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    B = 64
    base = synth.batch(16, seed=5100)
    noise = synth.batch(16, seed=6100, tonal=False)
    clean = np.concatenate([base * g for g in (1.0, 0.8, 0.6, 0.4)]).astype(np.float32)
    aug = np.concatenate([(0.7 * base + 0.3 * noise) * g for g in (1.0, 0.8, 0.6, 0.4)]).astype(np.float32)
    cm, cmax = ops.stft_mag(torch.from_numpy(clean).cuda(), torch.float64)
    am, amax = ops.stft_mag(torch.from_numpy(aug).cuda(), torch.float64)
    assert tuple(cm.shape) == (B, 257, 251)
    target = ops.normalize_(cm, cmax.max().expand(B).contiguous(), per_clip=True)
    den = amax.max().expand(B).contiguous()
    losses = {}
    for prec in (0, 1):
        net = UNet(1, 1, rate=0.05)
        net.load_state_dict(formula_state_dict(0))
        eng = UNetTrainEngine(net.cuda().train(), lr=1e-3, precision=prec, wgrad_precision=2 if prec else 0)   # bench.py's arithmetic
        losses[prec] = [float(eng.train_step(am, den, target)) for _ in range(3)]
        assert all(np.isfinite(losses[prec])) and losses[prec][-1] < losses[prec][0], losses
        del eng, net
        torch.cuda.empty_cache()
    assert abs(losses[0][0] - losses[1][0]) <= 1e-4 * abs(losses[0][0]), losses
    assert abs(losses[0][-1] - losses[1][-1]) <= 3e-2 * abs(losses[0][-1]), losses


def test_config4_train_step_with_the_augmentation_chain_inside_replayed_on_the_oracle():
    """BASELINE configs[3] "AugmentFP synthetic noise ... + L1 loss": what bench.py --mode train --augment does in a step --
    AugmentFP.batch_augment on the device, two spectrograms with their batch-global maxima, UNet train-mode forward, L1 -- against the
    same step on the CPU oracle with the augmentation DRAWS of that call replayed stage by stage (oracle/augment.py), the
    spectrograms of oracle/stft.py and torch autograd through oracle/unet.py (Dropout off: its Philox stream cannot be replayed)."""
    import random
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    from musicfpaugment_amd.augmentation.constants import DEFAULT_PARAMETERS
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    from oracle import augment as oau
    from oracle import stft as ostft
    from oracle import unet as ou
    irs, noises = synthetic_banks(2, noise_seconds=2.0)
    torch.manual_seed(11)
    random.seed(11)
    par = dict(DEFAULT_PARAMETERS)
    for k in par:
        if k.startswith("proba"):
            par[k] = 0.6
    af = AugmentFP(None, 8000, parameters=par, ir_bank=irs, noise_bank=noises, device="cuda")
    B, T = 4, 8000
    clean_np = synth.batch(B, seed=7300, n=T)
    clean = torch.from_numpy(clean_np).cuda()
    # ---- the device step (bench.py bench_train.step)
    aug = af.batch_augment(clean[:, None, :])[:, 0].contiguous()
    cm, cmax = ops.stft_mag(clean, torch.float64)
    am, amax = ops.stft_mag(aug, torch.float64)
    target = ops.normalize_(cm, cmax.max().expand(B).contiguous(), per_clip=True)
    net = UNet(1, 1, rate=0.0)
    sd = formula_state_dict(4)
    net.load_state_dict(sd)
    eng = UNetTrainEngine(net.cuda().train(), lr=1e-3, precision=0)
    loss = float(eng.train_step(am, amax.max().expand(B).contiguous(), target))
    grads = {k: v.detach().cpu().double() for k, v in eng.named_grads().items()}
    # ---- replay of the draws on the oracle
    tr = af.augmentation_pipeline.transforms
    gates = [t.transform_parameters["should_apply"] for t in tr]

    def gated(x, gate, fn):
        y = x.clone()
        for b in range(B):
            if gate[b]:
                y[b:b + 1] = fn(x[b:b + 1], b)
        return y

    x = torch.from_numpy(clean_np)[:, None, :].clone()
    x = gated(x, gates[0], lambda v, b: oau.highpass(v[:, 0], float(tr[0].draws["cutoff_freq"][b]) / 8000)[:, None])
    x = gated(x, gates[1], lambda v, b: oau.apply_ir(v, tr[1].draws["ir"][b][None, None, :]))
    bg = torch.stack([oau.rms_normalize(torch.cat([oau.rms_normalize(noises[sc][k][o:o + n]) for sc, k, o, n in pc]))
                      for pc in tr[2].draws["pieces"]])
    x = gated(x, gates[2], lambda v, b: oau.add_background(v, bg[b:b + 1], tr[2].draws["snr_in_db"][b:b + 1]))
    x = gated(x, gates[3], lambda v, b: oau.gain(v, tr[3].draws["gain_in_db"][b:b + 1]))
    x = gated(x, gates[4], lambda v, b: oau.clipping(v, tr[4].draws["percentile_threshold"][b:b + 1]))
    x = gated(x, gates[5], lambda v, b: oau.lowpass(v[:, 0], float(tr[5].draws["cutoff_freq"][b]) / 8000)[:, None])
    x = gated(x, gates[6], lambda v, b: oau.highpass(v[:, 0], float(tr[6].draws["cutoff_freq"][b]) / 8000)[:, None])
    x = oau.peak_normalize(x)[:, 0]
    np.testing.assert_allclose(aug.cpu().numpy(), x.numpy(), rtol=0, atol=5e-5)
    clean_spec = torch.from_numpy(ostft.spectrogram(clean_np))                      # float64, one max over the batch
    params = {k: (v.clone().double().requires_grad_(True) if v.dtype.is_floating_point and "running" not in k else v.clone())
              for k, v in sd.items()}
    # (i) the whole chain on the oracle: its own replayed waveform (within 5e-5 of the device's) through STFT, UNet, L1
    with torch.no_grad():
        aug_spec_o = torch.from_numpy(ostft.spectrogram(x.numpy().astype(np.float32)))
        loss_chain = torch.mean(torch.abs(ou.forward(aug_spec_o.float().double()[:, None], params, training=True).squeeze(1) - clean_spec))
    assert abs(loss - float(loss_chain)) <= 2e-3 * float(loss_chain), (loss, float(loss_chain))
    # (ii) from the device's augmented waveform on: the step itself, tightly, with autograd for the gradients
    aug_spec = torch.from_numpy(ostft.spectrogram(aug.cpu().numpy()))
    pred = ou.forward(aug_spec.float().double()[:, None], params, training=True).squeeze(1)
    loss_ref = torch.mean(torch.abs(pred - clean_spec))
    loss_ref.backward()
    assert abs(loss - float(loss_ref)) <= 2e-5 * float(loss_ref), (loss, float(loss_ref))
    # the gradients of the big blocks agree with float64 autograd at the level fp32 arithmetic allows through 18 BatchNorms
    for k in ("outc.conv.weight", "up4.conv.double_conv.3.weight", "down4.maxpool_conv.1.double_conv.0.weight", "inc.double_conv.0.weight"):
        g_ref = params[k].grad
        rel = float((grads[k] - g_ref).abs().sum() / g_ref.abs().sum())
        assert rel < 5e-2, (k, rel)


def test_config5_demucs_forward_256_clips_within_tolerance_and_batch_invariant():
    """BASELINE configs[4]: the Demucs waveform denoiser at 256 clips of 8 s.  Eight sampled clips go through the oracle; the rest is
    covered by determinism and by invariance to the batch composition -- a 37-clip shard runs other kernel shapes (32-clip LSTM
    tiles, the two layers pipelined on two streams), so that comparison is to rounding, not bit for bit."""
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
    from musicfpaugment_amd.training.model import Demucs
    from oracle import demucs as od
    from oracle.unet import relative_l1
    B = 256
    wav = np.stack([synth.clip(5000 + i, tonal=(i % 4 != 0)) for i in range(B)])
    wav[31] = 0.0                                                      # a silent clip: std 0, output exactly 0
    x = torch.from_numpy(wav).cuda()
    net = Demucs()
    sd = demucs_formula(0)
    net.load_state_dict(sd)
    net = net.cuda().eval()
    y = net(x)
    assert y.shape == (B, 1, 64000) and bool(torch.isfinite(y).all())
    assert float(y[31].abs().max()) == 0.0
    torch.set_num_threads(8)
    for i in (0, 30, 31, 32, 100, 128, 200, 255):                      # eight clips through the oracle (31: the silent one)
        with torch.no_grad():
            want = od.forward(torch.from_numpy(wav[i:i + 1]), sd)
        if i == 31:
            assert float(want.abs().max()) == 0.0
            continue
        assert relative_l1(y[i:i + 1].cpu(), want) <= 1e-4, i
    assert _digest(net(x)) == _digest(y)                               # no atomics on the forward path: bit-reproducible
    idx = list(range(100, 137))
    ys = net(x[idx].contiguous())
    assert relative_l1(ys.cpu(), y[idx].cpu()) <= 1e-5
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(net(x[perm].contiguous()), y[perm])             # same batch size, other order: the same kernels, bit for bit


def test_demucs_train_step_64_clips_precisions_agree_and_loss_falls():
    """The Demucs training step at the bench shape (64 clips of 8 s): the first step's loss terms agree between exact-fp32 and
    bf16x3 products, the loss falls over a few steps, and the parameters stay finite."""
    from musicfpaugment_amd.ops_demucs_train import DemucsTrainEngine
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
    B = 64
    base = synth.batch(16, seed=6000)
    noise = synth.batch(16, seed=6100, tonal=False)
    clean = torch.from_numpy(np.concatenate([base] * 4)[:B].copy()).cuda()
    aug = torch.from_numpy(np.concatenate([(0.7 * base + 0.3 * noise).astype(np.float32)] * 4)[:B].copy()).cuda()
    first = {}
    for prec in (0, 1):
        eng = DemucsTrainEngine(demucs_formula(0), "cuda", lr=3e-4, precision=prec)
        losses = [float(eng.train_step(clean, aug)) for _ in range(4 if prec else 1)]
        first[prec] = [float(v) for v in eng.last_losses] if not prec else None
        if prec:
            assert all(np.isfinite(losses)) and losses[-1] < losses[0]
            assert bool(torch.isfinite(eng.flat_p).all())
            eng2 = DemucsTrainEngine(demucs_formula(0), "cuda", lr=3e-4, precision=1)
            eng2.train_step(clean, aug)
            np.testing.assert_allclose([float(v) for v in eng2.last_losses], first[0], rtol=2e-4)


def test_demucs_train_step_lstm_schedules_agree():
    """One backward pass at the bench shape with both schedules of the two LSTM layers: persistent launches (the default) and the
    per-step kernels -- the same gradients to rounding (248 steps)."""
    from musicfpaugment_amd import ops_demucs as D
    from musicfpaugment_amd.ops_demucs_train import DemucsTrainEngine
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
    B = 64
    base = synth.batch(16, seed=6200)
    noise = synth.batch(16, seed=6300, tonal=False)
    clean = torch.from_numpy(np.concatenate([base] * 4)[:B].copy()).cuda()
    aug = torch.from_numpy(np.concatenate([(0.7 * base + 0.3 * noise).astype(np.float32)] * 4)[:B].copy()).cuda()
    old = (D.PERSISTENT_LSTM, D.PERSISTENT_LSTM_BWD)
    grads = {}
    try:
        for name, flags in [("default", old), ("per-step", (False, False))]:
            D.PERSISTENT_LSTM, D.PERSISTENT_LSTM_BWD = flags
            eng = DemucsTrainEngine(demucs_formula(0), "cuda", precision=1)
            pred = eng.forward(aug)
            _, _, _, dpred = eng.loss_and_grad(pred, clean)
            eng.backward(dpred)
            torch.cuda.synchronize()
            grads[name] = eng.flat_g.clone()
    finally:
        D.PERSISTENT_LSTM, D.PERSISTENT_LSTM_BWD = old
    assert not D.lstm_seq_error()
    ref = grads["per-step"]
    rel = float((grads["default"] - ref).abs().sum() / ref.abs().sum())
    assert rel < 2e-4, ("default", rel)


def test_config1_dejavu_picker_256_clips_bit_exact_and_batch_invariant(net):
    """configs[1] with the second picker: mlab.specgram PSD -> /max -> 10 ln -> -mean -> 21x21 local
    maxima on 256 clips; sampled clips through the oracle, the rest through batch-composition properties.  Then the denoised
    branch (UNet on the normalised PSD, squared, float32 log / mean) on 64 of them: the picker is checked against numpy on
    the device's own network output, and sub-batching must not change a bit."""
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.afp.dejavu.fingerprint import fingerprint_peaks_batch
    from oracle import dejavu as od
    B = 256
    wav = np.stack([synth.clip(5000 + i, tonal=(i % 4 != 0)) for i in range(B)])
    wav[9, 40000:] = 0.0                                               # half-silent: exact-zero PSD background (erosion term)
    x = torch.from_numpy(wav).cuda()
    mask, npk, spec = fingerprint_peaks_batch(x)
    assert mask.shape == (B, 257, 249) and spec.dtype == torch.float64
    for i in (0, 9, 101, 255):
        coords, want, want_spec = od.fingerprint_peaks(wav[i].astype(np.float64) * 32767.0)
        np.testing.assert_array_equal(mask[i].cpu().numpy(), want.astype(np.uint8))
        assert int(npk[i]) == len(coords)
        np.testing.assert_allclose(spec[i].cpu().numpy(), want_spec, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(npk.cpu().numpy(), mask.reshape(B, -1).sum(dim=1).cpu().numpy())
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).cuda()
    assert torch.equal(fingerprint_peaks_batch(x[perm].contiguous())[0], mask[perm])
    parts = torch.cat([fingerprint_peaks_batch(x[s:s + 53].contiguous())[0] for s in range(0, B, 53)])
    assert torch.equal(parts, mask)
    # denoised branch, 64 clips, low threshold so that the formula-weight network leaves peaks to compare
    xd = x[:64].contiguous()
    net.precision = 1
    mask_d, npk_d, spec_d = fingerprint_peaks_batch(xd, amp_min=5, denoising=True, denoising_model="unet", unet=net)
    assert spec_d.dtype == torch.float32 and int(npk_d.min()) > 0
    y = net.denoise_spectrogram(*ops.specgram_psd(xd, scale_in=32767.0), per_clip=True)
    assert torch.equal(spec_d, y * y)
    for i in (0, 9, 63):
        _, want = od.get_2d_peaks(od.preprocess_denoised(y[i].cpu().numpy())[0], 5)
        np.testing.assert_array_equal(mask_d[i].cpu().numpy(), want.astype(np.uint8))
    saved_pass = net.max_clips_per_pass
    try:
        net.max_clips_per_pass = 16
        mask_s, _, _ = fingerprint_peaks_batch(xd, amp_min=5, denoising=True, denoising_model="unet", unet=net)
    finally:
        net.max_clips_per_pass = saved_pass                            # the module-scoped fixture goes on at the class default
        net.precision = 0
    assert torch.equal(mask_s, mask_d)


def _masks_vs_oracle_both_logs(spec_np, mask_np, tag, max_clips=2, max_cells=4):
    """Device masks of a batch against the oracle picker on the device's own float32 spectrograms -- twice: with the
    float64 log rounded once to float32 (what the device computes: every clip must agree, same values in -> same peaks out) and with numpy's
    own SIMD float32 log (the reference's arithmetic to the last bit, not correctly rounded: agreement is statistical, a near-tie may fall the
    other way -- counted, printed, bounded: the 2 000-query run measures 0-1 such clips per 2 000, i.e. a 256-clip batch shows one in about one
    run of eight; the "trained" family's weights come out of float-atomic weight gradients and differ in the last bits from run to run, so the bound
    leaves room for two)."""
    from concurrent.futures import ThreadPoolExecutor
    from oracle import audfprint as oa
    with ThreadPoolExecutor(8) as ex:
        both = list(ex.map(oa.masks_both_logs, list(spec_np)))
    bad_rounded = [i for i in range(len(both)) if not np.array_equal(both[i][1] != 0, mask_np[i] != 0)]
    cells = [int(np.count_nonzero((both[i][0] != 0) != (mask_np[i] != 0))) for i in range(len(both))]
    bad_numpy = [i for i, c in enumerate(cells) if c]
    print(f"[{tag}] masks vs the oracle picker on the device's spectrogram: {len(bad_rounded)} of {len(both)} clips differ with the correctly rounded "
          f"float32 log, {len(bad_numpy)} ({sum(cells)} cells) with numpy's own float32 log")
    assert not bad_rounded, (tag, bad_rounded)
    assert len(bad_numpy) <= max_clips and sum(cells) <= max_cells, (tag, bad_numpy, cells)


def test_headline_chain_256_clips_end_to_end_as_benched(net):
    """The headline workload exactly as bench.py times it -- HotPath(net): STFT -> UNet eval forward -> Audfprint peak-pick on
    256 clips of 8 s built the way bench_infer builds them -- in BOTH arithmetic variants (bf16x3: the headline; fp32: the figure
    with the reference's own arithmetic), compared with the oracle end to end (afp/audfprint/peak_extractor.py:236-311):
      (i)   EVERY clip's peak mask == the oracle picker's on the device's denoised spectrogram (bit-exact index sets; identical spectrogram
            in -> identical peak set out, BASELINE.json north_star) with the correctly rounded float32 log the device computes; against numpy's
            own float32 log (the reference's, not correctly rounded) a near-tie may fall the other way: counted and bounded (<= 2 clips, <= 4 cells of 256 clips);
      (ii)  the denoised spectrogram of sampled clips vs oracle STFT -> oracle UNet: relative L1 <= 1e-4 (bf16x3) / 1e-5 (fp32);
      (iii) the masks-only path bench.py runs (want_spec=False) == the path that also returns the spectrogram; determinism; a
            ragged 37-clip sharding of the batch gives the same bits;
      (iv)  the UNet pass size is the one bench.py times (the class default of training/unet.UNet.max_clips_per_pass: bench.py only
            overrides it under --unet-pass), and 64-clip passes give the same bits as that default."""
    from concurrent.futures import ThreadPoolExecutor
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.pipeline import HotPath
    from oracle import audfprint as oa
    from oracle import stft as ostft
    from oracle import unet as ou
    B = 256
    base = synth.batch(32, seed=synth.BASE_SEED)                       # bench_infer's batch: 32 generated clips x 8 gains
    gains = (1.0 - 0.5 * np.arange(8) / 8).astype(np.float32)
    wav_np = np.ascontiguousarray(np.concatenate([base * g for g in gains])[:B])
    wav = torch.from_numpy(wav_np).cuda()
    sd = formula_state_dict(0)
    picks = [0, 100, 255]
    with torch.no_grad():
        torch.set_num_threads(8)
        sg = np.stack([ostft.magnitude(wav_np[i]) for i in picks])
        sg = sg / sg.max(axis=(1, 2), keepdims=True)                   # find_peaks normalises per clip (peak_extractor.py:258)
        want_den = ou.forward(torch.from_numpy(sg).float()[:, None], sd)[:, 0]
    from musicfpaugment_amd.training.unet import UNet
    import bench
    benched_pass = UNet(1, 1).max_clips_per_pass                       # what a fresh module -- bench_infer's -- runs with
    assert bench.build_parser().get_default("unet_pass") == 0          # ... and bench.py leaves it alone by default
    assert net.max_clips_per_pass == benched_pass, "an earlier test left the shared module at another pass size"
    try:
        for prec, tol in ((1, 1e-4), (0, 1e-5)):
            net.precision = prec
            hot = HotPath(net)
            mask, npk = hot(wav)                                       # what bench.py times
            if benched_pass != 64:                                     # (iv) the other pass size: same bits
                try:
                    net.max_clips_per_pass = 64
                    mask64, npk64 = hot(wav)
                finally:
                    net.max_clips_per_pass = benched_pass
                assert torch.equal(mask64, mask) and torch.equal(npk64, npk), prec
            assert mask.shape == (B, 256, 251) and mask.dtype == torch.uint8 and int(npk.min()) > 0
            ext = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net, device="cuda")
            mask_s, npk_s, spec = ext.find_peaks_batch(wav)            # the same chain, also returning the denoised spectrogram
            assert torch.equal(mask_s, mask) and torch.equal(npk_s, npk)
            assert spec.dtype == torch.float32 and spec.shape[0] == B
            # (ii) the network output of sampled clips against the oracle chain
            rl1 = ou.relative_l1(spec[picks].cpu(), want_den)
            assert rl1 <= tol, (prec, rl1)
            # (i) all 256 clips through the oracle pruner on the device's spectrogram
            spec_np, mask_np = spec.cpu().numpy(), mask.cpu().numpy()
            _masks_vs_oracle_both_logs(spec_np, mask_np, f"headline, precision {prec}")
            np.testing.assert_array_equal(npk.cpu().numpy(), mask_np.reshape(B, -1).sum(axis=1))
            # (iii) determinism and ragged shards (clips are independent units; 37 does not divide the 64-clip UNet pass)
            assert _digest(hot(wav)[0]) == _digest(mask)
            parts = torch.cat([hot(wav[s:s + 37].contiguous())[0] for s in range(0, B, 37)])
            assert torch.equal(parts, mask), prec
    finally:
        net.precision = 0


@pytest.mark.parametrize("family", ["bn_spread", "heavy_tail", "trained"])
def test_headline_chain_256_clips_on_stressed_and_trained_weight_families(family, trained_sd):
    """The headline chain at bench size in the headline arithmetic (bf16x3) with weights that are not the benign formula family
    (training/weights.py:stress_state_dict, conftest.trained_sd): every clip's mask must still equal the oracle pruner's on the
    device's denoised spectrogram (bit-exact), and the UNet output of sampled clips must stay inside the 1e-4 gate against the
    oracle's fp32 chain (the margin is printed)."""
    from concurrent.futures import ThreadPoolExecutor
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.pipeline import HotPath
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import stress_state_dict
    from oracle import audfprint as oa
    from oracle import stft as ostft
    from oracle import unet as ou
    B = 256
    sd = trained_sd() if family == "trained" else stress_state_dict(family, 0)
    m = UNet(1, 1, rate=0.05)
    m.load_state_dict(sd)
    m = m.cuda().eval()
    m.precision = 1
    base = synth.batch(32, seed=synth.BASE_SEED)
    gains = (1.0 - 0.5 * np.arange(8) / 8).astype(np.float32)
    wav_np = np.ascontiguousarray(np.concatenate([base * g for g in gains])[:B])
    wav = torch.from_numpy(wav_np).cuda()
    picks = [0, 100, 255]
    with torch.no_grad():
        torch.set_num_threads(8)
        sg = np.stack([ostft.magnitude(wav_np[i]) for i in picks])
        sg = sg / sg.max(axis=(1, 2), keepdims=True)
        want_den = ou.forward(torch.from_numpy(sg).float()[:, None], sd)[:, 0]
    mask, npk = HotPath(m)(wav)
    ext = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=m, device="cuda")
    mask_s, npk_s, spec = ext.find_peaks_batch(wav)
    assert torch.equal(mask_s, mask) and torch.equal(npk_s, npk)
    rl1 = ou.relative_l1(spec[picks].cpu(), want_den)
    print(f"[headline, family {family}] UNet relative L1 (bf16x3 vs oracle fp32) {rl1:.3e}, gate 1e-4, margin x{1e-4 / rl1:.1f}; "
          f"peaks per clip {float(npk.float().mean()):.1f}")
    assert rl1 <= 1e-4, (family, rl1)
    spec_np, mask_np = spec.cpu().numpy(), mask.cpu().numpy()
    _masks_vs_oracle_both_logs(spec_np, mask_np, f"headline, family {family}")
    np.testing.assert_array_equal(npk.cpu().numpy(), mask_np.reshape(B, -1).sum(axis=1))


@pytest.mark.parametrize("denoiser,N", [("demucs", 10000), ("unet", 2000)])
def test_config5_peak_metrics_experiment_at_size_sampled_queries_vs_oracle(net, denoiser, N):
    """BASELINE configs[4], second half, at the size bench.py's `configs.config5_peak_metrics*` entries run: the 10 000-query
    peak-metrics experiment with the Demucs denoiser (2 000 queries with the UNet), testing/audfprint_exps.py:86-157.  Eight
    sampled queries are recomputed by the oracle harness -- numpy STFT / find_peaks of the clean and the augmented query, the
    reference's Precision / Recall / F1 (oracle/metrics.py) and PSNR; for the denoised third the oracle picks peaks on the
    DEVICE's denoiser output of that query, re-run inside its own 256-query batch (identical input -> identical peak set) -- and
    must reproduce the device's per-query rows; the means of the whole run are the means of the rows."""
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.testing.audfprint_exps import compute_peaks_metrics
    from oracle import audfprint as oa
    from oracle import metrics as om
    from oracle import stft as ostft
    dev = torch.device("cuda")
    if denoiser == "demucs":
        from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
        from musicfpaugment_amd.training.model import Demucs
        dn = Demucs()
        dn.load_state_dict(demucs_formula(0))
        dn = dn.to(dev).eval()
        an_den = Audfprint_peaks(None, denoising=True, denoising_model="demucs", demucs=dn, device=dev)
    else:
        net.precision = 1
        an_den = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net, device=dev)
    an_no = Audfprint_peaks(None, device=dev)
    try:
        clean, aug = bench.metric_queries(N, dev)
        res, rows = compute_peaks_metrics(clean, aug, an_no, an_den, batch=256, per_query=True)
        assert rows.shape == (N, 8) and bool(torch.isfinite(rows[:, [0, 1, 2, 4, 5, 6]]).all()) and not bool(torch.isnan(rows).any())
        # (a query that AugmentFP left untouched has mse 0 against its clean clip: PSNR +inf, as 10 log10(range^2 / 0) gives the reference)
        keys = ["precision_no_den", "recall_no_den", "f1_score_no_den", "psnr_no_den_spec", "prec_den", "rec_den", "f1_den", "psnr_den_spec"]
        np.testing.assert_allclose([res[k] for k in keys], rows.mean(dim=0).cpu().numpy(), rtol=1e-12)      # inf == inf passes
        assert 0.0 < res["precision_no_den"] < 1.0 and 0.0 < res["recall_no_den"] < 1.0      # AugmentFP really changed the peaks
        rows = rows.cpu().numpy()
        for q in (0, 63, 256, 1023, N // 2 + 5, N - 257, N - 2, N - 1):
            s = (q // 256) * 256
            c_np, a_np = clean[q].cpu().numpy(), aug[q].cpu().numpy()
            _, m_clean, sg_clean = oa.find_peaks(c_np)
            _, m_aug, sg_aug = oa.find_peaks(a_np)
            mc, ma = np.asarray(m_clean).T[None], np.asarray(m_aug).T[None]
            want = [om.precision(ma, mc), om.recall(ma, mc), om.f1score(ma, mc)]
            np.testing.assert_allclose(rows[q, :3], want, rtol=0, atol=1e-12)
            psnr = lambda x, t: 10 * np.log10((t.max() - t.min()) ** 2 / np.mean((x.astype(np.float64) - t) ** 2))
            same = lambda got, want, tol: got == want or abs(got - want) < tol          # +inf for an untouched query
            with np.errstate(divide="ignore"):
                assert same(rows[q, 3], psnr(sg_aug, sg_clean), 1e-8)
            # the denoised third: the device's denoiser output of this query inside its own batch, then the oracle picker
            blk = aug[s:s + 256].contiguous()
            if denoiser == "demucs":
                den_wav = dn(blk)[q - s, 0].cpu().numpy()
                _, m_den, sg_den = oa.find_peaks(den_wav)
            else:
                sg_den = an_den.find_peaks_batch(blk)[2][q - s].cpu().numpy()
                m_den = oa.find_peaks_from_sgram(sg_den, order="C")[1]
            md = np.asarray(m_den).T[None]
            want_d = [om.precision(md, mc), om.recall(md, mc), om.f1score(md, mc)]
            np.testing.assert_allclose(rows[q, 4:7], want_d, rtol=0, atol=1e-12)
            assert same(rows[q, 7], psnr(sg_den, sg_clean), 1e-8 if denoiser == "demucs" else 1e-4)
        if denoiser == "unet":
            # EVERY denoised mask of the run, not a sample: the device's peak mask of each of the N queries against the oracle picker on
            # the device's float32 spectrogram of that query -- twice.  On this branch the reference takes np.log of a float32 array
            # (peak_extractor.py:275): numpy's SIMD float32 log, ~5 % of whose values differ from the correctly rounded ones by up to a
            # few ulp; the device computes the float64 log and rounds once.  So (1) against the oracle WITH THE CORRECTLY ROUNDED LOG the
            # device must agree on every query (same values in -> same peaks out, by construction), and (2) against the oracle with
            # numpy's log -- the reference's arithmetic to the last bit -- agreement is statistical: counted, printed, and bounded
            # (observed 0-1 queries of 2 000 with one differing cell; tests/test_oracle_vs_libs.py replays 2 048 more on the CPU).
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            vs_rounded, vs_numpy, cells_numpy = 0, 0, 0
            with ProcessPoolExecutor(max_workers=min(12, os.cpu_count() or 1), mp_context=mp.get_context("spawn")) as ex:
                for s0 in range(0, N, 256):
                    mask, _, spec = an_den.find_peaks_batch(aug[s0:s0 + 256].contiguous())
                    mask_np, spec_np = mask.cpu().numpy(), spec.cpu().numpy()
                    both = list(ex.map(oa.masks_both_logs, list(spec_np), chunksize=8))
                    for k in range(len(both)):
                        dn = int(np.count_nonzero((mask_np[k] != 0) != (both[k][0] != 0)))
                        dr = int(np.count_nonzero((mask_np[k] != 0) != (both[k][1] != 0)))
                        vs_numpy += dn > 0
                        cells_numpy += dn
                        vs_rounded += dr > 0
            print(f"[config 5, UNet] denoised masks vs the oracle picker on the device's spectrogram: {vs_rounded} of {N} queries differ with the correctly "
                  f"rounded float32 log, {vs_numpy} ({cells_numpy} cells) with numpy's own float32 log")
            assert vs_rounded == 0, vs_rounded
            assert vs_numpy <= 4 and cells_numpy <= 8, (vs_numpy, cells_numpy)
    finally:
        net.precision = 0
