"""The data-parallel training path on real GPU kernels with TWO processes: both ranks share cuda:0 and talk over gloo (RCCL needs
one GPU per rank; the single-GPU test box has one).  Checks the scalar MAX all-reduce of the spectrogram maximum, the bucketed
gradient all-reduce and the 1/world scaling inside the fused Adam step against an in-process emulation of the two ranks.  Adam's
parameter update is invariant to a constant gradient scale, so the 1/world factor is read off the MOMENTS the ranks dump: dropped,
exp_avg comes out 2x and exp_avg_sq 4x too large (relative L1 1.0 and 3.0)."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from musicfpaugment_amd.training.weights import formula_state_dict

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# torch.distributed.run binds its own rendezvous port (c10d endpoint 127.0.0.1:0 under --standalone): no fixed port to clash on a
# shared box.  Workers still find MASTER_ADDR / MASTER_PORT in their environment.
RDZV = ("--standalone", "--local-addr", "127.0.0.1")
# small nested train-step entries for the N > 1 inference line (bench.dist_configs; the defaults are 64 clips per GPU / global 512, 8 s)
DIST_SMALL = ("--dist-train-clips", "4", "--dist-strong-global", "8", "--dist-train-steps", "2", "--dist-train-seconds", "1")


def _check_nested_train_entries(out, world):
    """The N > 1 inference line carries the path's one collective: the train step weak- and strong-scaled, each with its own
    self-verification and all-reduce accounting."""
    sys.path.insert(0, ROOT)
    import bench
    for name, scaling, per_gpu in (("config4_unet_train_step", "weak", 4), ("config4_unet_train_step_strong", "strong", 8 // world)):
        ent = out["configs"][name]
        assert "error" not in ent and "skipped" not in ent, ent
        assert set(bench.TRAIN_LINE_KEYS) <= set(ent), sorted(set(bench.TRAIN_LINE_KEYS) - set(ent))
        assert ent["scaling"] == scaling and ent["ranks_seen"] == world and len(ent["per_rank_value"]) == world
        assert ent["clips_per_gpu_per_step"] == per_gpu and ent["clips_per_step_all_gpus"] == per_gpu * world
        assert ent["allreduce_bytes_per_step"] >= 31_036_481 * 4 and ent["allreduce_exposed_wait_ms_per_step"] >= 0
        assert ent["value"] > 0 and "AugmentFP chain on the device inside the step" in ent["config"]["workload"]
        assert np.isfinite(ent["config"]["loss_last"])


def _check(r):
    """A failed launch is an ERROR, also when it is the rendezvous that failed: these tests are the only multi-process (and the only
    RCCL) evidence a one-GPU box can give, so they must not turn into skips silently.  MFPA_REQUIRE_DIST=0 restores the skip for
    hosts where a second process cannot be started at all."""
    if r.returncode == 0:
        return
    tail = r.stdout[-2000:] + r.stderr[-4000:]
    if os.environ.get("MFPA_REQUIRE_DIST", "1") == "0":
        for marker in ("RendezvousError", "RendezvousConnectionError", "Address already in use", "EADDRINUSE",
                       "failed to connect", "Connection refused", "DistNetworkError"):
            if marker in tail:
                pytest.skip("two-process rendezvous unavailable here: " + marker)
    raise AssertionError(tail)


def _rel_l1(got, want):
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - want).sum() / np.abs(want).sum())


def _check_moments_against_emulation(got, want_m, want_v, again_m, want_g=None):
    """The two ranks' Adam moments after one data-parallel step against the emulation's (one Adam step at world 1 on the AVERAGED
    gradient).  The only legitimate difference is float-atomic summation noise in the gradients, which reaches exp_avg linearly and
    exp_avg_sq at twice the relative size.  It is measured, not assumed: `again_m` is exp_avg of a SECOND in-process run of the same
    emulation, and the relative L1 between the two runs is the noise (floored at one float32 rounding, 2^-24, should two runs ever
    agree to the bit).  Bounds: 10x the noise for exp_avg (and the gradient sum), 20x for exp_avg_sq; whatever the measurement
    says, both must stay below 0.1 -- a dropped 1/2 shows as 1.0 on exp_avg and 3.0 on exp_avg_sq.
    Measured on the MI355X: noise 7.6e-8 (UNet) / 7.5e-8 (Demucs); two ranks against the emulation 7.8e-8 / 8.1e-8 on exp_avg
    and 1.8e-7 / 1.7e-7 on exp_avg_sq, so the bounds in force are about 7.5e-7 and 1.5e-6."""
    for key in ("flat_m", "flat_v"):
        np.testing.assert_array_equal(got[0][key], got[1][key])               # the replicas hold the same optimiser state
    noise = max(_rel_l1(again_m, want_m), 2.0 ** -24)
    bound_m, bound_v = 10 * noise, 20 * noise
    assert bound_m < 0.1 and bound_v < 0.1, (noise, bound_m, bound_v)
    dm, dv = _rel_l1(got[0]["flat_m"], want_m), _rel_l1(got[0]["flat_v"], want_v)
    print(f"run-to-run noise of the emulation (relative L1 of exp_avg) {noise:.3e}; two ranks vs emulation: exp_avg {dm:.3e}, exp_avg_sq {dv:.3e}")
    assert dm <= bound_m, f"exp_avg: relative L1 {dm:.3e} to the emulation, measured run-to-run noise {noise:.3e}, bound {bound_m:.3e}"
    assert dv <= bound_v, f"exp_avg_sq: relative L1 {dv:.3e} to the emulation, measured run-to-run noise {noise:.3e}, bound {bound_v:.3e}"
    if want_g is not None:
        dg = _rel_l1(got[0]["flat_g"], want_g)
        assert dg <= bound_m, f"summed gradient: relative L1 {dg:.3e} to the emulation, measured run-to-run noise {noise:.3e}, bound {bound_m:.3e}"


def _emulated_unet_exp_avg(am, ga, target):
    """exp_avg of the emulated two-rank UNet step, run once more (the run-to-run noise of the emulation itself)."""
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    grads, e0 = [], None
    for k in range(2):
        net = UNet(1, 1, rate=0.0)
        net.load_state_dict(formula_state_dict(0))
        eng = UNetTrainEngine(net.cuda().train(), lr=1e-3, precision=0)
        pred = eng.forward(spec64=am[2 * k:2 * k + 2].contiguous(), denom=ga.expand(2).contiguous())
        _, dpred = eng.l1_loss(pred, target[2 * k:2 * k + 2].contiguous())
        eng.backward(dpred)
        grads.append(eng.flat_g.clone())
        e0 = eng if e0 is None else e0
    e0.flat_g.copy_((grads[0] + grads[1]) / 2)
    e0.optimizer_step()
    return e0.flat_m.cpu().numpy()


def _emulated_demucs_exp_avg(clean, aug):
    from musicfpaugment_amd.ops_demucs_train import DemucsTrainEngine
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
    gsum = None
    for k in range(2):
        eng = DemucsTrainEngine(demucs_formula(0), "cuda", lr=1e-3, precision=0)
        pred = eng.forward(torch.from_numpy(aug[2 * k:2 * k + 2]).cuda())
        _, _, _, dpred = eng.loss_and_grad(pred, torch.from_numpy(clean[2 * k:2 * k + 2]).cuda())
        eng.backward(dpred)
        gsum = eng.flat_g.clone() if gsum is None else gsum + eng.flat_g
    eng.flat_g.copy_(gsum / 2)
    eng.adam_step()
    return eng.flat_m.cpu().numpy()


def test_two_rank_train_step_matches_the_emulated_data_parallel_step():
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.ops_train import UNetTrainEngine
    from musicfpaugment_amd.training.unet import UNet
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "tests", "_dist_train_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        _check(r)
        got = [np.load(os.path.join(tmp, f"rank{k}.npz")) for k in range(2)]
    np.testing.assert_array_equal(got[0]["params"], got[1]["params"])            # the replicas stay in sync
    np.testing.assert_array_equal(got[0]["gmax"], got[1]["gmax"])
    # emulation: per-rank forward/backward (own BatchNorm statistics, as under DDP), gradients averaged, one Adam step
    clean = synth.batch(4, seed=900, n=8000)
    aug = (0.7 * clean + 0.3 * synth.batch(4, seed=901, n=8000, tonal=False)).astype(np.float32)
    cm, cmax = ops.stft_mag(torch.from_numpy(clean).cuda(), torch.float64)
    am, amax = ops.stft_mag(torch.from_numpy(aug).cuda(), torch.float64)
    gc, ga = cmax.max(), amax.max()
    np.testing.assert_array_equal(got[0]["gmax"], [float(gc), float(ga)])
    target = ops.normalize_(cm, gc.expand(4).contiguous(), per_clip=True)
    grads, losses, engines = [], [], []
    for k in range(2):
        net = UNet(1, 1, rate=0.0)
        net.load_state_dict(formula_state_dict(0))
        eng = UNetTrainEngine(net.cuda().train(), lr=1e-3, precision=0)
        pred = eng.forward(spec64=am[2 * k:2 * k + 2].contiguous(), denom=ga.expand(2).contiguous())
        loss, dpred = eng.l1_loss(pred, target[2 * k:2 * k + 2].contiguous())
        eng.backward(dpred)
        grads.append(eng.flat_g.clone()); losses.append(float(loss)); engines.append(eng)
    np.testing.assert_allclose([got[0]["loss"], got[1]["loss"]], losses, rtol=1e-6)
    e0 = engines[0]
    e0.flat_g.copy_((grads[0] + grads[1]) / 2)
    e0.optimizer_step()
    want = e0.flat_p.cpu().numpy()
    # Adam's first update is lr * g / (|g| + eps): where |g| ~ eps the sign of float-atomic summation noise decides it, so
    # compare the bulk of the 31 M updates tightly and bound the handful of near-zero-gradient entries by the step size
    diff = np.abs(got[0]["params"] - want)
    assert np.quantile(diff, 0.999) <= 1e-6, np.quantile(diff, 0.999)
    assert diff.max() <= 2.1e-3, diff.max()
    assert float(np.mean(diff > 1e-5)) < 1e-4
    # the 1/world factor: the ranks' moments against the emulation's (e0 stepped at world 1 on the averaged gradient)
    np.testing.assert_array_equal(got[0]["flat_g"], got[1]["flat_g"])
    _check_moments_against_emulation(got, e0.flat_m.cpu().numpy(), e0.flat_v.cpu().numpy(), _emulated_unet_exp_avg(am, ga, target),
                                     want_g=(grads[0] + grads[1]).cpu().numpy())


def test_two_rank_peak_metrics_experiment_equals_single_process():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("_dist_metrics_worker", os.path.join(ROOT, "tests", "_dist_metrics_worker.py"))
    worker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(worker)
    want = worker.run()                                                          # world size 1: no collective
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "tests", "_dist_metrics_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        _check(r)
        got = json.load(open(os.path.join(tmp, "metrics.json")))
    assert set(got) == set(want)
    for k in want:                                                               # per-query rows are gathered in query order
        assert got[k] == want[k], (k, got[k], want[k])


@pytest.mark.parametrize("mode", ["infer", "train"])
def test_bench_runs_under_torchrun_with_two_ranks(mode):
    """bench.py's N > 1 path (rank / world from the environment, barriers, MAX-over-ranks timing, one JSON line from rank 0, the
    bucketed gradient all-reduce in train mode) with two ranks sharing cuda:0 over gloo (MFPA_DIST_BACKEND; the driver uses RCCL)."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", MFPA_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--clips", "8",
           "--mode", mode, "--full", *DIST_SMALL]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    _check(r)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1                                                       # rank 0 only
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert out["scaling"] == "weak" and out["unit"] == "clips/s" and "roofline" in out
    assert "cpu_baseline" not in out                                             # N = 1 only
    assert abs(out["value"] - 2 * 8 * 2 / (out["ms_per_step"] * 2 / 1e3)) < 0.01 * out["value"]   # whole-job aggregate
    # the line verifies itself: a SUM all-reduce of 1 over the group saw both ranks, and each rank's own rate is there
    assert out["ranks_seen"] == 2 and len(out["per_rank_value"]) == 2 and min(out["per_rank_value"]) > 0
    assert sum(out["per_rank_value"]) >= 0.99 * out["value"]                     # value uses the MAX time over ranks
    if mode == "train":
        assert out["config"]["allreduce_exposed_wait_ms_per_step"] is not None and out["config"]["allreduce_exposed_wait_ms_per_step"] >= 0
    else:
        _check_nested_train_entries(out, 2)


@pytest.mark.parametrize("mode", ["infer", "train"])
def test_bench_self_launch_with_two_ranks(mode):
    """`python bench.py --gpus 2 ...` with no WORLD_SIZE in the environment (how the driver calls it): bench.py starts its own
    ranks (child `python -m torch.distributed.run`), the parent relays one JSON line.  Two ranks share cuda:0 over gloo here."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(HSA_ENABLE_IPC_MODE_LEGACY="0", MFPA_DIST_BACKEND="gloo")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--clips", "8", "--mode", mode, "--full", *DIST_SMALL]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    _check(r)
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout                                             # exactly rank 0's line, nothing else on stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["value"] > 0 and out["dist_backend"] == "gloo"
    assert out["config"]["clips_per_gpu_per_step"] == 8
    if mode == "train":
        assert out["config"]["allreduce_bytes_per_step"] >= 31_036_481 * 4
    else:                                    # `python bench.py --gpus 2`, the driver's own command form: headline + the collective, one line
        _check_nested_train_entries(out, 2)
        assert out["parity_in_run"]["rel_l1_bf16x3_vs_fp32"] <= 1e-4


@pytest.mark.parametrize("mode", ["train", "infer"])
def test_bench_on_rccl_at_world_size_one(mode):
    """The RCCL leg at the only world size a one-GPU box allows: under torch.distributed.run with one rank bench.py still calls
    init_process_group("nccl", device_id=...) -- RCCL on ROCm -- so the barriers, the MAX-over-ranks timing, and in train mode the
    two scalar MAX all-reduces of the spectrogram maxima and the nine asynchronous gradient-bucket all-reduces issued between
    ctypes-launched kernels (ops_train.UNetTrainEngine) all execute on RCCL."""
    import json
    env = {k: v for k, v in os.environ.items() if k != "MFPA_DIST_BACKEND"}
    env.update(MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", *RDZV, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--clips", "8",
           "--mode", mode, "--full", "--cpu-seconds", "0", "--no-configs"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    _check(r)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["value"] > 0 and out["dist_backend"].startswith("rccl")
    assert out["ranks_seen"] == 1 and len(out["per_rank_value"]) == 1           # all-reduce / all-gather on the device through RCCL
    if mode == "train":
        assert out["config"]["allreduce_calls_per_step"] == 11 and out["config"]["allreduce_bytes_per_step"] == 31_036_481 * 4 + 16 and np.isfinite(out["config"]["loss_last"])


def test_two_rank_sync_batchnorm_step_equals_the_single_gpu_step():
    """sync_bn=True: BatchNorm statistics over the global batch -- a 2 x 2-clip data-parallel step reproduces the 4-clip
    single-GPU step of the reference semantics (parameters, running statistics, mean loss)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("_dist_syncbn_worker", os.path.join(ROOT, "tests", "_dist_syncbn_worker.py"))
    worker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(worker)
    eng, loss = worker.step(0, 4, False)                                         # one process, the whole batch, plain BatchNorm
    want = eng.flat_p.cpu().numpy()
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "tests", "_dist_syncbn_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        _check(r)
        got = [np.load(os.path.join(tmp, f"rank{k}.npz")) for k in range(2)]
    np.testing.assert_array_equal(got[0]["params"], got[1]["params"])
    np.testing.assert_allclose(0.5 * (got[0]["loss"] + got[1]["loss"]), loss, rtol=1e-6)     # mean of the shard means
    np.testing.assert_allclose(got[0]["rm"], eng.running["inc.double_conv.1.running_mean"].cpu().numpy(), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(got[0]["rv"], eng.running["down4.maxpool_conv.1.double_conv.4.running_var"].cpu().numpy(), rtol=1e-4)
    diff = np.abs(got[0]["params"] - want)                                       # Adam's first step is lr * sign-like: see above
    assert np.quantile(diff, 0.999) <= 1e-6, np.quantile(diff, 0.999)
    assert float(np.mean(diff > 1e-5)) < 1e-4 and diff.max() <= 2.1e-3


def test_two_rank_trainer_loop_keeps_the_replicas_and_their_decisions_in_step():
    """Trainer.training_loop on two ranks with different training / validation shards: the validation loss that drives the
    plateau schedule, early stopping and the checkpoints is averaged over the ranks, so both take the same decisions (same lr,
    same epoch, same best loss), the parameters stay bit-identical, and rank 0 alone writes last_epoch.pt / best_epoch.pt."""
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "tests", "_dist_trainer_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
        _check(r)
        got = [np.load(os.path.join(tmp, f"rank{k}.npz")) for k in range(2)]
        from musicfpaugment_amd.training.train import _RefEarlyStopping
        with torch.serialization.safe_globals([_RefEarlyStopping]):
            ck = torch.load(os.path.join(tmp, "ckpt", "last_epoch.pt"), weights_only=True)
        assert os.path.exists(os.path.join(tmp, "ckpt", "best_epoch.pt"))
    np.testing.assert_array_equal(got[0]["params"], got[1]["params"])
    np.testing.assert_array_equal(got[0]["val"], got[1]["val"])                  # the rank-averaged losses
    assert float(got[0]["lr"]) == float(got[1]["lr"]) and int(got[0]["epoch"]) == int(got[1]["epoch"]) == 3
    assert float(got[0]["best"]) == float(got[1]["best"]) == float(ck["best_val_loss"]) == float(np.min(got[0]["val"]))
    np.testing.assert_array_equal(got[0]["sched"], got[1]["sched"])
    assert ck["epoch"] == 3 and len(got[0]["val"]) == 3


def test_two_rank_demucs_train_step():
    """Data-parallel Demucs step: the summed (all-reduced) gradients of two ranks and the 1/world scaling in Adam against an
    in-process emulation of the two shards.  Each rank's loss is over its own shard (as under DDP)."""
    from musicfpaugment_amd.ops_demucs_train import DemucsTrainEngine
    from musicfpaugment_amd.training.demucs_weights import formula_state_dict as demucs_formula
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", *RDZV, os.path.join(ROOT, "tests", "_dist_demucs_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        _check(r)
        got = [np.load(os.path.join(tmp, f"rank{k}.npz")) for k in range(2)]
    np.testing.assert_array_equal(got[0]["params"], got[1]["params"])            # the replicas stay in sync
    np.testing.assert_array_equal(got[0]["grads"], got[1]["grads"])              # ... on the same summed gradients
    clean = synth.batch(4, seed=910, n=4000)
    aug = (clean + 0.05 * synth.batch(4, seed=911, n=4000)).astype(np.float32)
    gsum = None
    for k in range(2):
        eng = DemucsTrainEngine(demucs_formula(0), "cuda", lr=1e-3, precision=0)
        pred = eng.forward(torch.from_numpy(aug[2 * k:2 * k + 2]).cuda())
        _, _, _, dpred = eng.loss_and_grad(pred, torch.from_numpy(clean[2 * k:2 * k + 2]).cuda())
        eng.backward(dpred)
        gsum = eng.flat_g.clone() if gsum is None else gsum + eng.flat_g
    g = gsum.cpu().numpy().astype(np.float64)
    rel = np.abs(got[0]["grads"] - g).sum() / np.abs(g).sum()
    assert rel < 1e-4, rel                                                       # float atomics: not bit-reproducible
    # one Adam step on the AVERAGED gradient: -lr * sign(g) wherever the sign is safe
    p0 = eng.flat_p.cpu().numpy()                                                # untouched initial parameters
    big = np.abs(g) > 1e-5
    np.testing.assert_allclose((got[0]["params"] - p0)[big], -1e-3 * np.sign(g[big]), atol=2e-5)
    # the 1/world factor: one Adam step at world 1 on the AVERAGED gradient, and the ranks' moments against its moments
    eng.flat_g.copy_(gsum / 2)
    eng.adam_step()
    _check_moments_against_emulation(got, eng.flat_m.cpu().numpy(), eng.flat_v.cpu().numpy(), _emulated_demucs_exp_avg(clean, aug))
