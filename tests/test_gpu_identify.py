"""GPU: the Audfprint hash table and matcher (match.hip) against the reference's goldens (g14) and the test oracle
(tests/_identify_oracle.py), and the identification experiment end to end."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from tests import _identify_oracle as io_

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _split(rows, off):
    return [rows[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _pad(lists):
    cap = max(1, max(len(x) for x in lists))
    uq = np.zeros((len(lists), cap, 2), np.int32)
    for i, x in enumerate(lists):
        uq[i, :len(x)] = x
    return torch.from_numpy(uq).cuda(), torch.tensor([len(x) for x in lists], dtype=torch.int32).cuda()


@pytest.fixture(scope="module")
def g14():
    return dict(np.load(os.path.join(GOLDEN, "g14_identify.npz")))


@pytest.fixture(scope="module")
def device_db(g14):
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    ht = HashTable(device="cuda")
    tracks = _split(g14["track_rows"], g14["track_off"])
    uq, n = _pad(tracks)
    ht.store_batch(["track_%03d" % i for i in range(len(tracks))], uq, n)
    return ht


@pytest.fixture(scope="module")
def oracle_db(g14):
    table, counts = io_.empty_table()
    for i, tr in enumerate(_split(g14["track_rows"], g14["track_off"])):
        io_.store(table, counts, tr, i)
    return table, counts, g14["hashesperid"]


def _sha256(a, dt):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


def _golden_equal(ht, g14):
    """Bit-identical to the reference's table: SHA-256 of the table (little-endian uint32) and of the counts (int32)."""
    c = ht.counts.cpu().numpy()
    assert int(c.sum()) == int(g14["n_entries"]) and np.count_nonzero(c) == int(g14["n_buckets"])
    np.testing.assert_array_equal(_sha256(c, "<i4"), g14["counts_sha256"])
    np.testing.assert_array_equal(_sha256(ht.table.cpu().numpy().view(np.uint32), "<u4"), g14["table_sha256"])
    np.testing.assert_array_equal(ht.hashesperid, g14["hashesperid"])


def test_store_batch_is_bit_identical_to_the_reference(device_db, g14):
    _golden_equal(device_db, g14)


def test_store_one_track_at_a_time_equals_store_batch(device_db, g14):
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    ht = HashTable(device="cuda")
    for i, tr in enumerate(_split(g14["track_rows"], g14["track_off"])):
        ht.store("track_%03d" % i, tr)
    assert torch.equal(ht.table, device_db.table) and torch.equal(ht.counts, device_db.counts)


def test_overflowing_store_is_deterministic_and_keeps_the_semantics(g14):
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    tracks = _split(g14["ovf_rows"], g14["ovf_off"])
    names = ["ovf_%02d" % i for i in range(len(tracks))]
    tabs = []
    for split in (len(tracks), 7):                                   # one batch, then batches of 7: same table
        ht = HashTable(device="cuda", seed=7)
        for s in range(0, len(tracks), split):
            uq, n = _pad(tracks[s:s + split])
            ht.store_batch(names[s:s + split], uq, n)
        tabs.append(ht)
    assert torch.equal(tabs[0].table, tabs[1].table) and torch.equal(tabs[0].counts, tabs[1].counts)
    ht = tabs[0]
    c = ht.counts.cpu().numpy()
    np.testing.assert_array_equal(np.flatnonzero(c), g14["ovf_counts_idx"])
    np.testing.assert_array_equal(c[c != 0], g14["ovf_counts_val"])
    np.testing.assert_array_equal(ht.hashesperid, g14["ovf_hashesperid"])
    assert c.max() > ht.depth
    table, counts = io_.empty_table()                               # the oracle's reservoir draw is the kernel's
    for i, tr in enumerate(tracks):
        io_.store(table, counts, tr, i, seed=7)
    np.testing.assert_array_equal(ht.table.cpu().numpy().view(np.uint32), table)
    tab = ht.table.cpu().numpy().view(np.uint32)
    for b in np.flatnonzero(c):                                      # every stored value is a row of that bucket
        allowed = set()
        for i, tr in enumerate(tracks):
            sel = tr[(tr[:, 1].astype(np.int64) & 0xFFFFF) == b]
            allowed |= {((i + 1) << 14) | (int(t) & 16383) for t in sel[:, 0]}
        assert set(tab[b, :min(100, c[b])].tolist()) <= allowed


def test_match_batch_and_match_hashes_equal_the_reference(device_db, oracle_db, g14):
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    queries = _split(g14["query_rows"], g14["query_off"])
    results = _split(g14["result_rows"], g14["result_off"])
    m = Matcher()
    uq, n = _pad(queries)
    rows, info = m.match_batch(device_db, uq, n, k=256)
    rows, info = rows.cpu().numpy(), info.cpu().numpy()
    for qi, (q, want) in enumerate(zip(queries, results)):
        ties = io_.rank_ties(*oracle_db, q)
        assert info[qi, 1] == info[qi, 2] == len(want), (qi, info[qi].tolist(), len(want))
        err = io_.rows_equivalent(rows[qi, :info[qi, 1]], want, ties)
        assert err is None, f"match_batch query {qi}: {err}"
        got, _ = m.match_hashes(device_db, q)
        err = io_.rows_equivalent(got, want, ties)
        assert err is None, f"match_hashes query {qi}: {err}"
        if len(want) and (len(want) == 1 or want[0, 1] != want[1, 1]):         # unique maximum: the top row is determined
            assert got[0, :3].tolist() == want[0, :3].tolist()
        np.testing.assert_array_equal(got, io_.match(*oracle_db, q))           # the device's tie order is the oracle's
    # k = 1 is the first row of the full result
    top, info1 = m.match_batch(device_db, uq, n, k=1)
    np.testing.assert_array_equal(top[:, 0].cpu().numpy()[info[:, 1] > 0], rows[info[:, 1] > 0, 0])
    assert np.array_equal(info1[:, 1].cpu().numpy(), np.minimum(info[:, 1], 1))


def test_hit_capacity_retry_gives_the_same_rows(device_db, g14):
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    queries = _split(g14["query_rows"], g14["query_off"])
    uq, n = _pad(queries)
    m = Matcher()
    want, winfo = m.match_batch(device_db, uq, n, k=256)
    small = Matcher()
    small.hit_capacity = 64                                          # most queries exceed it: reported, then run again
    got, info = small.match_batch(device_db, uq, n, k=256)
    assert small.hit_capacity > 64 and int(winfo[:, 0].max()) > 64
    assert torch.equal(got, want) and torch.equal(info, winfo)
    big = max(range(len(queries)), key=lambda i: int(winfo[i, 0]))
    assert int(winfo[big, 0]) > 4096                                 # a query on the global-memory sort path


def test_dense_query_on_the_multi_chunk_sort_path_equals_the_oracle():
    """~20 000 hits in one query (bitonic stages beyond several LDS chunks), against the oracle on the same table."""
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    rng = np.random.default_rng(21)
    pool = rng.choice(1 << 20, 220, replace=False)
    ht = HashTable(device="cuda")
    table, counts = io_.empty_table()
    tracks = []
    for i in range(100):
        tr = np.stack([rng.integers(0, 3000, 220), pool], 1).astype(np.int32)
        tr[:, 0] = np.where(rng.random(220) < 0.3, 500 + 3 * np.arange(220) + i % 3, tr[:, 0])   # partial alignments
        tracks.append(tr)
        io_.store(table, counts, tr, i)
    uq, n = _pad(tracks)
    ht.store_batch(["d%d" % i for i in range(100)], uq, n)
    np.testing.assert_array_equal(ht.table.cpu().numpy().view(np.uint32), table)
    q = np.stack([3 * np.arange(220), pool], 1).astype(np.int32)
    got, _ = Matcher().match_hashes(ht, q)
    want = io_.match(table, counts, ht.hashesperid, q)
    assert len(io_.hits(table, counts, q)[0]) > 16384 and len(want) > 0
    np.testing.assert_array_equal(got, want)


def test_load_reference_file_and_round_trip(g14, tmp_path):
    """g14_hashtable.pklz was written by the reference's HashTable.save (a hashbits-12, depth-8 table its store filled)."""
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    ht = HashTable(os.path.join(GOLDEN, "g14_hashtable.pklz"), device="cuda")
    assert (ht.hashbits, ht.depth, ht.maxtimebits) == (12, 8, 14)
    np.testing.assert_array_equal(ht.table.cpu().numpy().view(np.uint32), g14["small_table"])
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), g14["small_counts"])
    np.testing.assert_array_equal(ht.hashesperid, g14["small_hashesperid"])
    assert ht.names == ["track_%03d" % i for i in range(150, 170)]
    p = str(tmp_path / "db.pklz")
    ht.save(p)
    ht2 = HashTable(p, device="cuda")
    assert torch.equal(ht2.table, ht.table) and torch.equal(ht2.counts, ht.counts) and ht2.names == ht.names
    np.testing.assert_array_equal(ht2.hashesperid, ht.hashesperid)
    # the device store of the same tracks into a table of that shape gives the reference's table
    ht3 = HashTable(os.path.join(GOLDEN, "g14_hashtable.pklz"), device="cuda")
    ht3.reset()
    tracks = _split(g14["track_rows"], g14["track_off"])
    uq, n = _pad([tracks[i] for i in range(150, 170)])
    ht3.store_batch(["track_%03d" % i for i in range(150, 170)], uq, n)
    assert torch.equal(ht3.table, ht.table) and torch.equal(ht3.counts, ht.counts)
    # the main database round-trips too
    db = HashTable(device="cuda")
    tr = _split(g14["track_rows"], g14["track_off"])
    uq, n = _pad(tr)
    db.store_batch(["track_%03d" % i for i in range(len(tr))], uq, n)
    p = str(tmp_path / "big.pklz")
    db.save(p)
    _golden_equal(HashTable(p, device="cuda"), g14)


@pytest.fixture(scope="module")
def e2e():
    """Synthetic 30-s (and 20-s) tracks in a database; 8-s excerpts at whole-frame and sub-frame offsets, clean and augmented."""
    from musicfpaugment_amd.augmentation import AugmentFP, synthetic_banks
    from musicfpaugment_amd.testing.audfprint_exps import create_fp_database_batch
    long_ = synth.batch(8, seed=1410, n=240000)
    short = synth.batch(4, seed=1420, n=160000)
    tracks = [long_[0], short[0], long_[1], long_[2], short[1], long_[3], long_[4], short[2], long_[5], long_[6], short[3],
              long_[7]]
    names = ["trk%02d" % i for i in range(len(tracks))]
    ht = create_fp_database_batch(tracks, names, batch=5)
    rng = np.random.default_rng(5)
    owner, q = [], []
    for i in range(24):
        o = int(rng.integers(0, len(tracks)))
        start = 256 * int(rng.integers(0, (len(tracks[o]) - 64000) // 256))
        if i % 2:
            start = min(start + int(rng.integers(1, 256)), len(tracks[o]) - 64000)    # sub-frame offset
        owner.append(o)
        q.append(tracks[o][start:start + 64000])
    clean = torch.from_numpy(np.stack(q))
    irs, noises = synthetic_banks(0)
    import random
    random.seed(3)
    torch.manual_seed(3)
    aug = AugmentFP(None, 8000, ir_bank=irs, noise_bank=noises).batch_augment(clean[:, None, :].cuda())[:, 0].contiguous()
    return dict(ht=ht, tracks=tracks, names=names, owner=owner, clean=clean, aug=aug)


def _analyzers(shifts=4):
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    an1 = Audfprint_peaks(None)
    an1.shifts = shifts
    an2 = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net.cuda().eval())
    an2.shifts = shifts
    return an1, an2


def test_identification_end_to_end_equals_the_oracle(e2e):
    from musicfpaugment_amd.testing.audfprint_exps import compute_accuracy_batch
    ht = e2e["ht"]
    an1, an2 = _analyzers()
    table = ht.table.cpu().numpy().view(np.uint32)
    counts = ht.counts.cpu().numpy()
    for key in ("clean", "aug"):
        wav = e2e[key]
        res, rows = compute_accuracy_batch(wav, e2e["owner"], ht, an1, an2, batch=10, per_query=True)
        rows = rows.cpu().numpy()
        for col, an in ((0, an1), (2, an2)):
            uq, n = an.hashes_batch(wav.cuda().contiguous())
            uq, n = uq.cpu().numpy(), n.cpu().numpy()
            for i in range(wav.shape[0]):
                want = io_.match(table, counts, ht.hashesperid, uq[i, :n[i]])
                exp = (int(want[0, 0]), int(want[0, 1])) if len(want) else (-1, 0)
                assert (rows[i, col], rows[i, col + 1]) == exp, (key, col, i)
        if key == "clean":
            assert res["No Denoising"] == 1.0, res
        assert 0.0 <= res["Mix Pipeline"] <= 1.0


def test_file_based_experiment_equals_the_batched_one(e2e, tmp_path):
    from scipy.io import wavfile
    from musicfpaugment_amd.testing.audfprint_exps import (compute_accuracy, compute_accuracy_batch, create_fp_database,
                                                           create_fp_database_batch)
    files = []
    for name, t in zip(e2e["names"], e2e["tracks"]):
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, 8000, t.astype(np.float32))
        files.append(p)
    files.append(str(tmp_path / "unreadable.mp3"))                   # skipped with a message, as in the reference
    db = str(tmp_path / "db.pklz")
    create_fp_database(files, db)
    qdir = tmp_path / "q"
    qdir.mkdir()
    qfiles = []
    for i, (o, x) in enumerate(zip(e2e["owner"][:8], e2e["aug"][:8].cpu().numpy())):
        sub = qdir / str(i)
        sub.mkdir()
        p = str(sub / (e2e["names"][o] + ".wav"))
        wavfile.write(p, 8000, x.astype(np.float32))
        qfiles.append(p)
    an1, an2 = _analyzers()
    got = compute_accuracy(qfiles, db, an1, an2)
    ht = create_fp_database_batch(e2e["tracks"], files[:-1])
    want = compute_accuracy_batch(e2e["aug"][:8], e2e["owner"][:8], ht, an1, an2)
    assert got == want, (got, want)


def test_track_limits_are_enforced():
    from musicfpaugment_amd.testing.audfprint_exps import create_fp_database_batch
    with pytest.raises(ValueError, match="1500"):
        create_fp_database_batch([np.zeros(1500 * 256, np.float32)], ["long"])


def test_two_ranks_equal_one():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("_dist_identify_worker", os.path.join(ROOT, "tests", "_dist_identify_worker.py"))
    worker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(worker)
    want_res, want_rows = worker.run()
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--standalone", "--local-addr",
               "127.0.0.1", os.path.join(ROOT, "tests", "_dist_identify_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        import json as _j
        got = _j.load(open(os.path.join(tmp, "identify.json")))
    assert got["rows"] == want_rows and got["res"] == want_res
