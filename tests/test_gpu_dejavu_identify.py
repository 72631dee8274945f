"""GPU: the Dejavu fingerprint store and matcher (dejavu_match.hip) against the reference's goldens (g15) and the test oracle
(tests/_dejavu_oracle.py), and the identification experiment end to end."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from tests import _dejavu_oracle as do

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _split(a, n):
    off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    return [a[off[i]:off[i + 1]] for i in range(len(n))]


def _pad(queries):
    """[(digest bytes, t1)] lists -> (B, cap, 10) uint8, (B, cap) int32, (B,) int32 on the device."""
    cap = max(1, max(len(q) for q in queries))
    dig = np.zeros((len(queries), cap, 10), np.uint8)
    t1 = np.zeros((len(queries), cap), np.int32)
    for i, q in enumerate(queries):
        for j, (d, t) in enumerate(q):
            dig[i, j] = np.frombuffer(d, np.uint8)
            t1[i, j] = t
    n = torch.tensor([len(q) for q in queries], dtype=torch.int32)
    return torch.from_numpy(dig).cuda(), torch.from_numpy(t1).cuda(), n.cuda()


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(os.path.join(GOLDEN, "g15_dejavu_identify.npz")))


def _queries(g15):
    dig, off = _split(g15["q_dig"], g15["q_n"]), _split(g15["q_off"], g15["q_n"])
    return [list(zip([bytes(x) for x in d], o.tolist())) for d, o in zip(dig, off)]


def _songs(g15):
    return _split(np.arange(len(g15["ins_sid"])), np.bincount(g15["ins_sid"], minlength=len(g15["song_total"]) + 1)[1:])


def _device_db(g15):
    """The reference's ingest: insert_song then insert_hashes for every song, in order."""
    from musicfpaugment_amd.afp.dejavu.database import DeviceDatabase
    db = DeviceDatabase(device="cuda")
    for s, rows in enumerate(_songs(g15)):
        sid = db.insert_song("song_%03d" % s, "%040X" % (s + 1), int(g15["song_total"][s]))
        assert sid == s + 1
        db.insert_hashes(sid, [(bytes(g15["ins_dig"][i]).hex(), int(g15["ins_off"][i])) for i in rows])
        db.set_song_fingerprinted(sid)
    return db


@pytest.fixture(scope="module")
def device_db(g15):
    return _device_db(g15)


def test_store_equals_the_reference_set(device_db, g15):
    want = do.store(g15["fp_dig"], g15["fp_sid"], g15["fp_off"])
    np.testing.assert_array_equal(device_db.table.cpu().numpy(), want)
    assert device_db.get_num_fingerprints() == len(g15["fp_sid"]) and device_db.get_num_songs() == len(g15["song_total"])
    d = device_db.directory.cpu().numpy()
    top = want[:, 0].view(np.uint32) >> (32 - device_db.dirbits)
    np.testing.assert_array_equal(d, np.searchsorted(top, np.arange((1 << device_db.dirbits) + 1), side="left"))


def test_return_matches_equals_the_reference(device_db, g15):
    rm = list(zip(_split(g15["rm_sid"], g15["rm_n"]), _split(g15["rm_diff"], g15["rm_n"])))
    dd = list(zip(_split(g15["dd_sid"], g15["dd_n"]), _split(g15["dd_cnt"], g15["dd_n"])))
    for i, q in enumerate(_queries(g15)):
        res, dedup = device_db.return_matches({(d.hex(), t) for d, t in q})
        assert sorted(res) == list(zip(rm[i][0].tolist(), rm[i][1].tolist())), i
        assert sorted(dedup.items()) == list(zip(dd[i][0].tolist(), dd[i][1].tolist())), i


def test_recognizer_fields_equal_the_reference(device_db, g15):
    """Dejavu.align_matches + FileRecognizer's rule over the device return_matches: every field, the rounded ones included."""
    from musicfpaugment_amd.afp.dejavu.dejavu import MIN_HASHES, Dejavu
    from musicfpaugment_amd.constants import afp_settings
    djv = Dejavu({"database": device_db}, afp_settings["dejavu"], state=None)
    cols = ["song_id", "offset", "input_total_hashes", "fingerprinted_hashes_in_db", "hashes_matched_in_input",
            "nb_matches_with_offset"]
    fcols = ["input_confidence", "input_confidence_2", "fingerprinted_confidence", "offset_seconds"]
    for t in (1, 3):
        ints, floats = _split(g15[f"top{t}_int"], g15[f"top{t}_n"]), _split(g15[f"top{t}_float"], g15[f"top{t}_n"])
        for i, q in enumerate(_queries(g15)):
            hashes = {(d.hex(), o) for d, o in q}
            matches, dedup, _ = djv.find_matches(hashes)
            rows = djv.align_matches(matches, dedup, len(hashes), topn=t)
            assert [[r[c] for c in cols] for r in rows] == ints[i].tolist(), (t, i)
            assert [[r[c] for c in fcols] for r in rows] == floats[i].tolist(), (t, i)
            if t == 1:
                assert (bool(rows) and rows[0]["nb_matches_with_offset"] > MIN_HASHES) == bool(g15["match"][i])


def test_match_batch_equals_the_reference(device_db, g15):
    qs = _queries(g15)
    dig, t1, n = _pad(qs)
    rows, info = device_db.match_batch(dig, t1, n, k=3)
    rows, info = rows.cpu().numpy(), info.cpu().numpy()
    ints = _split(g15["top3_int"], g15["top3_n"])
    rm_n = g15["rm_n"]
    for i in range(len(qs)):
        want = ints[i]
        assert info[i, 0] == rm_n[i] and info[i, 1] == g15["queried"][i] and info[i, 2] == len(want), (i, info[i])
        got = rows[i, : len(want)]
        # [sid, offset, count, hashes_matched]; nb_matches_with_offset is the first row's count on every row
        np.testing.assert_array_equal(got[:, [0, 1, 3]], want[:, [0, 1, 4]], err_msg=str(i))
        if len(want):
            assert (want[:, 5] == got[0, 2]).all()
            assert ((got[0, 2] > 1) == bool(g15["match"][i])), i


def test_hit_capacity_retry_gives_the_same_rows(device_db, g15):
    from musicfpaugment_amd import ops
    dig, t1, n = _pad(_queries(g15))
    want, winfo, _ = ops.dejavu_match(device_db.table, device_db.directory, dig, t1, n, k=3, hcap=1 << 15)
    got, info, hcap = ops.dejavu_match(device_db.table, device_db.directory, dig, t1, n, k=3, hcap=64, scratch_budget=1 << 16)
    assert hcap > 64 and int(winfo[:, 0].max()) > 64
    assert torch.equal(got, want) and torch.equal(info, winfo)


def test_insertion_order_and_batching_give_identical_bytes(device_db, g15):
    from musicfpaugment_amd.afp.dejavu.database import DeviceDatabase
    rng = np.random.default_rng(1)
    db = DeviceDatabase(device="cuda")
    for s in range(len(g15["song_total"])):
        db.insert_song("song_%03d" % s, None, 0)
    perm = rng.permutation(len(g15["ins_sid"]))
    for k, chunk in enumerate(np.array_split(perm, 7)):     # 7 batches in a shuffled order, one flush in the middle
        dig = torch.from_numpy(g15["ins_dig"][chunk][None]).cuda()
        t1 = torch.from_numpy(g15["ins_off"][chunk][None]).cuda()
        for sid in np.unique(g15["ins_sid"][chunk]).tolist():
            sel = g15["ins_sid"][chunk] == sid
            db.insert_batch([sid], dig[:, torch.from_numpy(sel).cuda()], t1[:, torch.from_numpy(sel).cuda()],
                            torch.tensor([int(sel.sum())], dtype=torch.int32))
        if k == 3:
            db.get_num_fingerprints()
    assert torch.equal(db.table, device_db.table) and torch.equal(db.directory, device_db.directory)


def test_save_load_round_trip(device_db, tmp_path):
    from musicfpaugment_amd.afp.dejavu.database import DeviceDatabase
    p = str(tmp_path / "db.npz")
    device_db.save(p)
    db = DeviceDatabase(device="cuda")
    db.load(p)
    assert torch.equal(db.table, device_db.table) and torch.equal(db.directory, device_db.directory)
    assert db.get_songs() == device_db.get_songs()
    assert db.insert_song("next", None, 0) == len(device_db.get_songs()) + 1


def test_setup_empty_and_limits():
    from musicfpaugment_amd import ops
    from musicfpaugment_amd.afp.dejavu.database import DeviceDatabase
    db = DeviceDatabase(device="cuda")
    a = db.insert_song("a", None, 1)
    b = db.insert_song("b", None, 1)
    db.insert_hashes(a, [("00" * 10, 5)])
    db.insert_hashes(b, [("00" * 10, 7), ("11" * 10, 3)])
    db.set_song_fingerprinted(a)
    db.setup()                                               # b was never marked fingerprinted: it goes, with its rows
    assert db.get_num_fingerprints() == 1 and [s["song_id"] for s in db.get_songs()] == [a]
    assert db.insert_song("c", None, 0) == 3                 # SERIAL does not reuse ids
    db.empty()
    assert db.insert_song("d", None, 0) == 1 and db.get_num_fingerprints() == 0
    with pytest.raises(ValueError, match="not in the songs table"):
        db.insert_hashes(9, [("00" * 10, 1)])
    db._next_sid = ops.DEJAVU_MAX_SID + 1
    with pytest.raises(ValueError, match=str(ops.DEJAVU_MAX_SID)):
        db.insert_song("e", None, 0)
    for name in ("query", "get_iterable_kv_pairs"):
        with pytest.raises(NotImplementedError):
            getattr(db, name)()


# ----------------------------------------------------------------------------- end to end
N_TRACKS = 40
Q_LEN = 64000


@pytest.fixture(scope="module")
def e2e():
    """40 synthetic tracks of unequal lengths (10 to 30 s) in a database; 8-s excerpts starting on 256-sample boundaries,
    clean and with noise added on the device."""
    from musicfpaugment_amd.afp.dejavu.dejavu import Dejavu
    from musicfpaugment_amd.constants import afp_settings
    from musicfpaugment_amd.testing.dejavu_exps import create_fp_database_batch
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    lengths = [80000, 120000, 160000, 200000, 240000, 100352, 150016, 230400]
    tracks = [synth.track(1700 + i, lengths[i % len(lengths)]) for i in range(N_TRACKS)]
    names = ["trk%02d" % i for i in range(N_TRACKS)]
    db = create_fp_database_batch(tracks, names, batch=3)
    rng = np.random.default_rng(7)
    owner, start = [], []
    for _ in range(24):
        o = int(rng.integers(0, N_TRACKS))
        owner.append(o)
        start.append(256 * int(rng.integers(0, (len(tracks[o]) - Q_LEN) // 256 + 1)))
    clean = torch.from_numpy(np.stack([tracks[o][s:s + Q_LEN] for o, s in zip(owner, start)]))
    g = torch.Generator(device="cuda").manual_seed(3)
    aug = (clean.cuda() + 0.2 * torch.randn(clean.shape, generator=g, device="cuda")).contiguous()
    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    djv1 = Dejavu({"database": db}, afp_settings["dejavu"])
    djv2 = Dejavu({"database": db}, afp_settings["dejavu"], denoising=True, denoising_model="unet", unet=net.cuda().eval())
    return dict(db=db, tracks=tracks, names=names, owner=owner, start=start, clean=clean, aug=aug, djv1=djv1, djv2=djv2)


def test_identification_end_to_end_equals_the_oracle(e2e):
    from musicfpaugment_amd.testing.dejavu_exps import _clip_hashes, compute_accuracy_batch
    db, djv1, djv2 = e2e["db"], e2e["djv1"], e2e["djv2"]
    idx = do.index(db.table.cpu().numpy())
    assert db.get_num_songs() == N_TRACKS
    assert [s["total_hashes"] for s in db.get_songs()] == db.count_fingerprints(range(1, N_TRACKS + 1))
    gt = [o + 1 for o in e2e["owner"]]
    for key in ("clean", "aug"):
        wav = e2e[key].cuda()
        res, rows = compute_accuracy_batch(wav, gt, db, djv1, djv2, batch=10, per_query=True)
        rows = rows.cpu().numpy()
        for col, djv in ((0, djv1), (2, djv2)):
            dig, t1, n = (x.cpu().numpy() for x in _clip_hashes(djv, wav, key))
            for i in range(wav.shape[0]):
                pairs = [(bytes(dig[i, j]), int(t1[i, j])) for j in range(n[i])]
                want, _, match = do.recognize(idx, pairs)
                exp = (want[0][0], want[0][2]) if match else (-1, 0)
                assert (rows[i, col], rows[i, col + 1]) == exp, (key, col, i)
        if key == "clean":
            # each clean excerpt identifies its track at the excerpt's frame offset: the STFT frames of an excerpt starting
            # on a 256-sample boundary are frames of the track
            dig, t1, n = _clip_hashes(djv1, wav, key)
            top, info = db.match_batch(dig, t1, n, k=1)
            top, info = top.cpu().numpy(), info.cpu().numpy()
            detail = [(g, s // 256, top[i, 0].tolist(), info[i].tolist()) for i, (g, s) in enumerate(zip(gt, e2e["start"]))]
            assert top[:, 0, 0].tolist() == gt, detail
            assert top[:, 0, 1].tolist() == [s // 256 for s in e2e["start"]], detail
            assert res["No Denoising"] == 1.0, res
        assert 0.0 <= res["Mix Pipeline"] <= 1.0


def test_file_based_experiment_equals_the_batched_one(e2e, tmp_path):
    from scipy.io import wavfile

    from musicfpaugment_amd.afp.dejavu.dejavu import Dejavu
    from musicfpaugment_amd.constants import afp_settings
    from musicfpaugment_amd.testing.dejavu_exps import compute_accuracy, compute_accuracy_batch, create_fp_database
    files = []
    for name, t in list(zip(e2e["names"], e2e["tracks"]))[:12]:
        p = str(tmp_path / (name + ".wav"))
        wavfile.write(p, 8000, t.astype(np.float32))
        files.append(p)
    db_f = create_fp_database(files + files[:2])             # files already known by their SHA-1 are skipped
    assert db_f.get_num_songs() == 12
    sel = [i for i, o in enumerate(e2e["owner"]) if o < 12][:8]
    qfiles = []
    for i in sel:
        sub = tmp_path / "q" / e2e["names"][e2e["owner"][i]]
        sub.mkdir(parents=True, exist_ok=True)
        p = str(sub / ("%d.wav" % i))
        wavfile.write(p, 8000, e2e["aug"][i].cpu().numpy().astype(np.float32))
        qfiles.append(p)
    djv1 = Dejavu({"database": db_f}, afp_settings["dejavu"])
    djv2 = Dejavu({"database": db_f}, afp_settings["dejavu"], denoising=True, denoising_model="unet", unet=e2e["djv2"].unet)
    got = compute_accuracy(qfiles, djv1, djv2)
    want = compute_accuracy_batch(e2e["aug"][sel], [e2e["owner"][i] + 1 for i in sel], db_f, djv1, djv2)
    assert got == want, (got, want)
    # the file-based database equals the batched one over the same tracks
    from musicfpaugment_amd.testing.dejavu_exps import create_fp_database_batch
    db_b = create_fp_database_batch(e2e["tracks"][:12], e2e["names"][:12])
    assert torch.equal(db_b.table, db_f.table)
    assert [s["total_hashes"] for s in db_b.get_songs()] == [s["total_hashes"] for s in db_f.get_songs()]


def test_two_ranks_equal_one():
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("_dist_dejavu_worker", os.path.join(ROOT, "tests", "_dist_dejavu_worker.py"))
    worker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(worker)
    want_res, want_rows = worker.run()
    with tempfile.TemporaryDirectory() as tmp:
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--standalone", "--local-addr",
               "127.0.0.1", os.path.join(ROOT, "tests", "_dist_dejavu_worker.py"), tmp]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        got = json.load(open(os.path.join(tmp, "dejavu.json")))
    assert got["rows"] == want_rows and got["res"] == want_res
