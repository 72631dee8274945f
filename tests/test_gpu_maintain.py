"""GPU: HashTable.remove / retrieve on the device (audfprint_maintain.hip) against the reference's results
(tests/golden/g18_maintain.npz, bit for bit) and the test oracle (tests/_maintain_oracle.py), the matcher on a maintained
table, save / load after a removal, and DeviceDatabase.delete_songs_by_id."""
import hashlib

import numpy as np
import pytest
import torch

from tests import _identify_oracle as io_
from tests import _maintain_oracle as mo

pytestmark = pytest.mark.gpu


def _sha(a, dt):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, dt).tobytes()).digest(), np.uint8)


def _table(ht):
    return ht.table.cpu().numpy().view(np.uint32)


def _tiny(case, after=False):
    """A HashTable over the fixture's table, uploaded straight into ht.table and ht.counts."""
    from musicfpaugment_amd.afp.audfprint.hash_table import HT_VERSION, HashTable
    hashbits, depth, timebits, n_ids = (int(v) for v in case["shape"])
    s = "1" if after else "0"
    ht = HashTable.__new__(HashTable)
    ht.device, ht.seed, ht._hpid_dev = torch.device("cuda"), 0, None
    ht.hashbits, ht.depth, ht.maxtimebits = hashbits, depth, timebits
    ht.table = torch.from_numpy(case["table" + s].view(np.int32).copy()).cuda()
    ht.counts = torch.from_numpy(case["counts" + s].copy()).cuda()
    ht.names = [str(n) for n in case["names0"]]
    if after:
        ht.names = [None if gone else n for n, gone in zip(ht.names, case["names1_none"])]
    ht.hashesperid = case["hpid" + s].copy()
    ht.ht_version, ht.dirty = HT_VERSION, False
    return ht


@pytest.fixture(scope="module", params=range(len(mo.CASES)), ids=lambda i: "h%d_d%d_t%d" % mo.CASES[i])
def case(request):
    return mo.load_case(request.param)


def _split(rows, off):
    return [rows[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_remove_one_by_one_equals_the_reference(case, capsys):
    ht = _tiny(case)
    n_ids = int(case["shape"][3])
    for k, (id_, by_int) in enumerate(zip(case["order"].tolist(), case["by_int"].tolist())):
        name = id_ if by_int else ht.names[id_]
        ht.dirty, ht._hpid_dev = False, "stale"
        capsys.readouterr()
        assert ht.remove(name) is None
        assert capsys.readouterr().out == "Removed %s ( %d hashes).\n" % (name, int(case["printed"][k]))
        assert ht.dirty is True and ht._hpid_dev is None and ht.names[id_] is None and ht.hashesperid[id_] == 0
        np.testing.assert_array_equal(_sha(_table(ht), "<u4"), case["step_table_sha256"][k], err_msg=str(k))
        np.testing.assert_array_equal(_sha(ht.counts.cpu().numpy(), "<i4"), case["step_counts_sha256"][k], err_msg=str(k))
    np.testing.assert_array_equal(_table(ht), case["table1"])
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), case["counts1"])
    assert [n is None for n in ht.names] == case["names1_none"].tolist() and len(ht.names) == n_ids
    assert [n for n in ht.names if n is not None] == [str(n) for n in case["names1"] if str(n)]
    np.testing.assert_array_equal(ht.hashesperid, case["hpid1"])
    assert ht.hashesperid.dtype == np.uint32


@pytest.mark.parametrize("full_rows", [False, True], ids=["prefix", "full_rows"])
def test_remove_batch_of_the_set_equals_the_per_id_removes(case, capsys, full_rows):
    from musicfpaugment_amd import ops
    order = case["order"].tolist()
    if full_rows:                                                   # the other read shape, through the op
        ht = _tiny(case)
        timebits, n_ids = int(case["shape"][2]), int(case["shape"][3])
        removed = ops.audfprint_remove(ht.table, ht.counts, order, n_ids, timebits, full_rows=True).cpu().numpy()
        assert removed[order].tolist() == case["printed"].tolist() and removed.sum() == case["printed"].sum()
    else:
        ht = _tiny(case)
        names = [ht.names[i] for i in order[::-1]]
        assert ht.remove_batch(names) == case["printed"].tolist()[::-1]
        assert capsys.readouterr().out == "".join("Removed %s ( %d hashes).\n" % (n, c)
                                                  for n, c in zip(names, case["printed"].tolist()[::-1]))
        assert [n is None for n in ht.names] == case["names1_none"].tolist()
        np.testing.assert_array_equal(ht.hashesperid, case["hpid1"])
    np.testing.assert_array_equal(_table(ht), case["table1"])
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), case["counts1"])


def test_empty_set_unknown_name_and_removed_id(case, capsys):
    from musicfpaugment_amd import ops
    ht = _tiny(case)
    timebits, n_ids = int(case["shape"][2]), int(case["shape"][3])
    assert ht.remove_batch([]) == []
    assert not ops.audfprint_remove(ht.table, ht.counts, [], n_ids, timebits).any()
    np.testing.assert_array_equal(_table(ht), case["table0"])          # the empty set: every byte as it was
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), case["counts0"])
    with pytest.raises(ValueError, match="not found"):
        ht.remove("no such track")
    with pytest.raises(ValueError, match="not found"):
        ht.retrieve("no such track")
    with pytest.raises(IndexError):
        ht.remove(n_ids)
    np.testing.assert_array_equal(_table(ht), case["table0"])
    id_ = int(case["order"][0])
    ht.remove(id_)
    t, c = _table(ht), ht.counts.cpu().numpy()
    capsys.readouterr()
    ht.remove(id_)                                                    # an integer id that is already gone: nothing to remove
    assert capsys.readouterr().out == "Removed %d ( 0 hashes).\n" % id_
    np.testing.assert_array_equal(_table(ht), t)
    np.testing.assert_array_equal(ht.counts.cpu().numpy(), c)
    assert len(ht.retrieve(id_)) == 0


@pytest.mark.parametrize("after", [False, True], ids=["before", "after"])
def test_retrieve_equals_the_reference(case, after):
    from musicfpaugment_amd import ops
    ht = _tiny(case, after)
    n_ids, timebits = int(case["shape"][3]), int(case["shape"][2])
    s = "1" if after else "0"
    rows, off = case["ret" + s + "_rows"], case["ret" + s + "_off"]
    # every id in one batch, on the device
    got, goff = ht.retrieve_batch(list(range(n_ids)), on_device=True)
    assert got.dtype == torch.int32 and goff.dtype == torch.int32 and got.is_cuda
    np.testing.assert_array_equal(goff.cpu().numpy(), off)
    np.testing.assert_array_equal(got.cpu().numpy(), rows)
    # a permuted request with names, integer ids and a repeat; the single form
    want = _split(rows, off)
    ask = [n_ids - 1, 3, 0, n_ids // 2, 3, 1]
    names = [i if (k % 2 or ht.names[i] is None) else ht.names[i] for k, i in enumerate(ask)]
    for g, i in zip(ht.retrieve_batch(names), ask):
        assert g.dtype == np.int32 and g.shape == (len(want[i]), 2)
        np.testing.assert_array_equal(g, want[i])
    one = ht.retrieve(names[1])
    assert isinstance(one, np.ndarray) and one.dtype == np.int32
    np.testing.assert_array_equal(one, want[3])
    # the other read shape and determinism: the same bytes again
    r2, o2 = ops.audfprint_retrieve(ht.table, ht.counts, ask[:4], timebits, full_rows=True)
    r3, o3 = ops.audfprint_retrieve(ht.table, ht.counts, ask[:4], timebits)
    assert torch.equal(r2, r3) and torch.equal(o2, o3)
    np.testing.assert_array_equal(r2.cpu().numpy(), np.concatenate([want[i] for i in ask[:4]]))
    with pytest.raises(ValueError, match="distinct"):
        ops.audfprint_retrieve(ht.table, ht.counts, [1, 1], timebits)
    e_rows, e_off = ops.audfprint_retrieve(ht.table, ht.counts, [], timebits)
    assert e_rows.shape == (0, 2) and e_off.tolist() == [0]


def test_store_retrieve_remove_and_reuse_of_the_id_on_the_full_size_table():
    """The product table (2^20 x 100, 14 time bits), no overflow: store -> retrieve round trip, remove, the freed id."""
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    rng = np.random.default_rng(5)
    ht = HashTable(device="cuda")
    tracks = []
    for i in range(6):
        n = 700 + 13 * i
        t = rng.integers(0, 60000, n)                                      # times above the 14-bit mask
        h = rng.integers(0, 1 << 24, n)                                    # hashes above the 20-bit mask
        h[:40] = (1 << 20) - 1 - (np.arange(40) % 5)                       # shared buckets, the last one included
        h[40:45] = 0
        tracks.append(np.stack([t, h], 1).astype(np.int32))
        ht.store("t%d" % i, tracks[-1])
    assert int(ht.counts.max()) <= ht.depth

    def expect(tr):
        t, b = tr[:, 0].astype(np.int64) & 16383, tr[:, 1].astype(np.int64) & ((1 << 20) - 1)
        o = np.argsort(b, kind="stable")                                   # bucket ascending, then arrival
        return np.stack([t[o], b[o]], 1).astype(np.int32)

    for i in (0, 3, 5):
        np.testing.assert_array_equal(ht.retrieve("t%d" % i), expect(tracks[i]))
    # the oracle on the buckets that hold anything (the rest of the table stays empty)
    used = torch.nonzero(ht.counts).flatten()
    tab, cnt = ht.table[used].cpu().numpy().view(np.uint32).copy(), ht.counts[used].cpu().numpy().copy()
    total = int(torch.count_nonzero(ht.table))
    want_removed = mo.remove(tab, cnt, [1, 4], 6, 14)
    assert ht.remove_batch(["t4", "t1"]) == [len(tracks[4]), len(tracks[1])] == want_removed[[4, 1]].tolist()
    np.testing.assert_array_equal(ht.table[used].cpu().numpy().view(np.uint32), tab)
    np.testing.assert_array_equal(ht.counts[used].cpu().numpy(), cnt)
    assert int(torch.count_nonzero(ht.table)) == total - len(tracks[4]) - len(tracks[1]) == int(ht.counts.sum())
    assert ht.names == ["t0", None, "t2", "t3", None, "t5"] and ht.hashesperid.tolist()[1] == 0
    assert len(ht.retrieve(1)) == 0 and len(ht.retrieve(4)) == 0
    for i in (0, 2, 3, 5):                                                 # the others keep every row, in order
        np.testing.assert_array_equal(ht.retrieve(i), expect(tracks[i]))
    new = np.stack([rng.integers(0, 16384, 300), rng.integers(0, 1 << 20, 300)], 1).astype(np.int32)
    new[:10, 1] = (1 << 20) - 1
    ht.store("fresh", new)
    assert ht.names.index("fresh") == 1 and ht.hashesperid[1] == 300       # names.index(None): the freed id
    np.testing.assert_array_equal(ht.retrieve("fresh"), expect(new))
    rows, off = ht.retrieve_batch(["t5", "fresh", "t0"], on_device=True)
    np.testing.assert_array_equal(rows.cpu().numpy(), np.concatenate([expect(tracks[5]), expect(new), expect(tracks[0])]))
    assert off.tolist() == [0, len(tracks[5]), len(tracks[5]) + 300, len(tracks[5]) + 300 + len(tracks[0])]


def test_matcher_on_the_maintained_table_equals_the_oracle_on_the_after_table():
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    case = mo.load_case(1)                                                    # hashbits 8, depth 100
    timebits = int(case["shape"][2])
    ht = _tiny(case)
    order = case["order"].tolist()
    ht.remove_batch(order)
    before = _split(case["ret0_rows"], case["ret0_off"])
    gone, kept = order[2], 3                                               # id 0 (removed), id 3 (kept)
    after = (case["table1"], case["counts1"], case["hpid1"])
    m = Matcher()
    for id_, shift in ((gone, 11), (kept, 11), (kept, -40), (order[4], 0)):
        q = before[id_][::2].astype(np.int64).copy()
        assert len(q) > 10
        q[:, 0] -= shift
        q = q.astype(np.int32)
        got, _ = m.match_hashes(ht, q)
        want = io_.match(*after, q, timebits=timebits)
        err = io_.rows_equivalent(got, want, io_.rank_ties(*after, q, timebits=timebits))
        assert err is None, (id_, shift, err)
        assert not np.isin(np.asarray(got).reshape(-1, 7)[:, 0], order).any()       # a removed id never appears
        if id_ == kept:
            assert len(got) and got[0][0] == kept and got[0][2] == shift and got[0][1] >= len(q) // 2


def test_save_after_a_remove_and_load(case, tmp_path):
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    ht = _tiny(case)
    ht.remove_batch(case["order"].tolist())
    p = str(tmp_path / "maintained.pklz")
    ht.save(p)
    assert ht.dirty is False
    back = HashTable(p, device="cuda")
    assert torch.equal(back.table, ht.table) and torch.equal(back.counts, ht.counts)
    assert back.names == ht.names and None in back.names
    np.testing.assert_array_equal(back.hashesperid, ht.hashesperid)
    np.testing.assert_array_equal(_table(back), case["table1"])
    assert (back.hashbits, back.depth, back.maxtimebits) == tuple(int(v) for v in case["shape"][:3])


def test_dejavu_delete_songs_by_id():
    from musicfpaugment_amd.afp.dejavu.database import DeviceDatabase
    rng = np.random.default_rng(9)
    shared = [rng.integers(0, 256, 10, dtype=np.uint8).tobytes().hex() for _ in range(30)]
    songs = []
    for s in range(6):
        own = [(rng.integers(0, 256, 10, dtype=np.uint8).tobytes().hex(), int(o)) for o in rng.integers(0, 5000, 80)]
        songs.append(own + [(h, 100 * s + 3 * k) for k, h in enumerate(shared)])

    def build(skip=()):
        db = DeviceDatabase(device="cuda")
        for s, rows in enumerate(songs):
            sid = db.insert_song("song%d" % s, "%040X" % s, len(rows))
            if sid not in skip:
                db.insert_hashes(sid, rows)
                db.set_song_fingerprinted(sid)
        db.setup()                                                         # the songs never fingerprinted go (none without skip)
        return db

    gone = [2, 5]
    db, ref = build(), build(skip=gone)
    assert db.get_num_songs() == 6
    db.delete_songs_by_id(gone + [77, 0])                                  # unknown ids are ignored, as by SQL's IN
    assert torch.equal(db.table, ref.table) and torch.equal(db.directory, ref.directory)
    assert db.get_num_fingerprints() == ref.get_num_fingerprints() == sum(len(set(r)) for s, r in enumerate(songs) if s + 1 not in gone)
    assert db.get_songs() == ref.get_songs() and db.get_num_songs() == 4
    assert db.get_song_by_id(2) is None and db.get_song_by_id(3) == ref.get_song_by_id(3)
    assert db.count_fingerprints([1, 2, 3, 5, 6]) == ref.count_fingerprints([1, 2, 3, 5, 6])
    assert db.count_fingerprints([2, 5]) == [0, 0]
    cap = max(len(r) for r in songs)
    dig = np.zeros((len(songs), cap, 10), np.uint8)
    t1 = np.zeros((len(songs), cap), np.int32)
    for s, rows in enumerate(songs):                                       # every song as a query, the deleted ones included
        for j, (h, o) in enumerate(rows):
            dig[s, j] = np.frombuffer(bytes.fromhex(h), np.uint8)
            t1[s, j] = o + 7
    n = torch.tensor([len(r) for r in songs], dtype=torch.int32).cuda()
    got = db.match_batch(torch.from_numpy(dig).cuda(), torch.from_numpy(t1).cuda(), n, k=3)
    want = ref.match_batch(torch.from_numpy(dig).cuda(), torch.from_numpy(t1).cuda(), n, k=3)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    rows = got[0].cpu().numpy()
    assert not np.isin(rows[:, :, 0], gone).any() and rows[0, 0, 0] == 1
    assert db.insert_song("later", None, 0) == 7                           # SERIAL: a deleted id is not handed out again
    db.delete_songs_by_id([])
    db.delete_songs_by_id([7], batch_size=1)
    assert db.insert_song("again", None, 0) == 8 and torch.equal(db.table, ref.table)
    for name in ("query", "get_iterable_kv_pairs"):
        with pytest.raises(NotImplementedError):
            getattr(db, name)()
