"""GPU: the matcher's extended modes (mfpa_audfprint_match_ex: exact_count, find_time_range, hashesfor) against the
reference's goldens (g15) and the test oracle (tests/_identify_exact_oracle.py), on g14's table plus g15's four tracks."""
import os

import numpy as np
import pytest
import torch

from musicfpaugment_amd import synth
from tests import _identify_exact_oracle as xo
from tests import _identify_oracle as io_

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
COMBOS = {"ft": (False, True), "tf": (True, False), "tt": (True, True)}
K = 512


def _split(rows, off):
    return [rows[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _pad(lists):
    cap = max(1, max(len(x) for x in lists))
    uq = np.zeros((len(lists), cap, 2), np.int32)
    for i, x in enumerate(lists):
        uq[i, :len(x)] = x
    return torch.from_numpy(uq).cuda(), torch.tensor([len(x) for x in lists], dtype=torch.int32).cuda()


def _matcher(exact=False, trange=False, thresh=5, quantile=0.05):
    from musicfpaugment_amd.afp.audfprint.audfprint_match import Matcher
    m = Matcher()
    m.exact_count, m.find_time_range, m.threshcount, m.time_quantile = exact, trange, thresh, quantile
    return m


@pytest.fixture(scope="module")
def g15():
    return dict(np.load(os.path.join(GOLDEN, "g15_identify_exact.npz")))


@pytest.fixture(scope="module")
def tracks(g15):
    g14 = np.load(os.path.join(GOLDEN, "g14_identify.npz"))
    return _split(g14["track_rows"], g14["track_off"]) + _split(g15["extra_track_rows"], g15["extra_track_off"])


@pytest.fixture(scope="module")
def queries(g15):
    return _split(g15["query_rows"], g15["query_off"])


@pytest.fixture(scope="module")
def device_db(tracks):
    from musicfpaugment_amd.afp.audfprint.hash_table import HashTable
    ht = HashTable(device="cuda")
    uq, n = _pad(tracks)
    ht.store_batch(["track_%03d" % i for i in range(len(tracks))], uq, n)
    return ht


@pytest.fixture(scope="module")
def oracle_db(tracks, g15):
    table, counts = io_.empty_table()
    for i, tr in enumerate(tracks):
        io_.store(table, counts, tr, i)
    return table, counts, g15["hashesperid"]


@pytest.fixture(scope="module")
def ties(oracle_db, queries):
    return [xo.rank_ties(*oracle_db, q) for q in queries]


@pytest.fixture(scope="module")
def batched(device_db, queries):
    """One call per combination holding every query (the empty one and the no-hit one among them)."""
    uq, n = _pad(queries)
    out = {}
    for key, (ex, tr) in COMBOS.items():
        rows, info = _matcher(ex, tr).match_batch(device_db, uq, n, k=K)
        out[key] = rows.cpu().numpy(), info.cpu().numpy()
    return out


def test_table_is_the_goldens(device_db, oracle_db, g15):
    np.testing.assert_array_equal(device_db.table.cpu().numpy().view(np.uint32), oracle_db[0])
    np.testing.assert_array_equal(device_db.hashesperid, g15["hashesperid"])


@pytest.mark.parametrize("key", list(COMBOS))
def test_batched_rows_equal_the_reference(batched, oracle_db, queries, ties, g15, key):
    ex, tr = COMBOS[key]
    rows, info = batched[key]
    assert any(len(q) == 0 for q in queries)
    for qi, (q, want) in enumerate(zip(queries, _split(g15["rows_" + key], g15["off_" + key]))):
        assert info[qi, 1] == info[qi, 2] == len(want) <= K, (qi, info[qi].tolist(), len(want))
        got = rows[qi, :len(want)]
        err = xo.rows_equivalent(got, want, ties[qi])                # columns 5-6 are part of the row wherever it is determined
        assert err is None, f"{key} query {qi}: {err}"
        if len(q):                                                   # the device's tie order is the oracle's
            np.testing.assert_array_equal(got, xo.match(*oracle_db, q, exact_count=ex, find_time_range=tr)[0], err_msg=f"{key} {qi}")
        if not tr:
            assert not got[:, 5:].any()
    no_rows = [qi for qi, q in enumerate(queries) if len(q) and info[qi, 2] == 0]
    assert no_rows                                                   # a query with hashes and no result row


@pytest.mark.parametrize("key", list(COMBOS))
def test_one_by_one_equals_batched(batched, device_db, queries, key):
    rows, info = batched[key]
    m = _matcher(*COMBOS[key])
    for qi, q in enumerate(queries):
        got, hf = m.match_hashes(device_db, q)
        assert hf is None
        np.testing.assert_array_equal(got, rows[qi, :info[qi, 2]], err_msg=f"{key} query {qi}")


def test_k_below_the_total_reports_the_total(batched, device_db, queries):
    uq, n = _pad(queries)
    for key in COMBOS:
        rows, info = batched[key]
        top, info1 = _matcher(*COMBOS[key]).match_batch(device_db, uq, n, k=2)
        top, info1 = top.cpu().numpy(), info1.cpu().numpy()
        assert int(info[:, 2].max()) > 2
        np.testing.assert_array_equal(info1[:, 2], info[:, 2])
        np.testing.assert_array_equal(info1[:, 1], np.minimum(info[:, 2], 2))
        for qi in range(len(queries)):
            np.testing.assert_array_equal(top[qi, :info1[qi, 1]], rows[qi, :info1[qi, 1]])


def test_hit_capacity_retry_gives_the_same_rows(batched, device_db, queries):
    uq, n = _pad(queries)
    m = _matcher(True, True)
    m.hit_capacity = 64                                              # most queries exceed it: reported, then run again
    rows, info = m.match_batch(device_db, uq, n, k=K)
    assert m.hit_capacity > 64
    np.testing.assert_array_equal(rows.cpu().numpy(), batched["tt"][0])
    np.testing.assert_array_equal(info.cpu().numpy(), batched["tt"][1])
    assert int(info[:, 0].max()) > 4096                              # a query on the global-memory sort path


def test_hash_lists_equal_the_reference(device_db, oracle_db, queries, g15):
    lists = _split(g15["hf_rows"], g15["hf_off"])
    for (qi, ex, k), want in zip(g15["hf_spec"].tolist(), lists):
        rows, got = _matcher(bool(ex)).match_hashes(device_db, queries[qi], hashesfor=k)
        assert got.shape[1] == 2
        np.testing.assert_array_equal(got, want, err_msg=f"query {qi} exact {ex} row {k}")
        np.testing.assert_array_equal(rows, xo.match(*oracle_db, queries[qi], exact_count=bool(ex))[0])
    with pytest.raises(IndexError):
        _matcher(True).match_hashes(device_db, queries[0], hashesfor=10 ** 6)
    with pytest.raises(IndexError):
        _matcher().match_hashes(device_db, np.zeros((0, 2), np.int32), hashesfor=0)


def test_hash_lists_of_a_batch_and_buffer_growth(device_db, oracle_db, queries):
    """hashesfor through match_batch: every query's list of row 1 in one call, -1 where there is no such row; a buffer of 4
    rows is too small for most lists, which is reported and the call repeated with room."""
    from musicfpaugment_amd import ops
    uq, n = _pad(queries)
    m = _matcher(True, True)
    rows, info, hf, hf_n = m.match_batch(device_db, uq, n, k=K, hashesfor=1)
    hf, hf_n, info = hf.cpu().numpy(), hf_n.cpu().numpy(), info.cpu().numpy()
    small = ops.audfprint_match(device_db.table, device_db.counts, device_db.hashesperid_device(), uq, n, k=K, exact_count=True,
                                find_time_range=True, hashesfor=1, hashes_cap=4, timebits=device_db.maxtimebits)
    assert int(hf_n.max()) > 4 and torch.equal(small[4].cpu(), torch.from_numpy(hf_n))
    np.testing.assert_array_equal(small[3].cpu().numpy(), hf)
    np.testing.assert_array_equal(small[0].cpu().numpy(), rows.cpu().numpy())
    assert (hf_n[info[:, 2] < 2] == -1).all() and (hf_n[info[:, 2] >= 2] > 0).all() and (info[:, 2] < 2).any()
    for qi, q in enumerate(queries):
        if hf_n[qi] >= 0:
            want = xo.match(*oracle_db, q, exact_count=True, find_time_range=True, hashesfor=1)[1]
            np.testing.assert_array_equal(hf[qi, :hf_n[qi]], want, err_msg=f"query {qi}")


@pytest.mark.parametrize("key", list(COMBOS))
def test_threshcount_one(device_db, oracle_db, queries, ties, g15, key):
    ex, tr = COMBOS[key]
    m = _matcher(ex, tr, thresh=1)
    for qi, want in zip(g15["t1_queries"].tolist(), _split(g15["t1_rows_" + key], g15["t1_off_" + key])):
        got, _ = m.match_hashes(device_db, queries[qi])
        err = xo.rows_equivalent(got, want, ties[qi])
        assert err is None, f"{key} query {qi}: {err}"
        if len(queries[qi]):
            np.testing.assert_array_equal(got, xo.match(*oracle_db, queries[qi], threshcount=1, exact_count=ex, find_time_range=tr)[0])


@pytest.mark.parametrize("tag,quantile", [("q0", 0.0), ("q25", 0.25)])
def test_other_quantiles(device_db, queries, ties, g15, tag, quantile):
    for key in ("ft", "tt"):
        m = _matcher(COMBOS[key][0], True, quantile=quantile)
        for qi, want in zip(g15["quantile_queries"].tolist(), _split(g15[f"{tag}_rows_{key}"], g15[f"{tag}_off_{key}"])):
            got, _ = m.match_hashes(device_db, queries[qi])
            err = xo.rows_equivalent(got, want, ties[qi])
            assert err is None, f"{tag} {key} query {qi}: {err}"


def test_default_flags_through_the_new_entry_point_are_bitwise_the_default(device_db, queries):
    from musicfpaugment_amd import ops
    uq, n = _pad(queries)
    args = (device_db.table, device_db.counts, device_db.hashesperid_device(), uq, n)
    for k, hcap in ((K, 1 << 15), (1, 64)):
        old = ops.audfprint_match(*args, k=k, hcap=hcap, timebits=device_db.maxtimebits, extended=False)
        new = ops.audfprint_match(*args, k=k, hcap=hcap, timebits=device_db.maxtimebits, extended=True)
        assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1]) and old[2] == new[2]
        assert int(old[1][:, 2].max()) > 100


def test_host_checks(device_db, queries):
    with pytest.raises(ValueError, match="threshcount"):
        _matcher(True, thresh=0).match_hashes(device_db, queries[0])
    with pytest.raises(ValueError, match="time_quantile"):
        _matcher(False, True, quantile=1.0).match_hashes(device_db, queries[0])
    rows, _ = _matcher(False, True, thresh=0).match_hashes(device_db, queries[0])       # threshcount 0 without exact_count is fine
    assert len(rows)


def test_identification_with_exact_counts_names_the_same_tracks():
    """compute_accuracy_batch with an exact matcher: the identities of the default matcher (the counts may differ)."""
    from musicfpaugment_amd.afp.audfprint.peak_extractor import Audfprint_peaks
    from musicfpaugment_amd.testing.audfprint_exps import compute_accuracy_batch, create_fp_database_batch
    from musicfpaugment_amd.training.unet import UNet
    from musicfpaugment_amd.training.weights import formula_state_dict
    long_ = synth.batch(8, seed=1410, n=240000)
    short = synth.batch(4, seed=1420, n=160000)
    tracks = [long_[0], short[0], long_[1], long_[2], short[1], long_[3], long_[4], short[2], long_[5], long_[6], short[3], long_[7]]
    ht = create_fp_database_batch(tracks, ["trk%02d" % i for i in range(len(tracks))], batch=5)
    rng = np.random.default_rng(5)
    owner, q = [], []
    for i in range(8):
        o = int(rng.integers(0, len(tracks)))
        start = 256 * int(rng.integers(0, (len(tracks[o]) - 64000) // 256))
        if i % 2:
            start = min(start + int(rng.integers(1, 256)), len(tracks[o]) - 64000)
        owner.append(o)
        q.append(tracks[o][start:start + 64000])
    wav = torch.from_numpy(np.stack(q))
    net = UNet(1, 1)
    net.load_state_dict(formula_state_dict(0))
    an1 = Audfprint_peaks(None)
    an2 = Audfprint_peaks(None, denoising=True, denoising_model="unet", unet=net.cuda().eval())
    an1.shifts = an2.shifts = 4
    res0, rows0 = compute_accuracy_batch(wav, owner, ht, an1, an2, per_query=True)
    m = _matcher(True, True)
    res1, rows1 = compute_accuracy_batch(wav, owner, ht, an1, an2, per_query=True, matcher=m)
    assert torch.equal(rows0[:, [0, 2]], rows1[:, [0, 2]]) and res0["No Denoising"] == res1["No Denoising"] == 1.0
    assert (rows1[:, 1] > 0).all()
