"""DG_INDEX_HNSW on the GPU: k_hnsw_search against the Python model of the
reference search (tests/hnsw_reference.py) run over the graph that
Index.hnsw_export reads back from the device.

L2 and IP run on integer data (components in [-3, 3], d <= 200), where every
partial sum is exact in float32: ids, distances and both counters must equal
the model's exactly, whatever order the kernel sums in.  Cosine cannot be
exact: its scores are compared with a float64 dot of the normalised query and
the reconstructed rows within 4 * d * 2^-24 (a loose f32 summation bound for
O(1) scores, the form DESIGN.md §Flat exact path derives), and its recall@10
at ef = 64 must reach 0.9 (an answer counts if its score is >= the exact 10th
score).
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import hnsw_reference as hr  # noqa: E402

pytestmark = pytest.mark.gpu

N = 2000
NQ = 70
EFC = 40
CASES = [(1, 1), (10, 10), (10, 300), (100, 10)]
# d and M vary independently around (16, 16); M = 48 gives maxM0 = 96, more
# than one wave of neighbours; d = 17 is padded to 20, d = 200 is 50 float4
# per row (a partly filled wave), d = 16 four
SHAPES = [(16, 16), (17, 16), (200, 16), (16, 4), (16, 48)]
EINVAL, ENOT_SUPPORT, EINTERNAL, EIO, EDUP, ENOT_FOUND = 1, 3, 5, 6, 8, 9


def dg():
    import dingostore
    return dingostore


def ints(n, d, seed):
    return np.random.default_rng(seed).integers(-3, 4, (n, d)).astype(
        np.float32)


class Harness:
    """An HNSW index plus the rows in node order (deleted nodes included),
    which the model needs and the library does not hand out."""

    def __init__(self, metric, d, m, efc=EFC):
        self.metric, self.d = metric, d
        self.ix = dg().Index(dg().HNSW, metric, d)
        self.ix.hnsw_configure(m, efc, 100)
        self.rows = np.zeros((0, d), np.float32)

    def add(self, ids, x, upsert=False):
        (self.ix.upsert if upsert else self.ix.add)(ids, x)
        self.rows = np.concatenate([self.rows, np.asarray(x, np.float32)])

    def graph(self):
        e = self.ix.hnsw_export()
        assert len(e["ids"]) == len(self.rows)
        g = hr.Graph(min(self.metric, hr.IP), self.rows, e["deleted"],
                     e["counts"], e["links"], e["entry_point"],
                     e["max_level"])
        return g, e["ids"]

    def check(self, q, k, ef, filt=None, passes=None, model=None):
        """GPU == model for the queries q; returns the model's answer."""
        g, ids = self.graph()
        if model is None:
            model = [hr.search(g, x, k, ef, passes) for x in q]
        gd, gi = self.ix.search_hnsw(q, k, ef, filt)
        ctr = self.ix.hnsw_last_counters()
        for i, (nodes, keys, _, _) in enumerate(model):
            want_ids = np.where(nodes >= 0, ids[np.maximum(nodes, 0)], -1)
            want_d = keys if self.metric == hr.L2 else \
                np.where(nodes >= 0, -keys, np.float32(0))
            assert np.array_equal(gi[i], want_ids), (k, ef, i, gi[i],
                                                     want_ids)
            assert np.array_equal(gd[i], want_d), (k, ef, i, gd[i], want_d)
        assert ctr == (sum(m[2] for m in model), sum(m[3] for m in model)), \
            (k, ef, ctr)
        return model

    def close(self):
        self.ix.close()


def make_ids(n, start=0):
    return (np.arange(start, start + n, dtype=np.int64) * 3 + 7)


_cache = {}


def built(metric, d, m):
    """One index per (metric, d, M), shared by the tests that only read."""
    key = (metric, d, m)
    if key not in _cache:
        h = Harness(metric, d, m)
        h.add(make_ids(N), ints(N, d, 1000 + d + m))
        h.q = ints(NQ, d, 5000 + d)
        _cache[key] = h
    return _cache[key]


@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
@pytest.mark.parametrize("d,m", SHAPES)
def test_search_equals_model(metric, d, m):
    h = built(metric, d, m)
    info = h.ix.hnsw_info()
    assert info["nlinks"] == m and info["max_m0"] == 2 * m
    assert info["n_nodes"] == N and info["max_level"] >= 1
    g, _ = h.graph()
    if m == 48:
        assert max(g.counts[0]) > 64  # more than one wave pass of neighbours
    for k, ef in CASES:
        model = h.check(h.q, k, ef)
        h.check(h.q[:1], k, ef, model=model[:1])  # nq = 1


@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
@pytest.mark.parametrize("n", [0, 1, 5])
def test_small_indexes_pad(metric, n):
    h = Harness(metric, 16, 16)
    q = ints(3, 16, 77)
    if n:
        h.add(make_ids(n), ints(n, 16, 78))
    for k, ef in [(1, 1), (10, 10), (10, 300)]:
        if n:
            h.check(q, k, ef)
        gd, gi = h.ix.search_hnsw(q, k, ef)
        assert ((gi >= 0).sum(1) == min(n, k)).all()
        assert (gi[:, min(n, k):] == -1).all()
        assert (gd[:, min(n, k):] == 0).all()
    if n <= 1:
        assert h.ix.hnsw_info()["entry_point"] == n - 1
    h.close()


def test_a_batch_split_over_several_launches(monkeypatch):
    """The visited bitmaps of one launch stay below a bound (256 MB); a
    lowered bound splits 70 queries into launches of 3."""
    h = built(hr.L2, 16, 16)
    per_query = (N + 31) // 32 * 4
    monkeypatch.setenv("DG_HNSW_VISITED_BYTES", str(3 * per_query + 1))
    h.check(h.q, 10, 64)
    monkeypatch.setenv("DG_HNSW_VISITED_BYTES", "1")  # one query per launch
    h.check(h.q[:5], 10, 10)


@pytest.mark.parametrize("metric", [0, 1], ids=["L2", "IP"])
def test_the_limits_d_8192_ef_1024(metric):
    """The largest dynamic LDS a launch asks for: d = 8192 and ef' = 1024.
    Components in [-3, 3]: a sum stays below 8192 * 36 < 2^24, still exact."""
    d, n = 8192, 96
    h = Harness(metric, d, 16)
    h.add(make_ids(n), ints(n, d, 41))
    q = ints(3, d, 42)
    h.check(q, 10, 1024)
    h.check(q, 1024, 1)
    gd, gi = h.ix.search_hnsw(q, 1024, 1)
    assert ((gi >= 0).sum(1) == n).all()
    h.close()


@pytest.fixture(scope="module")
def mutable():
    """An index the mutation tests change, in file order."""
    h = Harness(hr.L2, 17, 16)
    h.add(make_ids(N), ints(N, 17, 31))
    h.q = ints(NQ, 17, 32)
    yield h
    h.close()


def test_tombstones_and_the_deleted_entry_point(mutable):
    h = mutable
    info = h.ix.hnsw_info()
    ids = make_ids(N)
    gone = np.unique(np.concatenate([
        ids[np.random.default_rng(5).random(N) < 0.3],
        ids[[info["entry_point"]]]]))
    h.ix.remove(gone)
    st = h.ix.stats()
    assert st["ntotal"] == N - len(gone) and st["deleted_count"] == len(gone)
    e = h.ix.hnsw_export()
    assert e["deleted"][info["entry_point"]] == 1
    assert e["deleted"].sum() == len(gone)
    for k, ef in CASES:
        model = h.check(h.q, k, ef)
        for nodes, _, _, _ in model:
            assert not e["deleted"][nodes[nodes >= 0]].any()
    gd, gi = h.ix.search_hnsw(h.q, 10, 64)
    assert not np.isin(gi, gone).any()


def test_filters(mutable):
    h = mutable
    g, ids = h.graph()
    D = dg()
    live = ~g.deleted
    lo, hi = int(ids[200]), int(ids[1400])
    some = np.sort(ids[np.random.default_rng(6).random(len(ids)) < 0.25])
    bits = np.zeros((int(ids.max()) + 64) // 64 + 1, np.uint64)
    chosen = ids[np.random.default_rng(7).random(len(ids)) < 0.5]
    for v in chosen - 7:  # bitmap_base = 7
        bits[v >> 6] |= np.uint64(1) << np.uint64(v & 63)
    few = np.sort(ids[live][:4])
    specs = [
        ("none", D.make_filter(kind=0), np.ones(len(ids), bool)),
        ("range", D.make_filter(kind=1, min_id=lo, max_id=hi),
         (ids >= lo) & (ids < hi)),
        ("sorted", D.make_filter(kind=2, ids=some), np.isin(ids, some)),
        ("bitmap", D.make_filter(kind=3, bitmap=bits, bitmap_base=7),
         np.isin(ids, chosen)),
        ("not-range", D.make_filter(kind=1, negate=True, min_id=lo,
                                    max_id=hi), ~((ids >= lo) & (ids < hi))),
        ("not-sorted", D.make_filter(kind=2, negate=True, ids=some),
         ~np.isin(ids, some)),
        ("nothing", D.make_filter(kind=1, min_id=0, max_id=0),
         np.zeros(len(ids), bool)),
        ("fewer-than-k", D.make_filter(kind=2, ids=few), np.isin(ids, few)),
    ]
    for name, filt, passes in specs:
        # with (almost) nothing admissible W never fills and a search walks
        # the whole graph: fewer queries keep the model quick
        q = h.q[:6] if name in ("nothing", "fewer-than-k") else h.q[:24]
        for k, ef in [(10, 10), (10, 300)]:
            model = h.check(q, k, ef, filt=filt, passes=passes)
            found = np.array([(m[0] >= 0).sum() for m in model])
            if name == "nothing":
                assert (found == 0).all()
            if name == "fewer-than-k" and ef == 300:
                assert (found <= 4).all() and found.max() > 0


def test_search_after_add_after_search(mutable):
    h = mutable
    before = h.ix.hnsw_info()["n_nodes"]
    new_ids = make_ids(300, start=N)
    x = ints(300, 17, 33)
    h.add(new_ids, x)
    assert h.ix.hnsw_info()["n_nodes"] == before + 300
    h.check(h.q[:24], 10, 64)
    gd, gi = h.ix.search_hnsw(x[:16], 1, 64)
    assert (gd[:, 0] == 0).all()  # the new rows are found (at distance 0)


def test_upsert_of_a_present_id(mutable):
    h = mutable
    g, ids = h.graph()
    live_ids = ids[~g.deleted][:5].copy()
    x = ints(5, 17, 34) + np.float32(7)  # far from everything else
    n0, del0 = h.ix.hnsw_info()["n_nodes"], h.ix.stats()["deleted_count"]
    nt0 = h.ix.stats()["ntotal"]
    h.add(live_ids, x, upsert=True)
    info = h.ix.hnsw_info()
    assert info["n_nodes"] == n0 + 5 and info["n_deleted"] == del0 + 5
    assert h.ix.stats()["ntotal"] == nt0
    gd, gi = h.ix.search_hnsw(x, 1, 64)
    assert np.array_equal(gi[:, 0], live_ids) and (gd[:, 0] == 0).all()
    assert np.array_equal(h.ix.reconstruct(live_ids), x)
    h.check(h.q[:24], 10, 64)


def test_add_device_downloads_the_rows():
    """dg_add_device: the build is on the host, so the rows come down."""
    import torch
    d, n = 17, 300
    h = Harness(hr.IP, d, 8)
    x = ints(n, d, 51)
    ids = make_ids(n)
    tx = torch.from_numpy(x).cuda()
    h.ix.add_device(ids, tx.data_ptr(), n)
    h.rows = x
    assert h.ix.hnsw_info()["n_nodes"] == n
    assert np.array_equal(h.ix.reconstruct(ids), x)
    h.check(ints(16, d, 52), 10, 64)
    # the same graph as a host add of the same rows
    h2 = Harness(hr.IP, d, 8)
    h2.add(ids, x)
    e1, e2 = h.ix.hnsw_export(), h2.ix.hnsw_export()
    for u, v in zip(e1["links"] + e1["counts"], e2["links"] + e2["counts"]):
        assert np.array_equal(u, v)
    bad = tx.clone()
    bad[3, 2] = float("nan")
    with pytest.raises(dg().DgError) as e:
        h.ix.add_device(make_ids(n, start=n), bad.data_ptr(), n)
    assert e.value.status == EINVAL and h.ix.hnsw_info()["n_nodes"] == n
    h.close()
    h2.close()


def test_search_while_another_thread_adds():
    """A search sees the graph of some completed add, never a mirror that is
    older than the graph it describes: every answer given while another
    thread adds equals the model on one of the graph's states.  The build is
    deterministic, so a second index that takes the same adds one by one
    shows every state."""
    import threading
    d, base, step, rounds = 16, 400, 20, 30
    x = ints(base + step * rounds, d, 61)
    ids = make_ids(len(x))
    q = ints(8, d, 62)
    k, ef = 10, 32

    ref = Harness(hr.L2, d, 8)
    ref.add(ids[:base], x[:base])
    states = []
    for r in range(rounds + 1):
        if r:
            lo = base + step * (r - 1)
            ref.add(ids[lo:lo + step], x[lo:lo + step])
        g, gids = ref.graph()
        want = [hr.search(g, v, k, ef) for v in q]
        states.append((np.stack([gids[m[0]] for m in want]),
                       np.stack([m[1] for m in want])))
    ref.close()

    h = Harness(hr.L2, d, 8)
    h.add(ids[:base], x[:base])
    h.ix.search_hnsw(q, k, ef)
    answers, errors, done = [], [], threading.Event()

    def searcher():
        try:
            while True:
                last = done.is_set()
                answers.append(h.ix.search_hnsw(q, k, ef))
                if last:
                    return
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=searcher)
    t.start()
    try:
        for r in range(1, rounds + 1):
            lo = base + step * (r - 1)
            h.add(ids[lo:lo + step], x[lo:lo + step])
    finally:
        done.set()
        t.join()
    assert not errors, errors
    assert answers
    cur = 0  # states only move forward (two states may answer alike)
    for i, (gd, gi) in enumerate(answers):
        match = [s for s, (wi, wd) in enumerate(states)
                 if s >= cur and np.array_equal(gi, wi)
                 and np.array_equal(gd, wd)]
        assert match, (i, cur, gi[0])
        cur = match[0]
    # the last search began after the last add
    assert np.array_equal(answers[-1][1], states[rounds][0])
    h.check(q, k, ef)
    h.close()


@pytest.mark.parametrize("d", [16, 17, 200])
def test_cosine(d):
    D = dg()
    rng = np.random.default_rng(900 + d)
    # clustered float data: a recall condition on isotropic noise in d = 200
    # would test the curse of dimensionality, not the search
    cents = rng.normal(size=(20, d)).astype(np.float32)
    x = (cents[rng.integers(0, 20, N)] +
         0.3 * rng.normal(size=(N, d))).astype(np.float32)
    q = (cents[rng.integers(0, 20, NQ)] +
         0.3 * rng.normal(size=(NQ, d))).astype(np.float32)
    ix = D.Index(D.HNSW, D.COSINE, d)
    ix.hnsw_configure(16, 100, 100)
    ids = make_ids(N)
    ix.add(ids, x)
    stored = ix.reconstruct(ids).astype(np.float64)
    assert np.abs(np.linalg.norm(stored, axis=1) - 1).max() < 1e-6
    x32 = x.astype(np.float32)
    want = x32 * (np.float32(1) / (np.sqrt((x32 * x32).sum(1, np.float32))
                                   + np.float32(1e-30)))[:, None]
    assert np.abs(stored - want).max() <= 2.0 ** -22
    gd, gi = ix.search_hnsw(q, 10, 64)
    assert (gi >= 0).all()
    qn = q.astype(np.float64)
    qn /= np.linalg.norm(qn, axis=1)[:, None]
    exact = qn @ stored.T
    pos = (gi - 7) // 3
    got = np.take_along_axis(exact, pos, 1)
    bound = 4 * d * 2.0 ** -24
    assert np.abs(gd - got).max() <= bound, np.abs(gd - got).max()
    assert (np.diff(gd, axis=1) <= 0).all()  # best (largest score) first
    tenth = -np.sort(-exact, axis=1)[:, 9]
    recall = (got >= tenth[:, None]).mean()
    assert recall >= 0.9, recall
    ix.close()


def test_contracts(tmp_path):
    D = dg()
    lib = D.lib()

    def status(fn, *a, **kw):
        try:
            fn(*a, **kw)
        except D.DgError as e:
            return e.status
        return 0

    d = 16
    ix = D.Index(D.HNSW, D.L2, d)
    info = ix.hnsw_info()
    assert (info["nlinks"], info["max_m0"], info["ef_construction"],
            info["ef_search"], info["max_level"], info["entry_point"],
            info["n_nodes"], info["seed"]) == (32, 64, 200, 10, -1, -1, 0, 100)
    st = ix.stats()
    assert st["kind"] == D.HNSW and st["is_trained"] == 1 and st["d"] == d
    # configure: the bounds
    for m, efc in [(1, 100), (129, 100), (16, 0), (16, 4097)]:
        assert status(ix.hnsw_configure, m, efc) == ENOT_SUPPORT
    ix.hnsw_configure(2, 1)
    ix.hnsw_configure(128, 4096)
    ix.hnsw_configure(8, 40, 5)
    assert ix.hnsw_info()["seed"] == 5
    for ef in (0, -1, 1025):
        assert status(ix.set_ef, ef) == EINVAL
    ix.train(ints(10, d, 1))  # an OK no-op
    # an empty index answers -1
    q = ints(4, d, 2)
    gd, gi = ix.search_hnsw(q, 5, 0)
    assert (gi == -1).all() and (gd == 0).all()
    assert ix.hnsw_last_counters() == (0, 0)
    x = ints(400, d, 3)
    ids = make_ids(400)
    # add: all-or-nothing
    bad = ids[:3].copy()
    bad[1] = -4
    assert status(ix.add, bad, x[:3]) == EINVAL
    assert status(ix.add, np.array([5, 9, 5]), x[:3]) == EDUP
    xn = x[:3].copy()
    xn[2, 5] = np.nan
    assert status(ix.add, ids[:3], xn) == EINVAL
    xn[2, 5] = np.inf
    assert status(ix.upsert, ids[:3], xn) == EINVAL
    assert ix.hnsw_info()["n_nodes"] == 0
    ix.add(ids, x)
    assert status(ix.add, ids[5:6], x[5:6]) == EDUP
    assert status(ix.hnsw_configure, 8, 40) == EINVAL  # not empty any more
    assert ix.hnsw_info()["n_nodes"] == 400
    # remove: a missing id removes nothing
    assert status(ix.remove, np.array([ids[0], 1])) == ENOT_FOUND
    assert ix.stats()["deleted_count"] == 0
    assert status(ix.reconstruct, np.array([1])) == ENOT_FOUND
    assert np.array_equal(ix.reconstruct(ids[7:9]), x[7:9])
    # search bounds
    assert status(ix.search_hnsw, q, 5, -1) == EINVAL
    assert status(ix.search_hnsw, q, 5, 1025) == EINVAL
    assert status(ix.search_hnsw, q, 1025, 0) == ENOT_SUPPORT
    assert status(ix.search, q, 1025) == ENOT_SUPPORT
    # a huge k is refused before any staging is sized from it
    od, oi = np.zeros((4, 1), np.float32), np.zeros((4, 1), np.int64)
    assert lib.dg_search_hnsw(ix.h, 4, q, 1 << 30, 0, None, od, oi) == \
        ENOT_SUPPORT
    assert lib.dg_search(ix.h, 4, q, 1 << 30, 0, None, od, oi) == ENOT_SUPPORT
    assert lib.dg_search_hnsw(ix.h, 4, q, 1 << 30, 2000, None, od, oi) == \
        EINVAL
    gd, gi = ix.search_hnsw(q, 0)
    assert gd.shape == (4, 0)  # k <= 0: an OK no-op
    ix.search_hnsw(q, 1024, 1024)
    # dg_search is search_hnsw with ef_search = 0 (the stored value)
    ix.set_ef(37)
    assert ix.hnsw_info()["ef_search"] == 37
    a = ix.search(q, 5, nprobe=3)
    c1 = ix.hnsw_last_counters()
    b = ix.search_hnsw(q, 5, 0)
    assert ix.hnsw_last_counters() == c1
    e = ix.search_hnsw(q, 5, 37)
    assert ix.hnsw_last_counters() == c1
    for u, v in zip(a, b):
        assert np.array_equal(u, v)
    for u, v in zip(a, e):
        assert np.array_equal(u, v)
    assert ix.search_hnsw(q, 5, 1) is not None
    assert ix.hnsw_last_counters() != c1
    # stats of the last search
    ix.search_hnsw(q, 5, 64)
    st = ix.stats()
    evals = ix.hnsw_last_counters()[1]
    assert st["last_nq"] == 4 and st["last_scan_ms"] > 0
    assert st["last_scan_bytes_algorithmic"] == evals * 4 * d
    assert st["device_bytes"] >= 400 * d * 4 + 400 * 16 * 4
    # the device form, on its own buffers
    import torch
    tq = torch.from_numpy(q).cuda()
    td = torch.empty((4, 5), dtype=torch.float32, device="cuda")
    ti = torch.empty((4, 5), dtype=torch.int64, device="cuda")
    ix.search_hnsw_device(tq.data_ptr(), 4, 5, 64, td.data_ptr(),
                          ti.data_ptr())
    ix.sync()
    want = ix.search_hnsw(q, 5, 64)
    assert np.array_equal(td.cpu().numpy(), want[0])
    assert np.array_equal(ti.cpu().numpy(), want[1])
    ix.search_device(tq.data_ptr(), 4, 5, 0, td.data_ptr(), ti.data_ptr())
    ix.sync()
    assert np.array_equal(ti.cpu().numpy(), a[1])
    # batched: passes through and counts as bypassed
    ix.enable_batching()
    got = ix.search_batched(q, 5)
    assert np.array_equal(got[1], a[1]) and np.array_equal(got[0], a[0])
    bs = ix.batching_stats()
    assert bs["bypassed"] == 1 and bs["flushes"] == 0
    ix.disable_batching()
    # not offered for this kind
    assert status(ix.range_search, q, 1.0) == ENOT_SUPPORT
    assert status(ix.save, str(tmp_path / "a.dgi")) == ENOT_SUPPORT
    assert status(ix.save_faiss, str(tmp_path / "a.faiss")) == ENOT_SUPPORT
    assert status(ix.set_storage, "f16") == ENOT_SUPPORT
    assert status(ix.set_storage, "sq8") == ENOT_SUPPORT
    ix.set_storage("f32")
    assert status(ix.set_list_mask, np.ones(4, np.uint8)) == ENOT_SUPPORT
    assert status(D.ShardedIndex, D.HNSW, D.L2, d, [0]) == ENOT_SUPPORT
    # the binary calls
    xb = np.zeros((2, d // 8), np.uint8)
    assert lib.dg_add_binary(ix.h, 2, np.array([1, 2], np.int64), xb) == EINVAL
    od, oi = np.zeros((2, 1), np.float32), np.zeros((2, 1), np.int64)
    assert lib.dg_search_binary(ix.h, 2, xb, 1, 0, None, od, oi) == EINVAL
    # the other kinds refuse the HNSW calls
    fl = D.Index(D.FLAT, D.L2, d)
    assert status(fl.hnsw_configure, 8, 40) == EINVAL
    assert status(fl.search_hnsw, q, 5) == EINVAL
    assert status(fl.hnsw_info) == EINVAL
    assert status(fl.save_hnswlib, str(tmp_path / "f.bin")) == EINVAL
    fl.close()
    # save / load round trip, tombstones kept
    ix.remove(ids[10:20])
    before = ix.search_hnsw(q, 10, 64)
    c_before = ix.hnsw_last_counters()
    path = str(tmp_path / "h.bin")
    ix.save_hnswlib(path)
    import hnswlib_format as hf
    p = hf.parse(open(path, "rb").read())
    assert p["n"] == 400 and p["M"] == 8 and p["deleted"].sum() == 10
    assert p["ef_construction"] == 40
    ld = D.Index.load_hnswlib(path, D.L2, d)
    assert ld.kind == D.HNSW and ld.stats()["ntotal"] == 390
    li = ld.hnsw_info()
    assert (li["n_nodes"], li["n_deleted"], li["nlinks"]) == (400, 10, 8)
    after = ld.search_hnsw(q, 10, 64)
    assert ld.hnsw_last_counters() == c_before
    for u, v in zip(before, after):
        assert np.array_equal(u, v)
    e1, e2 = ix.hnsw_export(), ld.hnsw_export()
    for key in ("ids", "deleted", "levels"):
        assert np.array_equal(e1[key], e2[key])
    for u, v in zip(e1["links"] + e1["counts"], e2["links"] + e2["counts"]):
        assert np.array_equal(u, v)
    # max_elements: the file's field, carried by the index
    assert lib.dg_hnsw_max_elements(ld.h, -1) == 400 == p["max_elements"]
    assert lib.dg_hnsw_max_elements(ld.h, 5000) == 5000
    ld.save_hnswlib(path)
    assert hf.parse(open(path, "rb").read())["max_elements"] == 5000
    ix.save_hnswlib(path)
    ld.add(np.array([5], np.int64), x[:1])  # a loaded index still grows
    ld.close()
    assert status(D.Index.load_hnswlib, path, D.L2, d + 1) == EIO
    blob = open(path, "rb").read()
    open(path, "wb").write(blob[:-3])
    assert status(D.Index.load_hnswlib, path, D.L2, d) == EIO
    open(path, "wb").write(hf.patch(blob, hf.H_M, "<Q", 200))
    assert status(D.Index.load_hnswlib, path, D.L2, d) == ENOT_SUPPORT
    assert status(D.Index.load_hnswlib, str(tmp_path / "none"), D.L2, d) == EIO
    ix.close()


def test_kind_above_hnsw_is_refused():
    D = dg()
    with pytest.raises(D.DgError) as e:
        D.Index(6, D.L2, 16)
    assert e.value.status == EINVAL
    with pytest.raises(D.DgError) as e:
        D.Index(D.HNSW, D.HAMMING, 16)
    assert e.value.status == EINVAL


def test_mirror_selftest():
    assert dg().lib().dg_mirror_selftest_hnsw() == 0


def test_release_shared_indexes():
    for h in _cache.values():
        h.close()
    _cache.clear()
