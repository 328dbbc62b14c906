"""GPU tests of search batching (dg_search_batched): concurrent one-query
calls of one index coalesced into device batches.

Shape: that of test_gpu_parity.test_concurrent_search, slightly widened:
gen_base(777, 20000, 64), 48 queries, IVF-Flat L2, nlist 32, centroids from
orc.kmeans(seed=1234) injected, nprobe 8, k 10.  The expected answer of every
query is a direct search with nq = 1.

Comparison rule.  The coarse GEMM is served by the hand MFMA kernel for <= 8
or >= 48 rows and by rocBLAS for 9..47 (sgemm_dots), so float results are not
promised bit-equal across batch compositions: ids must be EXACTLY equal,
distances within 1e-4 relative.  Exact ids are a fair
demand on these inputs; the precondition is recomputed here in float64 and
asserted: the relative gap between the nprobe-th and the next centroid of
every query, and between neighbours among each query's best k + 1 probed
rows, exceeds 1e-6 (measured for this data: 8.4e-5 and 1.7e-5; f32 error at
d = 64 is far below).  If someone changes the data, the precondition fails
instead of the parity.  Binary kinds have integer distances and a fixed row
order: array_equal on both outputs.  Flat: the precondition covers all rows;
a query whose gap falls under 1e-6 may differ in ids only where distances
tie within 1e-4.  IVF-PQ: the f16 table bound of DESIGN.md "IVF-PQ limits"
(tests/pq_reference.py) is the distance tolerance, and ids may differ only
between rows whose reference distances lie within that bound.
"""
import os
import sys
import threading

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "oracle"),
                os.path.join(REPO, "dingo-store_amd"), HERE]

import pyoracle as orc  # noqa: E402
import workload  # noqa: E402

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

N, D, NQ, NLIST, NPROBE, K = 20000, 64, 48, 32, 8, 10
THREADS = 16
REL = 1e-4
MIN_GAP = 1e-6


# ---------------------------------------------------------------- helpers
def assert_rule(got, exp, what=""):
    """ids exactly equal, distances within 1e-4 relative."""
    gd, gi = got
    ed, ei = exp
    assert np.array_equal(gi, ei), (what, gi, ei)
    assert (np.abs(gd - ed) <= REL * np.abs(ed)).all(), (what, gd, ed)


def rel_gaps(sorted_vals):
    """Relative gaps between neighbours of ascending positive values."""
    a = np.asarray(sorted_vals, np.float64)
    return (a[1:] - a[:-1]) / np.maximum(a[1:], 1e-300)


class Data:
    """The shared inputs and their float64 model (computed once)."""

    def __init__(self):
        self.base = workload.gen_base(777, N, D)
        self.q = workload.gen_queries(777, N, D, NQ)
        self.cents = orc.kmeans(orc.L2, self.base, NLIST, seed=1234)
        b64 = self.base.astype(np.float64)
        q64 = self.q.astype(np.float64)
        c64 = self.cents.astype(np.float64)
        # [NQ x N] and [NQ x NLIST] squared distances, float64
        self.row_d = ((q64 ** 2).sum(1)[:, None] + (b64 ** 2).sum(1)[None]
                      - 2.0 * q64 @ b64.T)
        self.cent_d = ((q64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None]
                       - 2.0 * q64 @ c64.T)
        bc = ((b64 ** 2).sum(1)[:, None] + (c64 ** 2).sum(1)[None]
              - 2.0 * b64 @ c64.T)
        self.assign = bc.argmin(1)

    def centroid_gap(self, nprobe):
        """Smallest relative gap between the nprobe-th and the next
        centroid over the queries."""
        s = np.sort(self.cent_d, axis=1)
        return ((s[:, nprobe] - s[:, nprobe - 1]) / s[:, nprobe]).min()

    def row_gaps(self, nprobe, k, passes=None):
        """Per query: smallest relative gap between neighbours among its
        best k + 1 admissible rows of the probed lists (nprobe None: all
        rows, Flat)."""
        out = np.empty(NQ)
        for r in range(NQ):
            ok = np.ones(N, bool) if passes is None else passes.copy()
            if nprobe is not None:
                probed = np.zeros(NLIST, bool)
                probed[np.argsort(self.cent_d[r], kind="stable")[:nprobe]] = \
                    True
                ok &= probed[self.assign]
            best = np.sort(self.row_d[r][ok])[:k + 1]
            out[r] = rel_gaps(best).min()
        return out


@pytest.fixture(scope="module")
def data():
    return Data()


def new_ivf(data):
    idx = dg.Index(dg.IVF_FLAT, dg.L2, D, nlist=NLIST)
    idx.set_centroids(data.cents)
    idx.add(np.arange(N, dtype=np.int64), data.base)
    return idx


def direct_rows(idx, q, k, nprobe=0, filt=None):
    """The expected answers: one direct nq = 1 search per query."""
    out = [idx.search(q[i:i + 1], k, nprobe=nprobe, filt=filt)
           for i in range(len(q))]
    return (np.concatenate([o[0] for o in out]),
            np.concatenate([o[1] for o in out]))


@pytest.fixture(scope="module")
def ivf(data):
    """One index for the IVF-Flat cases, with the direct answers of the 48
    queries taken before batching is ever enabled on it."""
    assert data.centroid_gap(NPROBE) > MIN_GAP
    assert data.row_gaps(NPROBE, K).min() > MIN_GAP
    idx = new_ivf(data)
    expect = direct_rows(idx, data.q, K, NPROBE)
    yield idx, expect
    idx.close()


def run_pool(n_threads, calls):
    """calls: list of zero-argument callables; thread t runs calls t,
    t + n_threads, ... after a common barrier.  Returns the results (or the
    exceptions) in call order."""
    out = [None] * len(calls)
    barrier = threading.Barrier(n_threads)

    def work(t):
        barrier.wait()
        for i in range(t, len(calls), n_threads):
            try:
                out[i] = calls[i]()
            except Exception as e:  # reported by the caller
                out[i] = e

    th = [threading.Thread(target=work, args=(t,)) for t in range(n_threads)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    return out


def stack(results):
    for r in results:
        assert not isinstance(r, Exception), r
    return (np.concatenate([r[0] for r in results]),
            np.concatenate([r[1] for r in results]))


def one_query_calls(idx, q, k, nprobe):
    return [lambda i=i: idx.search_batched(q[i:i + 1], k, nprobe=nprobe)
            for i in range(len(q))]


# ------------------------------------------------------------------ cases
def test_not_enabled_is_plain_search(data):
    """1. Without dg_batching_enable, search_batched is search."""
    idx = new_ivf(data)
    try:
        for nq in (1, NQ):
            ed, ei = idx.search(data.q[:nq], K, nprobe=NPROBE)
            gd, gi = idx.search_batched(data.q[:nq], K, nprobe=NPROBE)
            assert np.array_equal(gi, ei) and np.array_equal(gd, ed)
        st = idx.batching_stats()
        assert st["calls"] == 0 and st["flushes"] == 0
    finally:
        idx.close()


def test_batches_form(data, ivf):
    """2. 16 threads x 3 one-query calls, a batch may wait for company."""
    idx, expect = ivf
    idx.enable_batching(max_batch=16, max_wait_us=200000)
    try:
        got = stack(run_pool(THREADS,
                             one_query_calls(idx, data.q, K, NPROBE)))
        st = idx.batching_stats()
    finally:
        idx.disable_batching()
    print("batching stats:", st)
    assert_rule(got, expect)
    assert st["queries"] == st["calls"] == NQ
    assert st["max_flush_queries"] >= 2  # a batch really formed
    assert st["flushes"] < NQ
    assert st["bypassed"] == 0


def test_zero_wait(data, ivf):
    """3. The same traffic with max_wait_us 0 (no demand on batch sizes)."""
    idx, expect = ivf
    idx.enable_batching(max_batch=16, max_wait_us=0)
    try:
        got = stack(run_pool(THREADS,
                             one_query_calls(idx, data.q, K, NPROBE)))
        st = idx.batching_stats()
    finally:
        idx.disable_batching()
    print("batching stats:", st)
    assert_rule(got, expect)
    assert st["queries"] == st["calls"] == NQ


def test_mixed_traffic(data, ivf):
    """4. k 5 with k 10, nprobe 4 with nprobe 8, RANGE-filtered calls with
    equal bounds next to unfiltered ones, and SORTED_IDS calls (bypassed),
    all in one run; each answer equals its own direct call."""
    idx, _ = ivf
    low = np.arange(N) < 10000
    even = np.arange(N) % 2 == 0
    rng_f = dg.make_filter(kind=1, min_id=0, max_id=10000)
    ids_f = dg.make_filter(kind=2, ids=np.arange(0, N, 2, dtype=np.int64))
    variants = [  # (k, nprobe, filter, float64 pass mask)
        (10, 8, None, None), (5, 8, None, None), (10, 4, None, None),
        (10, 8, rng_f, low), (5, 8, rng_f, low), (10, 8, ids_f, even),
    ]
    assert data.centroid_gap(4) > MIN_GAP
    for k, nprobe, _, passes in variants:
        assert data.row_gaps(nprobe, k, passes).min() > MIN_GAP
    args = [variants[i % len(variants)] for i in range(NQ)]
    expect = [idx.search(data.q[i:i + 1], a[0], nprobe=a[1], filt=a[2])
              for i, a in enumerate(args)]
    for (ed, ei), a in zip(expect, args):
        if a[3] is not None:  # the filters do filter
            assert a[3][ei[ei >= 0]].all()
    idx.enable_batching(max_batch=16, max_wait_us=1000)
    try:
        got = run_pool(THREADS, [
            lambda i=i, a=a: idx.search_batched(
                data.q[i:i + 1], a[0], nprobe=a[1], filt=a[2])
            for i, a in enumerate(args)])
        st = idx.batching_stats()
    finally:
        idx.disable_batching()
    print("batching stats:", st)
    for i, (g, e) in enumerate(zip(got, expect)):
        assert not isinstance(g, Exception), g
        assert g[0].shape == (1, args[i][0])
        assert_rule(g, e, what=(i, args[i][:2]))
    n_sorted = sum(1 for a in args if a[2] is ids_f)
    assert n_sorted == 8 and st["bypassed"] == n_sorted
    assert st["calls"] == st["queries"] == NQ


def test_mixed_k_in_one_batch(data, ivf):
    """A batch of two that must fill (max_batch 2): k 5 and k 10 run as one
    flush at k 10, and each caller receives its own k columns."""
    idx, expect = ivf
    e10 = (expect[0][1:2], expect[1][1:2])
    e5 = idx.search(data.q[:1], 5, nprobe=NPROBE)
    idx.enable_batching(max_batch=2, max_wait_us=5000000)
    try:
        got = run_pool(2, [
            lambda: idx.search_batched(data.q[:1], 5, nprobe=NPROBE),
            lambda: idx.search_batched(data.q[1:2], 10, nprobe=NPROBE)])
        st = idx.batching_stats()
    finally:
        idx.disable_batching()
    assert st["flushes"] == 1 and st["max_flush_queries"] == 2
    for g in got:
        assert not isinstance(g, Exception), g
    assert got[0][0].shape == (1, 5) and got[1][0].shape == (1, 10)
    assert_rule(got[0], e5)
    assert_rule(got[1], e10)
    # the prefix argument itself: top-5 is the first 5 columns of top-10
    assert np.array_equal(e5[1], expect[1][:1, :5])


def test_flat(data):
    """5a. Flat L2, 16 threads x 2 calls."""
    gaps = data.row_gaps(None, K)
    idx = dg.Index(dg.FLAT, dg.L2, D)
    try:
        idx.add(np.arange(N, dtype=np.int64), data.base)
        q = data.q[:2 * THREADS]
        ed, ei = direct_rows(idx, q, K)
        idx.enable_batching(max_batch=16, max_wait_us=1000)
        gd, gi = stack(run_pool(THREADS, one_query_calls(idx, q, K, 0)))
        st = idx.batching_stats()
    finally:
        idx.close()
    print("batching stats:", st, "min gap", gaps.min())
    assert st["calls"] == len(q)
    assert (np.abs(gd - ed) <= REL * np.abs(ed)).all()
    for r in range(len(q)):
        if gaps[r] > MIN_GAP:
            assert np.array_equal(gi[r], ei[r]), r
        else:  # ids may differ only where the distances tie within 1e-4
            for c in np.nonzero(gi[r] != ei[r])[0]:
                d_g = data.row_d[r][gi[r, c]]
                d_e = data.row_d[r][ei[r, c]]
                assert abs(d_g - d_e) <= REL * abs(d_e), (r, c)


def test_ivfpq():
    """5b. IVF-PQ (m 8, nbits 8), 16 threads x 2 calls, under the f16
    table bound b of pq_reference: every distance within b of the float64
    reference of its row, and ids differ from the direct call only between
    rows whose reference distances lie within their bounds."""
    from pq_reference import add_all, grouped_case
    lens = [300, 257, 120, 64, 500, 33, 256, 90]
    case, lists, codes, x32 = grouped_case(dg.L2, 64, 8, lens, 2026, nbits=8)
    nprobe, k = 3, K
    q = case.queries(np.arange(2 * THREADS) % len(lens))
    idx = case.new_index()
    try:
        add_all(case, idx, lists, codes, x32)
        ed, ei = direct_rows(idx, q, k, nprobe)
        idx.enable_batching(max_batch=16, max_wait_us=1000)
        gd, gi = stack(run_pool(THREADS, one_query_calls(idx, q, k, nprobe)))
        st = idx.batching_stats()
    finally:
        idx.close()
    print("batching stats:", st)
    assert st["calls"] == len(q)
    case.check(q, k, nprobe, ed, ei)  # the direct answers, checks A-D
    case.check(q, k, nprobe, gd, gi)  # and the batched ones
    row_of = {int(i): r for r, i in enumerate(case.ids)}
    for r in range(len(q)):
        _, b, dist = case.reference(case._unit(q[r:r + 1])[0])
        for c in range(k):
            rg, re_ = row_of[int(gi[r, c])], row_of[int(ei[r, c])]
            assert abs(float(gd[r, c]) - dist[rg]) <= b[rg]
            assert abs(float(gd[r, c]) - float(ed[r, c])) <= b[rg] + b[re_]
            if rg != re_:
                assert abs(dist[rg] - dist[re_]) <= b[rg] + b[re_], (r, c)


def test_binary_ivf():
    """5c. Binary IVF-Flat, d = 256 bits: equal outputs."""
    rng = np.random.default_rng(99)
    n, d, nlist = 6000, 256, 16
    x = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    q = x[:2 * THREADS].copy()
    q[:, 5] ^= rng.integers(1, 256, len(q), dtype=np.uint8)
    idx = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, d, nlist=nlist)
    try:
        idx.set_centroids(x[1000:1000 + nlist])
        idx.add(np.arange(n, dtype=np.int64), x)
        ed, ei = direct_rows(idx, q, K, 4)
        idx.enable_batching(max_batch=16, max_wait_us=1000)
        gd, gi = stack(run_pool(THREADS, one_query_calls(idx, q, K, 4)))
        st = idx.batching_stats()
    finally:
        idx.close()
    print("batching stats:", st)
    assert st["calls"] == len(q)
    assert np.array_equal(gi, ei) and np.array_equal(gd, ed)


def test_mutation_under_search(data):
    """6. Eight threads search batched while the main thread adds 100 rows
    and removes them again: no call fails, and afterwards batched answers
    equal direct ones."""
    idx = new_ivf(data)
    extra_ids = np.arange(N, N + 100, dtype=np.int64)
    extra = workload.gen_base(778, 100, D)
    stop = threading.Event()
    errors, counts = [], [0] * 8
    try:
        idx.search(data.q[:1], K, nprobe=NPROBE)  # finalize before the race
        idx.enable_batching(max_batch=16, max_wait_us=0)

        def work(t):
            i = t
            while True:
                try:
                    d_, i_ = idx.search_batched(data.q[i % NQ:i % NQ + 1], K,
                                                nprobe=NPROBE)
                    assert i_.shape == (1, K) and (i_ >= 0).all()
                except Exception as e:
                    errors.append(e)
                    return
                counts[t] += 1
                i += 8
                if stop.is_set() and counts[t] >= 2:
                    return

        th = [threading.Thread(target=work, args=(t,)) for t in range(8)]
        for t in th:
            t.start()
        idx.add(extra_ids, extra)
        idx.remove(extra_ids)
        stop.set()
        for t in th:
            t.join()
        assert not errors, errors
        assert idx.stats()["ntotal"] == N
        expect = direct_rows(idx, data.q, K, NPROBE)
        got = stack(run_pool(THREADS,
                             one_query_calls(idx, data.q, K, NPROBE)))
    finally:
        idx.close()
    assert min(counts) >= 2
    assert_rule(got, expect)
    assert (got[1] < N).all()  # the removed rows are gone


def test_error_isolation(data, ivf):
    """7. A call with k = 2100 returns its error while 8 concurrent valid
    calls succeed."""
    idx, expect = ivf
    idx.enable_batching(max_batch=16, max_wait_us=1000)
    try:
        calls = one_query_calls(idx, data.q[:8], K, NPROBE)
        calls.append(lambda: idx.search_batched(data.q[8:9], 2100,
                                                nprobe=NPROBE))
        got = run_pool(9, calls)
    finally:
        idx.disable_batching()
    bad = got.pop()
    assert isinstance(bad, dg.DgError) and bad.status == 3, bad
    assert "k > 2048" in str(bad)
    assert_rule(stack(got), (expect[0][:8], expect[1][:8]))


def test_enabled_answers_like_search_at_the_edges():
    """Enabled, a call returns what dg_search would: blank results for an
    empty or untrained index, k <= 0 as a no-op, argument errors as errors,
    and none of the latter is counted as a batched call."""
    q = np.zeros((2, 32), np.float32)
    flat = dg.Index(dg.FLAT, dg.L2, 32)
    ivf_ = dg.Index(dg.IVF_FLAT, dg.L2, 32, nlist=4)  # never trained
    binary = dg.Index(dg.BINARY_FLAT, dg.HAMMING, 64)
    try:
        for idx in (flat, ivf_):
            idx.enable_batching()
            gd, gi = idx.search_batched(q, 4, nprobe=2)
            ed, ei = idx.search(q, 4, nprobe=2)
            assert (gi == -1).all() and (gd == 0).all()
            assert np.array_equal(gi, ei) and np.array_equal(gd, ed)
            assert idx.batching_stats()["calls"] == 1
            gd, gi = idx.search_batched(q, 0)  # k <= 0: OK, nothing done
            assert gd.shape == (2, 0)
            with pytest.raises(dg.DgError) as e:  # k above the limit
                idx.search_batched(q, 2100)
            assert e.value.status == 3 and "k > 2048" in str(e.value)
            assert idx.batching_stats()["calls"] == 1
        binary.enable_batching()
        lib = dg.lib()
        out_d = np.empty((1, 4), np.float32)
        out_i = np.empty((1, 4), np.int64)
        # the float entry point on a binary index, and the reverse
        st = lib.dg_search_batched(binary.h, 1, q[:1], 4, 0, None, out_d,
                                   out_i)
        assert st == 1 and "binary index" in dg.last_error()
        st = lib.dg_search_binary_batched(flat.h, 1, np.zeros((1, 8), np.uint8),
                                          4, 0, None, out_d, out_i)
        assert st == 1 and "float index" in dg.last_error()
        st = lib.dg_search_batched(flat.h, 0, q[:1], 4, 0, None, out_d, out_i)
        assert st == 1 and "bad search args" in dg.last_error()
        assert binary.batching_stats()["calls"] == 0
        # enable arguments
        with pytest.raises(dg.DgError):
            flat.enable_batching(max_batch=-1)
        with pytest.raises(dg.DgError):
            flat.enable_batching(max_batch=5000)
        with pytest.raises(dg.DgError):
            flat.enable_batching(max_wait_us=-5)
    finally:
        flat.close()
        ivf_.close()
        binary.close()


def test_disable_under_traffic(data, ivf):
    """8. dg_batching_disable while 8 threads are calling: no call is lost
    or fails, and later calls pass through."""
    idx, expect = ivf
    idx.enable_batching(max_batch=16, max_wait_us=0)
    started = threading.Event()
    rounds = 4  # every thread searches all its queries this many times

    def call(i):
        r = idx.search_batched(data.q[i:i + 1], K, nprobe=NPROBE)
        started.set()
        return r

    calls = [lambda i=i: call(i % NQ) for i in range(rounds * NQ)]
    res = {}
    t = threading.Thread(
        target=lambda: res.setdefault("out", run_pool(8, calls)))
    t.start()
    started.wait()
    idx.disable_batching()
    st = idx.batching_stats()
    t.join()
    got = res["out"]
    assert len(got) == rounds * NQ
    for r in range(rounds):
        assert_rule(stack(got[r * NQ:(r + 1) * NQ]), expect)
    assert 1 <= st["calls"] <= rounds * NQ
    # later calls pass through: plain searches, nothing counted
    for nq in (1, 5):
        ed, ei = idx.search(data.q[:nq], K, nprobe=NPROBE)
        gd, gi = idx.search_batched(data.q[:nq], K, nprobe=NPROBE)
        assert np.array_equal(gi, ei) and np.array_equal(gd, ed)
    after = idx.batching_stats()
    # disable returned once the open batches had finished: nothing since
    assert after == st


def test_mirror_selftest_batched():
    """9. 16 std::threads x nq = 1 through the mirror's Search."""
    assert dg.lib().dg_mirror_selftest_batched() == 0
