"""The one-kernel coarse probe selection (k_coarse_select) against the kernels
it replaces (k_select_dense [+ k_select_u64] + k_probe_unpack + k_hist_probes)
on a real MI355X.

Every search runs twice on one index, with DG_COARSE_WAVE=0 and with the
default.  dg_last_coarse_wave must say which path ran, the two probe arrays
(dg_last_probes) must be equal element by element, order and -1 entries
included, and the distances and ids byte-identical.  The probes feed the
probe histogram, the single-block offset scan (k_inv_offsets) and the scatter
on both sides, so equal results also cover those.

Independent of the old kernels, the geometry and the metric cases compare the
probe set of every query with ivf_reference's float64 coarse ranking; queries
whose nprobe-th and next centroid are closer than that module's tie margin
are left out (at most 2 %, asserted on the CPU by test_coarse_wave_cpu.py).
The binary case and the tie cases are exact: their scores are integers (the
tie cases hold small-integer centroids and queries, so every f32 sum is
exact), and the probes must equal the stable float64 ranking, ties to the
smaller list id, in order.

Shapes: coarse_wave_cases.py.
"""
import contextlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")
import coarse_wave_cases as cw  # noqa: E402
import hamming_oracle as ho  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

assert (dg.L2, dg.IP, dg.COSINE) == (L2, IP, COSINE)
VAR = "DG_COARSE_WAVE"


@contextlib.contextmanager
def coarse_env(wave):
    """DG_COARSE_WAVE for the calls inside (read per call)."""
    old = os.environ.get(VAR)
    try:
        if wave:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = "0"
        yield
    finally:
        if old is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = old


def search(idx, q, k, nprobe, wave, want_wave, where):
    """One search under the switch: (dist, ids, probes [nq, np])."""
    with coarse_env(wave):
        dist, ids = idx.search(q, k, nprobe=nprobe)
        assert idx.last_coarse_wave() == (wave and want_wave), (where, wave)
        probes = idx.last_probes()
    assert probes.size % len(q) == 0, (where, probes.size)
    return dist, ids, probes.reshape(len(q), -1)


def same(a, b, where):
    assert a[2].shape == b[2].shape, (where, "probes shape")
    assert np.array_equal(a[2], b[2]), (where, "probes",
                                        np.nonzero(a[2] != b[2])[0][:8])
    assert np.array_equal(a[1], b[1]), (where, "ids")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), \
        (where, "distance bits")


def both(idx, q, k, nprobe, want_wave, where):
    """Old path, then the default; returns the default's result."""
    old = search(idx, q, k, nprobe, False, want_wave, where)
    new = search(idx, q, k, nprobe, True, want_wave, where)
    same(old, new, where)
    return new


def ivf_flat(c):
    idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist)
    idx.set_centroids(c.cents)
    idx.add(c.ids, c.x)
    return idx


def check_reference(c, nprobe, probes, where):
    probed, clear = cw.unambiguous(c, nprobe)
    assert probes.shape == (len(c.q), nprobe), (where, probes.shape)
    got = np.zeros_like(probed)
    assert (probes >= 0).all() and (probes < c.nlist).all(), where
    np.put_along_axis(got, probes, True, axis=1)
    assert (got.sum(1) == nprobe).all(), (where, "repeated list")
    bad = clear & (got != probed).any(1)
    assert not bad.any(), (where, "probe set differs from the float64 "
                           "ranking for queries", np.nonzero(bad)[0][:8])


# 1. geometry of the column loop
@pytest.mark.parametrize("nlist", cw.GEOM_NLISTS)
def test_geometry(nlist):
    c = cw.geom_case(nlist)
    idx = ivf_flat(c)
    try:
        for nprobe in cw.geom_nps(nlist):
            where = ("geom", nlist, nprobe)
            got = both(idx, c.q, cw.K, nprobe, nprobe <= cw.CAP, where)
            check_reference(c, nprobe, got[2], where)
    finally:
        idx.close()


# 2. two segments on the old side
def test_segmented():
    c = cw.seg_case()
    idx = ivf_flat(c)
    try:
        for nprobe in cw.SEG_NPS:
            both(idx, c.q, cw.K, nprobe, True, ("seg", nprobe))
    finally:
        idx.close()


# 3. ties fall to the smaller list id
@pytest.mark.parametrize("identical", [False, True])
def test_ties(identical):
    c = cw.tie_case(identical)
    order = cw.tie_order(c)
    idx = ivf_flat(c)
    try:
        for nprobe in cw.TIE_NPS:
            where = ("ties", identical, nprobe)
            got = both(idx, c.q, cw.K, nprobe, True, where)
            assert np.array_equal(got[2], order[:, :nprobe]), where
            if identical:
                # every key equal: the nprobe smallest list ids, in order
                assert np.array_equal(got[2][0], np.arange(nprobe)), where
    finally:
        idx.close()


# 4. metrics (modes 1 and 2) ...
@pytest.mark.parametrize("metric", cw.KIND_METRICS)
def test_metrics(metric):
    c = cw.kind_case(metric)
    idx = ivf_flat(c)
    try:
        for nprobe in cw.KIND_NPS:
            where = ("metric", metric, nprobe)
            got = both(idx, c.q, cw.K, nprobe, True, where)
            check_reference(c, nprobe, got[2], where)
    finally:
        idx.close()


# ... IVF-PQ (it also reads the dots matrix in its scan) ...
def test_ivfpq():
    c = cw.kind_case(L2)
    m = 4
    cb = np.random.default_rng(9400).standard_normal(
        (m, 256, c.d // m)).astype(np.float32)
    idx = dg.Index(dg.IVF_PQ, L2, c.d, nlist=c.nlist, m=m)
    try:
        idx.set_centroids(c.cents)
        idx.set_codebooks(cb)
        idx.add(c.ids, c.x)
        for nprobe in cw.KIND_NPS:
            where = ("ivfpq", nprobe)
            got = both(idx, c.q, cw.K, nprobe, True, where)
            check_reference(c, nprobe, got[2], where)
    finally:
        idx.close()


# ... and binary IVF (mode 0: the Hamming distance itself is the key)
def test_binary_ivf():
    rng = np.random.default_rng(9500)
    d, nlist, n, nq = 64, cw.KIND_NLIST, cw.N_ROWS, cw.NQ
    cents = rng.integers(0, 256, (nlist, d // 8), dtype=np.uint8)
    x = rng.integers(0, 256, (n, d // 8), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, d // 8), dtype=np.uint8)
    coarse = np.asarray(ho.hamming(q, cents), np.float64)
    order = np.argsort(coarse, axis=1, kind="stable")  # ties: smaller list
    idx = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, d, nlist=nlist)
    try:
        idx.set_centroids(cents)
        idx.add(np.arange(n, dtype=np.int64), x)
        for nprobe in cw.KIND_NPS:
            where = ("binary", nprobe)
            got = both(idx, q, cw.K, nprobe, True, where)
            assert np.array_equal(got[2], order[:, :nprobe]), where
            # integer scores on 100 lists: the cut falls inside ties
            cut = coarse[np.arange(nq), order[:, nprobe - 1]] == \
                coarse[np.arange(nq), order[:, nprobe]]
            assert cut.any(), where
    finally:
        idx.close()


# 5. list mask: -1 in the same places
def test_list_mask():
    c = cw.kind_case(L2)
    idx = ivf_flat(c)
    try:
        nprobe = 32
        plain = both(idx, c.q, cw.K, nprobe, True, ("mask", "none"))
        mask = (np.random.default_rng(9600).permutation(c.nlist) % 2).astype(
            np.uint8)
        assert mask.sum() == c.nlist // 2
        idx.set_list_mask(mask)
        got = both(idx, c.q, cw.K, nprobe, True, ("mask", "half"))
        want = np.where(mask[plain[2]] != 0, plain[2], -1)
        assert (want == -1).any() and (want >= 0).any()
        assert np.array_equal(got[2], want)
        idx.set_list_mask(None)
        same(plain, both(idx, c.q, cw.K, nprobe, True, ("mask", "cleared")),
             ("mask", "cleared"))
    finally:
        idx.close()


# 6. query counts; nq <= 4 runs, captures and replays a graph
def test_query_counts():
    c = cw.geom_case(1024)
    idx = ivf_flat(c)
    nprobe = 32
    try:
        for nq in (3, 4, 5, 17, 100):
            q = np.ascontiguousarray(c.q[:nq])
            got = both(idx, q, cw.K, nprobe, True, ("nq", nq))
            assert got[2].shape == (nq, nprobe)
        # nq = 1: three searches in a row per switch value (run + capture,
        # replay, replay), the value switched four times on one index; a
        # stale graph would leave last_coarse_wave at the other value
        seen = {}
        for rnd in range(2):
            for wave in (False, True):
                for call in range(3):
                    qi = 3 * rnd + call
                    r = search(idx, c.q[qi:qi + 1], cw.K, nprobe, wave, True,
                               ("nq", 1, rnd, wave, call))
                    if qi in seen:
                        same(seen[qi], r, ("nq", 1, rnd, wave, call))
                    seen[qi] = r
        # and the batch of the same queries selects the same probes
        batch = search(idx, c.q[:6], cw.K, nprobe, True, True, ("nq", 6))
        for qi in range(6):
            assert np.array_equal(batch[2][qi], seen[qi][2][0]), qi
    finally:
        idx.close()


# 7. nprobe >= nlist probes every list on both sides
def test_probes_all():
    c = cw.geom_case(33)
    idx = ivf_flat(c)
    try:
        for nprobe in (c.nlist, c.nlist + 5):
            got = both(idx, c.q, cw.K, nprobe, False, ("all", nprobe))
            assert np.array_equal(
                got[2], np.tile(np.arange(c.nlist, dtype=np.int32),
                                (len(c.q), 1)))
    finally:
        idx.close()
