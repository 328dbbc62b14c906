"""f32-MFMA fused top-k scan, k_ivf_scan_mfma (marked gpu).

The default IVF-Flat top-k scan forms its dots with v_mfma_f32_16x16x4_f32
and selects each wave's k smallest from the MFMA register layout.  The MFMA
sums a k-ordered fmaf chain, which is what the VALU kernels compute, so every
search must be BIT-identical (ids, and distances viewed as uint32) on three
paths of one index in one process:

  default            k_ivf_scan_mfma             fused, mfma
  DG_SCAN_MFMA=0     k_ivf_scan_pipe<..,1,1>     fused, VALU
  DG_SCAN_FUSED=0    store-all scan + select     the independent yardstick

dg_last_scan_fused / dg_last_scan_mfma confirm which kernel ran, and every
result is also checked against the float64 model of ivf_reference.py under
that module's rules (ir.topk -> check_topk), unchanged.

Geometry the shapes rest on: a k-step is 4 dims, the load pipeline has a
period of 4 k-steps (16 dims) and a prologue of 4, so d = 4, 8, 12 are
shorter than the prologue and d % 16 in {4, 8, 12, 0} are the four tails; a
lane holds rows 64 m + 4 j + x (m, x = 0..3) of its wave's 256, a block one
1024-row chunk, a query tile 16 queries (4 per 16-lane row of the wave).
"""
import contextlib
import os
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")
import flat_reference as fr  # noqa: E402
import ivf_reference as ir  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

assert (dg.L2, dg.IP, dg.COSINE) == (L2, IP, COSINE)
MNAME = {L2: "L2", IP: "IP", COSINE: "COSINE"}

DIMS = [4, 8, 12, 16, 20, 28, 32, 48]
LENS = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]
# queries per list at nprobe = 1: every value of {1, 4, 5, 16, 17, 33} on a
# list of at most one wave and on a list of several waves or chunks
QPL = [4, 5, 16, 17, 33, 1, 17, 33, 1, 4, 5, 16]
KS = [1, 10, 64]
assert {d % 16 for d in DIMS} == {4, 8, 12, 0} and len(QPL) == len(LENS)
assert set(QPL) == {1, 4, 5, 16, 17, 33}


def cell24(nlist, d, scale):
    """Equal-norm centroids at least 60 degrees apart in the first four
    dimensions (vertices of the 24-cell), so that the L2, IP and cosine
    assignments agree and are far from ambiguous at every d >= 4."""
    v = []
    for a in range(4):
        for b in range(a + 1, 4):
            for sa in (1.0, -1.0):
                for sb in (1.0, -1.0):
                    p = np.zeros(4)
                    p[a], p[b] = sa, sb
                    v.append(p / np.sqrt(2.0))
    assert nlist <= len(v) and d >= 4
    c = np.zeros((nlist, d), np.float32)
    c[:, :4] = scale * np.array(v[:nlist])
    return c


def make_case(seed, lens, d, metric, qlists, x=None, q=None, sigma=0.3):
    """The fields ir.topk reads (see ivf_reference.make_case): rows list by
    list, row position p has id 5 p + 11.  Rows and queries are Gaussian
    around the centroids unless given: every value differs from every other,
    so a swapped query / row index or a permuted dim cannot pass."""
    rng = np.random.default_rng(seed)
    nlist = len(lens)
    cents = cell24(nlist, d, 10.0)
    owner = np.repeat(np.arange(nlist), lens).astype(np.int32)
    n = len(owner)
    if x is None:
        x = cents[owner] + sigma * rng.standard_normal((n, d))
    qlists = np.asarray(qlists)
    if q is None:
        q = cents[qlists] + sigma * rng.standard_normal((len(qlists), d))
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return types.SimpleNamespace(
        metric=metric, d=d, lens=list(lens), nlist=nlist, n=n, cents=cents,
        x=np.ascontiguousarray(x, np.float32),
        q=np.ascontiguousarray(q, np.float32), qlists=qlists, owner=owner,
        off=off, ids=5 * np.arange(n, dtype=np.int64) + 11)


@contextlib.contextmanager
def scan_env(fused, mfma):
    """DG_SCAN_FUSED / DG_SCAN_MFMA for the calls inside (read per call)."""
    old = {v: os.environ.get(v) for v in ("DG_SCAN_FUSED", "DG_SCAN_MFMA")}
    try:
        for var, on in (("DG_SCAN_FUSED", fused), ("DG_SCAN_MFMA", mfma)):
            if on:
                os.environ.pop(var, None)
            else:
                os.environ[var] = "0"
        yield
    finally:
        for var, val in old.items():
            if val is None:
                os.environ.pop(var, None)
            else:
                os.environ[var] = val


def make_dg_filter(spec):
    if spec is None:
        return None
    assert spec["kind"] == 1
    return dg.make_filter(kind=1, negate=spec["negate"],
                          min_id=spec["min_id"], max_id=spec["max_id"])


def same_bits(a, b, where):
    assert np.array_equal(a[1], b[1]), (where, "ids")
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), \
        (where, "distance bits")


class ThreePathOps:
    """ivf_reference driver operations on a real index; each search runs the
    MFMA, the VALU-fused and the store-all path."""

    def __init__(self, c):
        self.c = c
        self.idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist)
        self.idx.set_centroids(c.cents)
        self.idx.add(c.ids, c.x)
        self.searches = 0

    def verified_assign(self):
        c = self.c
        assign = self.idx.export_assign()
        ir.verify_assign(c.metric, c.x, c.cents, assign,
                         (MNAME[c.metric], c.d))
        assert np.array_equal(np.bincount(assign, minlength=c.nlist), c.lens)
        return assign

    def search(self, where, q, k, nprobe, spec, ref, b, ids, elig, fused):
        assert fused, (where, "the case must take the fused path")
        filt = make_dg_filter(spec)
        got = {}
        for name, f_on, m_on in (("mfma", True, True), ("valu", True, False),
                                 ("store_all", False, True)):
            with scan_env(f_on, m_on):
                got[name] = self.idx.search(q, k, nprobe=nprobe, filt=filt)
                assert self.idx.last_scan_fused() == f_on, (where, name)
                assert self.idx.last_scan_mfma() == (f_on and m_on), \
                    (where, name)
        same_bits(got["mfma"], got["valu"], (where, "mfma vs valu"))
        same_bits(got["mfma"], got["store_all"], (where, "mfma vs store-all"))
        ir.check_topk(self.c.metric, got["mfma"][0], got["mfma"][1], ref, b,
                      ids, elig, where)
        self.searches += 1

    def remove(self, ids):
        self.idx.remove(ids)

    def close(self):
        self.idx.close()


def run_case(c, body):
    ops = ThreePathOps(c)
    try:
        body(ops, ops.verified_assign())
        assert ops.searches > 0
    finally:
        ops.close()


# --------------------------------------------------------------------------
# shapes: d x list length x queries per list x k x metric
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", DIMS)
def test_shapes(d, metric):
    """nprobe = 1 (each list scanned by exactly its QPL queries) and
    nprobe = 3, k = 1, 10, 64; lists shorter than k give padding out of
    slots that are never written."""
    c = make_case(40000 + 10 * d + metric, LENS, d, metric,
                  np.repeat(np.arange(len(LENS)), QPL))
    ref, b = ir.refb(c)
    alive = np.ones(c.n, bool)

    def body(ops, assign):
        for nprobe, ks in ((1, KS), (3, [10])):
            for k in ks:
                ir.topk(ops, c, (MNAME[metric], d, "nprobe", nprobe, "k", k),
                        c.q, k, nprobe, None, ref, b, assign, alive)

    run_case(c, body)


# --------------------------------------------------------------------------
# the QTM = 8 and QTM = 4 instantiations (queries past the tile read zeros)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2308, 4612])
def test_narrow_tiles(d):
    """9 queries on a 258-row list: 8 + 1 at QTM = 8, 4 + 4 + 1 at QTM = 4;
    d % 16 = 4, a one-step tail after 144 or 288 whole periods."""
    assert ir.qtm_of(d) == (8 if d == 2308 else 4) and d % 16 == 4
    rng = np.random.default_rng(d)
    c = make_case(d, [3, 258], d, L2, rng.integers(0, 2, 9), sigma=0.125)
    ref, b = ir.refb(c)

    def body(ops, assign):
        ir.topk(ops, c, ("narrow", d), c.q, 10, c.nlist, None, ref, b, assign,
                np.ones(c.n, bool))

    run_case(c, body)


# --------------------------------------------------------------------------
# ties
# --------------------------------------------------------------------------
T_D, T_LEN = 16, 1100
# arrival positions of the copies of the best vector in the patterned list:
# x = 0, 1, 2 of one lane, other lanes, other 64-row groups, other waves, the
# chunk's last row and the second chunk (the CSR order follows the arrival
# order when the scatter's cursor retires in order; with any other order the
# copies still tie, somewhere else)
T_BEST_AT = [0, 1, 2, 4, 9, 64, 130, 256, 515, 1023, 1024, 1099]


@pytest.mark.parametrize("metric", [L2, IP], ids=lambda m: MNAME[m])
def test_ties(metric):
    """List 0: 1100 copies of one vector, so equal keys sit in every
    component, lane, 64-row group, wave and in both chunks, and the winners
    are decided by the row alone.  List 1: five distinct vectors, the best
    one at T_BEST_AT and the others cycling, so that the winners themselves
    come from different components, lanes, groups, waves and chunks.  All
    three paths must break every tie toward the smaller row."""
    rng = np.random.default_rng(77 + metric)
    lens = [T_LEN, T_LEN, 5]
    cents = cell24(3, T_D, 10.0)
    v1 = cents[0] + 0.3 * rng.standard_normal(T_D)
    u = cents[1] + 0.3 * rng.standard_normal((5, T_D))
    pat = 1 + np.arange(T_LEN) % 4
    pat[T_BEST_AT] = 0
    x = np.concatenate([np.repeat(v1[None], T_LEN, 0), u[pat],
                        cents[2] + 0.3 * rng.standard_normal((5, T_D))])
    # under IP the best row has the largest dot: push u0 / the queries along
    # the centroid direction so that u0 is the best under both metrics
    qdir = cents[1] / 10.0
    u0q = u[0] + 0.15 * rng.standard_normal((3, T_D)) + 2.0 * qdir
    x[T_LEN:2 * T_LEN][pat == 0] = u[0] + 2.0 * qdir
    q = np.concatenate([u0q, v1 + 0.15 * rng.standard_normal((2, T_D))])
    c = make_case(0, lens, T_D, metric, [1, 1, 1, 0, 0], x=x, q=q)
    ref, b = ir.refb(c)
    best = np.argsort(ref[0] * fr.better_sign(metric), kind="stable")
    assert set(best[:len(T_BEST_AT)]) == {T_LEN + p for p in T_BEST_AT}

    def body(ops, assign):
        for nprobe in (1, 3):
            for k in KS:
                ir.topk(ops, c, ("ties", MNAME[metric], nprobe, k), c.q, k,
                        nprobe, None, ref, b, assign, np.ones(c.n, bool))
        # the copies carry equal distances, and 64 of 1100 are returned
        with scan_env(True, True):
            gd, gi = ops.idx.search(c.q[3:], 64, nprobe=1)
        assert (gd == gd[:, :1]).all() and (gi < c.ids[T_LEN]).all()
        assert all(len(set(r)) == 64 for r in gi.tolist())

    run_case(c, body)


# --------------------------------------------------------------------------
# masks
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mask_case():
    return make_case(51000, LENS, 32, L2,
                     np.repeat(np.arange(len(LENS)), QPL))


def test_id_range_filter(mask_case):
    """A range that cuts through the 257- to 1025-row lists and leaves
    nothing of the short ones."""
    c = mask_case
    ref, b = ir.refb(c)
    spec = dict(kind=1, negate=False, min_id=int(c.ids[c.off[7] + 100]),
                max_id=int(c.ids[c.off[10] + 700]))

    def body(ops, assign):
        for nprobe, k in ((1, 10), (3, 64)):
            ir.topk(ops, c, ("range", nprobe, k), c.q, k, nprobe, spec, ref,
                    b, assign, np.ones(c.n, bool))

    run_case(c, body)


def test_tombstones(mask_case):
    """Removed: the whole 3-row list, the reference best row of every third
    query, and the last row of a full chunk of the long lists."""
    c = mask_case
    ref, b = ir.refb(c)
    probed, _ = ir.probe_sets(c.metric, c.q, c.cents, 1)
    alive = np.ones(c.n, bool)

    def body(ops, assign):
        elig = ir.eligible(probed, assign, alive)
        best = [int(np.nonzero(elig[i])[0][np.argmin(ref[i, elig[i]])])
                for i in range(0, len(c.q), 3)]
        edge = [int(c.off[9]) + 1023, int(c.off[10]) + 1023,
                int(c.off[11]) + 2047]
        short = list(range(int(c.off[1]), int(c.off[2])))
        victims = np.unique(np.array(short + best + edge))
        ops.remove(c.ids[victims])
        alive[victims] = False
        for nprobe, k in ((1, 10), (3, 64)):
            ir.topk(ops, c, ("tombstones", nprobe, k), c.q, k, nprobe, None,
                    ref, b, assign, alive)

    run_case(c, body)


# --------------------------------------------------------------------------
# graph replay
# --------------------------------------------------------------------------
def test_graph_key_holds_the_switch(mask_case):
    """nq = 1 without a filter is captured into a graph and replayed.  A
    flipped DG_SCAN_MFMA must not replay the other kernel's graph: the first
    call after each flip runs its kernels (dg_stats reports stage timings,
    last_nq != 0, and dg_last_scan_mfma follows the switch), the second
    replays (last_nq == 0)."""
    c = mask_case
    q = c.q[40:41]
    idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist)
    try:
        idx.set_centroids(c.cents)
        idx.add(c.ids, c.x)
        with scan_env(False, True):
            want = idx.search(q, 10, nprobe=3)
        for mfma in (True, False, True):
            for call in range(2):
                with scan_env(True, mfma):
                    got = idx.search(q, 10, nprobe=3)
                    replay = idx.stats()["last_nq"] == 0
                    assert replay == (call == 1), (mfma, call)
                    assert idx.last_scan_fused()
                    assert idx.last_scan_mfma() == mfma, (mfma, call)
                same_bits(got, want, ("graph", mfma, call))
    finally:
        idx.close()
