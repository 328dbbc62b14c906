"""Pair scan, k_ivf_scan_mfma2 (marked gpu).

A list probed by 17 or more queries is scanned two 16-query tiles per pass
over its rows by k_ivf_scan_mfma2; k_ivf_scan_mfma keeps single tiles and the
odd last tile (dg_scan_split.h; tests/test_scan_split_cpu.py covers the
split itself).  Every (query, row) dot is the same k-ordered MFMA chain on
either kernel, so every search must be BIT-identical (ids, and distances
viewed as uint32) under three settings of one index in one process:

  default            pair kernel + k_ivf_scan_mfma   last_scan_pair() as
                                                     intended by the case
  DG_SCAN_PAIR=0     k_ivf_scan_mfma alone           last_scan_pair() False
  DG_SCAN_FUSED=0    store-all scan + select         the independent yardstick

and pass the float64 rules of ivf_reference.py (ir.topk -> check_topk)
unchanged.  The pair kernel is intended exactly when the search is fused,
nq > 16 and d <= 2304.

Geometry the shapes rest on: see tests/test_scan_mfma.py (k-step 4 dims,
period 16 dims, wave 256 rows, chunk 1024 rows, tile 16 queries); the pair
kernel has one instance for d <= 16 (a single period, no dim loop) and one
for longer rows, and strides blockIdx.y over a list's pairs (grid.y 2 by
default, DG_SCAN_PAIR=1 / 4 set it).
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
KS = [1, 10, 64]
# queries per list: no pair; a pair whose second tile has 1 or 15 queries; an
# exact pair; pair + odd tile; pair + 15; two pairs; two pairs + odd tile (1
# query, and whole); three pairs + odd tile (more pairs than grid.y = 2)
QPLS = [16, 17, 31, 32, 33, 47, 48, 49, 64, 65, 97]
# every value once on a list of at most one 1024-row chunk (1 to 1024 rows:
# less than a wave, a wave, several waves) and once on a multi-chunk list
ONE_CHUNK = [1, 3, 255, 256, 257, 1023, 1024]
MULTI_CHUNK = [1025, 2049]
LENS, QPL = [], []
for _j, _n in enumerate(QPLS):
    LENS += [ONE_CHUNK[_j % len(ONE_CHUNK)], MULTI_CHUNK[_j % 2]]
    QPL += [_n, _n]
assert set(LENS) == {1, 3, 255, 256, 257, 1023, 1024, 1025, 2049}
assert {d % 16 for d in DIMS} == {4, 8, 12, 0} and len(LENS) <= 24


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
def scan_env(fused=True, pair=None):
    """DG_SCAN_FUSED / DG_SCAN_PAIR for the calls inside (read per call);
    pair None leaves the default, 0 turns the pair kernel off, 1 / 2 / 4 set
    its grid.y."""
    want = {"DG_SCAN_FUSED": None if fused else "0",
            "DG_SCAN_PAIR": None if pair is None else str(pair)}
    old = {v: os.environ.get(v) for v in want}
    try:
        for var, val in want.items():
            if val is None:
                os.environ.pop(var, None)
            else:
                os.environ[var] = val
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


def pair_intended(nq, d):
    return nq > 16 and ir.qtm_of(d) == 16


class ThreeSettingOps:
    """ivf_reference driver operations on a real index; each search runs
    under the default, DG_SCAN_PAIR=0 and DG_SCAN_FUSED=0 (and under the
    extra grid.y values of `pys`)."""

    def __init__(self, c, pys=()):
        self.c = c
        self.pys = tuple(pys)
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
        intended = pair_intended(len(q), self.c.d)
        got = {}
        settings = [("default", True, None, intended),
                    ("pair_off", True, 0, False),
                    ("store_all", False, None, False)]
        settings += [("py%d" % py, True, py, intended) for py in self.pys]
        for name, f_on, pair, want_pair in settings:
            with scan_env(f_on, pair):
                got[name] = self.idx.search(q, k, nprobe=nprobe, filt=filt)
                assert self.idx.last_scan_fused() == f_on, (where, name)
                assert self.idx.last_scan_mfma() == f_on, (where, name)
                assert self.idx.last_scan_pair() == want_pair, (where, name)
        for name in got:
            if name != "default":
                same_bits(got["default"], got[name],
                          (where, "default vs " + name))
        ir.check_topk(self.c.metric, got["default"][0], got["default"][1],
                      ref, b, ids, elig, where)
        self.searches += 1

    def remove(self, ids):
        self.idx.remove(ids)

    def close(self):
        self.idx.close()


def run_case(c, body, pys=()):
    ops = ThreeSettingOps(c, pys)
    try:
        body(ops, ops.verified_assign())
        assert ops.searches > 0
    finally:
        ops.close()


def shapes_case(seed, d, metric):
    return make_case(seed, LENS, d, metric,
                     np.repeat(np.arange(len(LENS)), QPL))


# --------------------------------------------------------------------------
# shapes: d x list length x queries per list x k x metric
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", DIMS)
def test_shapes(d, metric):
    """nprobe = 1: each list is scanned by exactly its QPL queries, so the
    tiles per list are 1 .. 7 as laid out above; k = 1, 10, 64 (lists shorter
    than k give padding out of slots that are never written).  At d = 32 / L2
    the pair kernel also runs with grid.y 1 (one block strides over all three
    pairs of the 97-query lists) and 4 (more blocks than pairs)."""
    c = shapes_case(60000 + 10 * d + metric, d, metric)
    ref, b = ir.refb(c)
    alive = np.ones(c.n, bool)

    def body(ops, assign):
        for k in KS:
            ir.topk(ops, c, (MNAME[metric], d, "k", k), c.q, k, 1, None, ref,
                    b, assign, alive)

    run_case(c, body, pys=(1, 4) if (d, metric) == (32, L2) else ())


# --------------------------------------------------------------------------
# d = 768 and the first d past the 16-query rung
# --------------------------------------------------------------------------
@pytest.mark.parametrize("d", [768, 2308])
def test_long_rows(d):
    """33 queries (a pair and an odd tile) on a 258-row list, 17 on a 3-row
    list.  d = 768: 48 whole periods.  d = 2308 is the first d above 2304:
    the tile ladder is at 8 queries, the pair kernel must not launch."""
    assert pair_intended(50, d) == (d == 768)
    c = make_case(d, [3, 258], d, L2, [0] * 17 + [1] * 33, sigma=0.125)
    ref, b = ir.refb(c)

    def body(ops, assign):
        ir.topk(ops, c, ("long rows", d), c.q, 10, 1, None, ref, b, assign,
                np.ones(c.n, bool))

    run_case(c, body)


# --------------------------------------------------------------------------
# mixed lists in one launch
# --------------------------------------------------------------------------
def test_mixed_lists():
    """nprobe = 3: a query sits in its own list at rank 0 and in two
    neighbours at ranks 1 and 2, so a list's tiles mix queries of different
    ranks.  The same launch holds lists with one tile, an even and an odd
    number (>= 3) of tiles, and a list nobody probes."""
    lens = [300, 1100, 40, 2100, 700, 5, 260, 90, 1500, 33, 64, 1024]
    qcount = [40, 3, 0, 21, 9, 0, 0, 0, 0, 0, 0, 0]
    c = make_case(71, lens, 20, L2, np.repeat(np.arange(len(lens)), qcount))
    ref, b = ir.refb(c)
    probed, amb = ir.probe_sets(c.metric, c.q, c.cents, 3)
    assert len(amb) == 0
    tiles = -(-probed.sum(0) // 16)
    assert (tiles == 0).any() and (tiles == 1).any()
    assert ((tiles >= 2) & (tiles % 2 == 0)).any()
    assert ((tiles >= 3) & (tiles % 2 == 1)).any()

    def body(ops, assign):
        for k in (10, 64):
            ir.topk(ops, c, ("mixed", k), c.q, k, 3, None, ref, b, assign,
                    np.ones(c.n, bool))

    run_case(c, body)


# --------------------------------------------------------------------------
# ties on paired lists
# --------------------------------------------------------------------------
T_D, T_LEN = 16, 1100
T_BEST_AT = [0, 1, 2, 4, 9, 64, 130, 256, 515, 1023, 1024, 1099]


@pytest.mark.parametrize("metric", [L2, IP], ids=lambda m: MNAME[m])
def test_ties(metric):
    """The tie lists of tests/test_scan_mfma.py, probed by 33 (list 0: 1100
    copies of one vector) and 20 (list 1: the best vector planted at
    T_BEST_AT) queries: equal keys in every component, lane, 64-row group,
    wave and in both chunks reach both accumulator sets of the pair kernel
    and the single-tile kernel, and every setting must break every tie
    toward the smaller row."""
    rng = np.random.default_rng(177 + metric)
    lens = [T_LEN, T_LEN, 5]
    cents = cell24(3, T_D, 10.0)
    v1 = cents[0] + 0.3 * rng.standard_normal(T_D)
    u = cents[1] + 0.3 * rng.standard_normal((5, T_D))
    pat = 1 + np.arange(T_LEN) % 4
    pat[T_BEST_AT] = 0
    x = np.concatenate([np.repeat(v1[None], T_LEN, 0), u[pat],
                        cents[2] + 0.3 * rng.standard_normal((5, T_D))])
    qdir = cents[1] / 10.0
    u0q = u[0] + 0.15 * rng.standard_normal((20, T_D)) + 2.0 * qdir
    x[T_LEN:2 * T_LEN][pat == 0] = u[0] + 2.0 * qdir
    q = np.concatenate([u0q, v1 + 0.15 * rng.standard_normal((33, T_D))])
    c = make_case(0, lens, T_D, metric, [1] * 20 + [0] * 33, x=x, q=q)
    ref, b = ir.refb(c)
    best = np.argsort(ref[0] * fr.better_sign(metric), kind="stable")
    assert set(best[:len(T_BEST_AT)]) == {T_LEN + p for p in T_BEST_AT}

    def body(ops, assign):
        for nprobe in (1, 3):
            for k in KS:
                ir.topk(ops, c, ("ties", MNAME[metric], nprobe, k), c.q, k,
                        nprobe, None, ref, b, assign, np.ones(c.n, bool))
        # the copies carry equal distances, and 64 of 1100 are returned
        with scan_env():
            gd, gi = ops.idx.search(c.q[20:], 64, nprobe=1)
            assert ops.idx.last_scan_pair()
        assert (gd == gd[:, :1]).all() and (gi < c.ids[T_LEN]).all()
        assert all(len(set(r)) == 64 for r in gi.tolist())

    run_case(c, body)


# --------------------------------------------------------------------------
# masks on paired lists
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mask_case():
    return shapes_case(61000, 32, L2)


def _first_list(n_rows):
    return LENS.index(n_rows)


def test_id_range_filter(mask_case):
    """A range that starts inside a 257-row list and ends inside a 2049-row
    list (lists in between pass whole, lists outside not at all)."""
    c = mask_case
    ref, b = ir.refb(c)
    lo, hi = _first_list(257), len(LENS) - 1 - LENS[::-1].index(2049)
    assert lo < hi
    spec = dict(kind=1, negate=False, min_id=int(c.ids[c.off[lo] + 100]),
                max_id=int(c.ids[c.off[hi] + 1700]))

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
        edge = [int(c.off[_first_list(1024)]) + 1023,
                int(c.off[_first_list(1025)]) + 1023,
                int(c.off[_first_list(2049)]) + 2047]
        s = _first_list(3)
        short = list(range(int(c.off[s]), int(c.off[s + 1])))
        victims = np.unique(np.array(short + best + edge))
        ops.remove(c.ids[victims])
        alive[victims] = False
        for nprobe, k in ((1, 10), (3, 64)):
            ir.topk(ops, c, ("tombstones", nprobe, k), c.q, k, nprobe, None,
                    ref, b, assign, alive)

    run_case(c, body)


# --------------------------------------------------------------------------
# small batches
# --------------------------------------------------------------------------
def test_small_nq(mask_case):
    """16 queries cannot fill two tiles: the pair kernel is not launched,
    whatever the switch says, and the results do not depend on it.  nq <= 4
    without a filter is captured into a graph on its first call and replayed
    on the second (last_nq == 0): the pair kernel is in neither, and a
    flipped DG_SCAN_PAIR captures afresh (it is part of the graph key)."""
    c = mask_case
    first = int(np.nonzero(c.qlists == _first_list(2049))[0][0])
    idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist)
    try:
        idx.set_centroids(c.cents)
        idx.add(c.ids, c.x)
        for nq in (16, 4, 1):
            q = c.q[first:first + nq]
            with scan_env(fused=False):
                want = idx.search(q, 10, nprobe=3)
            for pair in (None, 0, None):
                for call in range(2):
                    with scan_env(True, pair):
                        got = idx.search(q, 10, nprobe=3)
                        replay = idx.stats()["last_nq"] == 0
                        assert replay == (nq <= 4 and call == 1), \
                            (nq, pair, call)
                        assert idx.last_scan_fused() and idx.last_scan_mfma()
                        assert not idx.last_scan_pair(), (nq, pair, call)
                    same_bits(got, want, ("small nq", nq, pair, call))
    finally:
        idx.close()
