"""IVF-Flat scan, coarse probing and add-time assignment against the float64
reference model of ivf_reference.py (marked gpu).

The path under test is assign_rows (sgemm_dots -> k_argmin_rows) at add
time and, per search, the coarse selection (k_dots_mfma / rocBLAS ->
k_select_dense -> k_probe_unpack -> k_hist_probes / k_scatter_probes), the
scan k_ivf_scan_pipe in its fused and its store-all form, k_select_u64 and
k_emit, the candidate range kernels, and the row pass bitmap that filters
and tombstones feed.  Every query of every search is held to rules A-D of
flat_reference.check_topk (or to the range rules) over the rows the model
makes eligible: rows of the query's probed lists that are alive and pass the
filter.  The model, the kernel geometry behind the shapes and the QTM each
dimension of the ladder is expected to take are documented in
ivf_reference.py; the searches themselves are the drivers there, which
test_ivf_reference_cpu.py runs dry to assert the strength caps and the
unambiguous probe sets on the reference alone.

Each index first has its own assignment (export_assign) verified against the
float64 centroid scores; the verified assignment defines the lists, and the
list lengths are asserted to be the ones the case was written for.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, REPO, os.path.join(REPO, "dingo-store_amd")]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")
import ivf_reference as ir  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

assert (dg.L2, dg.IP, dg.COSINE) == (L2, IP, COSINE)
MNAME = {L2: "L2", IP: "IP", COSINE: "COSINE"}


@pytest.fixture(scope="module", autouse=True)
def _report_slack():
    yield
    print("\nIVF-Flat: largest |dist - ref| / b per metric:",
          {MNAME[m]: round(v, 4) for m, v in ir.MAX_RATIO.items()})


@pytest.fixture(autouse=True)
def _default_scan_path(monkeypatch):
    monkeypatch.delenv("DG_SCAN_FUSED", raising=False)


def make_dg_filter(spec):
    if spec is None:
        return None
    if spec["kind"] == 1:
        return dg.make_filter(kind=1, negate=spec["negate"],
                              min_id=spec["min_id"], max_id=spec["max_id"])
    if spec["kind"] == 2:
        return dg.make_filter(kind=2, negate=spec["negate"], ids=spec["ids"])
    f = dg.make_filter(kind=3, negate=spec["negate"], bitmap=spec["bitmap"],
                       bitmap_base=spec["bitmap_base"])
    f.bitmap_nbits = spec["bitmap_nbits"]  # not a multiple of 64
    return f


class GpuOps:
    """The driver operations of ivf_reference on a real index."""

    def __init__(self, c):
        self.c = c
        self.idx = dg.Index(dg.IVF_FLAT, c.metric, c.d, nlist=c.nlist)
        self.idx.set_centroids(c.cents)
        self.idx.add(c.ids, c.x)
        self.searches = 0

    def verified_assign(self):
        """The index's assignment, verified row by row; it must also give
        the list lengths the case's geometry rests on."""
        c = self.c
        assign = self.idx.export_assign()
        ir.verify_assign(c.metric, c.x, c.cents, assign,
                         (MNAME[c.metric], c.d))
        assert np.array_equal(np.bincount(assign, minlength=c.nlist), c.lens)
        return assign

    def search(self, where, q, k, nprobe, spec, ref, b, ids, elig, fused):
        gd, gi = self.idx.search(q, k, nprobe=nprobe,
                                 filt=make_dg_filter(spec))
        assert self.idx.last_scan_fused() == fused, where
        ir.check_topk(self.c.metric, gd, gi, ref, b, ids, elig, where)
        self.searches += 1

    def range_search(self, where, q, radius, ref, b, ids, elig):
        lims, rd, ri = self.idx.range_search(q, radius)
        assert not self.idx.last_scan_fused(), where
        ir.check_range(self.c.metric, radius, lims, rd, ri, ref, b, ids,
                       elig, where)
        self.searches += 1

    def remove(self, ids):
        self.idx.remove(ids)

    def upsert(self, ids, vectors):
        self.idx.upsert(ids, vectors)

    def replayed(self, where, expected):
        # dg_stats reports no per-stage timings (last_nq 0) for a replay
        assert (self.idx.stats()["last_nq"] == 0) == expected, where

    def close(self):
        self.idx.close()


def _run(c, driver, *args):
    ops = GpuOps(c)
    try:
        driver(c, ops.verified_assign(), ops, *args)
        assert ops.searches > 0
    finally:
        ops.close()


# --------------------------------------------------------------------------
# A. d pipeline at QTM = 16
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.A_METRICS, ids=lambda m: MNAME[m])
@pytest.mark.parametrize("d", ir.A_DIMS)
def test_d_pipeline(d, metric):
    """Every tail of the 16-dim column pipeline and every dp < 16, over a
    partial wave, a second wave of 4 rows and a second chunk of 3 rows, by a
    full tile of 16 and a half tile of 4 queries: k = 10 fused, and k = N
    store-all, which reads out every (query, row) pair of the scan."""
    assert ir.qtm_of(d) == 16
    _run(ir.case_a(d, metric), ir.run_full_probe, ir.A_K)


# --------------------------------------------------------------------------
# B. d ladder
# --------------------------------------------------------------------------
@pytest.mark.parametrize(
    "d,metric,nq", ir.B_CASES,
    ids=[f"{d}-{MNAME[m]}-nq{nq}" for d, m, nq in ir.B_CASES])
def test_d_ladder(d, metric, nq):
    """Both sides of each QTM threshold and the largest dimension.  QTM the
    dispatch code takes (ivf_scan_col / ivf_scan_topk, not observed): 2304
    -> 16, 2305 and 4608 -> 8, 4609, 8189 and 8192 -> 4.  Nine queries are 9
    of 16, 8 + 1 and 4 + 4 + 1; eight at d = 2304 take the half body at the
    largest LDS tile."""
    assert ir.qtm_of(d) == ir.B_QTM[d]
    _run(ir.case_b(d, metric, nq), ir.run_full_probe, ir.B_K)


# --------------------------------------------------------------------------
# C. wave, chunk and tile edges under partial probing
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP, COSINE], ids=lambda m: MNAME[m])
def test_edges_partial_probing(metric):
    """nprobe 1 and 3 with k 1, 10, 64 fused; k = 65 store-all by k; nprobe
    = 9 with k = 64 store-all by size (6912 slots > 5893 rows)."""
    _run(ir.case_c(metric), ir.run_c)


# --------------------------------------------------------------------------
# D. filters, tombstones and upsert under partial probing
# --------------------------------------------------------------------------
def test_filters_tombstones_upsert():
    _run(ir.case_c(L2), ir.run_d)


# --------------------------------------------------------------------------
# E. range search with partial probing
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.E_METRICS, ids=lambda m: MNAME[m])
def test_range_partial_probing(metric):
    """The default nprobe of 80 leaves 16 of 96 lists out; rows of those
    lists lie inside the widest radius and must not come back."""
    _run(ir.case_e(metric), ir.run_e)


# --------------------------------------------------------------------------
# F. graph replay
# --------------------------------------------------------------------------
@pytest.mark.parametrize("nq", ir.F_NQS)
def test_graph_replay(nq):
    """nq <= 4 without a filter: the first call runs and captures, the next
    three replay with other queries (other probe sets); a remove forces a
    recapture, and the two calls after it must leave the removed row out."""
    _run(ir.case_c(L2), ir.run_f, nq)
