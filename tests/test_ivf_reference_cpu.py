"""The IVF-Flat float64 reference model and its checks, without a GPU.

  1. every case table of test_ivf_exact.py has the assignment its geometry
     rests on, and its drivers run dry: the strength caps (1 % top-k, 5 %
     range band) and zero ambiguous probe sets hold on the reference alone,
     for exactly the searches the GPU file makes;
  2. the reference agrees with the CPU oracle (ivf_search /
     ivf_range_search) on a small case;
  3. planted defects: a numpy float32 emulation of the search (coarse top
     nprobe, chunks of 1024 rows stored dim-major and padded to 4 rows,
     query tiles, 4-dim column groups, per-wave top-k slots or all
     candidates, the merge, the emit) passes the checks clean and is
     rejected with each one of the defects.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "oracle")]

import flat_reference as fr  # noqa: E402
import ivf_reference as ir  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

orc = pytest.importorskip("pyoracle")

METRICS = [L2, IP, COSINE]


# --------------------------------------------------------------------------
# 1. the tables: assignment, strength, unambiguous probe sets
# --------------------------------------------------------------------------
def _assignment_is_the_tables(c):
    """The float64 assignment is the intended one and no row is a near tie,
    so a correct index has lists of exactly c.lens rows.  The exact-zero
    rows of the one-dimensional IP case tie by construction."""
    a, clear = ir.reference_assign(c.metric, c.x, c.cents)
    assert np.array_equal(a, c.owner)
    assert np.array_equal(np.bincount(a, minlength=c.nlist), c.lens)
    tie = ~clear
    if c.d == 1 and c.metric != L2:
        assert (c.x[tie] == 0).all() and (c.owner[tie] == 0).all()
    else:
        assert not tie.any()
    ir.verify_assign(c.metric, c.x, c.cents, c.owner)
    return a


def _dry(c, driver, *args):
    ops = ir.DryOps()
    driver(c, _assignment_is_the_tables(c), ops, *args)
    return ops.searches


def test_geometry_tables():
    assert [ir.qtm_of(d) for d in (1, 64, 2301, 2304)] == [16] * 4
    assert [ir.qtm_of(d) for d in (2305, 4605, 4608)] == [8] * 3
    assert [ir.qtm_of(d) for d in (4609, 8189, 8192)] == [4] * 3
    assert [ir.tail_of(d) for d in (1, 4, 5, 12, 13, 16, 17, 20, 32, 33,
                                    36, 2305, 4609, 8189)] == \
        [4, 4, 8, 12, 16, 16, 4, 4, 16, 4, 4, 4, 4, 16]
    # lists of 5, 260, 1027: 1, 2 and 5 waves, the last with 5, 4 and 3 rows
    assert [-(-n // 256) for n in ir.A_LENS] == [1, 2, 5]
    assert ir.expect_fused(10, 3, ir.A_LENS)
    assert not ir.expect_fused(65, 3, ir.A_LENS)
    assert ir.expect_fused(10, 2, ir.B_LENS)


@pytest.mark.parametrize("metric", ir.A_METRICS)
def test_tables_d_pipeline(metric):
    for d in ir.A_DIMS:
        assert _dry(ir.case_a(d, metric), ir.run_full_probe, ir.A_K) == 2


def test_tables_d_ladder():
    for d, metric, nq in ir.B_CASES:
        c = ir.case_b(d, metric, nq)
        assert len(c.q) == nq
        assert _dry(c, ir.run_full_probe, ir.B_K) == 2


@pytest.mark.parametrize("metric", METRICS)
def test_tables_edges_partial_probing(metric):
    c = ir.case_c(metric)
    assert np.array_equal(np.bincount(c.qlists), ir.C_QPL)
    assert _dry(c, ir.run_c) == len(ir.C_FUSED) + len(ir.C_STORE_ALL)


def test_tables_filters_tombstones_upsert():
    assert _dry(ir.case_c(L2), ir.run_d) == 2 * 6 * 2 + 2


@pytest.mark.parametrize("metric", ir.E_METRICS)
def test_tables_range_partial_probing(metric):
    assert _dry(ir.case_e(metric), ir.run_e) == 3


@pytest.mark.parametrize("nq", ir.F_NQS)
def test_tables_graph_replay(nq):
    assert _dry(ir.case_c(L2), ir.run_f, nq) == ir.F_CALLS + 2


def test_assignment_check_rejects_a_wrong_list():
    c = ir.case_c(L2)
    wrong = c.owner.copy()
    wrong[1000] = (wrong[1000] + 1) % c.nlist
    with pytest.raises(AssertionError):
        ir.verify_assign(c.metric, c.x, c.cents, wrong)


# --------------------------------------------------------------------------
# 2. reference vs the CPU oracle
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [L2, IP])
def test_reference_matches_oracle_topk(metric):
    c = ir.case_c(metric)
    assign = orc.ivf_assign(metric, c.x, c.cents)
    ir.verify_assign(metric, c.x, c.cents, assign)
    off, gv, gids = orc.ivf_build(c.x, c.ids, c.nlist, assign)
    ref, b = ir.refb(c)
    for nprobe, k in ((1, 10), (3, 10), (3, 65)):
        probed, amb = ir.probe_sets(metric, c.q, c.cents, nprobe)
        assert len(amb) == 0
        elig = ir.eligible(probed, assign, np.ones(c.n, bool))
        od, oi = orc.ivf_search(metric, c.cents, off, gv, gids, c.q, k,
                                nprobe)
        assert fr.check_topk(metric, od, oi, ref, b, c.ids, elig) <= 1.0


@pytest.mark.parametrize("metric", ir.E_METRICS)
def test_reference_matches_oracle_range(metric):
    c = ir.case_e(metric)
    assign = orc.ivf_assign(metric, c.x, c.cents)
    ir.verify_assign(metric, c.x, c.cents, assign)
    off, gv, gids = orc.ivf_build(c.x, c.ids, c.nlist, assign)
    ref, b = ir.refb(c)
    probed, amb = ir.probe_sets(metric, c.q, c.cents, 0)
    assert len(amb) == 0
    elig = ir.eligible(probed, assign, np.ones(c.n, bool))
    sg = fr.better_sign(metric)
    for radius in fr.range_radii(metric, ref, elig):
        lims, od, oi = orc.ivf_range_search(metric, c.cents, off, gv, gids,
                                            c.q, radius, ir.DEFAULT_NPROBE)
        for i in range(len(c.q)):  # the oracle lists rows in scan order
            a, z = lims[i], lims[i + 1]
            order = np.lexsort((oi[a:z], sg * od[a:z]))
            od[a:z], oi[a:z] = od[a:z][order], oi[a:z][order]
        fr.check_range(metric, radius, lims, od, oi, ref, b, c.ids, elig)


# --------------------------------------------------------------------------
# 3. planted defects
# --------------------------------------------------------------------------
def _f32_stored(metric, v):
    v = np.asarray(v, np.float32)
    if metric == COSINE:
        n = np.sqrt((v.astype(np.float64) ** 2).sum(1, keepdims=True))
        v = (v / n).astype(np.float32)
    return v


def emulate(c, k, nprobe, defect=None, at=None):
    """float32 model of one IVF-Flat top-k search of case c with one
    optional defect; `at` places it (see the callers).  Returns (dist
    [nq, k] f32, ids [nq, k] i64, -1 / 0.0 padded)."""
    metric, d = c.metric, c.d
    dp = ir.dp_of(d)
    qtm = ir.qtm_of(d)
    nq = len(c.q)
    x = np.zeros((c.n, dp), np.float32)
    x[:, :d] = _f32_stored(metric, c.x)
    q = np.zeros((nq, dp), np.float32)
    q[:, :d] = _f32_stored(metric, c.q)
    cents = np.zeros((c.nlist, dp), np.float32)
    cents[:, :d] = c.cents
    vnorm = (x * x).sum(1, dtype=np.float32)
    qn = (q * q).sum(1, dtype=np.float32)
    fused = ir.expect_fused(k, nprobe, c.lens)
    # coarse: the nprobe best lists, ties toward the smaller list
    cd = (q @ cents.T).astype(np.float32)
    cs = (cents * cents).sum(1, dtype=np.float32)[None, :] - \
        np.float32(2) * cd if metric == L2 else -cd
    np_ = min(nprobe, c.nlist)
    probes = []
    for qi in range(nq):
        order = np.lexsort((np.arange(c.nlist), cs[qi]))
        p = list(order[:np_])
        if defect == "probe_swap" and qi == at:
            p[-1] = order[np_]
        probes.append(p)
    cand = [[] for _ in range(nq)]  # (key f32, internal row) pairs
    csr = np.argsort(c.owner, kind="stable")  # CSR row -> arrival row
    for l in range(c.nlist):
        lrows = csr[c.off[l]:c.off[l + 1]]
        qs = [qi for qi in range(nq) if l in probes[qi]]
        for ch in range(-(-len(lrows) // ir.CHUNK)):
            rows = lrows[ch * ir.CHUNK:(ch + 1) * ir.CHUNK]
            nrows = len(rows)
            pad = (nrows + 3) // 4 * 4
            col = np.zeros((dp, pad), np.float32)  # dim-major, zero padded
            col[:, :nrows] = x[rows].T
            live = nrows
            if defect == "row_group" and (l, ch) == at:
                live = pad - 4  # the last group of 4 padded rows is skipped
            vn = vnorm[rows]
            if defect == "vnorm_shift":
                vn = vnorm[np.minimum(rows + 1, c.n - 1)]  # the neighbour's
            for t0 in range(0, len(qs), qtm):
                tile = qs[t0:t0 + qtm]
                qt = np.zeros((qtm, dp), np.float32)  # unused slots are zero
                qt[:len(tile)] = q[tile]
                acc = np.zeros((qtm, pad), np.float32)
                groups = dp // 4 - (1 if defect == "d_tail" else 0)
                for g in range(groups):
                    acc += qt[:, 4 * g:4 * g + 4] @ col[4 * g:4 * g + 4]
                for j, qi in enumerate(tile):
                    if defect == "tile_query" and (l, t0) == at[:2] and \
                            len(tile) == 16 and j == 8:
                        assert qi == at[2]
                        continue
                    key = (vn - np.float32(2) * acc[j, :nrows]
                           if metric == L2 else -acc[j, :nrows])
                    for w in range(-(-pad // ir.WAVE_ROWS)):
                        a = w * ir.WAVE_ROWS
                        z = min(a + ir.WAVE_ROWS, nrows, live)
                        if z <= a:
                            continue
                        if defect == "wave_slot" and (qi, l, ch, w) == at:
                            continue
                        kk, rr = key[a:z], rows[a:z]
                        if fused:  # the wave keeps its k smallest
                            keep = np.lexsort((rr, kk))[:k]
                            kk, rr = kk[keep], rr[keep]
                        cand[qi].append((kk, rr))
    dist = np.zeros((nq, k), np.float32)
    ids = np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        if not cand[qi]:
            continue
        kk = np.concatenate([a for a, _ in cand[qi]])
        rr = np.concatenate([r for _, r in cand[qi]])
        keep = np.lexsort((rr, kk))[:k]
        m = len(keep)
        ids[qi, :m] = c.ids[rr[keep]]
        dist[qi, :m] = (np.maximum(kk[keep] + qn[qi], np.float32(0))
                        if metric == L2 else -kk[keep])
        if defect == "unprobed_row" and qi == at[0]:
            ids[qi, m - 1] = c.ids[at[1]]
    return dist, ids


def _model(c, nprobe):
    ref, b = ir.refb(c)
    probed, amb = ir.probe_sets(c.metric, c.q, c.cents, nprobe)
    assert len(amb) == 0
    return ref, b, probed, ir.eligible(probed, c.owner, np.ones(c.n, bool))


def _wave_of(c, row):
    """(list, chunk, wave) of an arrival row in the emulation's CSR."""
    l = int(c.owner[row])
    pos = int(row - c.off[l])  # rows arrive list by list
    return l, pos // ir.CHUNK, pos % ir.CHUNK // ir.WAVE_ROWS


def _defect_case(metric, defect):
    """(case, k, nprobe, at).  The scan defects run on a case A shape with
    a 4-dim tail (d = 20), the probing defects on the case C index."""
    if defect in ("probe_swap", "unprobed_row"):
        c, nprobe, k = ir.case_c(metric), 3, 10
        ref, b, probed, elig = _model(c, nprobe)
        qi = int(np.nonzero(c.qlists == 1)[0][0])  # its own list has 3 rows
        if defect == "probe_swap":
            return c, k, nprobe, qi
        out = np.nonzero(~probed[qi, c.owner])[0]
        return c, k, nprobe, (qi, int(out[0]))
    if defect == "d_tail_ladder":
        return ir.case_b(2305, metric, 9), ir.B_LENS[0] + ir.B_LENS[1], 2, \
            None
    c, nprobe = ir.case_a(20, metric), 3
    assert ir.tail_of(c.d) == 4
    ref, b, probed, elig = _model(c, nprobe)
    if defect == "row_group":  # rows 256..259 of the 260-row list; k = N
        return c, c.n, nprobe, (1, 0)
    if defect == "tile_query":
        # nprobe = nlist: every list sees the queries in order, a tile of 16
        # and one of 4; query 8 loses the list of its best row
        qi = 8
        l = int(c.owner[np.argmin(fr.better_sign(metric) * ref[qi])])
        return c, ir.A_K, nprobe, (l, 0, qi)
    if defect == "wave_slot":
        qi = 17
        row = int(np.argmin(fr.better_sign(metric) * ref[qi]))
        return c, ir.A_K, nprobe, (qi,) + _wave_of(c, row)
    return c, (c.n if defect == "d_tail" else ir.A_K), nprobe, None


DEFECTS = ["d_tail", "d_tail_ladder", "row_group", "tile_query", "wave_slot",
           "probe_swap", "unprobed_row", "vnorm_shift"]


def _params():
    for defect in DEFECTS:
        for metric in ((L2,) if defect == "vnorm_shift" else (L2, IP)):
            yield pytest.param(metric, defect, id=f"{defect}-{metric}")


@pytest.mark.parametrize("metric,defect", _params())
def test_clean_emulation_passes_and_defect_is_rejected(metric, defect):
    c, k, nprobe, at = _defect_case(metric, defect)
    ref, b, probed, elig = _model(c, nprobe)
    fr.assert_topk_strength(metric, ref, b, elig, k)
    dist, ids = emulate(c, k, nprobe)
    assert fr.check_topk(metric, dist, ids, ref, b, c.ids, elig) <= 1.0
    planted = defect.replace("_ladder", "")
    dist, ids = emulate(c, k, nprobe, planted, at)
    with pytest.raises(AssertionError):
        fr.check_topk(metric, dist, ids, ref, b, c.ids, elig)


def test_clean_emulation_cosine_and_store_all():
    """The clean emulation over the case C searches (fused and store-all by
    k and by size), COSINE included."""
    for metric in METRICS:
        c = ir.case_c(metric)
        for nprobe, k in ((1, 10), (3, 64), (3, 65), (9, 64)):
            ref, b, probed, elig = _model(c, nprobe)
            dist, ids = emulate(c, k, nprobe)
            assert fr.check_topk(metric, dist, ids, ref, b, c.ids,
                                 elig) <= 1.0
