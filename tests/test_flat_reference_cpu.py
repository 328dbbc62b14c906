"""The Flat float64 reference and its checkers, without a GPU.

  1. the reference agrees with the CPU oracle (flat_search /
     flat_range_search), both being exact up to the bound;
  2. the strength conditions hold for every input the GPU file uses (the
     generators and shape tables are imported from flat_reference), so the
     bound is known to be tight before any kernel runs;
  3. planted defects: a float32 emulation of the pipeline (dots, key =
     cn - 2 s, 8 column segments, top-k, emit) with one defect at a time is
     handed to the checkers, and every one has to be rejected.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "oracle")]

import flat_reference as fr  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

orc = pytest.importorskip("pyoracle")

METRICS = [L2, IP, COSINE]


# --------------------------------------------------------------------------
# 1. reference vs the CPU oracle
# --------------------------------------------------------------------------
def _oracle_inputs(metric, q, x):
    if metric == COSINE:
        return orc.normalize(q.copy()), orc.normalize(x.copy())
    return q, x


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("d", [7, 64, 100])
def test_reference_matches_oracle_topk(metric, d):
    nq, n, k = 9, 700, 20
    q, x = fr.gaussian(100 + d, nq, n, d, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    elig = np.ones(n, bool)
    fr.assert_topk_strength(metric, ref, b, elig, k)
    oq, ox = _oracle_inputs(metric, q, x)
    od, oi = orc.flat_search(metric, ox, oq, k)
    ratio = fr.check_topk(metric, od, oi, ref, b, np.arange(n), elig)
    assert ratio <= 1.0


@pytest.mark.parametrize("metric", METRICS)
def test_reference_matches_oracle_range(metric):
    nq, n, d = 9, 700, 48
    q, x = fr.gaussian(200, nq, n, d, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    elig = np.ones(n, bool)
    sg = fr.better_sign(metric)
    fifth = np.sort(sg * ref, axis=1)[:, 4] * sg
    radius = float(np.float32(np.median(fifth)))
    fr.assert_range_strength(metric, [radius], ref, b, elig)
    oq, ox = _oracle_inputs(metric, q, x)
    lims, od, oi = orc.flat_range_search(metric, ox, oq, radius)
    # the oracle lists rows in arrival order; the contract under test is
    # best first with ties toward the smaller id
    for i in range(nq):
        a, z = lims[i], lims[i + 1]
        order = np.lexsort((oi[a:z], sg * od[a:z]))
        od[a:z], oi[a:z] = od[a:z][order], oi[a:z][order]
    fr.check_range(metric, radius, lims, od, oi, ref, b, np.arange(n), elig)


def test_filter_model():
    ids = fr.filter_ids()
    assert len(np.unique(ids)) == fr.FILT_N and (np.diff(ids) > 0).all()
    assert (ids > (1 << 33)).sum() == 1000
    specs = fr.filter_specs()
    for name, spec in specs.items():
        m = fr.filter_mask(spec, ids)
        # bit-by-bit restatement of the three functors
        for j in (0, 1, 142, 143, 500, 1147, 1148, 1150, 1999, 2000, 2999):
            i = int(ids[j])
            if spec["kind"] == 1:
                want = spec["min_id"] <= i < spec["max_id"]
            elif spec["kind"] == 2:
                want = i in set(spec["ids"].tolist())
            else:
                bit = i - spec["bitmap_base"]
                want = (0 <= bit < spec["bitmap_nbits"] and
                        (int(spec["bitmap"][bit // 64]) >> (bit % 64)) & 1
                        == 1)
            assert m[j] == (want != spec["negate"]), (name, j)
    assert fr.filter_mask(specs["range_empty"], ids).sum() == 0
    assert fr.filter_mask(specs["sorted_single"], ids).sum() == 1
    assert fr.filter_mask(specs["sorted_few"], ids).sum() == 4
    assert fr.filter_mask(specs["sorted_mixed"], ids).sum() == 400
    nb = fr.filter_mask(specs["bitmap_neg"], ids)
    assert nb[ids < fr.BITMAP_BASE].all()
    assert nb[ids >= fr.BITMAP_BASE + fr.BITMAP_NBITS].all()


# --------------------------------------------------------------------------
# 2. strength conditions of the inputs the GPU file uses
# --------------------------------------------------------------------------
def test_strength_gemm_shapes():
    worst = 0.0
    for metric, shapes in (
            (L2, fr.GEMM_TILE_SHAPES + fr.GEMM_LATENCY_SHAPES +
             fr.GEMM_ROCBLAS_SHAPES),
            (IP, fr.GEMM_TILE_SHAPES + fr.GEMM_LATENCY_SHAPES +
             fr.GEMM_ROCBLAS_SHAPES),
            (COSINE, fr.GEMM_COSINE_SHAPES)):
        for nq, n, d in shapes:
            q, x = fr.gaussian(fr.gemm_seed(nq, n, d), nq, n, d, metric)
            ref, b = fr.ref_and_bound(metric, q, x)
            worst = max(worst, fr.assert_topk_strength(
                metric, ref, b, np.ones(n, bool), n, (metric, nq, n, d)))
    assert worst <= fr.TOPK_CAP


def test_strength_selector_cases():
    for metric in (L2, IP):
        for n, k in fr.SELECT_SMALL:
            q, x = fr.gaussian(fr.select_seed(n), 4, n, fr.SELECT_D, metric)
            ref, b = fr.ref_and_bound(metric, q, x)
            fr.assert_topk_strength(metric, ref, b, np.ones(n, bool), k,
                                    (metric, n, k))
        for n, k in fr.SELECT_WIDE:
            q, x = fr.gaussian(fr.select_seed(n), 2, n, fr.SELECT_D, metric)
            ref, b = fr.ref_and_bound(metric, q, x)
            fr.assert_topk_strength(metric, ref, b, np.ones(n, bool), k,
                                    (metric, n, k))
    for nq in (4, 64):
        q, x, _ = fr.duplicates_case(nq)
        ref, b = fr.ref_and_bound(L2, q, x)
        fr.assert_topk_strength(L2, ref, b, np.ones(len(x), bool), 10)


@pytest.mark.parametrize("metric", [L2, IP])
def test_strength_multichunk(metric):
    q, x = fr.multichunk_data(metric)
    rows = fr.multichunk_samples()
    assert rows[0] == 0 and rows[-1] == fr.MC_NQ - 1 and \
        len(np.unique(rows)) == fr.MC_SAMPLES
    ref, b = fr.ref_and_bound(metric, q[rows], x)
    elig = np.ones(fr.MC_N, bool)
    fr.assert_topk_strength(metric, ref, b, elig, fr.MC_K)
    # both chunks hold nearest neighbours of sampled queries
    victims = fr.multichunk_victims(metric, ref)
    assert (victims < 65536).sum() == 3 and (victims >= 65536).sum() == 3
    elig[victims] = False
    fr.assert_topk_strength(metric, ref, b, elig, fr.MC_K)
    radius = fr.kth_radius(metric, ref, elig, 5)
    fr.assert_range_strength(metric, [radius], ref, b, elig)


@pytest.mark.parametrize("metric", METRICS)
def test_strength_filter_and_range_cases(metric):
    ids = fr.filter_ids()
    q, x = fr.gaussian(fr.FILT_SEED, fr.FILT_NQ, fr.FILT_N, fr.FILT_D,
                       metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    alive = np.ones(fr.FILT_N, bool)
    for removed in (False, True):
        if removed:
            alive[fr.filter_victims()] = False
        for name, spec in fr.filter_specs().items():
            elig = alive & fr.filter_mask(spec, ids)
            for k in (10, 200):
                fr.assert_topk_strength(metric, ref, b, elig, k, (name, k))
            if elig.sum() > 20:
                radius = fr.kth_radius(metric, ref, elig, 5)
                fr.assert_range_strength(metric, [radius], ref, b, elig,
                                         name)
    # the range-semantics case: reference radii on the unfiltered index
    elig = np.ones(fr.FILT_N, bool)
    fr.assert_range_strength(metric, fr.range_radii(metric, ref, elig),
                             ref, b, elig)
    # queries equal to stored rows
    qs = x[fr.self_query_rows()]
    ref, b = fr.ref_and_bound(metric, qs, x)
    fr.assert_range_strength(
        metric, fr.range_radii(metric, ref, elig) + [0.0, -1.0], ref, b,
        elig)


# --------------------------------------------------------------------------
# 3. planted defects
# --------------------------------------------------------------------------
NSEG = 8


def emulate(metric, q, x, k, elig, defect=None):
    """float32 model of the Flat pipeline with one optional defect.
    Returns (dist [nq, k] f32, rows [nq, k] i64, -1 padded)."""
    q = np.asarray(q, np.float32)
    x = np.asarray(x, np.float32)
    if metric == COSINE:
        q = (q / np.sqrt((q.astype(np.float64) ** 2).sum(1,
             keepdims=True))).astype(np.float32)
        x = (x / np.sqrt((x.astype(np.float64) ** 2).sum(1,
             keepdims=True))).astype(np.float32)
    nq, n = len(q), len(x)
    d = q.shape[1]
    kk = d - d % 32 if defect == "k_tail" else d
    dots = (q[:, :kk] @ x[:, :kk].T).astype(np.float32)
    if defect == "transpose":
        dots[0:32, 32:64] = dots[0:32, 32:64].T.copy()
    if metric == L2:
        cn = (x * x).sum(1, dtype=np.float32)
        qn = (q * q).sum(1, dtype=np.float32)
        key = cn[None, :] - np.float32(2.0) * dots
    else:
        key = -dots
    seg_w = -(-n // NSEG)
    dist = np.zeros((nq, k), np.float32)
    rows = np.full((nq, k), -1, np.int64)
    for qi in range(nq):
        cand = np.nonzero(elig)[0]
        if defect == "filtered_present" and qi == 1:
            out = np.nonzero(~elig)[0]
            planted = out[np.argmin(key[qi, out])]
            cand = np.append(cand, planted)
        order = cand[np.lexsort((cand, key[qi, cand]))]
        if defect == "filtered_present" and qi == 1:
            assert planted in order[:k]
        if defect == "best_missing" and qi == 2:
            order = order[1:]
        order = order[:k]
        m = len(order)
        kv = key[qi, order]
        if defect == "seg_start":  # segment 1 forgets its column offset
            in1 = (order >= seg_w) & (order < 2 * seg_w)
            order = np.where(in1, order - seg_w, order)
        rows[qi, :m] = order
        if metric == L2:
            dist[qi, :m] = np.maximum(kv + qn[qi], np.float32(0.0))
        else:
            dist[qi, :m] = -kv
        if defect == "stale_pad" and qi == 0:
            assert m < k
            rows[qi, k - 1] = order[0]
    return dist, rows


TOPK_DEFECTS = ["k_tail", "transpose", "seg_start", "best_missing",
                "filtered_present", "stale_pad"]


def _defect_case(metric, defect):
    # k = N reads the whole dots matrix out, like the GPU tile-edge tests;
    # the selection defects use k < eligible, the padding one k > eligible
    nq, n, d = 48, 128, 80
    q, x = fr.gaussian(5, nq, n, d, metric)
    elig = np.ones(n, bool)
    k = n
    if defect in ("best_missing", "seg_start"):
        k = 10
    if defect in ("filtered_present", "stale_pad"):
        elig[::3] = False
        k = 10 if defect == "filtered_present" else int(elig.sum()) + 2
    return q, x, elig, k


@pytest.mark.parametrize("metric", METRICS)
def test_checker_accepts_the_clean_emulation(metric):
    for defect in TOPK_DEFECTS:
        q, x, elig, k = _defect_case(metric, defect)
        ref, b = fr.ref_and_bound(metric, q, x)
        fr.assert_topk_strength(metric, ref, b, elig, k)
        dist, rows = emulate(metric, q, x, k, elig)
        ids = np.where(rows >= 0, 1000 + 3 * rows, -1)
        ratio = fr.check_topk(metric, dist, ids, ref, b,
                              1000 + 3 * np.arange(len(x)), elig)
        assert ratio <= 1.0


@pytest.mark.parametrize("defect", TOPK_DEFECTS)
@pytest.mark.parametrize("metric", METRICS)
def test_checker_rejects_planted_defect(metric, defect):
    q, x, elig, k = _defect_case(metric, defect)
    ref, b = fr.ref_and_bound(metric, q, x)
    dist, rows = emulate(metric, q, x, k, elig, defect)
    ids = np.where(rows >= 0, 1000 + 3 * rows, -1)
    with pytest.raises(AssertionError):
        fr.check_topk(metric, dist, ids, ref, b,
                      1000 + 3 * np.arange(len(x)), elig)


def _range_emulation(metric, q, x, radius):
    """Clean float32 range answer in the contract's order."""
    n = len(x)
    dist, rows = emulate(metric, q, x, n, np.ones(n, bool))
    sg = fr.better_sign(metric)
    lims, dd, ii = [0], [], []
    for qi in range(len(q)):
        keep = sg * dist[qi] < sg * np.float32(radius)
        order = np.lexsort((rows[qi][keep], sg * dist[qi][keep]))
        dd.append(dist[qi][keep][order])
        ii.append(rows[qi][keep][order])
        lims.append(lims[-1] + int(keep.sum()))
    return (np.array(lims, np.int64), np.concatenate(dd),
            np.concatenate(ii))


@pytest.mark.parametrize("metric", METRICS)
def test_range_checker_rejects_planted_defects(metric):
    nq, n, d = 6, 400, 40
    q, x = fr.gaussian(6, nq, n, d, metric)
    ref, b = fr.ref_and_bound(metric, q, x)
    elig = np.ones(n, bool)
    radius = fr.kth_radius(metric, ref, elig, 5)
    fr.assert_range_strength(metric, [radius], ref, b, elig)
    args = (ref, b, np.arange(n), elig)
    lims, dd, ii = _range_emulation(metric, q, x, radius)
    assert lims[-1] > nq
    fr.check_range(metric, radius, lims, dd, ii, *args)
    first = int(np.nonzero(np.diff(lims) >= 2)[0][0])
    a = int(lims[first])
    # a row within the radius missing
    l2 = lims.copy()
    l2[first + 1:] -= 1
    with pytest.raises(AssertionError):
        fr.check_range(metric, radius, l2, np.delete(dd, a),
                       np.delete(ii, a), *args)
    # an emitted distance that rounds onto the radius
    d2 = dd.copy()
    d2[int(lims[first + 1]) - 1] = np.float32(radius)
    with pytest.raises(AssertionError):
        fr.check_range(metric, radius, lims, d2, ii, *args)
    # a row far beyond the radius admitted
    far = int(np.argmax(fr.better_sign(metric) * ref[first]))
    z = int(lims[first + 1])
    l3 = lims.copy()
    l3[first + 1:] += 1
    with pytest.raises(AssertionError):
        fr.check_range(metric, radius, l3,
                       np.insert(dd, z, np.float32(ref[first, far])),
                       np.insert(ii, z, far), *args)
    # worst first
    d4, i4 = dd.copy(), ii.copy()
    d4[a:z], i4[a:z] = dd[a:z][::-1], ii[a:z][::-1]
    with pytest.raises(AssertionError):
        fr.check_range(metric, radius, lims, d4, i4, *args)
    # counts that disagree with the arrays
    l5 = lims.copy()
    l5[-1] += 1
    with pytest.raises(AssertionError):
        fr.check_range(metric, radius, l5, dd, ii, *args)
