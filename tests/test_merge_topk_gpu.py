"""dg_merge_topk (kernel k_merge_lists) against a model of the stated merge
order, exact in ids and in distance bits (marked gpu, device 0).

The order: element (list, pos) is smaller iff (is_pad, key, list, pos) is
lexicographically smaller; is_pad = id < 0; key = the order-preserving u32
image of the distance (L2) or of the negated score (IP).  The model is a
plain sorted() of those tuples.  Real rows keep their distance bits, pads
and the slots beyond n_lists * k_in come out as -1 / 0.0.
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

L2, IP = dg.L2, dg.IP


def key_u32(metric, dist):
    """The orderable image of float32 distances (array in, uint32 out)."""
    u = np.asarray(dist, np.float32).view(np.uint32).copy()
    if metric != L2:
        u ^= np.uint32(0x80000000)
    neg = (u & np.uint32(0x80000000)) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def model(dists, ids, k_out, metric):
    n_lists, nq, k_in = dists.shape
    key = key_u32(metric, dists)
    od = np.zeros((nq, k_out), np.float32)
    oi = np.full((nq, k_out), -1, np.int64)
    for q in range(nq):
        el = sorted((int(ids[t, q, p] < 0), int(key[t, q, p]), t, p)
                    for t in range(n_lists) for p in range(k_in))
        for r, (pad, _, t, p) in enumerate(el[:k_out]):
            if not pad:
                od[q, r] = dists[t, q, p]
                oi[q, r] = ids[t, q, p]
    return od, oi


def check(dists, ids, k_out, metric):
    dists = np.ascontiguousarray(dists, np.float32)
    ids = np.ascontiguousarray(ids, np.int64)
    gd, gi = dg.merge_topk_device(dists, ids, k_out, metric, device=0)
    wd, wi = model(dists, ids, k_out, metric)
    assert np.array_equal(gi, wi)
    assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


def sorted_lists(rng, n_lists, nq, k_in, metric, fill, values=None):
    """[n_lists, nq, k_in] best-first lists: fill(t, q) real rows, then pads
    with dist 0.0.  values = None draws distinct-ish random floats."""
    d = np.zeros((n_lists, nq, k_in), np.float32)
    i = np.full((n_lists, nq, k_in), -1, np.int64)
    for t in range(n_lists):
        for q in range(nq):
            f = fill(t, q)
            v = (rng.standard_normal(f) * 3 if values is None
                 else rng.choice(values, f)).astype(np.float32)
            v = v[np.argsort(key_u32(metric, v), kind="stable")]
            d[t, q, :f] = v
            # ids above 2^33 too: the id is copied, never ordered on
            i[t, q, :f] = (t << 34) + q * 4096 + np.arange(f)
    return d, i


SHAPES = [(1, 1, 1, 1), (2, 3, 1, 1), (3, 5, 10, 10), (8, 2, 64, 64),
          (8, 2, 65, 10), (2, 1, 2048, 2048), (32, 1, 7, 100),
          (3, 4, 10, 40),   # k_out above the 30 inputs: pads are emitted
          (4, 257, 5, 5)]   # 5140 elements: crosses blocks of 256 threads


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_full_lists(shape, metric):
    n_lists, nq, k_in, k_out = shape
    rng = np.random.default_rng(sum(shape) + metric)
    d, i = sorted_lists(rng, n_lists, nq, k_in, metric, lambda t, q: k_in)
    check(d, i, k_out, metric)


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_trailing_pads_and_ties(shape, metric):
    """Lists with trailing pads of different lengths and values drawn from a
    small set, so that equal keys meet across lists and within them."""
    n_lists, nq, k_in, k_out = shape
    rng = np.random.default_rng(1000 + sum(shape) + metric)
    vals = np.float32([0.0, 0.25, 0.25, 1.5, 2.0, 7.0])
    d, i = sorted_lists(rng, n_lists, nq, k_in, metric,
                        lambda t, q: int(rng.integers(0, k_in + 1)), vals)
    check(d, i, k_out, metric)


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_one_list_all_pad_and_all_lists_pad(metric):
    rng = np.random.default_rng(7)
    d, i = sorted_lists(rng, 4, 3, 9, metric, lambda t, q: [9, 0, 4, 1][t])
    for k_out in (1, 9, 14, 36, 50):
        check(d, i, k_out, metric)
    d, i = sorted_lists(rng, 4, 3, 9, metric, lambda t, q: 0)
    for k_out in (1, 36, 50):
        check(d, i, k_out, metric)


def test_same_distance_in_three_lists():
    """0.5 at positions 2, 0 and 1 of lists 0, 1, 2: the merged order of the
    ties is by list, then position."""
    d = np.float32([[[0.1, 0.2, 0.5, 0.5]],
                    [[0.5, 0.6, 0.7, 0.8]],
                    [[0.3, 0.5, 0.5, 0.9]]])
    i = np.int64([[[10, 11, 12, 13]], [[20, 21, 22, 23]],
                  [[30, 31, 32, 33]]])
    gd, gi = dg.merge_topk_device(d, i, 8, L2, device=0)
    assert gi[0].tolist() == [10, 11, 30, 12, 13, 20, 31, 32]
    check(d, i, 12, L2)
    check(-d, i, 12, IP)


@pytest.mark.parametrize("metric", [L2, IP], ids=["L2", "IP"])
def test_zero_distances_against_pads(metric):
    """Real rows at 0.0 (L2 is clamped there) and pads that also carry 0.0:
    every real row precedes every pad."""
    d = np.zeros((3, 2, 4), np.float32)
    i = np.int64([[[5, 6, -1, -1], [7, -1, -1, -1]],
                  [[-1, -1, -1, -1], [8, 9, 10, -1]],
                  [[11, -1, -1, -1], [-1, -1, -1, -1]]])
    gd, gi = dg.merge_topk_device(d, i, 6, metric, device=0)
    assert gi.tolist() == [[5, 6, 11, -1, -1, -1], [7, 8, 9, 10, -1, -1]]
    assert (gd == 0).all()
    check(d, i, 6, metric)


def test_negative_zero_orders_before_positive_zero():
    """L2: -0.0 < +0.0 under the integer image, whatever the list.  IP: the
    score is negated first, so +0.0 precedes -0.0.  Bits are preserved."""
    d = np.float32([[[0.0, 1.0]], [[-0.0, 2.0]]])
    i = np.int64([[[1, 2]], [[3, 4]]])
    gd, gi = dg.merge_topk_device(d, i, 4, L2, device=0)
    assert gi[0].tolist() == [3, 1, 2, 4]
    assert gd.view(np.uint32)[0].tolist() == [0x80000000, 0, 0x3f800000,
                                              0x40000000]
    check(d, i, 4, L2)
    d = np.float32([[[-0.0, -1.0]], [[0.0, -2.0]]])
    gd, gi = dg.merge_topk_device(d, i, 4, IP, device=0)
    assert gi[0].tolist() == [3, 1, 2, 4]
    check(d, i, 4, IP)


def test_infinite_distance_precedes_pads():
    d = np.float32([[[1.0, np.inf, 0.0]], [[np.inf, 0.0, 0.0]]])
    i = np.int64([[[1, 2, -1]], [[3, -1, -1]]])
    gd, gi = dg.merge_topk_device(d, i, 6, L2, device=0)
    assert gi[0].tolist() == [1, 2, 3, -1, -1, -1]
    assert gd[0].tolist() == [1.0, np.inf, np.inf, 0.0, 0.0, 0.0]
    check(d, i, 6, L2)
    # IP: a score of -inf is the worst real row
    check(-d, i, 6, IP)


def test_limits():
    d = np.zeros((1, 1, 1), np.float32)
    i = np.zeros((1, 1, 1), np.int64)
    for k in (0, 2049):
        with pytest.raises(dg.DgError) as e:
            dg.merge_topk_device(d, i, k, L2, device=0)
        assert e.value.status == 1  # DG_EINVAL
    with pytest.raises(dg.DgError) as e:
        dg.merge_topk_device(np.zeros((33, 1, 1), np.float32),
                             np.zeros((33, 1, 1), np.int64), 1, L2, device=0)
    assert e.value.status == 1
    with pytest.raises(dg.DgError) as e:
        dg.merge_topk_device(np.zeros((1, 1, 2049), np.float32),
                             np.zeros((1, 1, 2049), np.int64), 1, L2,
                             device=0)
    assert e.value.status == 1
