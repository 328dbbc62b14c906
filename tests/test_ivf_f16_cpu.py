"""The f16 row storage reference model and its checks, without a GPU.

  1. dry runs of exactly the searches test_ivf_f16.py makes, over the rows as
     an f16 index stores them (numpy's round-to-nearest-even half): the
     strength caps (1 % top-k, 5 % range band) and zero ambiguous probe sets
     hold on the reference and the derived bound b16 alone;
  2. a numpy emulation of an f16 search (ivf_f16_reference.emulate_search)
     passes rules A-D clean and is rejected with each planted defect: rows
     left unrounded, the query rounded to half, a lost last k-group, a lost
     padded row group.  For the first two, on tables A and C, rule A is
     violated within the ten best rows of at least 70 % of the queries.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE]

import flat_reference as fr  # noqa: E402
import ivf_f16_reference as h16  # noqa: E402
import ivf_reference as ir  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

METRICS = [L2, IP, COSINE]


def _dry(c, driver, *args):
    a, _ = ir.reference_assign(c.metric, c.x, c.cents)
    assert np.array_equal(a, c.owner)
    ops = ir.DryOps()
    driver(h16.f16_case(c), a, ops, *args)
    return ops.searches


# --------------------------------------------------------------------------
# 0. the helper itself
# --------------------------------------------------------------------------
def test_geometry():
    assert [h16.nkp_of(d) for d in (1, 8, 9, 32, 33, 64, 100)] == \
        [1, 1, 2, 4, 5, 8, 13]
    # every path of the 4-stage pipeline: last period alone, whole + partial,
    # loop + whole, loop + whole + partial, the loop twice
    assert {h16.nkp_of(d) for d in h16.A16_DIMS} == set(range(1, 14))


def test_stored_rows_are_nearest_even_halves():
    x = np.array([[1.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 65504.0,
                   2.0 ** -25, 3 * 2.0 ** -25, -0.1, 1e-8]], np.float32)
    s = h16.stored_rows_cpu(L2, x)
    assert s.dtype == np.float32
    # ties to even: 1 + 2^-11 -> 1, 1 + 3 2^-11 -> 1 + 2^-9; 2^-25 -> 0
    assert s[0, 0] == 1.0 and s[0, 1] == 1.0 and s[0, 2] == 1.0 + 2.0 ** -9
    assert s[0, 3] == 65504.0 and s[0, 4] == 0.0 and s[0, 5] == 2.0 ** -23
    assert abs(s[0, 6] + 0.1) <= 2.0 ** -11 * 0.1 and s[0, 7] == 0.0


def test_cosine_stored_rows_within_the_storage_bound():
    c = ir.case_c(COSINE)
    s = h16.stored_rows_cpu(COSINE, c.x).astype(np.float64)
    x = c.x.astype(np.float64)
    xh = x / np.sqrt((x * x).sum(1, keepdims=True))
    tol = (2.0 ** -11 + 4 * fr.U) * np.abs(xh) + 2.0 ** -25
    assert (np.abs(s - xh) <= tol).all()
    n2 = (s * s).sum(1)
    assert (np.abs(n2 - 1.0) < 2.0 ** -10).all() and (n2 != 1.0).any()


def test_bound_is_twice_the_f32_bound_plus_roundings():
    c = ir.case_c(L2)
    s = h16.stored_rows_cpu(L2, c.x)
    _, b16 = h16.ref_and_bound16(L2, c.q, s)
    _, b32 = fr.ref_and_bound(L2, c.q, s)
    assert np.allclose(b16 / b32, (2 * c.d + 7) / (c.d + 3))


def test_case_copy_leaves_the_shared_case_alone():
    c = ir.case_c(IP)
    had = hasattr(c, "_refb")
    c16 = h16.f16_case(c)
    assert hasattr(c, "_refb") == had and c16 is not c
    ref32, _ = fr.ref_and_bound(IP, c.q, c.x)
    assert not np.array_equal(c16._refb[0], ref32)  # the rounding shows


# --------------------------------------------------------------------------
# 1. the tables
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.A_METRICS)
def test_tables_d_pipeline(metric):
    for d in h16.A16_DIMS:
        assert _dry(ir.case_a(d, metric), ir.run_full_probe, ir.A_K) == 2


def test_tables_d_ladder():
    for d, metric, nq in h16.B16_CPU:
        assert _dry(ir.case_b(d, metric, nq), ir.run_full_probe, ir.B_K) == 2


@pytest.mark.parametrize("metric", METRICS)
def test_tables_edges_partial_probing(metric):
    assert _dry(ir.case_c(metric), ir.run_c) == \
        len(ir.C_FUSED) + len(ir.C_STORE_ALL)


def test_tables_filters_tombstones_upsert():
    assert _dry(ir.case_c(L2), h16.run_d16) == 2 * 6 * 2 + 2


@pytest.mark.parametrize("metric", ir.E_METRICS)
def test_tables_range_partial_probing(metric):
    assert _dry(ir.case_e(metric), ir.run_e) == 3


@pytest.mark.parametrize("nq", ir.F_NQS)
def test_tables_graph_replay(nq):
    assert _dry(ir.case_c(L2), ir.run_f, nq) == ir.F_CALLS + 2


# --------------------------------------------------------------------------
# 2. the emulation, clean and with planted defects
# --------------------------------------------------------------------------
def _emulated(c, k, nprobe, defect):
    c16 = h16.f16_case(c)
    ref, b = ir.refb(c16)
    probed, amb = ir.probe_sets(c.metric, c.q, c.cents, nprobe)
    assert len(amb) == 0
    elig = ir.eligible(probed, c.owner, np.ones(c.n, bool))
    dist, ids = h16.emulate_search(c16, c.owner, k, nprobe, defect)
    return c16, dist, ids, ref, b, elig


def _check(c, k, nprobe, defect=None):
    c16, dist, ids, ref, b, elig = _emulated(c, k, nprobe, defect)
    return h16.check_topk(c.metric, dist, ids, ref, b, c.ids, elig,
                          (c.metric, c.d, defect))


# the emulation's cases: table A at a half-empty last group, at one whole
# period and past it, and table C under partial probing
EMU_A = [(5, L2), (12, IP), (33, L2), (64, IP), (100, L2)]


@pytest.mark.parametrize("d,metric", EMU_A)
def test_emulation_passes_clean_table_a(d, metric):
    c = ir.case_a(d, metric)
    assert _check(c, ir.A_K, c.nlist) <= 1.0
    assert _check(c, c.n, c.nlist) <= 1.0


@pytest.mark.parametrize("metric", METRICS)
def test_emulation_passes_clean_table_c(metric):
    c = ir.case_c(metric)
    for nprobe, k in ((1, 10), (3, 64), (3, 65)):
        assert _check(c, k, nprobe) <= 1.0


def _rejected(c, k, nprobe, defect, message):
    """The emulation with the defect runs to its end; rules A-D alone
    reject its answer, with the message of the rule the defect breaks."""
    c16, dist, ids, ref, b, elig = _emulated(c, k, nprobe, defect)
    with pytest.raises(AssertionError) as e:
        h16.check_topk(c.metric, dist, ids, ref, b, c.ids, elig,
                       (c.metric, c.d, defect))
    assert message in str(e.value), e.value


# what each defect breaks: a wrong dot product shows in the best rows of the
# fused k (rule A); rows that are never candidates show where every eligible
# row has to come back (rule D)
REJECT_A = {"rows_unrounded": "distance off", "query_rounded": "distance off",
            "lost_last_kgroup": "distance off"}


@pytest.mark.parametrize("defect", h16.DEFECTS)
@pytest.mark.parametrize("d,metric", EMU_A)
def test_defects_rejected_table_a(d, metric, defect):
    c = ir.case_a(d, metric)
    if defect == "lost_padded_rows":  # k = N reads out every row
        _rejected(c, c.n, c.nlist, defect, "too few rows")
    else:
        _rejected(c, ir.A_K, c.nlist, defect, REJECT_A[defect])


@pytest.mark.parametrize("defect", h16.DEFECTS)
@pytest.mark.parametrize("metric", METRICS)
def test_defects_rejected_table_c(metric, defect):
    c = ir.case_c(metric)
    if defect == "lost_padded_rows":  # the 1- and 3-row lists lose all rows
        _rejected(c, 10, 1, defect, "too few rows")
    else:
        _rejected(c, 10, 3, defect, REJECT_A[defect])


@pytest.mark.parametrize("defect", ["rows_unrounded", "query_rounded"])
def test_rounding_defects_violate_rule_a_broadly(defect):
    """Tables A (the 18 dims of ivf_reference) and C, not the d >= 2304
    ladder, where the bound hides a rounding of 2^-11 per component."""
    fractions = {}
    for metric in ir.A_METRICS:
        for d in ir.A_DIMS:
            c = ir.case_a(d, metric)
            c16, dist, ids, *_ = _emulated(c, ir.A_K, c.nlist, defect)
            fractions[("A", d, metric)] = h16.rule_a_miss_fraction(
                c16, dist, ids)
    for metric in METRICS:
        c = ir.case_c(metric)
        c16, dist, ids, *_ = _emulated(c, 10, 3, defect)
        fractions[("C", metric)] = h16.rule_a_miss_fraction(c16, dist, ids)
    print(defect, {k: round(v, 2) for k, v in fractions.items()})
    low = {k: v for k, v in fractions.items() if v < 0.70}
    assert not low, low
