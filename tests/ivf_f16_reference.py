"""float64 reference model of an IVF-Flat search over f16 row storage
(DG_STORAGE_F16): the helper of test_ivf_f16.py (GPU) and
test_ivf_f16_cpu.py.  It builds on ivf_reference / flat_reference, whose
cases, drivers, acceptance rules A-D, range rules and strength caps are used
unchanged; what changes is the reference and the bound.

Reference.  float64 over the f32 queries and the STORED rows: on the GPU what
Index.reconstruct returns, without one numpy's astype(float16) of the rows
(stored_rows_cpu; for COSINE of the f32-normalised rows, normalised the way
k_normalize_rows does).  For COSINE the query is normalised in f64 and the
stored rows are used as they are, not renormalised: their norm is
1 +- ~2^-12 and that is part of the contract.

Bound, derived and not observed.  With u = 2^-24 the issue's scan sums at
most 2 d exact products in f32 (a hi/lo query split doubles the terms), the
split residual is at most 4 u per product, and there are three final
roundings (vnorm, key, emit):

  b16_L2(q, x)  = (2 d + 7)  u (||q||^2 + ||x||^2 + 2 sum|q_i x_i|)
  b16_IP(q, x)  = (2 d + 7)  u sum|q_i x_i|
  b16_COS(q, x) = (2 d + 10) u sum|qh_i x_i|

The shipped kernel (k_ivf_scan_f16) decodes the halves in registers and
feeds v_mfma_f32_16x16x4_f32 with the unsplit f32 query: one f32 chain of d
rounded products, inside the bound a fortiori.

Kernel geometry the shapes rest on (k_ivf_scan_f16, k_transpose_chunks_f16):
  - block, wave and row ownership are those of k_ivf_scan_mfma: one block per
    (list, 1024-row chunk), a wave 256 rows, chunks padded to 4 rows;
  - dims are padded to 8 inside a chunk (dp = ceil(d / 4) * 4 at the ABI,
    d8 = ceil(d / 8) * 8 in the chunk); a lane's 16-byte load is one "kp" =
    8 dims x 4 rows, feeding two MFMA k-steps;
  - the load pipeline has 4 stages of one kp: its period is 32 dims.  With
    nkp = d8 / 8 the paths are: nkp 1..4 the last period alone (1..4
    stages); 5..7 one whole period followed by a partial one; 8 the loop
    once and a whole last period; 9..11 loop, whole, partial; 12 the loop
    twice; 13 loop twice, whole, partial.  d % 8 in 1..4 leaves the last
    kp half empty;
  - QTM = 16 for dp <= 2304, 8 for dp <= 4608, 4 above (the ladder of the
    f32 scan), every tile through the same body;
  - fused and store-all are two epilogues of that one body, chosen as on an
    f32 index (ivf_reference.expect_fused).

Table A therefore runs ivf_reference.A_DIMS (nkp 1..8) plus A16_EXTRA, which
adds nkp 5 and 7 at a full last kp, and 9 (half and full), 10, 11, 12, 13.

Largest |dist - ref| / b16 over test_ivf_f16.py on an MI355X (a record, not
a threshold; the threshold is 1):  L2 0.19, IP 0.23, COSINE 0.10.
"""
import types

import numpy as np

import flat_reference as fr
import ivf_reference as ir
from flat_reference import COSINE, IP, L2, U

MAX_RATIO = {L2: 0.0, IP: 0.0, COSINE: 0.0}

A16_EXTRA = [40, 56, 68, 72, 80, 88, 96, 100]
A16_DIMS = ir.A_DIMS + A16_EXTRA
B16_GPU = [(d, m, 9) for d in (2304, 2305, 8192) for m in (L2, IP)] + \
    [(4609, COSINE, 9)]
B16_CPU = [(d, m, 9) for d in (2304, 2305, 4609, 8192) for m in (L2, IP)] + \
    [(4609, COSINE, 9)]


def nkp_of(d):
    return (ir.dp_of(d) + 7) // 8


assert {nkp_of(d) for d in A16_DIMS} == set(range(1, 14))
assert {d % 8 for d in A16_DIMS if 1 <= d % 8 <= 4} == {1, 3, 4}


# --------------------------------------------------------------------------
# stored rows, reference, bound
# --------------------------------------------------------------------------
def normalize_f32(x32):
    """k_normalize_rows: norm^2 accumulated in f64 and rounded to f32, the
    row scaled by the f32 1 / sqrt in f32; rows with |1 - n2| <= 1e-5 or
    n2 == 0 are left alone."""
    x = np.asarray(x32, np.float32)
    n2 = (x.astype(np.float64) ** 2).sum(1).astype(np.float32)
    inv = (np.float32(1.0) / np.sqrt(n2, dtype=np.float32)).astype(np.float32)
    scale = (n2 > 0) & (np.abs(np.float32(1.0) - n2) > np.float32(0.00001))
    out = x.copy()
    out[scale] = (x[scale] * inv[scale, None]).astype(np.float32)
    return out


def stored_rows_cpu(metric, x32):
    """What an f16 index holds for the rows x32, decoded to f32."""
    x = np.asarray(x32, np.float32)
    if metric == COSINE:
        x = normalize_f32(x)
    return x.astype(np.float16).astype(np.float32)


def ref_and_bound16(metric, q32, xs32):
    """(ref, b16), float64 [nq, n]: f32 queries against the stored rows."""
    q = np.asarray(q32, np.float32).astype(np.float64)
    x = np.asarray(xs32, np.float32).astype(np.float64)
    d = q.shape[1]
    if metric == COSINE:
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
    dot = q @ x.T
    adot = np.abs(q) @ np.abs(x).T
    if metric == L2:
        qn = (q * q).sum(1)[:, None]
        xn = (x * x).sum(1)[None, :]
        ref = np.maximum(qn + xn - 2.0 * dot, 0.0)
        small = ref < 1e-6 * (qn + xn)
        if small.any():
            qi, xi = np.nonzero(small)
            ref[qi, xi] = ((q[qi] - x[xi]) ** 2).sum(1)
        return ref, (2 * d + 7) * U * (qn + xn + 2.0 * adot)
    if metric == IP:
        return dot, (2 * d + 7) * U * adot
    return dot, (2 * d + 10) * U * adot


def f16_case(c, stored=None):
    """A copy of the ivf_reference case c (the cached original is shared with
    the f32 tests and stays untouched) that carries the stored rows and
    (ref, b16) as _refb, which the drivers of ivf_reference pick up."""
    c16 = types.SimpleNamespace(**{k: v for k, v in vars(c).items()
                                   if k != "_refb"})
    c16.stored = stored_rows_cpu(c.metric, c.x) if stored is None else stored
    c16._refb = ref_and_bound16(c.metric, c.q, c16.stored)
    return c16


def _recorded(fn, metric, *args, **kw):
    keep_fr, keep_ir = fr.MAX_RATIO[metric], ir.MAX_RATIO[metric]
    try:
        worst = fn(metric, *args, **kw)
    finally:  # the Flat and the f32 IVF tables stay their own records
        fr.MAX_RATIO[metric], ir.MAX_RATIO[metric] = keep_fr, keep_ir
    MAX_RATIO[metric] = max(MAX_RATIO[metric], worst)
    return worst


def check_topk(metric, *args, **kw):
    return _recorded(fr.check_topk, metric, *args, **kw)


def check_range(metric, *args, **kw):
    return _recorded(fr.check_range, metric, *args, **kw)


# --------------------------------------------------------------------------
# table D with upserted vectors that go through the same rounding
# --------------------------------------------------------------------------
def run_d16(c, assign, ops):
    """ivf_reference.run_d over an f16 case: the same filters, victims and
    upserts; the reference after the upsert is taken over the ROUNDED new
    vectors (c.stored with the rounded rows in place)."""
    ref, b = ir.refb(c)
    alive = np.ones(c.n, bool)
    specs = ir.case_d_specs(c)
    one = fr.filter_mask(specs["range_one_list"], c.ids)
    assert one.sum() == 40 and (c.owner[one] == 8).all()
    probed, _ = ir.probe_sets(c.metric, c.q, c.cents, ir.D_NPROBE)
    for removed in (False, True):
        if removed:
            victims = ir.case_d_victims(c, ref,
                                        ir.eligible(probed, assign, alive))
            assert alive[victims].all() and len(victims) > 20
            ops.remove(c.ids[victims])
            alive[victims] = False
            assert not alive[c.owner == 1].any()
        for name, spec in list(specs.items()) + [("none", None)]:
            if removed and spec is not None:
                assert (fr.filter_mask(spec, c.ids) & ~alive).any() or \
                    name == "range_one_list"
            for k in ir.D_KS:
                ir.topk(ops, c, ("D16", name, k, "removed", removed), c.q, k,
                        ir.D_NPROBE, spec, ref, b, assign, alive)
    rows, vec = ir.case_d_upsert(c, alive)
    ops.upsert(c.ids[rows], vec)
    stored2 = c.stored.copy()
    stored2[rows] = stored_rows_cpu(c.metric, vec)
    ref2, b2 = ref_and_bound16(c.metric, c.q, stored2)
    lens = list(c.lens)
    lens[2] += 8  # the new rows arrive in the 255-row list
    for k in ir.D_KS:
        ir.topk(ops, c, ("D16", "upsert", k), c.q, k, c.nlist, None, ref2, b2,
                assign, alive, lens=lens)
    near = np.nonzero(c.qlists == 2)[0][:8]
    best = np.argmin(np.where(alive[None, :], ref2[near], np.inf), axis=1)
    assert np.array_equal(best, rows)  # each new vector is a query's best


# --------------------------------------------------------------------------
# numpy emulation of an f16 search (the CPU file plants defects in it)
# --------------------------------------------------------------------------
DEFECTS = ("rows_unrounded", "query_rounded", "lost_last_kgroup",
           "lost_padded_rows")


def emulate_search(c, assign, k, nprobe, defect=None):
    """(dist, ids) [nq, k] of an f16 search of case c done in numpy: f32
    query, decoded half rows, f32 products summed in f32, key = vnorm - 2
    dot, dist = key + qnorm (clamped at 0) for L2 and the dot otherwise;
    -1 / 0.0 pads.  defect plants one of DEFECTS:
      rows_unrounded    the rows are scanned as f32, never rounded to half;
      query_rounded     the dot product takes the query rounded to half (a
                        hi/lo split that dropped its lo part);
      lost_last_kgroup  the last 8-dim group of the padded row is skipped;
      lost_padded_rows  the rows of a list's last, partial 4-row group are
                        never candidates."""
    metric, d = c.metric, c.d
    q = np.asarray(c.q, np.float32)
    rows = np.asarray(c.x, np.float32)
    if metric == COSINE:
        q = normalize_f32(q)
        rows = normalize_f32(rows)
    if defect != "rows_unrounded":
        rows = rows.astype(np.float16).astype(np.float32)
    # the split lives in the scan's dot product: the query norm of the L2
    # emit is still taken from the f32 query
    qdot = q.astype(np.float16).astype(np.float32) \
        if defect == "query_rounded" else q
    d8 = (d + 7) // 8 * 8
    use = d8 - 8 if defect == "lost_last_kgroup" else d
    qs, xs = qdot[:, :use], rows[:, :use]
    dot = np.zeros((len(q), len(rows)), np.float32)
    for i in range(use):  # the k-ordered f32 chain
        dot = (dot + qs[:, i:i + 1] * xs[None, :, i]).astype(np.float32)
    if metric == L2:
        vn = (rows.astype(np.float32) ** 2).sum(1, dtype=np.float32)
        qn = (q ** 2).sum(1, dtype=np.float32)
        key = (vn[None, :] - np.float32(2.0) * dot).astype(np.float32)
        dist = np.maximum(key + qn[:, None], np.float32(0.0)).astype(
            np.float32)
        order_key = dist
    else:
        dist = dot
        order_key = -dot
    probed, _ = ir.probe_sets(metric, c.q, c.cents, nprobe)
    cand = ir.eligible(probed, assign, np.ones(c.n, bool))
    if defect == "lost_padded_rows":
        lost = np.zeros(c.n, bool)
        for l in range(c.nlist):
            members = np.nonzero(np.asarray(assign) == l)[0]
            tail = len(members) % 4
            if tail:
                lost[members[-tail:]] = True
        cand = cand & ~lost[None, :]
    out_d = np.zeros((len(q), k), np.float32)
    out_i = np.full((len(q), k), -1, np.int64)
    for qi in range(len(q)):
        r = np.nonzero(cand[qi])[0]
        o = r[np.lexsort((r, order_key[qi, r]))][:k]
        out_d[qi, :len(o)] = dist[qi, o]
        out_i[qi, :len(o)] = c.ids[o]
    return out_d, out_i


def rule_a_miss_fraction(c, dist, ids, top=10):
    """Fraction of queries with a rule A violation (|dist - ref| > b16)
    within their `top` best returned rows."""
    ref, b = ir.refb(c)
    pos = {int(v): i for i, v in enumerate(c.ids)}
    bad = 0
    for qi in range(len(c.q)):
        got = [g for g in ids[qi, :top] if g >= 0]
        r = np.array([pos[int(g)] for g in got], np.int64)
        err = np.abs(dist[qi, :len(r)].astype(np.float64) - ref[qi, r])
        bad += bool((err > b[qi, r]).any())
    return bad / len(c.q)
