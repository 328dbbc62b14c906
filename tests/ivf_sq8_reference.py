"""float64 reference model of an IVF-Flat search over SQ8 row storage
(DG_STORAGE_SQ8): the helper of test_ivf_sq8.py (GPU) and
test_ivf_sq8_cpu.py.  It builds on ivf_reference / flat_reference, whose
cases, drivers, acceptance rules A-D, range rules and strength caps are used
unchanged; what changes is the reference and the bound.

Codec (dg_sq8_core.h, faiss QT_8bit), per dimension j with ranges (vmin,
vdiff), done here in float64:
  encode  t = vdiff > 0 ? (x - vmin) / vdiff : 0, clamped to [0, 1],
          code = floor(255 t)
  decode  vmin + (code + 0.5) / 255 * vdiff
sq8_case takes the ranges from the case's own rows: vmin = min, vdiff =
max - min in f32 (for COSINE over the f32-normalised rows).

Reference.  float64 over the f32 queries and the STORED rows: on the GPU what
Index.reconstruct returns, without one the float64 codec rounded to f32
(stored_rows_cpu).  For COSINE the query is normalised in f64 and the stored
rows are used as they are.

Bound, derived and not observed.  The scan never decodes a row.  It computes
  cq + sum_j q'_j code_j,   q'_j = fl(q_j step_j),  step_j = fl(vdiff_j / 255),
  cq = fl(sum_j q_j (vmin_j + step_j / 2))   (f64 sum, rounded once),
as an f32 chain of d multiply-adds that starts at cq.  With u = 2^-24 and
  M(q) = sum_j |q_j| (|vmin_j| + vdiff_j),
every partial sum of the chain and |q . x| itself are at most M (1 + 1/510).
Against the exact affine value sum_j q_j (vmin_j + (code_j + 1/2) vdiff_j /
255) the computed dot product is off by at most
  2 d u M   the chain: one rounding of the product and one of the sum a term,
  2 u M     step_j and q'_j, one rounding each,
  1 u M     cq, rounded once,
and the reference row the index returns is itself the f32 decode, three
roundings a component ((code + .5) / 255, times vdiff, plus vmin): 3 u M
between the exact affine value and q . stored.  Three final roundings (row
norm or key, emit, and the query norm of L2) and the 1/510 above round the
constant up to 10; COSINE adds the three roundings of the f32 query
normalisation:

  b8_IP(q, x)  = (2 d + 10) u M(q)
  b8_L2(q, x)  = (2 d + 10) u (||q||^2 + ||x||^2 + 2 M(q))
  b8_COS(q, x) = (2 d + 13) u M(qh)

M does not depend on the row: the bound is coarser than b16's sum|q_i x_i|
where a row sits low in its ranges, which is why (8192, IP) of ladder B
misses the 1 % strength cap (by 2.1x) and is left out.

Kernel geometry the shapes rest on (k_ivf_scan_sq8, k_transpose_chunks_sq8):
  - block, wave and row ownership are those of k_ivf_scan_f16;
  - dims are padded to 16 inside a chunk (code 0 against q' = 0); a lane's
    16-byte load is one "kp" = 16 dims x 4 rows, feeding four MFMA k-steps;
  - the load pipeline has 4 stages of one kp: its period is 64 dims.  With
    nkp = ceil(dp / 16) the paths are: nkp 1..4 the last period alone (1..4
    stages); 5..7 one whole period followed by a partial one; 8 the loop
    once and a whole last period; 9..11 loop, whole, partial; 12 the loop
    twice; 13 loop twice, whole, partial;
  - QTM = 16 for dp <= 2304, 8 for dp <= 4608, 4 above, every tile through
    the same body; fused and store-all are two epilogues of that body.

Table A therefore runs ivf_reference.A_DIMS (nkp 1..4) plus A8_EXTRA (nkp
5..13, partly filled last kps included).

Largest |dist - ref| / b8 over test_ivf_sq8.py on an MI355X (a record, not a
threshold; the threshold is 1):  L2 0.13, IP 0.14, COSINE 0.06.
"""
import types

import numpy as np

import flat_reference as fr
import ivf_f16_reference as h16
import ivf_reference as ir
from flat_reference import COSINE, IP, L2, U

MAX_RATIO = {L2: 0.0, IP: 0.0, COSINE: 0.0}

A8_EXTRA = [65, 80, 96, 100, 112, 113, 128, 129, 144, 160, 161, 176, 177,
            192, 193, 208]
A8_DIMS = ir.A_DIMS + A8_EXTRA
# ladder B: (8192, IP) misses the strength cap under b8 (docstring)
B8 = [(d, L2, 9) for d in (2304, 2305, 4609, 8192)] + \
    [(d, IP, 9) for d in (2304, 2305, 4609)] + [(4609, COSINE, 9)]

normalize_f32 = h16.normalize_f32


def nkp_of(d):
    return (ir.dp_of(d) + 15) // 16


assert {nkp_of(d) for d in A8_DIMS} == set(range(1, 14))
assert {d % 16 for d in A8_DIMS if d % 16} >= {1, 3, 4, 5, 8, 12, 13}


# --------------------------------------------------------------------------
# codec (float64), stored rows, reference, bound
# --------------------------------------------------------------------------
def ranges_of(rows32):
    """RS_minmax with argument 0, in f32: (min, max - min) per dimension."""
    r = np.asarray(rows32, np.float32)
    vmin = r.min(0)
    return vmin, (r.max(0) - vmin).astype(np.float32)


def encode_t(x32, vmin, vdiff):
    """255 t of the codec in f64, t clamped to [0, 1]; floor gives the code."""
    x = np.asarray(x32, np.float32).astype(np.float64)
    lo = np.asarray(vmin, np.float32).astype(np.float64)
    w = np.asarray(vdiff, np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(w > 0, (x - lo) / np.where(w > 0, w, 1.0), 0.0)
    return 255.0 * np.clip(t, 0.0, 1.0)


def encode(x32, vmin, vdiff):
    return np.floor(encode_t(x32, vmin, vdiff)).astype(np.uint8)


def decode(code, vmin, vdiff):
    """float64 decode (round with .astype(np.float32) for a stored row)."""
    lo = np.asarray(vmin, np.float32).astype(np.float64)
    w = np.asarray(vdiff, np.float32).astype(np.float64)
    return lo + (np.asarray(code).astype(np.float64) + 0.5) / 255.0 * w


def stored_rows_cpu(metric, x32, vmin, vdiff):
    """What an SQ8 index with these ranges holds for the rows x32, decoded
    to f32."""
    x = np.asarray(x32, np.float32)
    if metric == COSINE:
        x = normalize_f32(x)
    return decode(encode(x, vmin, vdiff), vmin, vdiff).astype(np.float32)


def ref_and_bound8(metric, q32, xs32, vmin, vdiff):
    """(ref, b8), float64 [nq, n]: f32 queries against the stored rows."""
    q = np.asarray(q32, np.float32).astype(np.float64)
    x = np.asarray(xs32, np.float32).astype(np.float64)
    d = q.shape[1]
    if metric == COSINE:
        q = q / np.sqrt((q * q).sum(1, keepdims=True))
    span = np.abs(np.asarray(vmin, np.float32).astype(np.float64)) + \
        np.asarray(vdiff, np.float32).astype(np.float64)
    dot = q @ x.T
    m = np.broadcast_to((np.abs(q) @ span)[:, None], dot.shape)
    if metric == L2:
        qn = (q * q).sum(1)[:, None]
        xn = (x * x).sum(1)[None, :]
        ref = np.maximum(qn + xn - 2.0 * dot, 0.0)
        small = ref < 1e-6 * (qn + xn)
        if small.any():
            qi, xi = np.nonzero(small)
            ref[qi, xi] = ((q[qi] - x[xi]) ** 2).sum(1)
        return ref, (2 * d + 10) * U * (qn + xn + 2.0 * m)
    if metric == IP:
        return dot, (2 * d + 10) * U * m
    return dot, (2 * d + 13) * U * m


def sq8_case(c, stored=None):
    """A copy of the ivf_reference case c (the cached original is shared with
    the other tests and stays untouched) that carries the ranges (the
    per-dimension min and max of its rows), the stored rows and (ref, b8) as
    _refb, which the drivers of ivf_reference pick up."""
    c8 = types.SimpleNamespace(**{k: v for k, v in vars(c).items()
                                  if k != "_refb"})
    rows = normalize_f32(c.x) if c.metric == COSINE else c.x
    c8.vmin, c8.vdiff = ranges_of(rows)
    c8.stored = stored_rows_cpu(c.metric, c.x, c8.vmin, c8.vdiff) \
        if stored is None else stored
    c8._refb = ref_and_bound8(c.metric, c.q, c8.stored, c8.vmin, c8.vdiff)
    return c8


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
# table D with upserted vectors that go through the same codec
# --------------------------------------------------------------------------
def run_d8(c, assign, ops, reconstruct=None):
    """ivf_reference.run_d over an SQ8 case: the same filters, victims and
    upserts; the reference after the upsert is taken over the RE-ENCODED new
    vectors (the case's ranges; a component outside them saturates).
    reconstruct(ids), when given, supplies the rows the index holds."""
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
                ir.topk(ops, c, ("D8", name, k, "removed", removed), c.q, k,
                        ir.D_NPROBE, spec, ref, b, assign, alive)
    rows, vec = ir.case_d_upsert(c, alive)
    ops.upsert(c.ids[rows], vec)
    stored2 = c.stored.copy()
    stored2[rows] = stored_rows_cpu(c.metric, vec, c.vmin, c.vdiff) \
        if reconstruct is None else reconstruct(c.ids[rows])
    ref2, b2 = ref_and_bound8(c.metric, c.q, stored2, c.vmin, c.vdiff)
    lens = list(c.lens)
    lens[2] += 8  # the new rows arrive in the 255-row list
    for k in ir.D_KS:
        ir.topk(ops, c, ("D8", "upsert", k), c.q, k, c.nlist, None, ref2, b2,
                assign, alive, lens=lens)
    near = np.nonzero(c.qlists == 2)[0][:8]
    best = np.argmin(np.where(alive[None, :], ref2[near], np.inf), axis=1)
    assert np.array_equal(best, rows)  # each new vector is a query's best


# --------------------------------------------------------------------------
# numpy emulation of an SQ8 search (the CPU file plants defects in it)
# --------------------------------------------------------------------------
DEFECTS = ("rows_unquantised", "half_dropped", "cq_dropped", "lost_last_kp",
           "lost_padded_rows")


def emulate_search(c, assign, k, nprobe, defect=None):
    """(dist, ids) [nq, k] of an SQ8 search of the sq8_case c done in numpy
    the way the kernels do it: codes of the (normalised) rows, q' = q * step
    in f32, cq summed in f64 and rounded once, the f32 chain cq + sum q'_j
    code_j, key = vnorm(decoded row) - 2 dot, dist = key + qnorm (clamped at
    0) for L2 and the dot otherwise; -1 / 0.0 pads.  defect plants one of:
      rows_unquantised  the rows are scanned as f32, never encoded;
      half_dropped      the + 0.5 of the decode is missing from the fold
                        (cq = sum q_j vmin_j);
      cq_dropped        the accumulators start at 0 instead of cq;
      lost_last_kp      the last 16-dim group of the padded row is skipped;
      lost_padded_rows  the rows of a list's last, partial 4-row group are
                        never candidates."""
    metric, d = c.metric, c.d
    f32 = np.float32
    q = np.asarray(c.q, f32)
    rows = np.asarray(c.x, f32)
    if metric == COSINE:
        q = normalize_f32(q)
        rows = normalize_f32(rows)
    vmin, vdiff = c.vmin.astype(f32), c.vdiff.astype(f32)
    code = encode(rows, vmin, vdiff).astype(f32)
    dec = decode(code, vmin, vdiff).astype(f32)
    step = (vdiff / f32(255.0)).astype(f32)
    if defect == "rows_unquantised":
        qp, code, dec = q, rows, rows
        cq = np.zeros(len(q), f32)
    else:
        qp = (q * step[None, :]).astype(f32)
        half = 0.0 if defect == "half_dropped" else 0.5
        cq = (q.astype(np.float64) @
              (vmin.astype(np.float64) + half * step.astype(np.float64))
              ).astype(f32)
        if defect == "cq_dropped":
            cq = np.zeros(len(q), f32)
    d16 = (d + 15) // 16 * 16
    use = d16 - 16 if defect == "lost_last_kp" else d
    dot = np.repeat(cq[:, None], len(rows), axis=1).astype(f32)
    for i in range(use):  # the k-ordered f32 chain
        dot = (dot + qp[:, i:i + 1] * code[None, :, i]).astype(f32)
    if metric == L2:
        vn = (dec ** 2).sum(1, dtype=f32)
        qn = (q ** 2).sum(1, dtype=f32)
        key = (vn[None, :] - f32(2.0) * dot).astype(f32)
        dist = np.maximum(key + qn[:, None], f32(0.0)).astype(f32)
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
    out_d = np.zeros((len(q), k), f32)
    out_i = np.full((len(q), k), -1, np.int64)
    for qi in range(len(q)):
        r = np.nonzero(cand[qi])[0]
        o = r[np.lexsort((r, order_key[qi, r]))][:k]
        out_d[qi, :len(o)] = dist[qi, o]
        out_i[qi, :len(o)] = c.ids[o]
    return out_d, out_i
