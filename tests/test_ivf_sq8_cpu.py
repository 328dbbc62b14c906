"""The SQ8 row storage codec, reference model and checks, without a GPU.

  0. tests/host/sq8_core_test.cpp drives dingo-store_amd/csrc/dg_sq8_core.h,
     the one definition of the codec and of the chunk byte layout that the
     kernels, the host code and the loaders share: its codes and decodes
     equal a numpy restatement of the f32 codec bit for bit and the float64
     codec of ivf_sq8_reference away from code boundaries, on random and
     edge inputs (endpoints, saturation, vdiff = 0, ranges of 1e-30 and
     1e30).  The header includes no HIP.  The program can also be built with
     -fsanitize=address,undefined and run stand-alone (no arguments: its
     self-check).
  1. dry runs of exactly the searches test_ivf_sq8.py makes, over the rows as
     an SQ8 index stores them with ranges equal to the min and max of the
     case's rows: the strength caps (1 % top-k, 5 % range band) and zero
     ambiguous probe sets hold on the reference and the derived bound b8
     alone;
  2. a numpy emulation of an SQ8 search (ivf_sq8_reference.emulate_search)
     passes rules A-D clean and is rejected with each planted defect: rows
     left unquantised, the + 0.5 dropped, cq dropped, a lost last kp, a lost
     padded row group.
"""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE]

import flat_reference as fr  # noqa: E402
import ivf_reference as ir  # noqa: E402
import ivf_sq8_reference as h8  # noqa: E402
from flat_reference import COSINE, IP, L2  # noqa: E402

METRICS = [L2, IP, COSINE]
SRC = os.path.join(HERE, "host", "sq8_core_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_sq8_core.h")


# --------------------------------------------------------------------------
# 0. the shared header
# --------------------------------------------------------------------------
def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sq8_core") / "sq8_core_test")
    r = subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_self_check(exe):
    assert _run(exe).strip().endswith("OK")


def test_core_is_free_of_hip():
    src = open(CORE).read()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert includes == ["cstdint"], includes
    assert "__device__" not in src and "__host__" not in src


def _codec_inputs():
    rng = np.random.default_rng(808)
    f32 = np.float32
    parts = []
    # random values in and around random ranges
    n = 20000
    lo = rng.normal(0, 3, n).astype(f32)
    w = np.abs(rng.normal(0, 2, n)).astype(f32) + f32(1e-3)
    x = (lo + w * rng.uniform(-0.1, 1.1, n)).astype(f32)
    parts.append(np.stack([x, lo, w], 1))
    # endpoints, saturation, vdiff = 0, tiny and huge ranges
    for lo1, w1 in ((0.0, 1.0), (-2.5, 5.0), (1e-30, 1e-30), (-1e30, 2e30),
                    (3.0, 0.0), (0.0, 1e30), (-1e-30, 1e-30)):
        lo1, w1 = f32(lo1), f32(w1)
        xs = [lo1, f32(lo1 + w1), f32(lo1 - f32(1.0)), f32(lo1 + f32(2) * w1),
              f32(lo1 + w1 * f32(0.5)), f32(-3e38), f32(3e38), f32(0.0)]
        xs += list((lo1 + w1 * rng.uniform(0, 1, 64)).astype(f32))
        # the centre of every code cell
        xs += list(h8.decode(np.arange(256), lo1, w1).astype(f32))
        parts.append(np.stack([np.array(xs, f32),
                               np.full(len(xs), lo1, f32),
                               np.full(len(xs), w1, f32)], 1))
    return np.ascontiguousarray(np.concatenate(parts), f32)


def test_codec_equals_numpy(exe, tmp_path):
    v = _codec_inputs()
    n = len(v)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(n).tobytes())
        f.write(v.tobytes())
    _run(exe, "codec", fin, fout)
    raw = open(fout, "rb").read()
    assert len(raw) == 9 * n
    code = np.frombuffer(raw[:n], np.uint8)
    dec = np.frombuffer(raw[n:5 * n], np.float32)
    step = np.frombuffer(raw[5 * n:], np.float32)
    x, lo, w = v[:, 0], v[:, 1], v[:, 2]
    f32 = np.float32
    # the f32 codec restated in numpy, one rounding per operation
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = np.where(w > 0, ((x - lo).astype(f32) /
                             np.where(w > 0, w, f32(1))).astype(f32), f32(0))
        t = np.clip(t, f32(0), f32(1)).astype(f32)
        want_code = (f32(255.0) * t).astype(f32).astype(np.int32)
        tt = ((code.astype(f32) + f32(0.5)) / f32(255.0)).astype(f32)
        want_dec = (lo + (tt * w).astype(f32)).astype(f32)
    assert np.array_equal(code, want_code.astype(np.uint8))
    assert np.array_equal(dec.view(np.uint32), want_dec.view(np.uint32))
    assert np.array_equal(step.view(np.uint32),
                          (w / f32(255.0)).astype(f32).view(np.uint32))
    # against the float64 codec: equal away from code boundaries
    t64 = h8.encode_t(x, lo, w)
    # x - vmin rounds in f32: with |x| or |vmin| far above vdiff the cell of
    # the f32 codec moves by that rounding, so the boundary band scales
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        slack = 1e-3 + 255.0 * 4 * fr.U * \
            (np.abs(x.astype(np.float64)) + np.abs(lo.astype(np.float64))) / \
            np.where(w > 0, w.astype(np.float64), 1.0)
    clear = np.abs(t64 - np.round(t64)) > slack
    assert clear.mean() > 0.5
    assert np.array_equal(code[clear], np.floor(t64[clear]).astype(np.uint8))
    d64 = h8.decode(code, lo, w)
    assert (np.abs(dec.astype(np.float64) - d64) <=
            4 * fr.U * (np.abs(lo.astype(np.float64)) + w)).all()
    assert np.isfinite(dec).all()


def test_codec_saturates_and_handles_flat_dimensions(exe, tmp_path):
    v = np.array([[-5.0, 0.0, 1.0], [9.0, 0.0, 1.0], [0.0, 0.0, 1.0],
                  [1.0, 0.0, 1.0], [7.0, 3.0, 0.0], [-7.0, 3.0, 0.0]],
                 np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.int32(len(v)).tobytes())
        f.write(v.tobytes())
    _run(exe, "codec", fin, fout)
    raw = open(fout, "rb").read()
    n = len(v)
    assert list(raw[:n]) == [0, 255, 0, 255, 0, 0]
    dec = np.frombuffer(raw[n:5 * n], np.float32)
    assert dec[4] == 3.0 and dec[5] == 3.0


def test_chunk_offsets_are_a_permutation(exe):
    for d, nrp in ((5, 8), (17, 12), (100, 260)):
        rows = np.array([ln.split() for ln in
                         _run(exe, "offset", d, nrp).splitlines()], np.int64)
        d16 = (d + 15) // 16 * 16
        assert len(rows) == d16 * nrp
        assert np.array_equal(np.sort(rows[:, 2]), np.arange(d16 * nrp))
        # a lane's 16 bytes: dims 16kp + 4h + g (h = 0..3) of 4 rows
        dim, row, off = rows.T
        base = ((4 * (dim // 16) + dim % 4) * nrp + row // 4 * 4) * 4
        assert np.array_equal(off, base + 4 * (dim // 4 % 4) + row % 4)


def test_sanitizer_build_runs_its_self_check(tmp_path):
    out = str(tmp_path / "sq8_core_test_asan")
    r = subprocess.run([_cxx(), "-std=c++17", "-O1", "-g",
                        "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", SRC, "-o", out],
                       capture_output=True, text=True)
    if r.returncode != 0:  # the plain build above is the compile check
        pytest.skip("no sanitizer runtime for this compiler")
    assert _run(out).strip().endswith("OK")


# --------------------------------------------------------------------------
# the helper itself
# --------------------------------------------------------------------------
def _dry(c, driver, *args):
    a, _ = ir.reference_assign(c.metric, c.x, c.cents)
    assert np.array_equal(a, c.owner)
    ops = ir.DryOps()
    driver(h8.sq8_case(c), a, ops, *args)
    return ops.searches


def test_geometry():
    assert [h8.nkp_of(d) for d in (1, 16, 17, 64, 65, 128, 129, 208)] == \
        [1, 1, 2, 4, 5, 8, 9, 13]
    # every path of the 4-stage pipeline: last period alone, whole + partial,
    # loop + whole, loop + whole + partial, the loop twice
    assert {h8.nkp_of(d) for d in h8.A8_DIMS} == set(range(1, 14))
    assert (8192, IP, 9) not in h8.B8 and (8192, L2, 9) in h8.B8


def test_ranges_are_min_and_max_of_the_rows():
    c = ir.case_c(L2)
    c8 = h8.sq8_case(c)
    assert np.array_equal(c8.vmin, c.x.min(0))
    assert np.array_equal(c8.vdiff, c.x.max(0) - c.x.min(0))
    code = h8.encode(c.x, c8.vmin, c8.vdiff)
    # the extremes of every dimension are the end codes (vdiff is max - min
    # rounded to f32: where it rounds up, t of the max is a hair under 1)
    assert (code.min(0) == 0).all() and (code.max(0) >= 254).all()
    # a stored row is within half a step of its row
    step = c8.vdiff.astype(np.float64) / 255.0
    span = np.abs(c8.vmin.astype(np.float64)) + c8.vdiff
    assert (np.abs(c8.stored.astype(np.float64) - c.x) <=
            0.5 * step + 4 * fr.U * span).all()


def test_case_copy_leaves_the_shared_case_alone():
    c = ir.case_c(IP)
    had = hasattr(c, "_refb")
    c8 = h8.sq8_case(c)
    assert hasattr(c, "_refb") == had and c8 is not c
    ref32, _ = fr.ref_and_bound(IP, c.q, c.x)
    assert not np.array_equal(c8._refb[0], ref32)  # the quantisation shows


def test_bound_form():
    c = ir.case_c(L2)
    c8 = h8.sq8_case(c)
    q = c.q.astype(np.float64)
    m = np.abs(q) @ (np.abs(c8.vmin.astype(np.float64)) + c8.vdiff)
    _, b = h8.ref_and_bound8(IP, c.q, c8.stored, c8.vmin, c8.vdiff)
    assert np.allclose(b, ((2 * c.d + 10) * fr.U * m)[:, None])
    _, bc = h8.ref_and_bound8(COSINE, c.q, c8.stored, c8.vmin, c8.vdiff)
    qh = q / np.sqrt((q * q).sum(1, keepdims=True))
    mh = np.abs(qh) @ (np.abs(c8.vmin.astype(np.float64)) + c8.vdiff)
    assert np.allclose(bc, ((2 * c.d + 13) * fr.U * mh)[:, None])
    # M covers every |q . x| of the case, which the derivation relies on
    assert (np.abs(q @ c8.stored.astype(np.float64).T) <=
            m[:, None] * (1 + 1 / 510)).all()


# --------------------------------------------------------------------------
# 1. the tables
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ir.A_METRICS)
def test_tables_d_pipeline(metric):
    for d in h8.A8_DIMS:
        assert _dry(ir.case_a(d, metric), ir.run_full_probe, ir.A_K) == 2


def test_tables_d_ladder():
    for d, metric, nq in h8.B8:
        assert _dry(ir.case_b(d, metric, nq), ir.run_full_probe, ir.B_K) == 2


@pytest.mark.parametrize("metric", METRICS)
def test_tables_edges_partial_probing(metric):
    assert _dry(ir.case_c(metric), ir.run_c) == \
        len(ir.C_FUSED) + len(ir.C_STORE_ALL)


def test_tables_filters_tombstones_upsert():
    assert _dry(ir.case_c(L2), h8.run_d8) == 2 * 6 * 2 + 2


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
    c8 = h8.sq8_case(c)
    ref, b = ir.refb(c8)
    probed, amb = ir.probe_sets(c.metric, c.q, c.cents, nprobe)
    assert len(amb) == 0
    elig = ir.eligible(probed, c.owner, np.ones(c.n, bool))
    dist, ids = h8.emulate_search(c8, c.owner, k, nprobe, defect)
    return c8, dist, ids, ref, b, elig


def _check(c, k, nprobe, defect=None):
    c8, dist, ids, ref, b, elig = _emulated(c, k, nprobe, defect)
    return h8.check_topk(c.metric, dist, ids, ref, b, c.ids, elig,
                         (c.metric, c.d, defect))


# the emulation's cases: table A at a partly filled last kp, at one whole
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
    c8, dist, ids, ref, b, elig = _emulated(c, k, nprobe, defect)
    with pytest.raises(AssertionError) as e:
        h8.check_topk(c.metric, dist, ids, ref, b, c.ids, elig,
                      (c.metric, c.d, defect))
    assert message in str(e.value), e.value


@pytest.mark.parametrize("defect", h8.DEFECTS)
@pytest.mark.parametrize("d,metric", EMU_A)
def test_defects_rejected_table_a(d, metric, defect):
    c = ir.case_a(d, metric)
    if defect == "lost_padded_rows":  # k = N reads out every row
        _rejected(c, c.n, c.nlist, defect, "too few rows")
    else:
        _rejected(c, ir.A_K, c.nlist, defect, "distance off")


@pytest.mark.parametrize("defect", h8.DEFECTS)
@pytest.mark.parametrize("metric", METRICS)
def test_defects_rejected_table_c(metric, defect):
    c = ir.case_c(metric)
    if defect == "lost_padded_rows":  # the 1- and 3-row lists lose all rows
        _rejected(c, 10, 1, defect, "too few rows")
    else:
        _rejected(c, 10, 3, defect, "distance off")
