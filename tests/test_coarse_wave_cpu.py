"""When the one-kernel coarse probe selection applies, and the inputs of its
GPU test, no GPU.

tests/host/coarse_wave_test.cpp drives dingo-store_amd/csrc/dg_coarse_wave.h,
the one definition that k_coarse_select, k_inv_offsets and search_core share:
the cap on nprobe, nprobe = nlist (nothing to select), nlist below one wave,
and the bound and the ownership of the single-block offset scan.  The program
can also be built with -fsanitize=address,undefined and run stand-alone (no
arguments: its self-check).

The second half checks the reference side of test_coarse_wave.py: for every
case that file compares with ivf_reference's float64 coarse ranking, at most
2 % of the queries have an ambiguous probe set, and the tie cases really tie.
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
SRC = os.path.join(HERE, "host", "coarse_wave_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_coarse_wave.h")

import coarse_wave_cases as cw  # noqa: E402


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("coarse_wave") / "coarse_wave_test")
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


def test_constants(exe):
    cap, threads, inv_threads, inv_max = map(int, _run(exe, "consts").split())
    assert cap == cw.CAP >= 128       # the default nprobe of 80 is covered
    assert threads == 256 and threads % 64 == 0
    assert inv_threads == 1024 and inv_max >= 65536


@pytest.mark.parametrize("np_,nlist,want", [
    # the cap boundary
    (cw.CAP, 4096, 1), (cw.CAP + 1, 4096, 0), (cw.CAP, cw.CAP + 1, 1),
    (2048, 4096, 0), (2049, 1 << 20, 0),
    # np = nlist probes every list: nothing to select; np > nlist is clamped
    # by the caller and never applies
    (32, 32, 0), (cw.CAP, cw.CAP, 0), (1, 1, 0), (33, 32, 0),
    # nlist below one wave, and the smallest selection there is
    (1, 2, 1), (31, 32, 1), (32, 33, 1), (5, 63, 1), (63, 64, 1),
    # any nlist, the segmented range of the old kernel included
    (32, 16400, 1), (80, 1 << 20, 1),
    (0, 100, 0), (-1, 100, 0)])
def test_applies(exe, np_, nlist, want):
    assert int(_run(exe, "applies", np_, nlist)) == want


@pytest.mark.parametrize("nlist,want,per", [
    (0, 0, 0), (1, 1, 1), (1024, 1, 1), (1025, 1, 2), (4096, 1, 4),
    (16400, 1, 17), (65536, 1, 64), (65537, 0, 65)])
def test_offsets_bound(exe, nlist, want, per):
    assert tuple(map(int, _run(exe, "offsets", nlist).split())) == (want, per)


def test_case_tables():
    assert cw.geom_nps(33) == [1, 2, 31, 32]
    assert cw.geom_nps(65) == [1, 2, 31, 32, 33, 64]
    assert cw.geom_nps(100) == [1, 2, 31, 32, 33, 64, 80, 99]
    assert cw.geom_nps(1024) == cw.GEOM_NPS == cw.geom_nps(4099)
    assert {n % 4 == 0 for n in cw.GEOM_NLISTS} == {True, False}
    assert min(cw.GEOM_NLISTS) < 64 < 256 < max(cw.GEOM_NLISTS)


def test_reference_is_unambiguous_enough():
    checked = 0
    for name, c, nprobe in cw.reference_checked():
        probed, clear = cw.unambiguous(c, nprobe)
        assert (probed.sum(1) == nprobe).all(), (name, nprobe)
        left_out = int((~clear).sum())
        assert left_out <= cw.AMBIGUOUS_MAX * len(clear), \
            (name, nprobe, left_out)
        checked += 1
    assert checked == sum(len(cw.geom_nps(n)) for n in cw.GEOM_NLISTS) + \
        len(cw.KIND_METRICS) * len(cw.KIND_NPS)


def test_tie_cases_tie():
    c = cw.tie_case(False)
    _, inv, cnt = np.unique(c.cents, axis=0, return_inverse=True,
                            return_counts=True)
    assert (cnt == 4).all() and len(cnt) == cw.TIE_NLIST // 4
    # scattered: the copies of a vector are not neighbours
    first = np.array([np.nonzero(inv.reshape(-1) == g)[0] for g in range(8)])
    assert (np.diff(first, axis=1) > 1).any()
    # the cut at nprobe falls inside a run of equal scores for some query
    o = cw.tie_order(c)
    q, ce = c.q.astype(np.float64), c.cents.astype(np.float64)
    s = (ce * ce).sum(1)[None, :] - 2.0 * (q @ ce.T)
    rows = np.arange(len(q))
    for nprobe in cw.TIE_NPS:
        assert (s[rows, o[:, nprobe - 1]] == s[rows, o[:, nprobe]]).any()
    c = cw.tie_case(True)
    assert (c.cents == c.cents[0]).all()
    assert np.array_equal(cw.tie_order(c)[3], np.arange(cw.TIE_NLIST))
