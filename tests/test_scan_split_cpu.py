"""Tile partition of the fused MFMA scan between its two kernels, no GPU.

tests/host/scan_split_test.cpp drives dingo-store_amd/csrc/dg_scan_split.h,
the one definition that k_ivf_scan_mfma2 (tile pairs), k_ivf_scan_mfma (what
is left) and the host launcher share.  For nql = 0 .. 200 probing queries the
tiles the two kernels take are rebuilt here from the printed numbers and every
tile must be taken exactly once; with pairing off the single-tile kernel takes
all of them.  The program can also be built with -fsanitize=address,undefined
and run stand-alone (no arguments: its self-check).
"""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "scan_split_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_scan_split.h")
TILE = 16


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("scan_split") / "scan_split_test")
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


def test_every_tile_taken_once(exe):
    rows = [tuple(map(int, ln.split()))
            for ln in _run(exe, "table", 200).splitlines()]
    assert len(rows) == 2 * 201
    for nql, pairing, tiles, pairs, first in rows:
        assert tiles == -(-nql // TILE), nql
        taken = [0] * tiles
        for p in range(pairs):
            # the pair kernel assumes tile 2p whole and tile 2p+1 non-empty
            assert nql - 2 * TILE * p - TILE >= 1, (nql, p)
            taken[2 * p] += 1
            taken[2 * p + 1] += 1
        for t in range(first, tiles):
            taken[t] += 1
        assert taken == [1] * tiles, (nql, pairing, taken)
        if pairing:
            assert pairs == tiles // 2 and first == 2 * pairs
            assert tiles - first == tiles % 2
        else:
            assert pairs == 0 and first == 0


@pytest.mark.parametrize("d,nq,want", [
    (768, 16, 0), (768, 17, 1), (4, 17, 1), (2304, 1024, 1), (2308, 1024, 0),
    (768, 1, 0), (768, 8192, 1),
    # 32-bit byte offsets into the image: (nq + 1) * 144 * 64 < 2^32
    (2304, 466032, 1), (2304, 466033, 0)])
def test_applies(exe, d, nq, want):
    got, nbytes = map(int, _run(exe, "applies", d, nq).split())
    assert got == want
    assert nbytes == (nq + 1) * -(-d // 16) * 64
