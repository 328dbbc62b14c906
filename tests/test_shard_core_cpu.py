"""Shard routing and the merge order of the sharded index, without a GPU.

tests/host/shard_core_test.cpp drives dingo-store_amd/csrc/dg_shard_core.h:
dg_shard_of against splitmix64 computed here, the balance of the hash over
consecutive ids, and the merge against a plain sorted() of the tuples
(is_pad, key, list, pos).  The program answers with the scalar host merge
and with the rank placement the GPU kernel k_merge_lists performs (it calls
the same dg_merge_rank), so the kernel's arithmetic is checked here too.
The program can also be built with -fsanitize=address,undefined and run
stand-alone (no arguments: its self-check).
"""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "host", "shard_core_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_shard_core.h")
M64 = (1 << 64) - 1


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("shard_core") / "shard_core_test")
    r = subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def splitmix64(i):
    z = (i + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_self_check(exe):
    assert _run(exe).strip().endswith("OK")


def test_core_is_free_of_hip():
    src = open(CORE).read()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert includes and all("/" not in i and not i.startswith("dg_")
                            for i in includes), includes
    assert "hip" not in " ".join(includes)


@pytest.mark.parametrize("n_shards", [1, 2, 3, 8, 32])
def test_shard_of_fixed_ids(exe, n_shards):
    ids = [0, 1, 2, 41, (1 << 64) - 1,  # -1 cast to u64
           (1 << 33) + 5, (1 << 63) - 1, 123456789012345]
    got = [int(x) for x in _run(exe, "shard", n_shards, *ids).split()]
    assert got == [splitmix64(i) % n_shards for i in ids]


@pytest.mark.parametrize("n_shards", [2, 3, 8])
def test_shard_balance(exe, n_shards):
    n = 100000
    cnt = [int(x) for x in _run(exe, "balance", n, n_shards).split()]
    assert len(cnt) == n_shards and sum(cnt) == n
    mine = np.bincount([splitmix64(i) % n_shards for i in range(n)],
                       minlength=n_shards)
    assert cnt == mine.tolist()
    for c in cnt:
        assert abs(c - n / n_shards) <= 0.05 * n / n_shards, cnt


# ---- merge against sorted() ----
def _bits(f):
    return struct.unpack("<I", struct.pack("<f", f))[0]


def _key(metric, dist_bits, id_):
    u = dist_bits ^ (0x80000000 if metric else 0)
    enc = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    return (1 if id_ < 0 else 0, enc)


def model_merge(n_lists, nq, k_in, k_out, metric, bits, ids):
    """bits / ids: [n_lists][nq][k_in] python ints."""
    out = []
    for q in range(nq):
        el = sorted((_key(metric, bits[t][q][p], ids[t][q][p]), t, p)
                    for t in range(n_lists) for p in range(k_in))
        row = []
        for r in range(k_out):
            if r < len(el):
                _, t, p = el[r]
                if ids[t][q][p] >= 0:
                    row.append((bits[t][q][p], ids[t][q][p]))
                    continue
            row.append((0, -1))
        out.append(row)
    return out


def _sorted_list(rng, metric, k_in, fill, values):
    """One best-first list: `fill` real rows drawn from `values` (float32
    distances for L2, scores for IP), then pads with dist 0.0."""
    v = sorted((np.float32(x) for x in rng.choice(values, fill)),
               key=lambda x: _key(metric, _bits(x), 0))
    return [_bits(x) for x in v] + [0] * (k_in - fill)


def _case(rng, n_lists, nq, k_in, metric, fills, values):
    bits = [[None] * nq for _ in range(n_lists)]
    ids = [[None] * nq for _ in range(n_lists)]
    for t in range(n_lists):
        for q in range(nq):
            fill = fills(t, q)
            bits[t][q] = _sorted_list(rng, metric, k_in, fill, values)
            ids[t][q] = [t * 1000000 + q * 5000 + p if p < fill else -1
                         for p in range(k_in)]
    return bits, ids


def _check(exe, tmp_path, n_lists, nq, k_in, k_out, metric, bits, ids):
    path = tmp_path / "case.txt"
    with open(path, "w") as f:
        f.write(f"{n_lists} {nq} {k_in} {k_out} {metric}\n")
        for t in range(n_lists):
            for q in range(nq):
                for p in range(k_in):
                    f.write(f"{bits[t][q][p]:x} {ids[t][q][p]}\n")
    lines = _run(exe, "merge", path).split("\n")
    got = [(int(a, 16), int(b)) for a, b in
           (ln.split() for ln in lines if ln)]
    assert len(got) == 2 * nq * k_out
    want = [e for row in model_merge(n_lists, nq, k_in, k_out, metric, bits,
                                     ids) for e in row]
    assert got[:nq * k_out] == want, "scalar host merge"
    assert got[nq * k_out:] == want, "rank placement"


WIDE = np.linspace(-3, 3, 1001).astype(np.float32)
TIES = np.array([0.0, -0.0, 0.5, 1.0, 1.0, 2.5, np.inf], np.float32)


@pytest.mark.parametrize("metric", [0, 1])
@pytest.mark.parametrize("values", [WIDE, TIES], ids=["random", "ties"])
@pytest.mark.parametrize("shape", [
    (1, 1, 1, 1), (2, 3, 1, 1), (3, 5, 10, 10), (8, 2, 65, 10),
    (32, 1, 7, 100), (3, 4, 10, 40), (4, 3, 5, 50)])
def test_merge_matches_sorted(exe, tmp_path, shape, values, metric):
    """Full and partly filled lists, planted equal keys across lists (the
    `ties` value set holds few values, +-0.0 and +inf), k_out below and
    above the number of real elements and of all elements."""
    n_lists, nq, k_in, k_out = shape
    rng = np.random.default_rng(hash((shape, metric)) & 0xffff)
    fills = lambda t, q: int(rng.integers(0, k_in + 1))  # noqa: E731
    bits, ids = _case(rng, n_lists, nq, k_in, metric, fills, values)
    _check(exe, tmp_path, n_lists, nq, k_in, k_out, metric, bits, ids)


@pytest.mark.parametrize("metric", [0, 1])
def test_merge_all_pad_and_mixed_fill(exe, tmp_path, metric):
    rng = np.random.default_rng(5)
    # every list pad
    bits, ids = _case(rng, 4, 2, 6, metric, lambda t, q: 0, TIES)
    _check(exe, tmp_path, 4, 2, 6, 9, metric, bits, ids)
    # list 1 entirely pad, the others of different fill, real 0.0 against
    # the pads' 0.0
    bits, ids = _case(rng, 4, 2, 6, metric,
                      lambda t, q: [6, 0, 3, 1][t], np.float32([0.0, 1.0]))
    for k_out in (3, 10, 24, 30):
        _check(exe, tmp_path, 4, 2, 6, k_out, metric, bits, ids)
