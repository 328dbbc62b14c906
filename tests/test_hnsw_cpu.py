"""The HNSW host core, no GPU: graph build, reference search and the hnswlib
container of dingo-store_amd/csrc/dg_hnsw_core.h, driven through the
stand-alone program tests/host/hnsw_core_test.cpp.

Data (fixed by the program): n = 2000 rows and 64 queries of d = 16 integer
components in [-3, 3] (splitmix64 streams 7 and 99991), M = 8 and M = 4,
ef_construction = 100, seed 100.  With integers of this size every partial
sum is exact in float32, so the keys of the C++ search and of the Python model
(tests/hnsw_reference.py) must agree bit for bit whatever the summation
order; equal keys are frequent, so the (key, node) order is exercised.

The recall condition (model, ef = 64, k = 10, an answer counts if its key is
<= the exact 10th key, mean over the 64 queries >= 0.9) holds on this data
for both M and both metrics; the test records nothing, it asserts.
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
SRC = os.path.join(HERE, "host", "hnsw_core_test.cpp")
CORE = os.path.join(REPO, "dingo-store_amd", "csrc", "dg_hnsw_core.h")

import hnsw_reference as hr  # noqa: E402
import hnswlib_format as hf  # noqa: E402

CASES = [(1, 1), (10, 10), (10, 64), (20, 8)]
BUILDS = [(8, hr.L2), (4, hr.L2), (8, hr.IP)]
OK, ENOT_SUPPORT, EIO = 0, 3, 6


def _cxx():
    for c in ("g++", "c++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(c)
        if p:
            return p
    raise AssertionError("no C++ compiler found")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hnsw_core") / "hnsw_core_test")
    r = subprocess.run([_cxx(), "-std=c++17", "-O2", "-Wall", SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


class Dump:
    def __init__(self, path):
        self.path = path
        self.meta = {}
        for ln in open(os.path.join(path, "meta.txt")):
            k, v = ln.split()
            self.meta[k] = float(v) if k == "mult" else int(v)
        m = self.meta
        f = lambda name, dt: np.fromfile(os.path.join(path, name), dt)  # noqa
        self.rows = f("rows.f32", np.float32).reshape(m["n"], m["d"])
        self.queries = f("queries.f32", np.float32).reshape(m["nq"], m["d"])
        self.ids = f("ids.i64", np.int64)
        self.levels = f("levels.i32", np.int32)
        self.cnt0 = f("cnt0.i32", np.int32)
        self.links0 = f("links0.u32", np.uint32).reshape(m["n"], m["maxM0"])
        self.up_off = f("up_off.i64", np.int64)
        self.up_cnt = f("up_cnt.i32", np.int32)
        self.up_links = f("up_links.u32", np.uint32)
        self.deleted1 = f("deleted1.u8", np.uint8)
        self.container = open(os.path.join(path, "container.bin"),
                              "rb").read()
        self.container_deleted = open(
            os.path.join(path, "container_deleted.bin"), "rb").read()

    def graph(self, deleted):
        m = self.meta
        return hr.from_upper_lists(
            m["metric"], self.rows, deleted, self.levels, self.cnt0,
            self.links0, self.up_off, self.up_cnt, self.up_links, m["M"],
            m["entry"], m["max_level"])

    def result(self, scenario, k, ef):
        tag = os.path.join(self.path, f"res_{scenario}_{k}_{ef}")
        nq = self.meta["nq"]
        return (np.fromfile(tag + ".nodes.i64", np.int64).reshape(nq, k),
                np.fromfile(tag + ".keys.f32", np.float32).reshape(nq, k),
                np.fromfile(tag + ".ctr.i64", np.int64).reshape(nq, 2))


@pytest.fixture(scope="module", params=BUILDS,
                ids=lambda p: f"M{p[0]}-metric{p[1]}")
def dump(request, exe, tmp_path_factory):
    m, metric = request.param
    path = str(tmp_path_factory.mktemp(f"hnsw_dump_{m}_{metric}"))
    _run(exe, "dump", m, metric, path)
    return Dump(path)


def test_self_check(exe):
    assert _run(exe).strip().endswith("OK")


def test_core_is_free_of_hip():
    src = open(CORE).read()
    includes = re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", src)
    assert all("hip" not in i and "rocblas" not in i for i in includes), \
        includes
    assert "__device__" not in src and "__global__" not in src


def test_sanitizer_build_runs_its_self_check(tmp_path):
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=undefined"]
    # whether this compiler has the sanitizer runtimes is decided on an empty
    # program, before the project's source is touched
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run([_cxx(), *flags, str(probe), "-o",
                        str(tmp_path / "probe")],
                       capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("no sanitizer runtime for this compiler")
    out = str(tmp_path / "hnsw_core_test_asan")
    r = subprocess.run([_cxx(), *flags, SRC, "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert _run(out).strip().endswith("OK")


def test_graph_invariants(dump):
    m = dump.meta
    n, M = m["n"], m["M"]
    assert m["maxM0"] == 2 * M and m["max_level"] >= 1
    assert (dump.levels > 0).any()
    assert dump.levels[m["entry"]] == m["max_level"] == dump.levels.max()
    assert np.array_equal(np.diff(dump.up_off), dump.levels)
    assert ((0 <= dump.cnt0) & (dump.cnt0 <= 2 * M)).all()
    assert ((0 <= dump.up_cnt) & (dump.up_cnt <= M)).all()
    g = dump.graph(np.zeros(n, bool))
    for level in range(m["max_level"] + 1):
        for i in np.nonzero(dump.levels >= level)[0]:
            nb = g.neighbours(i, level)
            assert len(set(nb)) == len(nb) and i not in nb
            assert all(0 <= e < n and dump.levels[e] >= level for e in nb)
    assert len(set(dump.ids.tolist())) == n and (dump.ids >= 0).all()
    # the level draw: floor(-ln(u) / ln(M)), so about 1 / M of the nodes
    # have a level above 0
    frac = (dump.levels > 0).mean()
    assert 0.5 / M < frac < 2.0 / M, frac


@pytest.mark.parametrize("scenario", [0, 1, 2])
def test_model_reproduces_the_reference_search(dump, scenario):
    n = dump.meta["n"]
    deleted = dump.deleted1 if scenario == 1 else np.zeros(n, np.uint8)
    passes = np.zeros(n, bool) if scenario == 2 else None
    g = dump.graph(deleted)
    if scenario == 1:
        assert deleted[dump.meta["entry"]] and 0.2 < deleted.mean() < 0.4
    for k, ef in CASES:
        nodes, keys, ctr = dump.result(scenario, k, ef)
        for qi, q in enumerate(dump.queries):
            mn, mk, pops, evals = hr.search(g, q, k, ef, passes)
            assert np.array_equal(mn, nodes[qi]), (k, ef, qi)
            assert np.array_equal(mk.view(np.uint32),
                                  keys[qi].view(np.uint32)), (k, ef, qi)
            assert (pops, evals) == tuple(ctr[qi]), (k, ef, qi)
        if scenario == 2:
            assert (nodes == -1).all() and (keys == 0).all()
        elif scenario == 1:
            assert not deleted[nodes[nodes >= 0]].any()
            assert (nodes >= 0).all()
        assert (ctr[:, 0] >= 1).all() and (ctr[:, 1] > ctr[:, 0]).all()


def test_ties_are_exercised(dump):
    """The order rule matters only if equal keys meet: they do."""
    g = dump.graph(np.zeros(dump.meta["n"], bool))
    nodes, keys, _ = dump.result(0, 10, 64)
    tied = sum(len(np.unique(r)) < len(r) for r in keys)
    assert tied >= len(keys) // 2
    for r, nd in zip(keys, nodes):  # ascending by (key, node)
        pairs = list(zip(r.tolist(), nd.tolist()))
        assert pairs == sorted(pairs)
    assert g.n == 2000


def test_recall_condition(dump):
    g = dump.graph(np.zeros(dump.meta["n"], bool))
    nodes, keys, _ = dump.result(0, 10, 64)
    hits = 0
    for qi, q in enumerate(dump.queries):
        tenth = np.sort(hr.exact_keys(g, q))[9]
        hits += int((keys[qi][nodes[qi] >= 0] <= tenth).sum())
    assert hits / (10 * len(dump.queries)) >= 0.9


def test_container_bytes_equal_the_graph(dump):
    for blob, deleted in ((dump.container, np.zeros(2000, np.uint8)),
                          (dump.container_deleted, dump.deleted1)):
        p = hf.parse(blob)
        m = dump.meta
        assert (p["n"], p["d"], p["M"], p["maxM"], p["maxM0"]) == \
            (m["n"], m["d"], m["M"], m["M"], 2 * m["M"])
        assert p["max_elements"] >= p["n"]
        assert p["maxlevel"] == m["max_level"]
        assert p["enterpoint"] == m["entry"]
        assert p["ef_construction"] == m["ef_construction"]
        assert p["mult"] == m["mult"] == 1.0 / np.log(float(m["M"]))
        assert np.array_equal(p["cnt0"], dump.cnt0)
        assert np.array_equal(p["deleted"], deleted)
        assert np.array_equal(p["links0"], dump.links0)
        assert np.array_equal(p["rows"].view(np.uint32),
                              dump.rows.view(np.uint32))
        assert np.array_equal(p["labels"], dump.ids)
        assert np.array_equal(p["levels"], dump.levels)
        ul = dump.up_links.reshape(-1, m["M"])
        for i in np.nonzero(dump.levels > 0)[0]:
            for l, (c, lk) in enumerate(p["upper"][i]):
                at = dump.up_off[i] + l
                assert c == dump.up_cnt[at] and np.array_equal(lk, ul[at])


def _status(exe, tmp_path, blob, metric, d, name="v.bin"):
    path = str(tmp_path / name)
    with open(path, "wb") as f:
        f.write(blob)
    return int(_run(exe, "load", path, metric, d).split()[0])


def test_container_reader_refuses_malformed_files(dump, exe, tmp_path):
    blob, m = dump.container, dump.meta
    p = hf.parse(blob)
    metric, d = m["metric"], m["d"]
    st = lambda b, dd=d: _status(exe, tmp_path, b, metric, dd)  # noqa: E731
    out = _run(exe, "load", os.path.join(dump.path, "container.bin"), metric,
               d).split()
    assert list(map(int, out)) == [OK, m["n"], m["max_level"], m["entry"], 0]
    out = _run(exe, "load", os.path.join(dump.path, "container_deleted.bin"),
               metric, d).split()
    assert int(out[0]) == OK and int(out[4]) == int(dump.deleted1.sum())
    # d must be what the sizes say
    assert st(blob, d + 1) == EIO and st(blob, d - 1) == EIO
    # length: short, long, empty
    assert st(blob[:-1]) == EIO and st(blob + b"\0") == EIO
    assert st(blob[:50]) == EIO and st(b"") == EIO
    # inconsistent sizes
    assert st(hf.patch(blob, 0, "<Q", 8)) == EIO
    assert st(hf.patch(blob, hf.H_PER_ELEM, "<Q", p["per_elem"] + 4)) == EIO
    assert st(hf.patch(blob, hf.H_OFF_DATA, "<Q", p["off_data"] + 4)) == EIO
    assert st(hf.patch(blob, hf.H_MAXM0, "<Q", p["maxM0"] + 1)) == EIO
    assert st(hf.patch(blob, hf.H_MAXM, "<Q", p["maxM"] + 1)) == EIO
    assert st(hf.patch(blob, hf.H_COUNT, "<Q", p["n"] + 1)) == EIO
    assert st(hf.patch(blob, hf.H_MAX_ELEMENTS, "<Q", p["n"] - 1)) == EIO
    # M outside 2 .. 128
    assert st(hf.patch(blob, hf.H_M, "<Q", 1)) == ENOT_SUPPORT
    assert st(hf.patch(blob, hf.H_M, "<Q", 129)) == ENOT_SUPPORT
    # a node with full level-0 list and one with an upper level
    r0 = p["rec_off"][0]
    i_up = int(np.nonzero(dump.levels > 0)[0][0])
    i_flat = int(np.nonzero(dump.levels == 0)[0][0])
    # count above its cap, at level 0 and above
    assert st(hf.patch(blob, r0, "<I", p["maxM0"] + 1)) == EIO
    assert st(hf.patch(blob, p["ll_off"][i_up] + 4, "<I",
                       p["maxM"] + 1)) == EIO
    # link out of range, link to the node itself
    assert dump.cnt0[0] > 0
    assert st(hf.patch(blob, r0 + 4, "<I", p["n"])) == EIO
    assert st(hf.patch(blob, r0 + 4, "<I", 0)) == EIO
    # an upper-level link to a node that lacks the level
    assert dump.up_cnt[dump.up_off[i_up]] > 0
    assert st(hf.patch(blob, p["ll_off"][i_up] + 8, "<I", i_flat)) == EIO
    # entry point not on maxlevel; maxlevel wrong
    assert st(hf.patch(blob, hf.H_ENTER, "<I", i_flat)) == EIO
    assert st(hf.patch(blob, hf.H_ENTER, "<I", p["n"])) == EIO
    assert st(hf.patch(blob, hf.H_MAXLEVEL, "<i", m["max_level"] + 1)) == EIO
    # linkListSize not a whole number of lists
    assert st(hf.patch(blob, p["ll_off"][i_up], "<I",
                       4 + 4 * p["maxM"] + 4)) == EIO
    # labels: negative, repeated among live nodes (fine if one is deleted)
    lab = lambda i: p["rec_off"][i] + p["label_off"]  # noqa: E731
    assert st(hf.patch(blob, lab(3), "<q", -1)) == EIO
    dup = hf.patch(blob, lab(3), "<q", int(dump.ids[4]))
    assert st(dup) == EIO
    assert st(hf.patch(dup, p["rec_off"][3] + 2, "<B", 1)) == OK
    # rows must be finite
    at = p["rec_off"][5] + p["off_data"]
    assert st(hf.patch(blob, at, "<f", float("nan"))) == EIO
    assert st(hf.patch(blob, at + 4, "<f", float("inf"))) == EIO
