"""4-bit IVF-PQ through the own container and the faiss IwPQ container
(marked gpu): packed codes, low nibble first, code_size = m/2.

The faiss files are parsed with tests/faiss_format.py and, for the loader,
assembled here from numpy arrays with this file's own writer and packer, so
the layout is stated twice, independently of the library.
"""
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd"), HERE]

pytestmark = pytest.mark.gpu

dg = pytest.importorskip("dingostore")

import faiss_format as ff  # noqa: E402
from pq_reference import add_all, grouped_case, pack4, unpack4  # noqa: E402

LENS = [300, 257, 1025, 0, 3]  # an empty list too
D, M = 32, 8


def _same_bits(a, b):
    return (np.array_equal(a[1], b[1]) and
            np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)))


@pytest.fixture(scope="module")
def built():
    """A 4-bit index with shuffled rows and ids that are not positions."""
    case, lists, codes, x32 = grouped_case(dg.L2, D, M, LENS, 311)
    perm = case.rng.permutation(len(lists))
    lists, codes, x32 = lists[perm], codes[perm], x32[perm]
    ids = 5 * np.arange(len(lists), dtype=np.int64) + 11
    idx = case.new_index()
    add_all(case, idx, lists, codes, np.ascontiguousarray(x32), ids)
    q = case.queries(np.array([0, 0, 1, 2, 2, 4, 1]))
    yield case, idx, q
    idx.close()


def test_own_container_round_trip(built, tmp_path):
    case, idx, q = built
    path = str(tmp_path / "pq4.dgi")
    idx.save(path)
    # m * 16 * dsub codebook floats and m/2 code bytes per row, not the
    # 8-bit sizes: the file is smaller than codes alone would be at 8 bits
    n = len(case.ids)
    assert os.path.getsize(path) < (D * len(LENS) * 4 + M * 16 * (D // M) * 4
                                    + n * (M // 2 + 12) + 4096)
    back = dg.Index.load(path)
    try:
        assert (back.m, back.nbits) == (M, 4)
        assert np.array_equal(back.get_codebooks(), case.cb32)
        for nprobe in (1, len(LENS)):
            want = idx.search(q, 10, nprobe=nprobe)
            got = back.search(q, 10, nprobe=nprobe)
            assert _same_bits(got, want)
            case.check(q, 10, nprobe, *got)
    finally:
        back.close()


def test_save_faiss_layout(built, tmp_path):
    case, idx, q = built
    path = str(tmp_path / "pq4.faissindex")
    idx.save_faiss(path)
    f = ff.read_index(path)
    assert f["kind"] == "ivfpq" and f["by_residual"] == 1
    assert f["pq"]["nbits"] == 4
    assert f["pq"]["M"] == M and f["pq"]["d"] == D
    assert f["code_size"] == M // 2
    assert f["invlists"]["code_size"] == M // 2
    cents = f["pq"]["centroids"]
    assert len(cents) == M * 16 * (D // M)
    assert np.array_equal(cents.reshape(M, 16, D // M), case.cb32)
    assert f["header"]["ntotal"] == len(case.ids)
    by_id = dict(zip(case.ids.tolist(), range(len(case.ids))))
    for l in range(len(LENS)):
        ids = f["invlists"]["ids"][l]
        assert len(ids) == LENS[l]
        rows = np.array([by_id[i] for i in ids.tolist()], np.int64)
        assert (case.lists[rows] == l).all()
        # each byte: sub-quantizer 2j low nibble, 2j+1 high nibble
        got = unpack4(f["invlists"]["codes"][l], M)
        assert np.array_equal(got, case.codes[rows].reshape(-1, M))


def test_save_faiss_load_faiss_same_search(built, tmp_path):
    case, idx, q = built
    path = str(tmp_path / "pq4.faissindex")
    idx.save_faiss(path)
    back = dg.Index.load_faiss(path)
    try:
        assert (back.m, back.nbits) == (M, 4)
        for nprobe in (1, len(LENS)):
            want = idx.search(q, 10, nprobe=nprobe)
            got = back.search(q, 10, nprobe=nprobe)
            # the file groups rows by list: positions, and so tie order, may
            # differ; distances may not
            assert np.array_equal(got[0].view(np.uint32),
                                  want[0].view(np.uint32))
            case.check(q, 10, nprobe, *got)
    finally:
        back.close()


# ---- a writer of this file's own -------------------------------------
def _header(d, ntotal, metric_l2=True):
    return (struct.pack("<iqqq", d, ntotal, 1 << 20, 1 << 20) +
            struct.pack("<B", 1) + struct.pack("<i", 1 if metric_l2 else 0))


def _iwpq_bytes(case, nbits, pq_code_size, list_code_size, packed_by_list,
                ids_by_list):
    d, m, nlist = case.d, case.m, case.nlist
    ntotal = sum(len(i) for i in ids_by_list)
    out = [b"IwPQ", _header(d, ntotal), struct.pack("<QQ", nlist, 1)]
    out += [b"IxF2", _header(d, nlist), struct.pack("<Q", nlist * d),
            case.cents32.tobytes()]
    out += [struct.pack("<BQ", 0, 0)]  # direct map: none
    out += [struct.pack("<B", 1), struct.pack("<Q", pq_code_size),
            struct.pack("<QQQ", d, m, nbits),
            struct.pack("<Q", case.cb32.size), case.cb32.tobytes()]
    out += [b"ilar", struct.pack("<QQ", nlist, list_code_size), b"full",
            struct.pack("<Q", nlist),
            np.array([len(i) for i in ids_by_list], np.uint64).tobytes()]
    for codes, ids in zip(packed_by_list, ids_by_list):
        out += [np.ascontiguousarray(codes, np.uint8).tobytes(),
                np.ascontiguousarray(ids, np.int64).tobytes()]
    return b"".join(out)


def _model_lists(case):
    packed, ids = [], []
    for l in range(case.nlist):
        rows = np.nonzero(case.lists == l)[0]
        packed.append(pack4(case.codes[rows].reshape(-1, case.m)))
        ids.append(case.ids[rows])
    return packed, ids


def test_load_faiss_file_built_from_numpy(tmp_path):
    """No encoder in the loop: codes packed here, searched to A-D."""
    case, lists, codes, _ = grouped_case(dg.L2, D, M, LENS, 313)
    ids = 3 * np.arange(len(lists), dtype=np.int64) + 7
    case.record(ids, lists, codes)
    packed, ids_by_list = _model_lists(case)
    path = str(tmp_path / "numpy.faissindex")
    with open(path, "wb") as f:
        f.write(_iwpq_bytes(case, 4, M // 2, M // 2, packed, ids_by_list))
    assert ff.read_index(path)["pq"]["nbits"] == 4  # the writer is sound
    idx = dg.Index.load_faiss(path)
    try:
        assert (idx.m, idx.nbits) == (M, 4)
        q = case.queries(np.array([0, 0, 1, 2, 2, 4, 1]))
        for nprobe in (1, len(LENS)):
            gd, gi = idx.search(q, 10, nprobe=nprobe)
            case.check(q, 10, nprobe, gd, gi)
    finally:
        idx.close()


@pytest.mark.parametrize("pq_cs,list_cs", [(M, M // 2), (M // 2, M),
                                           (M // 2 + 1, M // 2 + 1)])
def test_load_faiss_code_size_mismatch(tmp_path, pq_cs, list_cs):
    """code_size that disagrees with M * nbits / 8, in the PQ block or in
    the inverted lists, is refused like the loader's other mismatches."""
    case, lists, codes, _ = grouped_case(dg.L2, D, M, [5, 4, 0, 0, 3], 317)
    case.record(np.arange(len(lists)), lists, codes)
    packed, ids_by_list = _model_lists(case)
    packed = [np.resize(p, (len(p), list_cs)) for p in packed]
    path = str(tmp_path / "bad.faissindex")
    with open(path, "wb") as f:
        f.write(_iwpq_bytes(case, 4, pq_cs, list_cs, packed, ids_by_list))
    with pytest.raises(dg.DgError) as e:
        dg.Index.load_faiss(path)
    assert e.value.status in (3, 6), e.value  # DG_ENOT_SUPPORT or DG_EIO
