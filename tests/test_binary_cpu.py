"""Binary (Hamming) indexes, checks that need no GPU: the C-ABI exports the
binary entry points, the wrapper has the constants, parameter validation of
dg_index_create runs before any device is touched, and the numpy oracle the
GPU tests rely on agrees with a per-bit loop."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(REPO, "dingo-store_amd")]
SO = os.path.join(REPO, "dingo-store_amd", "libdingo_gpu.so")

import hamming_oracle as ho  # noqa: E402

needs_so = pytest.mark.skipif(not os.path.exists(SO),
                              reason="libdingo_gpu.so not built")

BINARY_SYMBOLS = [
    "dg_train_binary", "dg_set_centroids_binary", "dg_get_centroids_binary",
    "dg_add_binary", "dg_upsert_binary", "dg_search_binary",
    "dg_search_binary_device", "dg_mirror_selftest_binary",
]


@needs_so
def test_binary_symbols_exported():
    lib = C.CDLL(SO)
    missing = [s for s in BINARY_SYMBOLS if not hasattr(lib, s)]
    assert not missing, f"missing exports: {missing}"


@needs_so
def test_wrapper_constants():
    import dingostore as dg
    assert (dg.BINARY_FLAT, dg.BINARY_IVF_FLAT, dg.HAMMING) == (3, 4, 3)
    dg.lib()  # binds the binary argtypes


@needs_so
@pytest.mark.parametrize("kind", [3, 4])
@pytest.mark.parametrize("d,metric", [(12, 3), (0, 3), (32776, 3), (64, 0),
                                      (64, 1)])
def test_bad_binary_create_is_einval(kind, d, metric):
    """d % 8 != 0, d out of [8, 32768] and a non-Hamming metric are rejected
    with DG_EINVAL before the device is looked at."""
    import dingostore as dg
    with pytest.raises(dg.DgError) as e:
        dg.Index(kind, metric, d, nlist=4)
    assert e.value.status == 1, str(e.value)


@needs_so
def test_hamming_metric_on_float_kind_is_einval():
    import dingostore as dg
    with pytest.raises(dg.DgError) as e:
        dg.Index(dg.FLAT, dg.HAMMING, 64)
    assert e.value.status == 1, str(e.value)


@pytest.mark.parametrize("d", [8, 40, 1000])
def test_oracle_matches_per_bit_loop(d):
    rng = np.random.default_rng(d)
    a = rng.integers(0, 256, (50, d // 8), dtype=np.uint8)
    b = rng.integers(0, 256, (50, d // 8), dtype=np.uint8)
    full = ho.hamming(a, b)
    for i in range(50):
        assert full[i, i] == ho.hamming_naive(a[i], b[i], d)
    assert (ho.hamming(a, a).diagonal() == 0).all()


def test_flip_bits_and_probe_order():
    rng = np.random.default_rng(1)
    rows = np.zeros((200, 32), np.uint8)
    flipped = ho.flip_bits(rows, 0.05, rng)
    mean = ho.POPCOUNT[flipped].sum() / 200
    assert 5 < mean < 21  # 5 % of 256 bits = 12.8 expected
    coarse = np.array([[3, 1, 1, 0], [2, 2, 2, 2]], np.int32)
    assert ho.probed_lists(coarse, 3).tolist() == [[3, 1, 2], [0, 1, 2]]


def test_check_row_rejects_wrong_rows():
    adm_ids = np.array([10, 11, 12, 13], np.int64)
    adm_dist = np.array([2, 1, 2, 5], np.int32)
    ok_d = np.array([1, 2, 2], np.float32)
    ho.check_row(ok_d, np.array([11, 12, 10]), adm_ids, adm_dist)
    with pytest.raises(AssertionError):  # strictly-below id missing
        ho.check_row(np.array([2, 2], np.float32), np.array([10, 12]),
                     adm_ids, adm_dist)
    with pytest.raises(AssertionError):  # duplicate id
        ho.check_row(ok_d, np.array([11, 12, 12]), adm_ids, adm_dist)
    with pytest.raises(AssertionError):  # inadmissible id
        ho.check_row(ok_d, np.array([11, 12, 99]), adm_ids, adm_dist)
    with pytest.raises(AssertionError):  # padding expected past 4 rows
        ho.check_row(np.array([1, 2, 2, 5, 0], np.float32),
                     np.array([11, 12, 10, 13, 11]), adm_ids, adm_dist)
    ho.check_row(np.array([1, 2, 2, 5, 0], np.float32),
                 np.array([11, 12, 10, 13, -1]), adm_ids, adm_dist)
