"""numpy Hamming oracle and the exact acceptance rule shared by the binary
index tests (test_binary_cpu.py, test_binary_gpu.py).

Bit vectors are np.uint8 rows of d // 8 bytes.  Distances are exact
integers, so every check below is exact: no tolerance, no skipped rows.
"""
import numpy as np

POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b, block=64):
    """[len(a), len(b)] int32 Hamming distances via a 256-entry LUT over
    a[:, None, :] ^ b[None, :, :] (blocked over a to bound the temporary)."""
    a = np.ascontiguousarray(a, np.uint8)
    b = np.ascontiguousarray(b, np.uint8)
    out = np.empty((a.shape[0], b.shape[0]), np.int32)
    for s in range(0, a.shape[0], block):
        x = a[s:s + block, None, :] ^ b[None, :, :]
        out[s:s + block] = POPCOUNT[x].sum(axis=2, dtype=np.int32)
    return out


def hamming_naive(a, b, d):
    """Per-bit loop over two single rows (the check of the LUT helper)."""
    n = 0
    for j in range(d):
        ba = (int(a[j // 8]) >> (j % 8)) & 1
        bb = (int(b[j // 8]) >> (j % 8)) & 1
        n += ba != bb
    return n


def flip_bits(rows, frac, rng):
    """Each bit of each row flipped with probability frac."""
    rows = np.ascontiguousarray(rows, np.uint8)
    flips = rng.random((rows.shape[0], rows.shape[1] * 8)) < frac
    return rows ^ np.packbits(flips, axis=1, bitorder="little")


def probed_lists(coarse, nprobe):
    """[nq, nprobe] lists by (distance, list id): the stated tie rule."""
    nq, nlist = coarse.shape
    lid = np.broadcast_to(np.arange(nlist), (nq, nlist))
    order = np.lexsort((lid, coarse), axis=1)
    return order[:, :nprobe]


def check_row(dist, ids, adm_ids, adm_dist, where=""):
    """Exact acceptance of one result row against the admissible rows
    (probed lists, filter-passing, not removed):
      1. returned distances = the k smallest admissible distances, ascending
      2. every id >= 0 is admissible, unique, and its oracle distance equals
         the returned one
      3. every admissible id strictly below the k-th distance is returned
      4. slots beyond the admissible count hold id -1
    adm_ids must be unique."""
    k = len(ids)
    m = min(k, len(adm_ids))
    want = np.sort(adm_dist)[:m]
    assert np.array_equal(dist[:m], want.astype(np.float32)), (
        where, dist[:m], want)
    assert (ids[m:] == -1).all(), (where, ids[m:])
    got = ids[:m]
    assert (got >= 0).all(), (where, got)
    assert len(np.unique(got)) == m, (where, got)
    order = np.argsort(adm_ids, kind="stable")
    sid = adm_ids[order]
    pos = np.searchsorted(sid, got)
    assert (pos < len(sid)).all() and (sid[np.minimum(pos, len(sid) - 1)]
                                       == got).all(), (where, got)
    assert np.array_equal(adm_dist[order][pos].astype(np.float32),
                          dist[:m]), (where, got)
    if m:
        must = adm_ids[adm_dist < want[-1]] if m == k else adm_ids
        assert np.isin(must, got).all(), (where, must, got)
