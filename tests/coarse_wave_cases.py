"""Inputs of test_coarse_wave.py (GPU) and test_coarse_wave_cpu.py: the case
tables of the coarse probe selection (k_coarse_select against k_select_dense
+ k_probe_unpack) and, for the cases that are also checked against
ivf_reference's float64 coarse ranking, which queries have an unambiguous
probe set.  The CPU file asserts that at most AMBIGUOUS_MAX of the queries of
every such case are ambiguous, so the GPU file can rely on it.
"""
import functools
import types

import numpy as np

import ivf_reference as ir
from flat_reference import COSINE, IP, L2

CAP = 128            # kCoarseWaveMaxNp (dg_coarse_wave.h)
D, N_ROWS, NQ, K = 32, 3000, 100, 10
AMBIGUOUS_MAX = 0.02

# 1. geometry of the column loop: rows of 33 and 65 floats are not 16-byte
# aligned (scalar loads), 100 and 1024 are (float4 loads, 1024 = one float4
# per thread), 4099 is neither a multiple of 4 nor of the block; 33 < one
# wave.  129 = CAP + 1 keeps the old path.
GEOM_NLISTS = [33, 65, 100, 1024, 4099]
GEOM_NPS = [1, 2, 31, 32, 33, 64, 80, CAP, CAP + 1]


def geom_nps(nlist):
    """GEOM_NPS clipped to < nlist, without repeats, in order."""
    out = []
    for p in GEOM_NPS:
        p = min(p, nlist - 1)
        if p not in out:
            out.append(p)
    return out


def _case(seed, nlist, d, metric, n=N_ROWS, nq=NQ, cents=None,
          integer=False):
    rng = np.random.default_rng(seed)
    if cents is None:
        cents = rng.standard_normal((nlist, d)).astype(np.float32)
    if integer:
        x = rng.integers(-3, 4, (n, d)).astype(np.float32)
        q = rng.integers(-3, 4, (nq, d)).astype(np.float32)
    else:
        x = rng.standard_normal((n, d)).astype(np.float32)
        q = rng.standard_normal((nq, d)).astype(np.float32)
        # away from the "already normalised" rule of the cosine path
        x[:, 0] += 2.0
        q[:, 0] += 2.0
    c = types.SimpleNamespace(
        metric=metric, d=d, nlist=nlist, n=n, cents=cents, x=x, q=q,
        ids=7 * np.arange(n, dtype=np.int64) + 3)
    for a in (c.cents, c.x, c.q, c.ids):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def geom_case(nlist):
    return _case(9000 + nlist, nlist, D, L2)


# 2. nlist 16400 = 2 segments of the old kernel (nlist / 8192)
SEG_NLIST, SEG_D, SEG_NPS, SEG_NQ = 16400, 8, (32, 80), 17
assert SEG_NLIST // 8192 == 2


@functools.lru_cache(maxsize=None)
def seg_case():
    return _case(9100, SEG_NLIST, SEG_D, L2, n=4000, nq=SEG_NQ)


# 3. ties: every centroid four times at scattered list ids; all identical.
# Centroids and queries hold small integers, so every dot product, norm and
# key is an exact integer in f32 whatever the summation order: equal scores
# are equal bits, other centroids tie by chance too, and the float64 ranking
# with ties to the smaller list id (tie_order) is the exact answer.
TIE_NLIST, TIE_NPS = 1024, (1, 3, 32, 80, CAP)


@functools.lru_cache(maxsize=None)
def tie_case(identical):
    rng = np.random.default_rng(9200 + int(identical))
    if identical:
        cents = np.tile(rng.integers(-3, 4, (1, D)), (TIE_NLIST, 1))
    else:
        base = rng.integers(-3, 4, (TIE_NLIST // 4, D))
        cents = np.tile(base, (4, 1))[rng.permutation(TIE_NLIST)]
    return _case(9210 + int(identical), TIE_NLIST, D, L2,
                 cents=np.ascontiguousarray(cents, np.float32), integer=True)


def tie_order(c):
    """int [nq, nlist]: the lists by ||c||^2 - 2 q.c, ties by list id."""
    q, ce = c.q.astype(np.float64), c.cents.astype(np.float64)
    s = (ce * ce).sum(1)[None, :] - 2.0 * (q @ ce.T)
    assert np.abs(s).max() < 2 ** 24 and (s == np.round(s)).all()
    return np.argsort(s, axis=1, kind="stable")


# 4. metrics and kinds
KIND_NLIST, KIND_NPS = 100, (32, 80)
KIND_METRICS = (L2, IP, COSINE)


@functools.lru_cache(maxsize=None)
def kind_case(metric):
    return _case(9300 + metric, KIND_NLIST, D, metric)


def unambiguous(c, nprobe):
    """(probed bool [nq, nlist], bool [nq]: the float64 gap between the
    nprobe-th and the next centroid exceeds ivf_reference's tie margin)."""
    probed, amb = ir.probe_sets(c.metric, c.q, c.cents, nprobe)
    clear = np.ones(len(c.q), bool)
    clear[amb] = False
    return probed, clear


def reference_checked():
    """Every (case, nprobe) the GPU file compares with the reference."""
    for nlist in GEOM_NLISTS:
        for p in geom_nps(nlist):
            yield ("geom", nlist), geom_case(nlist), p
    for metric in KIND_METRICS:
        for p in KIND_NPS:
            yield ("kind", metric), kind_case(metric), p
