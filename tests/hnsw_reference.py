"""An independent Python model of the HNSW reference search
over a graph given as plain arrays: the dump of tests/host/hnsw_core_test.cpp
or what Index.hnsw_export returns.  It shares no code with dg_hnsw_core.h.

Everything is ordered by the pair (key, internal node), ascending.  Keys are
float32: sum (q - x)^2 for L2, 0 - sum q * x for IP / cosine.  On the integer
data of the exact tests every partial sum is exact, so the summation order of
an implementation cannot show.
"""
import bisect

import numpy as np

L2, IP, COSINE = 0, 1, 2


class Graph:
    """rows [n, d] float32; deleted [n] bool; counts[l] [n] int (-1: the node
    has no level l) and links[l] [n, cap(l)] for l = 0 .. max_level."""

    def __init__(self, metric, rows, deleted, counts, links, entry,
                 max_level):
        self.metric = metric
        self.rows = np.ascontiguousarray(rows, np.float32)
        self.n = len(self.rows)
        self.deleted = np.asarray(deleted, bool)
        self.counts, self.links = counts, links
        self.entry, self.max_level = int(entry), int(max_level)

    def neighbours(self, node, level):
        c = int(self.counts[level][node])
        assert c >= 0, (node, level)
        return [int(e) for e in self.links[level][node, :c]]

    def keys(self, q, nodes):
        x = self.rows[nodes]
        if self.metric == L2:
            df = x - q[None, :]
            return (df * df).sum(1, dtype=np.float32)
        return np.float32(0) - (x * q[None, :]).sum(1, dtype=np.float32)


def from_upper_lists(metric, rows, deleted, levels, cnt0, links0, up_off,
                     up_cnt, up_links, max_m, entry, max_level):
    """The per-(node, level) list form of the C++ dump as per-level arrays."""
    n = len(levels)
    counts, links = [np.asarray(cnt0, np.int64)], [np.asarray(links0)]
    up_links = np.asarray(up_links).reshape(-1, max_m)
    for l in range(1, max_level + 1):
        c = np.full(n, -1, np.int64)
        lk = np.zeros((n, max_m), np.uint32)
        for i in np.nonzero(np.asarray(levels) >= l)[0]:
            at = int(up_off[i]) + l - 1
            c[i] = up_cnt[at]
            lk[i] = up_links[at]
        counts.append(c)
        links.append(lk)
    return Graph(metric, rows, deleted, counts, links, entry, max_level)


def search(g, q, k, ef, passes=None):
    """-> (nodes [k] int64, keys [k] float32, expansions, dist_evals); nodes
    are internal, padded with -1 / 0.0.  passes: [n] bool or None."""
    nodes = np.full(k, -1, np.int64)
    keys = np.zeros(k, np.float32)
    if g.n == 0 or g.entry < 0:
        return nodes, keys, 0, 0
    q = np.asarray(q, np.float32)
    efp = max(ef, k)

    def admissible(e):
        return not g.deleted[e] and (passes is None or bool(passes[e]))

    cur = (float(g.keys(q, [g.entry])[0]), g.entry)
    evals, pops = 1, 0
    for level in range(g.max_level, 0, -1):
        while True:
            nb = g.neighbours(cur[1], level)
            best = cur
            if nb:
                kk = g.keys(q, nb)
                evals += len(nb)
                best = min(best, min((float(a), b) for a, b in zip(kk, nb)))
            if best == cur:
                break
            cur = best
    visited = {cur[1]}
    C = [cur]
    W = [cur] if admissible(cur[1]) else []
    while C:
        if len(W) == efp and C[0] > W[-1]:
            break
        c = C.pop(0)
        pops += 1
        fresh = []
        for e in g.neighbours(c[1], 0):
            if e not in visited:
                visited.add(e)
                fresh.append(e)
        if not fresh:
            continue
        kk = g.keys(q, fresh)
        evals += len(fresh)
        for key, e in zip(kk, fresh):
            item = (float(key), e)
            if len(W) < efp or item < W[-1]:
                if len(C) < efp:
                    bisect.insort(C, item)
                elif item < C[-1]:
                    C.pop()
                    bisect.insort(C, item)
                if admissible(e):
                    bisect.insort(W, item)
                    if len(W) > efp:
                        W.pop()
    for i, (key, e) in enumerate(W[:k]):
        nodes[i], keys[i] = e, key
    return nodes, keys, pops, evals


def search_batch(g, queries, k, ef, passes=None):
    out = [search(g, q, k, ef, passes) for q in queries]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]),
            sum(o[2] for o in out), sum(o[3] for o in out))


def exact_keys(g, q):
    """Every node's key, for recall conditions."""
    return g.keys(np.asarray(q, np.float32), np.arange(g.n))
