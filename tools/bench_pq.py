#!/usr/bin/env python3
"""bench_pq.py — 8-bit against 4-bit IVF-PQ on one MI355X, in one process.

Builds one data set on the device from a seed (a Gaussian mixture with a
decaying per-dimension scale, so that PQ has structure to find), trains an
nbits=8 and an nbits=4 IVF-PQ index on the same sample, gives both the same
coarse centroids, and adds the same rows to both:

  d 768, m 96, n 10M, nlist 4096, nprobe 64, batch 4096, k 10

After --warmup untimed steps of each, --steps timed steps alternate between
the two indexes (8, 4, 8, 4, ...), so drift of clocks or temperature falls
on both alike.  A step is dg_search_device on device pointers plus one
dg_sync.  The JSON reports, per index, the median and the range of the step
time and of last_scan_ms (hipEvents around T build + scan kernel), the
algorithmic code bytes of a step, code bytes per row, and recall@10 against
a Flat index over the same rows for the first --recall-queries queries.

The comparison the 4-bit scan has to meet: its median scan time must not
exceed the 8-bit median by more than the run-to-run range (max - min) the
tool itself saw; "scan4_within_range_of_scan8" states it.

  python tools/bench_pq.py --out profiles/bench_pq4.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "dingo-store_amd"))

import dingostore as dg  # noqa: E402


class Data:
    """Rows of a seeded Gaussian mixture, generated chunk by chunk on the
    device: x = centre[c] + noise * scale, scale decaying over dimensions."""

    def __init__(self, torch, d, ncent, seed):
        self.torch, self.d, self.seed = torch, d, seed
        g = torch.Generator(device="cuda")
        g.manual_seed(seed)
        self.scale = (1.0 / torch.sqrt(
            1.0 + torch.arange(d, device="cuda", dtype=torch.float32) / 16.0))
        self.centres = torch.randn((ncent, d), device="cuda",
                                   generator=g) * self.scale * 2.0

    def chunk(self, start, count, stream=0):
        torch = self.torch
        g = torch.Generator(device="cuda")
        g.manual_seed(self.seed + 1000 * stream + 1 + start)
        c = torch.randint(0, self.centres.shape[0], (count,), device="cuda",
                          generator=g)
        x = torch.randn((count, self.d), device="cuda", generator=g)
        return (self.centres[c] + x * self.scale).contiguous()


def log(msg):
    print(f"[bench_pq] {msg}", file=sys.stderr, flush=True)


def add_rows(torch, data, indexes, n, step):
    for s in range(0, n, step):
        if (s // step) % 8 == 0:
            log(f"adding rows {s} / {n}")
        c = min(step, n - s)
        x = data.chunk(s, c)
        torch.cuda.synchronize()
        ids = np.arange(s, s + c, dtype=np.int64)
        for idx in indexes:
            idx.add_device(ids, x.data_ptr(), c)
        del x


def summarize(ms, scan, st, m, nbits):
    ms, scan = np.array(ms), np.array(scan)
    return {
        "nbits": nbits, "code_bytes_per_row": m * nbits // 8,
        "step_ms_median": float(np.median(ms)),
        "step_ms_min": float(ms.min()), "step_ms_max": float(ms.max()),
        "scan_ms_median": float(np.median(scan)),
        "scan_ms_min": float(scan.min()), "scan_ms_max": float(scan.max()),
        "scan_bytes_algorithmic": st["last_scan_bytes_algorithmic"],
        "scan_gbps_algorithmic_median":
            st["last_scan_bytes_algorithmic"] / np.median(scan) / 1e6,
        "device_bytes": st["device_bytes"],
    }


def recall_at_k(got, truth):
    hit = 0
    for g, t in zip(got, truth):
        hit += len(set(g.tolist()) & set(t.tolist()))
    return hit / truth.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--m", type=int, default=96)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--nprobe", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=262_144)
    ap.add_argument("--recall-queries", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 5:
        ap.error("--steps must be at least 5")
    import torch
    assert torch.cuda.is_available(), "bench_pq needs a GPU"
    d, m, n, nq, k = a.d, a.m, a.rows, a.batch, a.k
    data = Data(torch, d, 2048, a.seed)
    t_build = time.perf_counter()

    # one train sample, the same coarse centroids for both widths
    xt = data.chunk(0, min(a.train_rows, n), stream=7).cpu().numpy()
    ix = {}
    for nbits in (8, 4):
        ix[nbits] = dg.Index(dg.IVF_PQ, dg.L2, d, nlist=a.nlist, m=m,
                             nbits=nbits)
        ix[nbits].train(xt)
        log(f"trained nbits={nbits}")
    c8, c4 = ix[8].get_centroids(), ix[4].get_centroids()
    same_cents = bool(np.array_equal(c8, c4))
    if not same_cents:  # the ADC tables are rebuilt from the new centroids
        ix[4].set_centroids(c8)
    del xt
    flat = dg.Index(dg.FLAT, dg.L2, d)
    add_rows(torch, data, [ix[8], ix[4], flat], n, 1 << 18)
    build_s = time.perf_counter() - t_build

    # queries: fresh draws of the same mixture
    q = data.chunk(0, nq, stream=3)
    dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def step(idx):
        t0 = time.perf_counter()
        idx.search_device(q.data_ptr(), nq, k, a.nprobe, dist.data_ptr(),
                          ids.data_ptr())
        idx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        return ms, idx.stats()

    log(f"built in {build_s:.1f} s; warm-up")
    for _ in range(a.warmup):
        for nbits in (8, 4):
            step(ix[nbits])
    log("timed steps")
    ms = {8: [], 4: []}
    scan = {8: [], 4: []}
    last = {}
    for _ in range(a.steps):
        for nbits in (8, 4):
            t, st = step(ix[nbits])
            ms[nbits].append(t)
            scan[nbits].append(st["last_scan_ms"])
            last[nbits] = st
    res = {nbits: summarize(ms[nbits], scan[nbits], last[nbits], m, nbits)
           for nbits in (8, 4)}

    log("recall")
    # recall@k against Flat on the same rows
    nr = min(a.recall_queries, nq)
    qr = q[:nr].contiguous()
    torch.cuda.synchronize()
    _, truth = flat.search(qr.cpu().numpy(), k)
    for nbits in (8, 4):
        _, got = ix[nbits].search(qr.cpu().numpy(), k, nprobe=a.nprobe)
        res[nbits][f"recall_at_{k}"] = recall_at_k(got, truth)

    rng8 = res[8]["scan_ms_max"] - res[8]["scan_ms_min"]
    rng4 = res[4]["scan_ms_max"] - res[4]["scan_ms_min"]
    out = {
        "tool": "tools/bench_pq.py", "build": dg.build_info(),
        "rows": n, "d": d, "m": m, "nlist": a.nlist, "nprobe": a.nprobe,
        "batch": nq, "k": k, "steps": a.steps, "warmup": a.warmup,
        "train_rows": min(a.train_rows, n), "recall_queries": nr,
        "centroids_identical_after_train": same_cents,
        "build_seconds": build_s,
        "nbits8": res[8], "nbits4": res[4],
        "scan4_over_scan8_median":
            res[4]["scan_ms_median"] / res[8]["scan_ms_median"],
        "run_to_run_range_ms": max(rng8, rng4),
        "scan4_within_range_of_scan8": bool(
            res[4]["scan_ms_median"] <=
            res[8]["scan_ms_median"] + max(rng8, rng4)),
    }
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for i in (ix[8], ix[4], flat):
        i.close()


if __name__ == "__main__":
    main()
