#!/usr/bin/env python3
"""bench_hnsw.py — the HNSW index (DG_INDEX_HNSW) on one MI355X.

For each dimension (default 128 and 768) it draws --rows clustered rows
(256 Gaussian centres, sigma 0.35 around them; uniform noise has no
neighbourhood structure for a graph to find) and 1024 queries from the same
mixture, builds an HNSW index (M 16, ef_construction 100; the build is one
host thread and its wall time is reported) and a Flat index over the same
rows, and takes the Flat index's top-10 as the exact answers.

Per batch size (1 and 1024) and ef (16, 64, 256) it runs --warmup untimed and
--steps timed searches through dg_search_hnsw_device on device pointers, one
dg_sync per step, and reports

  qps            queries per second of wall time (median step)
  recall_at_10   against the Flat answers on the same rows
  dist_evals_q   keys computed per query (dg_hnsw_last_counters)
  kernel_ms      k_hnsw_search, hipEvents around it (median)
  gather_tbps    dist_evals * 4 * d / kernel time: the rate at which row
                 bytes were gathered.  The guide's datum for random whole
                 rows gathered once into registers is 5.5 TB/s; it is printed
                 beside the figure as a comparison, not asserted.

and, beside them, the Flat index's QPS on the same data at the same batch.
Nothing here is a pass mark.  At 100k rows the Flat GEMM may simply win at
batch 1024; the JSON says so plainly in "flat_faster".

  python tools/bench_hnsw.py --out profiles/bench_hnsw.json
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

GUIDE_GATHER_TBPS = 5.5


def log(msg):
    print(f"[bench_hnsw] {msg}", file=sys.stderr, flush=True)


def mixture(rng, cents, n, sigma):
    pick = rng.integers(0, len(cents), n)
    return (cents[pick] + sigma * rng.standard_normal(
        (n, cents.shape[1]), dtype=np.float32)).astype(np.float32)


def timed(fn, sync, warmup, steps):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return float(np.median(out))


def run_dim(torch, d, args):
    rng = np.random.default_rng(args.seed + d)
    cents = rng.standard_normal((256, d), dtype=np.float32)
    x = mixture(rng, cents, args.rows, 0.35)
    q = mixture(rng, cents, 1024, 0.35)
    ids = np.arange(args.rows, dtype=np.int64)

    flat = dg.Index(dg.FLAT, dg.L2, d)
    flat.add(ids, x)
    _, truth = flat.search(q, 10)

    hn = dg.Index(dg.HNSW, dg.L2, d)
    hn.hnsw_configure(args.m, args.efc, 100)
    t0 = time.perf_counter()
    hn.add(ids, x)
    build_s = time.perf_counter() - t0
    info = hn.hnsw_info()
    log(f"d={d}: host build of {args.rows} rows {build_s:.1f} s, "
        f"max_level {info['max_level']}")

    tq = torch.from_numpy(q).cuda()
    res = {"d": d, "rows": args.rows, "nlinks": args.m,
           "ef_construction": args.efc, "host_build_s": build_s,
           "max_level": info["max_level"], "runs": []}
    for nq in (1, 1024):
        td = torch.empty((nq, 10), dtype=torch.float32, device="cuda")
        ti = torch.empty((nq, 10), dtype=torch.int64, device="cuda")
        flat_s = timed(lambda: flat.search_device(
            tq.data_ptr(), nq, 10, 0, td.data_ptr(), ti.data_ptr()),
            flat.sync, args.warmup, args.steps)
        flat_qps = nq / flat_s
        for ef in (16, 64, 256):
            step = lambda: hn.search_hnsw_device(  # noqa: E731
                tq.data_ptr(), nq, 10, ef, td.data_ptr(), ti.data_ptr())
            wall = timed(step, hn.sync, args.warmup, args.steps)
            kern = []
            for _ in range(args.steps):
                step()
                hn.sync()
                kern.append(hn.stats()["last_scan_ms"])
            kernel_ms = float(np.median(kern))
            _, evals = hn.hnsw_last_counters()
            got = ti.cpu().numpy()
            hit = sum(len(set(g.tolist()) & set(t.tolist()))
                      for g, t in zip(got, truth[:nq]))
            run = {
                "batch": nq, "ef": ef, "qps": nq / wall,
                "recall_at_10": hit / (10 * nq),
                "dist_evals_q": evals / nq, "kernel_ms": kernel_ms,
                "gather_tbps": evals * 4 * d / (kernel_ms * 1e-3) / 1e12,
                "guide_gather_tbps": GUIDE_GATHER_TBPS,
                "flat_qps": flat_qps, "flat_faster": flat_qps > nq / wall,
            }
            log(json.dumps(run))
            res["runs"].append(run)
    # the mirror is uploaded by the first search: read its size after them
    res["device_bytes"] = hn.stats()["device_bytes"]
    flat.close()
    hn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--dims", type=int, nargs="+", default=[128, 768])
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--efc", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_hnsw needs a GPU"
    out = {"bench": "hnsw", "device": torch.cuda.get_device_name(0),
           "k": 10, "steps": args.steps, "warmup": args.warmup,
           "dims": [run_dim(torch, d, args) for d in args.dims]}
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
