#!/usr/bin/env python3
"""bench_concurrent.py — the reference search pool's call shape on one MI355X:
T threads, each issuing searches of ONE query from host memory
(src/vector/vector_index.cc:53-54,244-271), against one IVF-Flat index.

Index: bench.py's --quick shape (1M x 768 fp32, nlist 1024, nprobe 32, k 10),
built by bench.build_index.  Queries are resident host rows.

Modes
  direct      dg_search, nq = 1 per call
  batched_w0  dg_search_batched, max_wait_us 0
  batched_w100  dg_search_batched, max_wait_us 100
for T in --threads (default 1,4,16,64).  The modes alternate --rounds times
(default 3) in one process; the JSON gives the median and the range over the
rounds of: QPS, p50 and p99 call latency, mean and largest flush.

Two drivers.  "python": threading.Thread workers calling through ctypes,
which releases the GIL during the call but holds it between calls, so its
figure includes the interpreter's hand-over between T threads.  "native":
dg_bench_threads, the same loop on T std::threads inside the library (wall
time only), which shows what a C++ host program gets.

Conditions recorded in the JSON (none is asserted, the figures decide):
  (a) T = 1: batched_w0 is not slower than direct beyond the range of the
      direct rounds
  (b) T = 16: batched QPS exceeds direct QPS by more than that range

  python tools/bench_concurrent.py --out profiles/bench_batched.json
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd")]

import dingostore as dg  # noqa: E402

MODES = [("direct", None), ("batched_w0", 0), ("batched_w100", 100)]


def run_python(idx, q, k, nprobe, threads, calls, batched):
    """threads x calls one-query searches; returns (wall s, latencies ms)."""
    lat = np.zeros((threads, calls))
    barrier = threading.Barrier(threads + 1)
    fn = idx.search_batched if batched else idx.search
    nq = len(q)

    def work(t):
        rows = [q[(t * calls + c) % nq][None] for c in range(calls)]
        for c in range(2):  # untimed: this thread's staging in dg_search
            fn(rows[c], k, nprobe=nprobe)
        barrier.wait()
        for c in range(calls):
            t0 = time.perf_counter()
            fn(rows[c], k, nprobe=nprobe)
            lat[t, c] = time.perf_counter() - t0

    th = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    for t in th:
        t.start()
    barrier.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    return time.perf_counter() - t0, lat.reshape(-1) * 1e3


def run_native(idx, q, k, nprobe, threads, calls, batched):
    sec = dg.lib().dg_bench_threads(idx.h, threads, calls, 1 if batched else 0,
                                    q, len(q), k, nprobe)
    if sec < 0:
        raise RuntimeError(f"dg_bench_threads failed ({sec})")
    return sec


def med_range(vals):
    v = np.asarray(vals, float)
    return {"median": float(np.median(v)), "min": float(v.min()),
            "max": float(v.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=4244)
    ap.add_argument("--threads", default="1,4,16,64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=1536,
                    help="calls per measurement, split over the threads")
    ap.add_argument("--max-batch", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import bench
    assert torch.cuda.is_available(), "needs a GPU"
    device = torch.device("cuda:0")
    torch.cuda.set_device(0)
    a.kind, a.m = "ivf_flat", 96
    idx, _ = bench.build_index(a, 0, 1, device)
    q = bench.gen_queries_device(a.seed, a.n, a.d, 256, device).cpu().numpy()
    q = np.ascontiguousarray(q, np.float32)
    k, nprobe = a.k, a.nprobe
    t_list = [int(t) for t in a.threads.split(",")]

    # warm-up: finalize, capture the nq = 1 graph, size every workspace a
    # flush of up to max_batch queries needs, all before any thread starts
    for _ in range(20):
        idx.search(q[:1], k, nprobe=nprobe)
    idx.enable_batching(a.max_batch, 0)
    for nq in (1, 2, 3, 4, 8, 16, 32, 63):
        idx.search(q[:nq], k, nprobe=nprobe)
    run_python(idx, q, k, nprobe, 16, 8, True)
    idx.disable_batching()
    for _ in range(20):
        idx.search(q[:1], k, nprobe=nprobe)

    rows = {}  # (driver, mode, T) -> list of per-round dicts
    for rnd in range(a.rounds):
        for mode, wait in MODES:
            if wait is not None:
                idx.enable_batching(a.max_batch, wait)
            for T in t_list:
                calls = max(a.calls // T, 16)
                for driver in ("python", "native"):
                    if wait is not None:
                        idx.enable_batching(a.max_batch, wait)  # zero stats
                    if driver == "python":
                        sec, lat = run_python(idx, q, k, nprobe, T, calls,
                                              wait is not None)
                    else:
                        sec = run_native(idx, q, k, nprobe, T, calls,
                                         wait is not None)
                        lat = None
                    r = {"qps": T * calls / sec, "calls": T * calls}
                    if lat is not None:
                        r["p50_ms"] = float(np.percentile(lat, 50))
                        r["p99_ms"] = float(np.percentile(lat, 99))
                    if wait is not None:
                        st = idx.batching_stats()
                        r["flush_mean"] = st["queries"] / max(st["flushes"], 1)
                        r["flush_max"] = st["max_flush_queries"]
                    rows.setdefault((driver, mode, T), []).append(r)
                    print(rnd, driver, mode, T, json.dumps(r), flush=True)
            if wait is not None:
                idx.disable_batching()

    results = []
    for (driver, mode, T), rs in sorted(rows.items()):
        e = {"driver": driver, "mode": mode, "threads": T,
             "calls": rs[0]["calls"], "rounds": len(rs),
             "qps": med_range([r["qps"] for r in rs])}
        for key in ("p50_ms", "p99_ms", "flush_mean", "flush_max"):
            if key in rs[0]:
                e[key] = med_range([r[key] for r in rs])
        results.append(e)

    def qps(driver, mode, T):
        return next(e["qps"] for e in results if e["driver"] == driver and
                    e["mode"] == mode and e["threads"] == T)

    cond = {}
    for driver in ("python", "native"):
        if 1 in t_list:
            d1, b1 = qps(driver, "direct", 1), qps(driver, "batched_w0", 1)
            cond[f"a_{driver}"] = {
                "direct_qps": d1, "batched_w0_qps": b1,
                "direct_range": d1["max"] - d1["min"],
                "holds": b1["median"] >= d1["median"] - (d1["max"] - d1["min"]),
            }
        if 16 in t_list:
            d16 = qps(driver, "direct", 16)
            for mode in ("batched_w0", "batched_w100"):
                b16 = qps(driver, mode, 16)
                cond[f"b_{driver}_{mode}"] = {
                    "direct_qps": d16, "batched_qps": b16,
                    "factor": b16["median"] / d16["median"],
                    "holds": b16["median"] - d16["median"] >
                    d16["max"] - d16["min"],
                }
    out = {
        "tool": "tools/bench_concurrent.py",
        "workload": f"IVF-Flat {a.n} x {a.d} fp32 nlist={a.nlist} "
                    f"nprobe={nprobe} k={k}, nq=1 per call from host memory",
        "protocol": f"modes alternate {a.rounds} times in one process; "
                    "median and range over the rounds",
        "max_batch": a.max_batch or 64,
        "results": results, "conditions": cond,
    }
    print(json.dumps(out), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    idx.close()


if __name__ == "__main__":
    main()
