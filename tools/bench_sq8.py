#!/usr/bin/env python3
"""bench_sq8.py — f32, f16 and SQ8 row storage of IVF-Flat on one MI355X, in
one process (the protocol of bench_f16.py).

Generates one data set on the device from a seed (uniform rows, queries =
rows plus N(0, 0.05) noise, the protocol of bench.py), trains the coarse
centroids once, gives an f32, an f16 and an SQ8 IVF-Flat index the same
centroids and adds the same rows to all three.  The SQ8 ranges are trained
from the rows: the per-dimension min and max - min over all of them (what
dg_train computes from its training rows).  Default is the quick shape

  d 768, n 1M, nlist 1024, nprobe 32, batch 1024, k 10

and `--rows 10000000 --nlist 4096` is cfg C (about 160 GB of device memory
for the three indexes and the finalize staging).

After --warmup untimed steps of each, --rounds rounds of --steps steps
alternate between the indexes (f32, f16, sq8, f32, ...), so drift of clocks
or temperature falls on all alike.  A step is dg_search_device on device
pointers plus one dg_sync.  The f32 and the f16 index are the yardsticks:
they run code that SQ8 storage does not touch.  The JSON reports per index
and round the median and the range of last_scan_ms (hipEvents around the
scan; for SQ8 that includes the per-batch query fold), over all rounds the
algorithmic bytes of a step, TB/s and QPS, the device bytes, and recall@k of
the f16 and the SQ8 answers against the f32 answers (recorded, no threshold:
uniform data is the worst case for a scalar quantiser).
"sq8_below_f16_every_round" states the expectation: in every round the
largest SQ8 scan time is below the smallest f16 scan time.

  python tools/bench_sq8.py --out profiles/bench_sq8_quick.json
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

GEN_CHUNK = 1 << 18
LEGS = ("f32", "f16", "sq8")


def log(msg):
    print(f"[bench_sq8] {msg}", file=sys.stderr, flush=True)


def gen_chunk(torch, seed, c, rows, d):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed * 1000003 + c)
    return torch.rand((rows, d), generator=g, device="cuda",
                      dtype=torch.float32)


def summarize(scan, step):
    scan, step = np.array(scan), np.array(step)
    return {
        "scan_ms_median": float(np.median(scan)),
        "scan_ms_min": float(scan.min()), "scan_ms_max": float(scan.max()),
        "step_ms_median": float(np.median(step)),
    }


def recall_at_k(got, truth):
    hit = 0
    for g, t in zip(got, truth):
        hit += len(set(g.tolist()) & set(t.tolist()))
    return hit / truth.size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.rounds < 3:
        ap.error("--rounds must be at least 3")
    import torch
    assert torch.cuda.is_available(), "bench_sq8 needs a GPU"
    d, n, nq, k = a.d, a.rows, a.batch, a.k
    t_build = time.perf_counter()

    ix = {name: dg.Index(dg.IVF_FLAT, dg.L2, d, nlist=a.nlist, storage=name)
          for name in LEGS}
    n_train = min(n, 256 * a.nlist)
    xt = torch.cat([gen_chunk(torch, a.seed, c, min(GEN_CHUNK,
                                                    n_train - c * GEN_CHUNK),
                              d)
                    for c in range(-(-n_train // GEN_CHUNK))])
    ix["f32"].train(xt.cpu().numpy())
    del xt
    cents = ix["f32"].get_centroids()
    ix["f16"].set_centroids(cents)
    ix["sq8"].set_centroids(cents)
    log(f"trained on {n_train} rows")
    # the SQ8 ranges over all rows: f32 min and max - min per dimension
    lo = hi = None
    for c in range(-(-n // GEN_CHUNK)):
        x = gen_chunk(torch, a.seed, c, min(GEN_CHUNK, n - c * GEN_CHUNK), d)
        cl, ch = x.min(0).values, x.max(0).values
        lo = cl if lo is None else torch.minimum(lo, cl)
        hi = ch if hi is None else torch.maximum(hi, ch)
        del x
    ix["sq8"].set_sq_ranges(lo.cpu().numpy(), (hi - lo).cpu().numpy())
    for c in range(-(-n // GEN_CHUNK)):
        rows = min(GEN_CHUNK, n - c * GEN_CHUNK)
        x = gen_chunk(torch, a.seed, c, rows, d)
        torch.cuda.synchronize()
        ids = np.arange(c * GEN_CHUNK, c * GEN_CHUNK + rows, dtype=np.int64)
        for idx in ix.values():
            idx.add_device(ids, x.data_ptr(), rows)
        del x
    q = gen_chunk(torch, a.seed, 0, nq, d)
    g = torch.Generator(device="cuda")
    g.manual_seed(a.seed + 7)
    q = (q + 0.05 * torch.randn((nq, d), generator=g, device="cuda"))
    q = q.contiguous()
    dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ids_t = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def step(idx):
        t0 = time.perf_counter()
        idx.search_device(q.data_ptr(), nq, k, a.nprobe, dist.data_ptr(),
                          ids_t.data_ptr())
        idx.sync()
        return (time.perf_counter() - t0) * 1e3, idx.stats()

    for name in LEGS:  # the first search finalizes the index
        step(ix[name])
    build_s = time.perf_counter() - t_build
    log(f"built in {build_s:.1f} s; warm-up")
    for _ in range(a.warmup):
        for name in LEGS:
            step(ix[name])
    assert ix["sq8"].last_scan_sq8() and not ix["sq8"].last_scan_f16()
    assert ix["f16"].last_scan_f16() and not ix["f16"].last_scan_sq8()
    assert not ix["f32"].last_scan_f16() and not ix["f32"].last_scan_sq8()
    rounds, last, flags = [], {}, {}
    allscan = {name: [] for name in LEGS}
    allstep = {name: [] for name in LEGS}
    for r in range(a.rounds):
        scan = {name: [] for name in LEGS}
        stepms = {name: [] for name in LEGS}
        for _ in range(a.steps):
            for name in LEGS:
                t, st = step(ix[name])
                stepms[name].append(t)
                scan[name].append(st["last_scan_ms"])
                last[name] = st
                flags[name] = (ix[name].last_scan_fused(),
                               ix[name].last_scan_pair())
        rounds.append({name: summarize(scan[name], stepms[name])
                       for name in LEGS})
        for name in LEGS:
            allscan[name] += scan[name]
            allstep[name] += stepms[name]
        log(f"round {r}: " + ", ".join(
            f"{name} scan {rounds[-1][name]['scan_ms_median']:.3f} ms"
            for name in LEGS))
    res = {}
    for name in LEGS:
        s = summarize(allscan[name], allstep[name])
        b = last[name]["last_scan_bytes_algorithmic"]
        s.update({
            "scan_bytes_algorithmic": b,
            "scan_tbps_algorithmic_median": b / s["scan_ms_median"] / 1e9,
            "qps_median": nq / s["step_ms_median"] * 1e3,
            "device_bytes": last[name]["device_bytes"],
            "scan_fused": flags[name][0],
            "scan_pair": flags[name][1],
        })
        res[name] = s

    log("recall")
    qh = q.cpu().numpy()
    _, truth = ix["f32"].search(qh, k, nprobe=a.nprobe)
    _, got16 = ix["f16"].search(qh, k, nprobe=a.nprobe)
    _, got8 = ix["sq8"].search(qh, k, nprobe=a.nprobe)
    out = {
        "tool": "tools/bench_sq8.py", "build": dg.build_info(),
        "rows": n, "d": d, "nlist": a.nlist, "nprobe": a.nprobe,
        "batch": nq, "k": k, "rounds": a.rounds, "steps": a.steps,
        "warmup": a.warmup, "build_seconds": build_s,
        "f32": res["f32"], "f16": res["f16"], "sq8": res["sq8"],
        "per_round": rounds,
        f"recall_at_{k}_f16_vs_f32": recall_at_k(got16, truth),
        f"recall_at_{k}_sq8_vs_f32": recall_at_k(got8, truth),
        "scan8_over_scan32_median":
            res["sq8"]["scan_ms_median"] / res["f32"]["scan_ms_median"],
        "scan8_over_scan16_median":
            res["sq8"]["scan_ms_median"] / res["f16"]["scan_ms_median"],
        "sq8_below_f16_every_round": bool(all(
            r["sq8"]["scan_ms_max"] < r["f16"]["scan_ms_min"]
            for r in rounds)),
        "sq8_below_f32_every_round": bool(all(
            r["sq8"]["scan_ms_max"] < r["f32"]["scan_ms_min"]
            for r in rounds)),
    }
    print(json.dumps(out), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for i in ix.values():
        i.close()


if __name__ == "__main__":
    main()
