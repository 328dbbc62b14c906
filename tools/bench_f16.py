#!/usr/bin/env python3
"""bench_f16.py — f32 against f16 row storage of IVF-Flat on one MI355X, in
one process.

Generates one data set on the device from a seed (uniform rows, queries =
rows plus N(0, 0.05) noise, the protocol of bench.py), trains the coarse
centroids once, gives an f32 and an f16 IVF-Flat index the same centroids
and adds the same rows to both.  Default is the quick shape

  d 768, n 1M, nlist 1024, nprobe 32, batch 1024, k 10

and `--rows 10000000 --nlist 4096` is cfg C (about 110 GB of device memory
for the two indexes and the finalize staging).

After --warmup untimed steps of each, --rounds rounds of --steps steps
alternate between the two indexes (f32, f16, f32, f16, ...), so drift of
clocks or temperature falls on both alike.  A step is dg_search_device on
device pointers plus one dg_sync.  The f32 index is the yardstick: it runs
the code an index without dg_set_storage always ran.  The JSON reports per
index and round the median and the range of last_scan_ms (hipEvents around
the scan kernel), over all rounds the algorithmic bytes of a step, TB/s and
QPS, the device bytes, and recall@k of the f16 answers against the f32
answers.  "f16_below_f32_every_round" states the acceptance: in every round
the largest f16 scan time is below the smallest f32 scan time.  A third leg,
"f32_nopair", is the f32 index with DG_SCAN_PAIR=0: the pair scan (two query
tiles per pass over lists probed by 17+ queries) is not ported to f16, and
this leg shows how much of a difference is the pairing and how much the
bytes.

  python tools/bench_f16.py --out profiles/bench_f16.json
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


def log(msg):
    print(f"[bench_f16] {msg}", file=sys.stderr, flush=True)


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
    assert torch.cuda.is_available(), "bench_f16 needs a GPU"
    d, n, nq, k = a.d, a.rows, a.batch, a.k
    t_build = time.perf_counter()

    ix = {"f32": dg.Index(dg.IVF_FLAT, dg.L2, d, nlist=a.nlist),
          "f16": dg.Index(dg.IVF_FLAT, dg.L2, d, nlist=a.nlist,
                          storage="f16")}
    n_train = min(n, 256 * a.nlist)
    xt = torch.cat([gen_chunk(torch, a.seed, c, min(GEN_CHUNK,
                                                    n_train - c * GEN_CHUNK),
                              d)
                    for c in range(-(-n_train // GEN_CHUNK))])
    ix["f32"].train(xt.cpu().numpy())
    del xt
    ix["f16"].set_centroids(ix["f32"].get_centroids())
    log(f"trained on {n_train} rows")
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

    def step(idx, pair=True):
        # DG_SCAN_PAIR is read per call: "0" keeps the f32 index off its
        # pair scan, the one scan path the f16 storage does not have
        if pair:
            os.environ.pop("DG_SCAN_PAIR", None)
        else:
            os.environ["DG_SCAN_PAIR"] = "0"
        t0 = time.perf_counter()
        idx.search_device(q.data_ptr(), nq, k, a.nprobe, dist.data_ptr(),
                          ids_t.data_ptr())
        idx.sync()
        ms = (time.perf_counter() - t0) * 1e3
        os.environ.pop("DG_SCAN_PAIR", None)
        return ms, idx.stats()

    # legs: the f32 index as it runs by default (the yardstick), the f16
    # index, and the f32 index without its pair scan (what f16 would be
    # compared with if both scanned one query tile per pass)
    legs = {"f32": (ix["f32"], True), "f16": (ix["f16"], True),
            "f32_nopair": (ix["f32"], False)}
    for name in ix:  # the first search finalizes the index
        step(ix[name])
    build_s = time.perf_counter() - t_build
    log(f"built in {build_s:.1f} s; warm-up")
    for _ in range(a.warmup):
        for idx, pair in legs.values():
            step(idx, pair)
    assert ix["f16"].last_scan_f16() and not ix["f32"].last_scan_f16()
    rounds, last, flags = [], {}, {}
    allscan = {name: [] for name in legs}
    allstep = {name: [] for name in legs}
    for r in range(a.rounds):
        scan = {name: [] for name in legs}
        stepms = {name: [] for name in legs}
        for _ in range(a.steps):
            for name, (idx, pair) in legs.items():
                t, st = step(idx, pair)
                stepms[name].append(t)
                scan[name].append(st["last_scan_ms"])
                last[name] = st
                flags[name] = (idx.last_scan_fused(), idx.last_scan_pair())
        rounds.append({name: summarize(scan[name], stepms[name])
                       for name in legs})
        for name in legs:
            allscan[name] += scan[name]
            allstep[name] += stepms[name]
        log(f"round {r}: " + ", ".join(
            f"{name} scan {rounds[-1][name]['scan_ms_median']:.3f} ms"
            for name in legs))
    res = {}
    for name in legs:
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
    _, got = ix["f16"].search(qh, k, nprobe=a.nprobe)
    out = {
        "tool": "tools/bench_f16.py", "build": dg.build_info(),
        "rows": n, "d": d, "nlist": a.nlist, "nprobe": a.nprobe,
        "batch": nq, "k": k, "rounds": a.rounds, "steps": a.steps,
        "warmup": a.warmup, "build_seconds": build_s,
        "f32": res["f32"], "f16": res["f16"],
        "f32_nopair": res["f32_nopair"], "per_round": rounds,
        f"recall_at_{k}_f16_vs_f32": recall_at_k(got, truth),
        "scan16_over_scan32_median":
            res["f16"]["scan_ms_median"] / res["f32"]["scan_ms_median"],
        "f16_below_f32_every_round": bool(all(
            r["f16"]["scan_ms_max"] < r["f32"]["scan_ms_min"]
            for r in rounds)),
        "f16_below_f32_nopair_every_round": bool(all(
            r["f16"]["scan_ms_max"] < r["f32_nopair"]["scan_ms_min"]
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
