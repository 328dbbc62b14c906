#!/usr/bin/env python3
"""bench_binary.py — timing of the binary (Hamming) indexes on one MI355X.

Times dg_search_binary_device on a resident index (device pointers in and
out, one dg_sync per step) for

  flat      binary Flat, 1M x 768 bits, batch 256, k 10
  ivf       binary IVF-Flat, 10M x 768 bits, nlist 4096, nprobe 32,
            batch 1024, k 10
  baseline  what a user had before the binary kinds: the same 1M rows
            unpacked to 0/1 float32 in a float FLAT / IP index, batch 256,
            k 10 (32x the bytes, popcount through an f32 GEMM)

Data is generated on the device from a seed.  Each shape runs --warmup
untimed steps and then --steps timed ones; the JSON line reports the
median and the range of the step time, the scan time dg_stats records for
one step, and the achieved (query, row) pairs/s against the VALU bound of
2 * ceil(d/32) lane-ops per pair at 256 CUs x 64 lane-ops/cycle x the
clock given with --clock-mhz.

  python tools/bench_binary.py --shapes flat,ivf,baseline --out result.json

--range R replaces the shapes with one measurement of binary Flat range
search (1M x 768 bits, batch 256, radius R; uniform random rows give about
10 hits per query at R = 326): per step the wall time of
dg_range_search_binary, the device time of the two k_hamming_range passes
together (hipEvents on the index stream, from dg_stats) and their
difference, the host-side remainder (two synchronizes, copies, sort).  The
same index then runs the top-k search of the flat shape, so the scan time
with the distance-matrix round trip stands beside it.

  python tools/bench_binary.py --range 326 --out range.json
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

CUS, LANE_OPS_PER_CU_CYCLE = 256, 64


def gen_bits(torch, n, nbytes, seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randint(0, 256, (n, nbytes), dtype=torch.uint8,
                         device="cuda", generator=g)


def time_steps(torch, idx, q, k, nprobe, steps, warmup):
    nq = q.shape[0]
    dist = torch.empty((nq, k), dtype=torch.float32, device="cuda")
    ids = torch.empty((nq, k), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def step():
        idx.search_device(q.data_ptr(), nq, k, nprobe, dist.data_ptr(),
                          ids.data_ptr())
        idx.sync()

    for _ in range(warmup):
        step()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        ms.append((time.perf_counter() - t0) * 1e3)
    st = idx.stats()
    return np.array(ms), st, dist, ids


def summarize(name, ms, st, nq, pairs, d_bits, clock_mhz, extra):
    med = float(np.median(ms))
    out = {
        "shape": name, "batch": nq, "steps": len(ms),
        "step_ms_median": med, "step_ms_min": float(ms.min()),
        "step_ms_max": float(ms.max()), "qps_median": nq / med * 1e3,
        "scan_ms_stats": st["last_scan_ms"],
        "coarse_ms_stats": st["last_coarse_ms"],
        "select_ms_stats": st["last_select_ms"],
        "scan_bytes_algorithmic": st["last_scan_bytes_algorithmic"],
        "device_bytes": st["device_bytes"],
    }
    if pairs:
        words = (d_bits + 31) // 32
        bound = CUS * LANE_OPS_PER_CU_CYCLE * clock_mhz * 1e6 / (2 * words)
        out["pairs"] = pairs
        out["pairs_per_s_step"] = pairs / (med * 1e-3)
        if st["last_scan_ms"] > 0:
            out["pairs_per_s_scan"] = pairs / (st["last_scan_ms"] * 1e-3)
            out["scan_frac_of_valu_bound"] = out["pairs_per_s_scan"] / bound
        out["valu_bound_pairs_per_s"] = bound
        out["clock_mhz"] = clock_mhz
    out.update(extra)
    return out


def run_flat(torch, a):
    d, n, nq, k = 768, a.flat_rows, 256, 10
    base = gen_bits(torch, n, d // 8, a.seed)
    q = gen_bits(torch, nq, d // 8, a.seed + 1)
    idx = dg.Index(dg.BINARY_FLAT, dg.HAMMING, d)
    idx.add(np.arange(n, dtype=np.int64), base.cpu().numpy())
    ms, st, dist, _ = time_steps(torch, idx, q, k, 0, a.steps, a.warmup)
    out = summarize("binary_flat", ms, st, nq, nq * n, d, a.clock_mhz,
                    {"rows": n, "d_bits": d, "k": k,
                     "dist_checksum": float(dist.double().sum())})
    idx.close()
    return out


def run_range(torch, a):
    d, n, nq, k = 768, a.flat_rows, 256, 10
    base = gen_bits(torch, n, d // 8, a.seed)
    q = gen_bits(torch, nq, d // 8, a.seed + 1)
    idx = dg.Index(dg.BINARY_FLAT, dg.HAMMING, d)
    idx.add(np.arange(n, dtype=np.int64), base.cpu().numpy())
    qh = q.cpu().numpy()
    wall, dev = [], []
    for i in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        lims, dist, _ = idx.range_search_binary(qh, a.range)
        ms = (time.perf_counter() - t0) * 1e3
        if i >= a.warmup:
            wall.append(ms)
            dev.append(idx.stats()["last_scan_ms"])
    wall, dev = np.array(wall), np.array(dev)
    rest = wall - dev
    # the same resident index through the top-k path (dists matrix + select)
    ms, st, tk_dist, _ = time_steps(torch, idx, q, k, 0, a.steps, a.warmup)
    out = {
        "shape": "binary_flat_range", "batch": nq, "rows": n, "d_bits": d,
        "radius": a.range, "steps": a.steps, "warmup": a.warmup,
        "hits_total": int(lims[-1]), "hits_per_query": float(lims[-1]) / nq,
        "dist_checksum": float(dist.astype(np.float64).sum()),
        "range_call_ms_median": float(np.median(wall)),
        "range_call_ms_min": float(wall.min()),
        "range_call_ms_max": float(wall.max()),
        "range_kernels_ms_median": float(np.median(dev)),
        "range_kernels_ms_min": float(dev.min()),
        "range_kernels_ms_max": float(dev.max()),
        "range_host_rest_ms_median": float(np.median(rest)),
        "range_host_rest_ms_min": float(rest.min()),
        "range_host_rest_ms_max": float(rest.max()),
        "topk_k": k,
        "topk_step_ms_median": float(np.median(ms)),
        "topk_step_ms_min": float(ms.min()),
        "topk_step_ms_max": float(ms.max()),
        "topk_scan_ms_stats": st["last_scan_ms"],
        "topk_dist_checksum": float(tk_dist.double().sum()),
    }
    idx.close()
    return out


def run_baseline(torch, a):
    d, n, nq, k = 768, a.flat_rows, 256, 10
    base = gen_bits(torch, n, d // 8, a.seed)
    q = gen_bits(torch, nq, d // 8, a.seed + 1)
    shifts = torch.arange(8, device="cuda", dtype=torch.uint8)

    def unpack(x):
        return ((x[:, :, None] >> shifts) & 1).reshape(x.shape[0], -1).float()

    idx = dg.Index(dg.FLAT, dg.IP, d)
    ids = np.arange(n, dtype=np.int64)
    step = 1 << 18
    for s in range(0, n, step):
        xf = unpack(base[s:s + step]).contiguous()
        torch.cuda.synchronize()
        idx.add_device(ids[s:s + step], xf.data_ptr(), xf.shape[0])
    qf = unpack(q).contiguous()
    ms, st, _, _ = time_steps(torch, idx, qf, k, 0, a.steps, a.warmup)
    out = summarize("float_flat_ip_unpacked", ms, st, nq, 0, d, a.clock_mhz,
                    {"rows": n, "d_bits": d, "k": k})
    idx.close()
    return out


def run_ivf(torch, a):
    d, n, nq, k, nlist, nprobe = 768, a.ivf_rows, 1024, 10, 4096, 32
    cents = gen_bits(torch, nlist, d // 8, a.seed + 2)
    idx = dg.Index(dg.BINARY_IVF_FLAT, dg.HAMMING, d, nlist=nlist)
    idx.set_centroids(cents.cpu().numpy())
    step = 1 << 20
    for s in range(0, n, step):
        c = min(step, n - s)
        x = gen_bits(torch, c, d // 8, a.seed + 10 + s // step)
        idx.add(np.arange(s, s + c, dtype=np.int64), x.cpu().numpy())
    q = gen_bits(torch, nq, d // 8, a.seed + 1)
    ms, st, dist, _ = time_steps(torch, idx, q, k, nprobe, a.steps, a.warmup)
    # every probing query meets every row of its lists: pairs = sum over
    # lists of (queries probing it x its length); uniform random data makes
    # that nq * nprobe * n / nlist to within sampling noise
    pairs = int(nq * nprobe * (n / nlist))
    out = summarize("binary_ivf_flat", ms, st, nq, pairs, d, a.clock_mhz,
                    {"rows": n, "d_bits": d, "k": k, "nlist": nlist,
                     "nprobe": nprobe, "pairs_is_estimate": True,
                     "dist_checksum": float(dist.double().sum())})
    idx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="flat,ivf,baseline")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--flat-rows", type=int, default=1_000_000)
    ap.add_argument("--ivf-rows", type=int, default=10_000_000)
    ap.add_argument("--clock-mhz", type=float, default=0.0,
                    help="engine clock for the VALU bound; 0 = read it "
                         "after each shape's timed steps, 2400 if it "
                         "cannot be read")
    ap.add_argument("--range", type=int, default=0, metavar="R",
                    help="measure binary Flat range search at radius R "
                         "instead of the --shapes")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.steps < 20:
        ap.error("--steps must be at least 20")
    import torch
    assert torch.cuda.is_available(), "bench_binary needs a GPU"
    runners = {"flat": run_flat, "ivf": run_ivf, "baseline": run_baseline}
    results = []
    fixed_clock = a.clock_mhz
    if a.range > 0:
        results.append(run_range(torch, a))
        print(json.dumps(results[0]), flush=True)
        a.shapes = ""
    for name in filter(None, a.shapes.split(",")):
        a.clock_mhz, a.clock_source = fixed_clock, "argument"
        if not fixed_clock:
            # read right after a warm run of the same shape would be ideal;
            # the driver reports the current engine clock, so sample it
            # under load: a short burst of the GEMM keeps the device busy
            x = torch.randn(4096, 4096, device="cuda")
            for _ in range(20):
                x @ x
            try:
                a.clock_mhz = float(torch.cuda.clock_rate())
                a.clock_source = "torch.cuda.clock_rate under load"
            except Exception:
                a.clock_mhz, a.clock_source = 2400.0, "assumed peak"
            torch.cuda.synchronize()
        r = runners[name](torch, a)
        r["clock_source"] = a.clock_source
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/bench_binary.py",
                       "build": dg.build_info(), "results": results}, f,
                      indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
