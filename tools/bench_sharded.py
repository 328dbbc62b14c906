#!/usr/bin/env python3
"""bench_sharded.py — the sharded index (dingostore.ShardedIndex) on the
IVF-Flat cfg-C structure, scaled: n x 768 fp32 uniform rows (default 1M, the
--quick size of bench.py), nlist 1024, nprobe 32, batch 1024, k 10.  The rows
are generated once on the host from a seed and added to every index of the
run; k-means runs once and its centroids are installed everywhere, so all
indexes hold the same lists.

Reported (a record, none of it is asserted):
  (a) same-device overhead: S = 2 shards on device 0 against the plain
      dg_search_device of one index holding the same rows; the two alternate
      for --rounds rounds in this process, the JSON carries the median and
      the range of the wall time per batch and their ratio;
  (b) the merge kernel k_merge_lists at (S = 8, nq = 8192, k = 10) and
      (S = 8, nq = 1, k = 2048): device-event time, and that time over the
      slowest shard's scan time of the same search;
  (c) with two or more devices: QPS at S = 1, 2, 4, 8 over distinct devices
      (S capped at the device count) and the efficiency QPS_S / (S QPS_1);
      with one device the JSON says so and claims nothing.
Per S in {1, 2, 4, 8} on device 0 it also lists QPS, each shard's scan ms
and the merge ms.

Time is a host clock around device work that ends in a synchronise.

  python tools/bench_sharded.py --out profiles/bench_sharded.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "dingo-store_amd")]

import dingostore as dg  # noqa: E402


def gen_chunk(seed, c, rows, d):
    return np.random.default_rng(seed * 1_000_003 + c).random(
        (rows, d), dtype=np.float32)


def timed(fn, sync, warmup, iters):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    sync()
    return (time.perf_counter() - t0) / iters


def merge_ms(sh):
    """The merge kernel's time of the last search: dg_sharded_stats adds it
    to the largest last_select_ms of the shards."""
    own = max(sh.shard(i).stats()["last_select_ms"]
              for i in range(sh.n_shards))
    return sh.stats()["last_select_ms"] - own


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=768)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=20240521)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles",
                                                  "bench_sharded.json"))
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available() or dg.device_count() == 0:
        raise SystemExit("bench_sharded.py needs a GPU (no fallback)")
    ndev = dg.device_count()
    n, d, nlist = args.n, args.d, args.nlist
    shard_counts = [1, 2, 4, 8]

    def log(*a):
        print("[bench_sharded]", *a, file=sys.stderr, flush=True)

    # ---- build: one plain index, S shards on device 0, S over devices ----
    t0 = time.time()
    plain = dg.Index(dg.IVF_FLAT, dg.L2, d, nlist=nlist, device=0, reserve=n)
    n_train = min(n, 256 * nlist)
    train = np.concatenate([
        gen_chunk(args.seed, c, min(args.chunk, n_train - c * args.chunk), d)
        for c in range((n_train + args.chunk - 1) // args.chunk)])
    plain.train(train)
    del train
    cents = plain.get_centroids()
    log(f"train {time.time() - t0:.1f}s")
    same = {S: dg.ShardedIndex(dg.IVF_FLAT, dg.L2, d, [0] * S, nlist=nlist,
                               reserve=n) for S in shard_counts}
    multi = {}
    if ndev >= 2:
        for S in shard_counts:
            if 1 < S <= ndev:
                multi[S] = dg.ShardedIndex(dg.IVF_FLAT, dg.L2, d,
                                           list(range(S)), nlist=nlist,
                                           reserve=n)
    for sh in list(same.values()) + list(multi.values()):
        sh.set_centroids(cents)
    t0 = time.time()
    for c in range((n + args.chunk - 1) // args.chunk):
        rows = min(args.chunk, n - c * args.chunk)
        x = gen_chunk(args.seed, c, rows, d)
        ids = np.arange(c * args.chunk, c * args.chunk + rows, dtype=np.int64)
        plain.add(ids, x)
        for sh in list(same.values()) + list(multi.values()):
            sh.add(ids, x)
    log(f"add {n} rows to {1 + len(same) + len(multi)} indexes "
        f"{time.time() - t0:.1f}s")

    dev = torch.device("cuda:0")
    qh = gen_chunk(args.seed, 0, args.batch, d) + \
        0.05 * np.random.default_rng(args.seed + 7).standard_normal(
            (args.batch, d)).astype(np.float32)
    q = torch.from_numpy(qh).to(dev)
    nq, k, nprobe = args.batch, args.k, args.nprobe
    dist_t = torch.empty((nq, k), dtype=torch.float32, device=dev)
    ids_t = torch.empty((nq, k), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def run_plain():
        plain.search_device(q.data_ptr(), nq, k, nprobe, dist_t.data_ptr(),
                            ids_t.data_ptr())

    def run_sharded(sh):
        return lambda: sh.search_device(q.data_ptr(), nq, k, nprobe,
                                        dist_t.data_ptr(), ids_t.data_ptr())

    # the sharded answer is the plain one (same rows, same lists): ids may
    # differ only where distances tie
    run_plain()
    plain.sync()
    pd, pi = dist_t.cpu().numpy().copy(), ids_t.cpu().numpy().copy()
    agree = {}
    for S, sh in same.items():
        run_sharded(sh)()
        sh.sync()
        sd, si = dist_t.cpu().numpy(), ids_t.cpu().numpy()
        agree[S] = {"ids_equal_fraction": float((si == pi).mean()),
                    "max_abs_dist_diff": float(np.abs(sd - pd).max())}

    res = {"workload": "IVF-Flat cfg C structure, scaled", "n": n, "d": d,
           "nlist": nlist, "nprobe": nprobe, "batch": nq, "k": k,
           "iters": args.iters, "warmup": args.warmup, "rounds": args.rounds,
           "devices_visible": ndev, "build_info": dg.build_info(),
           "agreement_with_plain_index": agree}

    # ---- (a) same-device overhead, alternating ----
    t_plain, t_s2 = [], []
    for _ in range(args.rounds):
        t_plain.append(timed(run_plain, plain.sync, args.warmup, args.iters))
        t_s2.append(timed(run_sharded(same[2]), same[2].sync, args.warmup,
                          args.iters))
    mp, ms = float(np.median(t_plain)), float(np.median(t_s2))
    res["a_same_device_overhead"] = {
        "plain_ms_per_batch": {"median": mp * 1e3,
                               "range": [min(t_plain) * 1e3,
                                         max(t_plain) * 1e3]},
        "s2_ms_per_batch": {"median": ms * 1e3,
                            "range": [min(t_s2) * 1e3, max(t_s2) * 1e3]},
        "ratio_s2_over_plain": ms / mp,
        "plain_qps": nq / mp, "s2_qps": nq / ms}
    log("(a)", res["a_same_device_overhead"])

    # ---- per S on device 0 ----
    per_s = []
    for S, sh in same.items():
        t = timed(run_sharded(sh), sh.sync, args.warmup, args.iters)
        per_s.append({
            "S": S, "devices": [0] * S, "qps": nq / t,
            "ms_per_batch": t * 1e3,
            "shard_scan_ms": [sh.shard(i).stats()["last_scan_ms"]
                              for i in range(S)],
            "merge_ms": merge_ms(sh)})
        log(per_s[-1])
    res["same_device"] = per_s

    # ---- (b) merge kernel against the scan of the same search ----
    b_rows = []
    sh8 = same[8]
    for bnq, bk in ((8192, 10), (1, 2048)):
        bq = torch.from_numpy(np.tile(qh, (-(-bnq // nq), 1))[:bnq]).to(dev)
        bd = torch.empty((bnq, bk), dtype=torch.float32, device=dev)
        bi = torch.empty((bnq, bk), dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        mm, scan = [], []
        for it in range(args.warmup + 5):
            sh8.search_device(bq.data_ptr(), bnq, bk, nprobe, bd.data_ptr(),
                              bi.data_ptr())
            sh8.sync()
            if it >= args.warmup:
                mm.append(merge_ms(sh8))
                scan.append(max(sh8.shard(i).stats()["last_scan_ms"]
                                for i in range(8)))
        b_rows.append({"S": 8, "nq": bnq, "k": bk,
                       "merge_ms_median": float(np.median(mm)),
                       "merge_ms_range": [min(mm), max(mm)],
                       "slowest_shard_scan_ms_median": float(np.median(scan)),
                       "merge_over_scan": float(np.median(mm) /
                                                np.median(scan))})
        log("(b)", b_rows[-1])
    res["b_merge_kernel"] = b_rows

    # ---- (c) distinct devices ----
    if not multi:
        res["c_multi_device_scaling"] = (
            f"not measured: {ndev} device visible, the multi-device path "
            "was not run")
    else:
        t1 = timed(run_sharded(same[1]), same[1].sync, args.warmup,
                   args.iters)
        rows = [{"S": 1, "devices": [0], "qps": nq / t1, "efficiency": 1.0}]
        for S, sh in multi.items():
            t = timed(run_sharded(sh), sh.sync, args.warmup, args.iters)
            rows.append({"S": S, "devices": list(range(S)), "qps": nq / t,
                         "efficiency": (nq / t) / (S * nq / t1),
                         "shard_scan_ms": [sh.shard(i).stats()["last_scan_ms"]
                                           for i in range(S)],
                         "merge_ms": merge_ms(sh)})
        res["c_multi_device_scaling"] = rows
    log("(c)", res["c_multi_device_scaling"])

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))
    for sh in list(same.values()) + list(multi.values()):
        sh.close()
    plain.close()


if __name__ == "__main__":
    main()
