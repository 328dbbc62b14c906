#!/usr/bin/env python3
"""Sum the counters of `rocprofv3 --pmc ... -f csv` runs per kernel.

  python tools/pmc_csv_sum.py OUT.json DIR [DIR ...] [--only SUBSTRING ...]

Every *counter_collection.csv under the directories is read; the result
maps kernel name (template arguments kept, argument list cut) to
{"dispatches": n, COUNTER: sum over the dispatches, ...}.  --only keeps
the kernels whose name contains one of the substrings.
"""
import csv
import glob
import json
import os
import sys


def main():
    args = sys.argv[1:]
    only = []
    if "--only" in args:
        i = args.index("--only")
        only, args = args[i + 1:], args[:i]
    out_path, dirs = args[0], args[1:]
    res = {}
    for d in dirs:
        for path in glob.glob(os.path.join(d, "**", "*counter_collection.csv"),
                              recursive=True):
            seen = {}
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row["Kernel_Name"].split("(")[0]
                    if only and not any(s in name for s in only):
                        continue
                    k = res.setdefault(name, {"dispatches": 0})
                    cn = row["Counter_Name"]
                    k[cn] = k.get(cn, 0.0) + float(row["Counter_Value"])
                    seen.setdefault((name, cn), set()).add(row["Dispatch_Id"])
            for (name, cn), ids in seen.items():
                res[name]["dispatches"] = max(res[name]["dispatches"],
                                              len(ids))
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path, len(res), "kernels")


if __name__ == "__main__":
    main()
