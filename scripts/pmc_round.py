#!/usr/bin/env python3
"""SQ counters of the round kernel per wave and round over bench.py's timed
region, from `rocprofv3 --pmc ... --output-format csv` runs of bench.py (no
tracing in the same run, so no marker: the timed region's dispatches are the
kernel's last `timed_batches`, the bench line's count -- nothing launches the
kernel after the region in a run with --no-cpu-baseline --lossy-edge-loss-max 0).

    python3 scripts/pmc_round.py <bench JSON line file> <pmc dir> [<pmc dir> ...] [--kernel k_round_ps]

Each counter is summed over those dispatches and divided by waves x rounds
(SQ_WAVES per dispatch x the line's `rounds`).
"""
import argparse
import csv
import glob
import json
import os
from collections import defaultdict


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("bench_json")
    ap.add_argument("dirs", nargs="+")
    ap.add_argument("--kernel", default=None)
    a = ap.parse_args()
    lines = [l for l in open(a.bench_json).read().splitlines() if l.strip().startswith("{")]
    bench = json.loads(lines[-1])
    kernel = a.kernel or bench["roofline"]["kernel"]
    nb, rounds = int(bench["timed_batches"]), int(bench["rounds"])
    tot, waves = defaultdict(float), None
    for d in a.dirs:
        per = defaultdict(dict)   # dispatch id -> counter -> value
        for f in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
            with open(f) as fh:
                for row in csv.DictReader(fh):
                    if kernel in row["Kernel_Name"]:
                        c = per[int(row["Dispatch_Id"])]
                        c[row["Counter_Name"]] = c.get(row["Counter_Name"], 0.0) + float(row["Counter_Value"])
        ids = sorted(per)[-nb:]
        if len(ids) < nb:
            raise SystemExit(f"{d}: {len(ids)} dispatches of {kernel}, the bench line has {nb} timed batches")
        for i in ids:
            for k, v in per[i].items():
                tot[k] += v
        if "SQ_WAVES" in per[ids[0]]:
            waves = per[ids[0]]["SQ_WAVES"]
            tot.pop("SQ_WAVES", None)
    if not waves:
        raise SystemExit("no SQ_WAVES among the counters")
    print(f"{kernel}: {nb} dispatches of the timed region, {rounds} rounds, {waves:.0f} waves a dispatch; "
          f"bench {bench['roofline']['avg_in_kernel_us']} us in kernel per round under the counters")
    print("per wave and round:")
    for k in sorted(tot):
        print(f"  {k:22s} {tot[k] / (waves * rounds):10.1f}")
    kinds = ("SQ_INSTS_VALU", "SQ_INSTS_SALU", "SQ_INSTS_SMEM", "SQ_INSTS_VMEM_RD", "SQ_INSTS_VMEM_WR", "SQ_INSTS_LDS",
             "SQ_INSTS_BRANCH")
    insts = sum(tot.get(k, 0.0) for k in kinds)
    print(f"  instructions (of the counted kinds) {insts / (waves * rounds):.1f}")


if __name__ == "__main__":
    main()
