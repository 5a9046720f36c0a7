"""FETCH_SIZE per launch of the attention kernels in a `rocprofv3 --kernel-trace --pmc FETCH_SIZE` pass over
`tools/gqa_bench.py --only decode_b64_c4096`, grouped by kernel and grid (the MHA op on the 8-head and on the replicated 32-head cache
run the same kernel on different grids):  python tools/summarize_gqa_fetch.py RAW_DIR > out.txt
gfx950 counts half the bytes of wide streaming reads in FETCH_SIZE (measuring-on-mi355x): compare the ops as ratios."""
import collections
import csv
import glob
import os
import sys


def main(raw):
    acc = collections.defaultdict(list)
    for f in glob.glob(os.path.join(raw, "**", "*counter_collection.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if r["Counter_Name"] != "FETCH_SIZE" or not any(k in r["Kernel_Name"] for k in ("prefill", "decode")):
                continue
            grid = r.get("Grid_Size") or r.get("Grid_Size_X") or "?"
            acc[(r["Kernel_Name"][:90], grid)].append(float(r["Counter_Value"]))
    print(f"{'kernel':92s} {'grid':>9s} {'launches':>8s} {'FETCH_SIZE KiB/launch':>22s}")
    for (name, grid), v in sorted(acc.items(), key=lambda kv: -sum(kv[1]) / len(kv[1])):
        print(f"{name:92s} {grid:>9s} {len(v):8d} {sum(v) / len(v):22.0f}")


if __name__ == "__main__":
    main(sys.argv[1])
