"""Per-case counter table of `rocprofv3 --pmc ... -- tools/ubench/slide_bench pmc`.
usage: slide_pmc_table.py DIR   (every DIR/**/*counter_collection.csv)

One row per slide_kern instantiation (the template arguments name the case:
TSH, G, waves, chains, rare path), counters per tested wave-byte.  A case is
launched once in pmc mode, with the same reps and segment as the timed runs.
"""
import collections
import csv
import glob
import re
import sys

REPS, S = 8, 1536  # slide_bench.hip: reps, kS
NAMES = {(105, 116, 16, 1, 1): "V0", (105, 116, 16, 1, 0): "V0r0", (105, 216, 16, 1, 1): "T1",
         (205, 116, 16, 1, 1): "A", (205, 16, 16, 1, 1): "A16",
         (105, 16, 16, 1, 1): "V16", (205, 1016, 16, 1, 1): "A16m", (105, 1016, 16, 1, 1): "V16m", (105, 116, 12, 1, 1): "W12",
         (105, 116, 12, 2, 1): "W12x2", (205, 116, 12, 2, 1): "A12x2"}

agg = collections.defaultdict(lambda: collections.defaultdict(float))
grid = {}
for f in sorted(glob.glob(f"{sys.argv[1]}/**/*counter_collection.csv", recursive=True)):
    for r in csv.DictReader(open(f)):
        m = re.search(r"slide_kern<(-?\d+), (\d+), (\d+), (\d+), (true|false|[01])>", r["Kernel_Name"])
        if not m:
            continue
        key = (int(m[1]), int(m[2]), int(m[3]), int(m[4]), int(m[5] in ("true", "1")))
        agg[key][r["Counter_Name"]] += float(r["Counter_Value"])
        grid[key] = int(r["Grid_Size"]) // 64  # waves launched

cols = ["SQ_INSTS_VALU", "SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE",
        "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_VALU"]
print("per tested wave-byte (counter / (waves x reps x S)); cycles are per wave\n")
print(f"{'case':6s} " + " ".join(f"{c[3:]:>18s}" for c in cols))
for key, name in NAMES.items():
    if key not in agg:
        continue
    wb = grid[key] * REPS * S
    print(f"{name:6s} " + " ".join(f"{agg[key].get(c, float('nan')) / wb:18.3f}" for c in cols))
