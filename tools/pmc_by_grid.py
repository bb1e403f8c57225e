"""Per (kernel, grid size) mean of every counter of rocprofv3 --pmc passes (usage: pmc_by_grid.py DIR
[FILTER_REGEX] -> one line per group). pmc_summary.py averages over a kernel name; two products that run
the same GEMM instance (dW_ih of layer 1 and a plain dW_hh) differ only in their grid, so they are told
apart here. FETCH_SIZE is in KB and counts half the bytes of wide coalesced reads (pmc_summary.py)."""
import csv
import glob
import os
import re
import sys
from collections import defaultdict




def main(d, pat):
    acc = defaultdict(lambda: defaultdict(list))
    for f in glob.glob(os.path.join(d, "p*", "*counter_collection.csv")):
        for r in csv.DictReader(open(f)):
            k = short(r["Kernel_Name"])
            if re.search(pat, k):
                acc[(k, r.get("Grid_Size", "?"))][r["Counter_Name"]].append(float(r["Counter_Value"]))
    for (k, grid), cs in sorted(acc.items()):
        m = {c: sum(v) / len(v) for c, v in cs.items()}
        n = max(len(v) for v in cs.values())
        line = f"{k} grid {grid} dispatches {n}"
        if "FETCH_SIZE" in m:
            line += f" fetch_GB {2 * m['FETCH_SIZE'] * 1024 / 1e9:.3f}"
        if "TCC_HIT_sum" in m and "TCC_MISS_sum" in m:
            line += f" l2_hit {m['TCC_HIT_sum'] / max(1.0, m['TCC_HIT_sum'] + m['TCC_MISS_sum']):.3f}"
        print(line)


sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pmc_summary import short  # noqa: E402

if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ".")
