"""Per (kernel, grid, counter) mean counter value out of rocprofv3 --pmc csv directories (pmc_* under argv[1])."""
import csv
import glob
import os
import statistics
import sys

rows = {}
for path in glob.glob(os.path.join(sys.argv[1], "pmc_*", "**", "*counter_collection.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name", "?")
            if not any(k in name for k in ("consistency", "residual", "texture", "export_flows")):
                continue
            grid = r.get("Grid_Size", "") or "x".join(r.get(k, "") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            rows.setdefault((name.split("(")[0], grid, r.get("Counter_Name", "?")), []).append(float(r.get("Counter_Value", "nan")))
for (name, grid, c), v in sorted(rows.items()):
    print(f"{name:20s} grid {grid:>14s}  {c:28s} launches {len(v):3d}  mean {statistics.mean(v):16.1f}")
if not rows:
    print("no counter rows found")
