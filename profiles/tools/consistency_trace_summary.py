"""Per (kernel, grid) launch counts and mean / median durations out of a rocprofv3 --kernel-trace csv directory."""
import csv
import glob
import os
import statistics
import sys

rows = {}
for path in glob.glob(os.path.join(sys.argv[1], "**", "*kernel_trace.csv"), recursive=True):
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            name = r.get("Kernel_Name") or r.get("Name") or "?"
            if not any(k in name for k in ("consistency", "residual", "texture", "export_flows")):
                continue
            grid = tuple(r.get(k, "") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            rows.setdefault((name.split("(")[0], grid), []).append(dur)
for (name, grid), v in sorted(rows.items()):
    print(f"{name:40s} grid {'x'.join(grid):>18s}  launches {len(v):4d}  mean {statistics.mean(v):9.2f} us  median {statistics.median(v):9.2f} us  "
          f"min {min(v):9.2f} us")
if not rows:
    print("no matching kernel rows found under", sys.argv[1])
    sys.exit(1)
