"""Per (kernel, grid) launch counts and mean / median / min durations out of a rocprofv3 --kernel-trace csv directory:
trace_summary.py DIR NAME_FRAGMENT...  (kernels whose name contains one of the fragments).  SPLIT=k in the environment cuts
the launches of every (kernel, grid), in time order, into k equal consecutive parts -- a tool that visits k shapes one after
the other with a grid that does not depend on the shape (k_track: one workgroup per track)."""
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
            if not any(k in name for k in sys.argv[2:]):
                continue
            grid = tuple(r.get(k, "") for k in ("Grid_Size_X", "Grid_Size_Y", "Grid_Size_Z"))
            dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            rows.setdefault((name.split("(")[0], grid), []).append((int(r["Start_Timestamp"]), dur))
split = int(os.environ.get("SPLIT", "1"))
parts = {}
for (name, grid), v in rows.items():
    v = [d for _, d in sorted(v)]
    for k in range(split):
        part = v[k * len(v) // split:(k + 1) * len(v) // split]
        if part:
            parts[(name + (f" [part {k + 1}/{split}]" if split > 1 else ""), grid)] = part
for (name, grid), v in sorted(parts.items()):
    print(f"{name:40s} grid {'x'.join(grid):>18s}  launches {len(v):4d}  mean {statistics.mean(v):9.2f} us  median {statistics.median(v):9.2f} us  "
          f"min {min(v):9.2f} us")
if not rows:
    print("no matching kernel rows found under", sys.argv[1])
    sys.exit(1)
