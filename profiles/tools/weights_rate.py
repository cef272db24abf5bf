"""Cost of the weight maps, timed with HIP events in one process, repetitions interleaved:

  window  us per call of ffl_radial_window_axes against ffl_radial_window_axes_weighted -- k_window_plan plus the
          four-component pair, unweighted / under one shared map / under one map per item -- for 32 items at 1920x1080 and
          256 items at 256x256 (events on the caller's stream around `calls` back-to-back calls; each call makes that
          stream wait for its records, so the interval ends when the last records are written)
  pass1   us per call of ffl_pass1_weighted for the same items (shared map, per-item maps)

    python profiles/tools/weights_rate.py [--reps 7] [--calls 20] [--out file.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from funscript_flow_amd import _capi  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, calls):
    """us per call between an event before `calls` calls of fn() and one after them on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def case(w, h, n, reps, calls, out):
    g = torch.Generator(device=DEV).manual_seed(1)
    ctx = _capi.Context(w, h, max_batch=n, frame_slots=2, flow_slots=n)
    slots = list(range(n))
    ctx.import_flows(torch.randn((n, h, w, 2), device=DEV, generator=g), slots)
    maps = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=DEV, generator=g)
    maps[torch.rand((n, h, w), device=DEV, generator=g) < 1 / 3] = 0
    rec = torch.empty(n * 80, dtype=torch.uint8, device=DEV)
    thr = 1e30
    runs = {"window unweighted": lambda: ctx.radial_window_axes(slots, 0, n, rec, 6, thr),
            "window shared map": lambda: ctx.radial_window_axes_weighted(slots, 0, n, maps[0], rec, 6, thr),
            "window per-item maps": lambda: ctx.radial_window_axes_weighted(slots, 0, n, maps, rec, 6, thr),
            "pass1 shared map": lambda: ctx.pass1_weighted(slots, maps[0]),
            "pass1 per-item maps": lambda: ctx.pass1_weighted(slots, maps)}
    us = {k: [] for k in runs}
    for r in range(reps + 1):
        for k, fn in runs.items():
            t = timed(fn, calls)
            if r:
                us[k].append(t)
    base = float(np.median(us["window unweighted"]))
    for k, v in us.items():
        med = float(np.median(v))
        r = {"what": k, "size": f"{w}x{h}", "items": n, "median_us_per_call": round(med, 2), "min_us": round(min(v), 2),
             "max_us": round(max(v), 2), "reps": reps, "calls": calls}
        if k.startswith("window"):
            r["ratio_to_unweighted"] = round(med / base, 4)
        print(json.dumps(r), flush=True)
        out.append(r)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    case(1920, 1080, 32, a.reps, a.calls, out)
    case(256, 256, 256, a.reps, a.calls, out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
