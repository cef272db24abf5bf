"""Cost of the per-cell statistics grid, in one process:

  kernels  us of ffl_cell_stats (k_cell_stats + k_grid_centre) per call for 32 slots at 1920x1080 and 256 slots at 256x256
           under a 32 x 32 grid -- HIP events on the caller's stream around `calls` back-to-back calls, each of which makes
           that stream wait for its records, so the figure includes a call's two stream hand-offs -- against the k_pass1 +
           k_pass1_final pair on the same slots, which the library's own event brackets time inside a Farneback batch
           (profile class k_pass1).  Both read 8 B per pixel once.  Repetitions interleaved, medians.
  chunk    pairs/s of process_chunk(center="variance", post_out=True) against process_chunk(axes=True, post_out=True) over one
           chunk of --frames 256x256 frames at B = 256, interleaved, one read of the records each.

    python profiles/tools/cell_stats_rate.py [--reps 21] [--calls 10] [--frames 3000] [--only kernels|chunk] [--shape 1080p|256]
                                             [--out file.json]

At 256x256 a call's host cost exceeds its kernels' time, so the per-call figure there is the host's; the kernels' own
durations come from a kernel trace of one shape:  rocprofv3 --kernel-trace --stats -d DIR -o NAME --output-format csv --
python profiles/tools/cell_stats_rate.py --only kernels --shape 256 --reps 5 --calls 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from funscript_flow_amd import _capi, pipeline  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / calls


def kernels(w, h, n, G, reps, calls, out):
    fr = sine_translate_frames(n + 1, w, h, seed=2, zoom=0.01)
    with _capi.Context(w, h, max_batch=n, frame_slots=n + 1, flow_slots=n) as ctx:
        slots = list(range(n))
        ctx.upload_frames(0, list(fr))
        cells = torch.empty(n * G * G * 32, dtype=torch.uint8, device=DEV)
        cen = torch.empty(n * 32, dtype=torch.uint8, device=DEV)
        us = {"cell_stats cells+centres": [], "cell_stats centres only": [], "pass1 pair": []}
        for r in range(reps + 1):
            ctx.profile_enable(["k_pass1"])
            ctx.flow_pairs(slots, list(range(1, n + 1)), slots)
            launches, ms = ctx.profile_read()["k_pass1"]
            ctx.profile_enable(False)
            ctx.sync()
            a = timed(lambda: ctx.cell_stats(slots, G, cells, cen), calls)
            b = timed(lambda: ctx.cell_stats(slots, G, None, cen), calls)
            if r:
                us["pass1 pair"].append(ms * 1e3 / launches)
                us["cell_stats cells+centres"].append(a)
                us["cell_stats centres only"].append(b)
        base = float(np.median(us["pass1 pair"]))
        for k, v in us.items():
            rec = {"what": k, "size": f"{w}x{h}", "items": n, "cells": G, "median_us": round(float(np.median(v)), 2),
                   "min_us": round(min(v), 2), "max_us": round(max(v), 2), "reps": reps, "ratio_to_pass1": round(float(np.median(v)) / base, 3)}
            print(json.dumps(rec), flush=True)
            out.append(rec)


def chunk(frames, reps, out):
    w = h = B = 256
    fr = list(sine_translate_frames(frames, w, h, seed=4, zoom=0.01))
    n = frames - 1
    with _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
        eng = pipeline.PairEngine(ctx)
        runs = {"axes": lambda: eng.process_chunk(fr, post_out=True, axes=True),
                "variance centre": lambda: eng.process_chunk(fr, post_out=True, center="variance")}
        rate = {k: [] for k in runs}
        for r in range(reps + 1):
            for k, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipeline.post_records(fn(), n, axes=True)
                dt = time.perf_counter() - t0
                if r:
                    rate[k].append(n / dt)
        for k, v in rate.items():
            rec = {"what": f"process_chunk {k}", "size": "256x256", "B": B, "pairs": n, "median_pairs_per_s": round(float(np.median(v)), 1),
                   "min": round(min(v), 1), "max": round(max(v), 1), "reps": reps}
            print(json.dumps(rec), flush=True)
            out.append(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--only", default=None)
    ap.add_argument("--shape", default=None, help="kernels: 1080p or 256 alone (for a kernel trace of one shape)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    if a.only in (None, "kernels"):
        if a.shape in (None, "1080p"):
            kernels(1920, 1080, 32, 32, a.reps, a.calls, out)
        if a.shape in (None, "256"):
            kernels(256, 256, 256, 32, a.reps, a.calls, out)
    if a.only in (None, "chunk"):
        chunk(a.frames, max(3, a.reps // 4), out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
