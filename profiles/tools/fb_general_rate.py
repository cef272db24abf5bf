"""Farneback through the general-parameter kernels (ffl_flow_pairs_farneback) vs the tuned path, one
process, alternating; resident rate = batches of pairs on frames already on the device + pass-1 results (host clock around
synchronised batches):
  * 256x256, B = 256: tuned ffl_flow_pairs; the defaults forced through the general kernels ("fb_general" = 1);
    poly_n 7 / poly_sigma 1.5 / winsize 21
  * 1920x1080, B = 32: tuned; defaults forced general; levels 5
--window W[,W...] measures the two windows of the general kernels instead: at each winsize W, the box
(ffl_flow_pairs_farneback) against the Gaussian (ffl_flow_pairs_farneback_ex, FFL_FB_GAUSSIAN_WINDOW), other numbers at
their defaults, alternating in one process.
python profiles/tools/fb_general_rate.py [--reps R] [--batches K] [--only 256|1080] [--window 15,63] [--out result.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
from funscript_flow_amd import _capi  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=10)
ap.add_argument("--only", default=None)
ap.add_argument("--window", default=None, help="comma-separated winsizes: box against Gaussian window")
ap.add_argument("--out", default=None)
a = ap.parse_args()

SETUPS = [("256", 256, 256, 256, {"poly_n": 7, "poly_sigma": 1.5, "winsize": 21}),
          ("1080", 1920, 1080, 32, {"levels": 5})]
res = {"reps": a.reps, "batches": a.batches}
for tag, W, H, B, over in SETUPS:
    if a.only and a.only != tag:
        continue
    fr = sine_translate_frames(B + 1, W, H, seed=1, amp=(3.0, 2.0), zoom=0.02)
    ctx = _capi.Context(W, H, frame_slots=B + 1, flow_slots=2 * B, max_batch=B)
    ctx.upload_frames(0, list(fr))
    f0, f1 = list(range(B)), list(range(1, B + 1))
    slots = [list(range(B)), list(range(B, 2 * B))]

    def resident(call, batches):
        for k in range(2):   # warm-up (graph capture of the tuned shape, the general work area, clocks)
            call(f0, f1, slots[k])
        ctx.sync()
        t0 = time.perf_counter()
        for k in range(batches):
            call(f0, f1, slots[k & 1])
            if k >= 1:
                ctx.pass1_results(slots[(k - 1) & 1])
        ctx.pass1_results(slots[(batches - 1) & 1])
        ctx.sync()
        return batches * B / (time.perf_counter() - t0)

    if a.window:
        r = {"size": [W, H], "batch": B}
        ctx.set_option("fb_general", 1)   # winsize 15 is the default set: keep the box on the general kernels too
        for ws in [int(v) for v in a.window.split(",")]:
            q = _capi.FarnebackParams(winsize=ws)
            rates = {"box": [], "gaussian": []}
            for rep in range(a.reps):
                for win in ("box", "gaussian"):
                    rates[win].append(resident(lambda x, y, s: ctx.flow_pairs_farneback(x, y, s, False, q, window=win), a.batches))
                print(f"{W}x{H} B={B} winsize {ws} rep {rep}: box {rates['box'][-1]:.0f}, gaussian {rates['gaussian'][-1]:.0f} "
                      f"pairs/s", flush=True)
            r[f"winsize{ws}"] = {**rates, "median": {k: float(np.median(v)) for k, v in rates.items()}}
        ctx.close()
        res[tag] = r
        continue
    p = _capi.FarnebackParams(**over)
    d = _capi.FarnebackParams()
    r = {"size": [W, H], "batch": B, "params": over, "tuned": [], "general_defaults": [], "general_params": []}
    for rep in range(a.reps):
        ctx.set_option("fb_general", 0)
        r["tuned"].append(resident(lambda x, y, s: ctx.flow_pairs(x, y, s), a.batches))
        ctx.set_option("fb_general", 1)
        r["general_defaults"].append(resident(lambda x, y, s: ctx.flow_pairs_farneback(x, y, s, False, d), a.batches))
        ctx.set_option("fb_general", 0)
        r["general_params"].append(resident(lambda x, y, s: ctx.flow_pairs_farneback(x, y, s, False, p), a.batches))
        print(f"{W}x{H} B={B} rep {rep}: tuned {r['tuned'][-1]:.0f}, general (defaults) {r['general_defaults'][-1]:.0f}, "
              f"general {over} {r['general_params'][-1]:.0f} pairs/s", flush=True)
    r["median"] = {k: float(np.median(r[k])) for k in ("tuned", "general_defaults", "general_params")}
    r["tuned_over_general_defaults"] = r["median"]["tuned"] / r["median"]["general_defaults"]
    r["graphs"] = ctx.graph_stats()
    ctx.close()
    res[tag] = r
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
