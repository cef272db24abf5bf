"""DIS vs Farneback throughput at the reference's operating point (256x256, B = 256), one process, alternating:
  * resident rate of each algorithm: ffl_flow_pairs_dis / ffl_flow_pairs + pass-1 results on frames already on the device
    (host clock around synchronised batches)
  * DIS through backend.precompute_all from host frames, one 3000-frame chunk
python profiles/tools/dis_rate.py [--reps R] [--batches K] [--out result.json]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
from funscript_flow_amd import _capi, backend  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--batches", type=int, default=20)
ap.add_argument("--out", default=None)
a = ap.parse_args()
W = H = 256
B = 256
fr = sine_translate_frames(B + 1, W, H, seed=1, amp=(3.0, 2.0), zoom=0.02)
ctx = _capi.Context(W, H, frame_slots=B + 1, flow_slots=2 * B, max_batch=B)
ctx.upload_frames(0, list(fr))
f0, f1 = list(range(B)), list(range(1, B + 1))
slots = [list(range(B)), list(range(B, 2 * B))]


def resident(call):
    for k in range(2):   # warm-up (graph capture of the Farneback shape, clocks)
        call(f0, f1, slots[k])
    ctx.sync()
    t0 = time.perf_counter()
    for k in range(a.batches):
        call(f0, f1, slots[k & 1])
        if k >= 1:
            ctx.pass1_results(slots[(k - 1) & 1])
    ctx.pass1_results(slots[(a.batches - 1) & 1])
    ctx.sync()
    return a.batches * B / (time.perf_counter() - t0)


N = int(os.environ.get("FRAMES", "3000"))
base = sine_translate_frames(17, W, H, seed=1)
frames = [base[i % 17][:] for i in range(N)]
pairs = list(zip(frames[:-1], frames[1:]))
res = {"size": [W, H], "batch": B, "dis_resident": [], "farneback_resident": [], "dis_precompute_all": []}
for rep in range(a.reps):
    res["dis_resident"].append(resident(ctx.flow_pairs_dis))
    res["farneback_resident"].append(resident(ctx.flow_pairs))
    t0 = time.perf_counter()
    backend.precompute_all(pairs, {"backend": "HIP", "hip_flow": "dis"})
    res["dis_precompute_all"].append((N - 1) / (time.perf_counter() - t0))
    print(f"rep {rep}: DIS resident {res['dis_resident'][-1]:.0f} pairs/s, Farneback resident "
          f"{res['farneback_resident'][-1]:.0f} pairs/s, DIS precompute_all {res['dis_precompute_all'][-1]:.0f} pairs/s", flush=True)
res["median"] = {k: float(np.median(res[k])) for k in ("dis_resident", "farneback_resident", "dis_precompute_all")}
res["graphs"] = ctx.graph_stats()
backend.release_contexts()
ctx.close()
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
