"""k_texture (radius 3 and 7) against k_residual and k_export_flows (NHWC) on the same slots, real Farneback fields.
Run under rocprofv3 --kernel-trace --stats for kernel times (and --pmc, in runs of their own, for counters); prints
device-event times of the calls as a second figure."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

REPS = int(os.environ.get("REPS", "20"))
out = {}
for (w, h, n) in ((1920, 1080, 32), (256, 256, 256)):
    fr = sine_translate_frames(n + 1, w, h, seed=5)
    print("frames", w, h, flush=True)
    with _capi.Context(w, h, max_batch=n, frame_slots=n + 1, flow_slots=n) as ctx:
        ctx.upload_frames(0, list(fr))
        f0, f1 = list(range(n)), list(range(1, n + 1))
        fwd = list(range(n))
        ctx.flow_pairs(f0, f1, fwd)
        ctx.sync()
        maps = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((n, h, w, 2), dtype=torch.float32, device="cuda:0")
        gate = torch.full((h, w), 200, dtype=torch.uint8, device="cuda:0")
        calls = {
            "texture_r3": lambda: ctx.texture_weights(f0, maps, {"radius": 3}),
            "texture_r7": lambda: ctx.texture_weights(f0, maps),
            "texture_r7_hard": lambda: ctx.texture_weights(f0, maps, {"soft": 0}),
            "texture_r7_gate": lambda: ctx.texture_weights(f0, maps, gate=gate),
            "texture_r7_in_place": lambda: ctx.texture_weights(f0, maps, gate=maps),
            "residual_soft": lambda: ctx.residual_weights(f0, f1, fwd, maps),
            "export_nhwc": lambda: ctx.export_flows(fwd, dst, "nhwc"),
        }
        for c in calls.values():   # warm-up
            c()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(REPS):      # alternating
            for k, c in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        ctx.texture_weights(f0, maps)
        m = maps.cpu().numpy()
        res = {k: {"median_us": float(np.median(v)), "min_us": float(np.min(v))} for k, v in times.items()}
        res["share_255"] = float((m == 255).mean())
        res["share_0"] = float((m == 0).mean())
        res["mean_map"] = float(m.mean())
        out[f"{w}x{h}_n{n}"] = res
        print(json.dumps({f"{w}x{h}_n{n}": res}), flush=True)
path = os.environ.get("OUT")
if path:
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
