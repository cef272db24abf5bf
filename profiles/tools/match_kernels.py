"""k_track_match (PS = "p,s" in the environment, 1 and 8 tracks) beside k_track (radius 12, one track) and k_texture on the same
slots of real frames and Farneback fields.  Run under rocprofv3 --kernel-trace --stats for kernel times (one (p, s) per run:
a trace tells k_track_match launches apart by their grid, tracks x items, alone); prints device-event times of the calls as a
second figure."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

REPS = int(os.environ.get("REPS", "20"))
P, S = (int(v) for v in os.environ.get("PS", "8,8").split(","))
out = {"p": P, "s": S}
for (w, h, n) in ((256, 256, 256), (1920, 1080, 32)):
    fr = sine_translate_frames(n + 1, w, h, seed=5)
    print("frames", w, h, flush=True)
    with _capi.Context(w, h, max_batch=n, frame_slots=n + 1, flow_slots=n) as ctx:
        ctx.upload_frames(0, list(fr))
        slots = list(range(n))
        ctx.flow_pairs(slots, list(range(1, n + 1)), slots)
        ctx.sync()
        rng = np.random.default_rng(1)
        pts = np.stack([rng.uniform(0.25 * w, 0.75 * w, 8), rng.uniform(0.25 * h, 0.75 * h, 8)], axis=1)
        states = {T: pipeline.track_state(ctx, pts[:T]) for T in (1, 8)}
        start = {T: states[T].clone() for T in states}
        recs = {T: pipeline.track_buffer(ctx, n, T) for T in (1, 8)}
        mrec = {T: pipeline.match_buffer(ctx, n, T) for T in (1, 8)}
        tmpl = {T: pipeline.match_templates(ctx, T, P) for T in (1, 8)}
        maps = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        never = float("inf")
        prm = {"p": P, "s": S}
        for T in (1, 8):   # the records the matcher corrects: one advected path per track count, made once
            ctx.track_template(0, states[T], tmpl[T], P)
            ctx.track_advance(slots, states[T], recs[T], {"radius": 12, "cut_threshold": never})
        keep = {T: recs[T].clone() for T in recs}

        calls = {f"match_p{P}_s{S}_T{T}": (lambda T=T: ctx.track_match(slots, tmpl[T], (recs[T], 48 * T), mrec[T], prm, T, True))
                 for T in (1, 8)}
        calls.update({
            "track_r12_T1": lambda: ctx.track_advance(slots, states[1], recs[1], {"radius": 12, "cut_threshold": never}),
            "texture_r7": lambda: ctx.texture_weights(slots, maps),
        })
        for c in calls.values():   # warm-up
            c()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(REPS):      # alternating
            for k, c in calls.items():
                for T in states:   # every call sees the same centres and walks the same path
                    states[T].copy_(start[T])
                    recs[T].copy_(keep[T])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        res = {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2)} for k, v in times.items()}
        m = pipeline.match_records(mrec[8], 8)
        res["accepted_of_T8"] = [int((m["status"] == 0).sum()), int(m.size)]
        out[f"{w}x{h}_n{n}"] = res
        print(json.dumps({f"{w}x{h}_n{n}": res}), flush=True)
path = os.environ.get("OUT")
if path:
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
