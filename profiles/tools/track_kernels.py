"""k_track (radius 12 and 32, 1 and 8 tracks) against k_cell_stats + k_grid_centre -- the other centre estimator -- and
k_roi_weights against k_export_flows (NHWC), all on the same slots, real Farneback fields.  Run under rocprofv3 --kernel-trace
--stats for kernel times; prints device-event times of the calls as a second figure."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

REPS = int(os.environ.get("REPS", "20"))
# a kernel trace tells k_track launches apart by their grid (the tracks) alone: trace one radius per run, without the map call
RADII = [int(r) for r in os.environ.get("RADII", "12,32").split(",")]
MAPS = os.environ.get("MAPS", "1") == "1"
out = {}
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
        recs = {T: pipeline.track_buffer(ctx, n, T) for T in (1, 8)}
        centres = torch.empty(n * _capi.GRID_CENTRE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:0")
        maps = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        wmap = torch.full((h, w), 200, dtype=torch.uint8, device="cuda:0")
        dst = torch.empty((n, h, w, 2), dtype=torch.float32, device="cuda:0")
        never = float("inf")

        start = {T: states[T].clone() for T in states}

        def track(T, r, weights=None):
            return lambda: ctx.track_advance(slots, states[T], recs[T], {"radius": r, "cut_threshold": never}, weights)

        calls = {f"track_r{r}_T{T}": track(T, r) for r in RADII for T in (1, 8)}
        if MAPS:
            calls[f"track_r{RADII[0]}_T8_map"] = track(8, RADII[0], wmap)
        calls.update({
            "cell_stats_centres_G32": lambda: ctx.cell_stats(slots, 32, None, centres),
            "roi_soft": lambda: ctx.roi_weights(n, (recs[1], 48), maps),
            "roi_hard_gate": lambda: ctx.roi_weights(n, (recs[1], 48), maps, {"soft": 0}, gate=wmap),
            "export_nhwc": lambda: ctx.export_flows(slots, dst, "nhwc"),
        })
        for c in calls.values():   # warm-up
            c()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(REPS):      # alternating
            for k, c in calls.items():
                for T in states:   # every call walks the same path from the same start
                    states[T].copy_(start[T])
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                c()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3)
        res = {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2)} for k, v in times.items()}
        tr = pipeline.track_records(recs[8], 8)
        res["track_lost_or_clamped"] = int((tr["status"] != 0).sum())
        res["mean_step_px"] = round(float(np.hypot(tr["du"], tr["dv"]).mean()), 4)
        out[f"{w}x{h}_n{n}"] = res
        print(json.dumps({f"{w}x{h}_n{n}": res}), flush=True)
path = os.environ.get("OUT")
if path:
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
