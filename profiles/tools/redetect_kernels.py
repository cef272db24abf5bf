"""The four launches of ffl_track_redetect (k_redetect_sweep, k_redetect_pick, k_redetect_sweep masked, k_redetect_final) for one
shape, one (p, reach) and one trigger state per process, 1 and 8 tracks, beside k_track_match at (8, 8) and k_texture at r = 7
on the same frame slots.  Environment: SHAPE = "w,h,n" (default 256,256,256), PR = "p,reach" (default 8,0), TRIG = all | none.
Run under rocprofv3 --kernel-trace --stats for kernel times (a trace tells the launches of 1 and 8 tracks apart by their
grids; shapes, (p, reach) and trigger states share grids, hence a process each); prints device-event times of the whole
calls as a second figure."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

REPS = int(os.environ.get("REPS", "10"))
W, H, N = (int(v) for v in os.environ.get("SHAPE", "256,256,256").split(","))
P, REACH = (int(v) for v in os.environ.get("PR", "8,0").split(","))
TRIG = os.environ.get("TRIG", "all")
fr = sine_translate_frames(N, W, H, seed=5)
with _capi.Context(W, H, max_batch=N, frame_slots=N, flow_slots=2) as ctx:
    ctx.upload_frames(0, list(fr))
    ctx.sync()
    slots = list(range(N))
    rng = np.random.default_rng(1)
    pts = np.stack([rng.uniform(0.25 * W, 0.75 * W, 8), rng.uniform(0.25 * H, 0.75 * H, 8)], axis=1)
    cen, trig, out, mout, tmpl, tmpl8 = {}, {}, {}, {}, {}, {}
    for T in (1, 8):
        state = pipeline.track_state(ctx, pts[:T])
        tmpl[T] = pipeline.match_templates(ctx, T, P)
        ctx.track_template(0, state, tmpl[T], P)
        tmpl8[T] = pipeline.match_templates(ctx, T, 8)
        ctx.track_template(0, state, tmpl8[T], 8)
        rec = np.zeros((N, T), _capi.MATCH_DTYPE)           # 48-byte records whose heads are the centres, 20 px off the capture
        rec["x"], rec["y"] = pts[None, :T, 0] + 20.0, pts[None, :T, 1] - 20.0
        rec["status"] = _capi.MATCH_POOR if TRIG == "all" else 0
        cen[T] = torch.from_numpy(np.frombuffer(rec.tobytes(), np.uint8).copy()).to("cuda:0")
        trig[T] = cen[T].clone()
        out[T], mout[T] = pipeline.match_buffer(ctx, N, T), pipeline.match_buffer(ctx, N, T)
    maps = torch.empty((N, H, W), dtype=torch.uint8, device="cuda:0")
    prm = {"p": P, "exclude": P, "reach": REACH}
    calls = {f"redetect_p{P}_reach{REACH}_{TRIG}_T{T}": (lambda T=T: ctx.track_redetect(slots, tmpl[T], (cen[T], 48 * T), out[T], prm, T,
                                                                                        trig[T], False)) for T in (1, 8)}
    calls.update({f"match_p8_s8_T{T}": (lambda T=T: ctx.track_match(slots, tmpl8[T], (cen[T], 48 * T), mout[T], {"p": 8, "s": 8}, T, False))
                  for T in (1, 8)})
    calls["texture_r7"] = lambda: ctx.texture_weights(slots, maps)
    for c in calls.values():   # warm-up
        c()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(REPS):      # alternating; write_back is off, so every call sees the same centres
        for k, c in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            c()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3)
    res = {k: {"median_us": round(float(np.median(v)), 2), "min_us": round(float(np.min(v)), 2)} for k, v in times.items()}
    r = pipeline.match_records(out[8], 8)
    res["status_counts_T8"] = {str(int(s)): int((r["status"] == s).sum()) for s in np.unique(r["status"])}
    print(json.dumps({f"{W}x{H}_n{N}": res}), flush=True)
