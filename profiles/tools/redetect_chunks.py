"""Chunk rate of process_chunk(center="track") with track["match"] alone, with track["match"]["redetect"] where nothing triggers
(mask 0) and where every batch triggers (max_mse 0: every search about the state reads POOR), against the plain device schedule
and the tracked one, alternating in one process, wall clock around a device synchronise.  On a tree without the re-detector
(the parent commit) its runs are left out, so that the same script gives that build's figures (TREE=<root of that build>)."""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.environ.get("TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))   # TREE: another build's root
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

REPS = int(os.environ.get("REPS", "4"))   # rep 0 is the warm-up
HAS = hasattr(_capi, "RedetectParams")
out = {"has_redetect": HAS, "lib": _capi.LIB_PATH}
for (w, h, B, frames) in ((256, 256, 256, 1025), (1920, 1080, 32, 97)):
    fr = list(sine_translate_frames(frames, w, h, seed=5))
    n = frames - 1
    print("frames", w, h, flush=True)
    with _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
        eng = pipeline.PairEngine(ctx)
        post = pipeline.post_buffer(ctx, n, axes=True)
        tout = pipeline.track_buffer(ctx, n, 1)
        rout = pipeline.match_buffer(ctx, n, 1)

        def track(match=None):
            trk = {"start": [(w / 2.0, h / 2.0)], "radius": 12}
            if match is not None:
                trk["match"] = match
            kw = {"redetect_out": rout} if match and "redetect" in match else {}
            return lambda: eng.process_chunk(fr, center="track", track=trk, track_out=tout, post_out=post, **kw)

        runs = {"plain": lambda: eng.process_chunk(fr, axes=True, post_out=post), "track_r12_T1": track(),
                "match_p8_s8": track({"p": 8, "s": 8}), "match_p8_s8_poor": track({"p": 8, "s": 8, "max_mse": 0.0})}
        if HAS:
            runs["match_p8_s8_redetect_untriggered"] = track({"p": 8, "s": 8, "redetect": {"mask": 0}})
            runs["match_p8_s8_poor_redetect_every_batch"] = track({"p": 8, "s": 8, "max_mse": 0.0, "redetect": True})
        t = {k: [] for k in runs}
        for rep in range(REPS):
            for k, r in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rep:
                    t[k].append(dt)
        res = {k: {"pairs_per_s": [round(n / x, 1) for x in v], "median_pairs_per_s": round(n / float(np.median(v)), 1)} for k, v in t.items()}
        if HAS:
            r = pipeline.match_records(rout, 1)
            last = list(range(B - 1, n, B))
            res["redetect_status_of_the_last_run"] = [int(s) for s in r["status"][last, 0]]
        res["depth"], res["pairs"] = eng.depth, n
        res["graph_stats"] = ctx.graph_stats()
        out[f"{w}x{h}_B{B}"] = res
        print(json.dumps({f"{w}x{h}_B{B}": res}), flush=True)
with open(os.environ["OUT"], "w") as f:
    json.dump(out, f, indent=1)
