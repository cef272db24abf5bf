"""Chunk rate of process_chunk(weights="texture") and process_chunk(weights="residual", texture=True) against
process_chunk(weights=<static map>), weights="residual" and the plain device schedule, alternating in one process, wall clock
around a device synchronise.  On a tree without the texture mode (the parent commit) the two new runs are left out, so that
the same script gives that build's static-map, residual and plain figures (TREE=<root of that build>)."""
import inspect
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
HAS_TEXTURE = "texture" in inspect.signature(pipeline.PairEngine.process_chunk).parameters
out = {"has_texture": HAS_TEXTURE}
for (w, h, B, frames) in ((256, 256, 256, 1025), (1920, 1080, 32, 97)):
    fr = list(sine_translate_frames(frames, w, h, seed=5))
    n = frames - 1
    print("frames", w, h, flush=True)
    with _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
        eng = pipeline.PairEngine(ctx)
        static = torch.full((h, w), 255, dtype=torch.uint8, device="cuda:0")
        post = pipeline.post_buffer(ctx, n, axes=True)
        M = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        runs = {"plain": lambda: eng.process_chunk(fr, axes=True, post_out=post),
                "static_map": lambda: eng.process_chunk(fr, weights=static, post_out=post),
                "residual": lambda: eng.process_chunk(fr, weights="residual", weights_out=M, post_out=post)}
        if HAS_TEXTURE:
            runs.update({
                "texture": lambda: eng.process_chunk(fr, weights="texture", weights_out=M, post_out=post),
                "residual_texture": lambda: eng.process_chunk(fr, weights="residual", texture=True, weights_out=M, post_out=post),
                "texture_compensate": lambda: eng.process_chunk(fr, weights="texture", weights_out=M, post_out=post,
                                                                compensate="translation"),
            })
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
        for k in res.copy():
            if k not in ("plain", "static_map"):
                res[f"ratio_{k}_to_static_map"] = round(res[k]["median_pairs_per_s"] / res["static_map"]["median_pairs_per_s"], 3)
        res["depth"], res["pairs"] = eng.depth, n
        res["graph_stats"] = ctx.graph_stats()
        out[f"{w}x{h}_B{B}"] = res
        print(json.dumps({f"{w}x{h}_B{B}": res}), flush=True)
with open(os.environ["OUT"], "w") as f:
    json.dump(out, f, indent=1)
