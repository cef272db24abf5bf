"""Chunk rate of process_chunk(center="track") with and without track["match"] against the plain device schedule, alternating
in one process, wall clock around a device synchronise.  On a tree without the matcher (the parent commit) the matched runs are
left out, so that the same script gives that build's figures (TREE=<root of that build>); ONLY_COMMON=1 leaves them out on this
tree too, so that both builds' processes do the same work."""
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
HAS_MATCH = hasattr(_capi, "MatchParams") and os.environ.get("ONLY_COMMON") != "1"   # ONLY_COMMON=1: the parent's runs alone
out = {"has_match": HAS_MATCH, "lib": _capi.LIB_PATH}
for (w, h, B, frames) in ((256, 256, 256, 1025), (1920, 1080, 32, 97)):
    fr = list(sine_translate_frames(frames, w, h, seed=5))
    n = frames - 1
    print("frames", w, h, flush=True)
    with _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
        eng = pipeline.PairEngine(ctx)
        post = pipeline.post_buffer(ctx, n, axes=True)
        M = torch.empty((n, h, w), dtype=torch.uint8, device="cuda:0")
        start = (w / 2.0, h / 2.0)
        tout = {T: pipeline.track_buffer(ctx, n, T) for T in (1, 8)}

        def track(T, match=None, roi=None):
            trk = {"start": [start] * T, "radius": 12, "roi": roi}
            if match is not None:
                trk["match"] = {"p": match[0], "s": match[1]}
            return lambda: eng.process_chunk(fr, center="track", track=trk, track_out=tout[T], post_out=post,
                                             **({"weights_out": M} if roi else {}))

        runs = {"plain": lambda: eng.process_chunk(fr, axes=True, post_out=post),
                "track_r12_T1": track(1), "track_r12_T8": track(8), "track_r12_T1_roi": track(1, roi=(48.0, 48.0))}
        if HAS_MATCH:
            runs.update({"track_r12_T1_match_p8_s8": track(1, (8, 8)), "track_r12_T8_match_p8_s8": track(8, (8, 8)),
                         "track_r12_T1_match_p16_s16": track(1, (16, 16)), "track_r12_T8_match_p16_s16": track(8, (16, 16)),
                         "track_r12_T1_match_p8_s8_roi": track(1, (8, 8), (48.0, 48.0))})
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
            if k != "plain":
                res[f"ratio_{k}_to_plain"] = round(res[k]["median_pairs_per_s"] / res["plain"]["median_pairs_per_s"], 3)
        res["depth"], res["pairs"] = eng.depth, n
        res["graph_stats"] = ctx.graph_stats()
        out[f"{w}x{h}_B{B}"] = res
        print(json.dumps({f"{w}x{h}_B{B}": res}), flush=True)
with open(os.environ["OUT"], "w") as f:
    json.dump(out, f, indent=1)
