"""Rate of the 4:2:0 front-end (ffl_upload_frames_yuv) against the BGR one (ffl_upload_frames_raw):
decoded frames/s with the H2D transfer included (host clock around a synchronised run of uploads), bytes each frame
sends, and the mean launch time of k_frontend (HIP events), for BGR, I420 and NV12, staged (pageable
arrays) and zero-copy (frames in the context's page-locked memory), at 1080p -> 256², 4K -> 256² and 5760x2880 VR -> 256².
--depth 9..16 adds, after every 4:2:0 row, the same source as uint16 frames of that depth (ffl_upload_frames_yuv16, rule
Y5: yuv420p10le for I420, P010 for NV12), so that the 8-bit row and its 16-bit row are measured side by side.

    python profiles/tools/frontend_yuv_rate.py [--reps 5] [--frames 16] [--out file.json] [--only-yuv] [--depth 10]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (its HIP runtime first)
from funscript_flow_amd import _capi, frontend  # noqa: E402

SOURCES = [(1920, 1080, False), (3840, 2160, False), (5760, 2880, True)]


def frames_of(fmt, sw, sh, n, depth=8):
    rng = np.random.default_rng(1)
    shape = (sh, sw, 3) if fmt == "bgr" else (sh * 3 // 2, sw)
    if depth == 8:
        return [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)]
    shift = 16 - depth if fmt == "nv12" else 0   # P010-style surfaces carry the bits high
    return [(rng.integers(0, 1 << depth, shape, dtype=np.uint16) << shift).astype(np.uint16) for _ in range(n)]


def run(ctx, fmt, up, vr, depth=8):
    if fmt == "bgr":
        frontend.upload_decoded(ctx, 0, up, vr_mode=vr)
    elif depth == 8:
        frontend.upload_decoded(ctx, 0, up, vr_mode=vr, yuv=fmt)
    else:
        frontend.upload_decoded(ctx, 0, up, vr_mode=vr, yuv=fmt, depth=depth)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-yuv", action="store_true", help="skip the BGR rows (for a kernel trace of k_frontend on 4:2:0 frames)")
    ap.add_argument("--depth", type=int, default=8, help="9..16: also measure every 4:2:0 row as uint16 frames of this depth")
    a = ap.parse_args()
    out = []
    for sw, sh, vr in SOURCES:
        n = a.frames if sw * sh <= 3840 * 2160 else max(a.frames // 2, 2)
        resize, crop = frontend.geometry(256, 256, vr)
        fmts = [(f, 8) for f in (["i420", "nv12"] if a.only_yuv else ["bgr", "i420", "nv12"])]
        if a.depth != 8:
            fmts = [fd for f, _ in fmts for fd in ([(f, 8)] if f == "bgr" else [(f, 8), (f, a.depth)])]
        for fmt, depth in fmts:
            frames = frames_of(fmt, sw, sh, n, depth)
            if fmt == "bgr":
                nbytes = sw * sh * 3
            elif depth == 8:
                nbytes = _capi.frontend_yuv_window((sw, sh), fmt, resize, crop, (256, 256))[1]
            else:
                nbytes = _capi.frontend_yuv_window((sw, sh), fmt, resize, crop, (256, 256), depth=depth)[1]
            for zero_copy in (False, True):
                with _capi.Context(256, 256, max_batch=8, frame_slots=n) as ctx:
                    if zero_copy:   # as if the decoder wrote into page-locked memory of the context
                        pin = (ctx.pinned_frames(n, channels=3, size=(sw, sh)) if fmt == "bgr"
                               else ctx.pinned_frames(n, size=(sw, sh), yuv=True) if depth == 8
                               else ctx.pinned_frames(n, size=(sw, sh), yuv=True, depth=depth))
                        pin[:] = np.stack(frames)
                        up = [pin[i] for i in range(n)]
                    else:
                        up = frames
                    run(ctx, fmt, up, vr, depth)
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        run(ctx, fmt, up, vr, depth)
                    ctx.sync()
                    dt = (time.perf_counter() - t0) / (a.reps * n)
                    ctx.profile_enable(["k_frontend"])
                    run(ctx, fmt, up, vr, depth)
                    ctx.sync()
                    launches, ms = ctx.profile_read()["k_frontend"]
                rec = {"source": f"{sw}x{sh}", "vr_mode": vr, "format": fmt, "depth": depth, "zero_copy": zero_copy,
                       "frames_per_s_incl_h2d": round(1.0 / dt, 1), "bytes_per_frame": nbytes,
                       "h2d_GBps": round(nbytes / dt / 1e9, 2), "kernel_us": round(1e3 * ms / max(launches, 1), 2),
                       "frames": n, "reps": a.reps}
                print(json.dumps(rec), flush=True)
                out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
