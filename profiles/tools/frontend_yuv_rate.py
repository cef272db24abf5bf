"""Rate of the 4:2:0 front-end (ffl_upload_frames_yuv) against the BGR one (ffl_upload_frames_raw):
decoded frames/s with the H2D transfer included (host clock around a synchronised run of uploads), bytes each frame
sends, and the mean launch time of k_frontend (HIP events), for BGR, I420 and NV12, staged (pageable
arrays) and zero-copy (frames in the context's page-locked memory), at 1080p -> 256², 4K -> 256² and 5760x2880 VR -> 256².

    python profiles/tools/frontend_yuv_rate.py [--reps 5] [--frames 16] [--out file.json] [--only-yuv]
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


def frames_of(fmt, sw, sh, n):
    rng = np.random.default_rng(1)
    shape = (sh, sw, 3) if fmt == "bgr" else (sh * 3 // 2, sw)
    return [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)]


def run(ctx, fmt, up, vr):
    if fmt == "bgr":
        frontend.upload_decoded(ctx, 0, up, vr_mode=vr)
    else:
        frontend.upload_decoded(ctx, 0, up, vr_mode=vr, yuv=fmt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-yuv", action="store_true", help="skip the BGR rows (for a kernel trace of k_frontend on 4:2:0 frames)")
    a = ap.parse_args()
    out = []
    for sw, sh, vr in SOURCES:
        n = a.frames if sw * sh <= 3840 * 2160 else max(a.frames // 2, 2)
        resize, crop = frontend.geometry(256, 256, vr)
        for fmt in (["i420", "nv12"] if a.only_yuv else ["bgr", "i420", "nv12"]):
            frames = frames_of(fmt, sw, sh, n)
            if fmt == "bgr":
                nbytes = sw * sh * 3
            else:
                nbytes = _capi.frontend_yuv_window((sw, sh), fmt, resize, crop, (256, 256))[1]
            for zero_copy in (False, True):
                with _capi.Context(256, 256, max_batch=8, frame_slots=n) as ctx:
                    if zero_copy:   # as if the decoder wrote into page-locked memory of the context
                        pin = (ctx.pinned_frames(n, channels=3, size=(sw, sh)) if fmt == "bgr"
                               else ctx.pinned_frames(n, size=(sw, sh), yuv=True))
                        pin[:] = np.stack(frames)
                        up = [pin[i] for i in range(n)]
                    else:
                        up = frames
                    run(ctx, fmt, up, vr)
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(a.reps):
                        run(ctx, fmt, up, vr)
                    ctx.sync()
                    dt = (time.perf_counter() - t0) / (a.reps * n)
                    ctx.profile_enable(["k_frontend"])
                    run(ctx, fmt, up, vr)
                    ctx.sync()
                    launches, ms = ctx.profile_read()["k_frontend"]
                rec = {"source": f"{sw}x{sh}", "vr_mode": vr, "format": fmt, "zero_copy": zero_copy,
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
