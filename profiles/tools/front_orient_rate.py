"""Front-end launch durations and host rates with and without stream metadata (rules Y6 / Y7;
sections 11 and 12), repetitions interleaved in one process.  Launch durations are the library's own event pairs around
each k_frontend / k_frontend_dev launch (ffl_profile_enable / ffl_profile_read, class k_frontend).

  plain    the launches every earlier commit has too, for comparing two builds (run this mode once per build, alternating:
           --root names the tree whose package and library are loaded): k_frontend from one 1080p BGR and one 1080p NV12
           frame into 256x256, k_frontend_dev from 64 4K BGR frames and from 64 1080p NV12 frames into 256x256
  rotated  rotate 0 / 90 / 180 / 270 + mirror in the same process: one k_frontend_dev launch of 64 1080p NV12 frames into
           256x256, and frames/s of ffl_upload_frames_yuv_src for 64 1080p NV12 frames out of ffl_host_alloc memory
           (host clock around the call and ctx.sync())

    python profiles/tools/front_orient_rate.py plain|rotated [--reps 20] [--root DIR] [--tag NAME] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["plain", "rotated"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--tag", default="")
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from funscript_flow_amd import _capi  # noqa: E402

DEV = torch.device("cuda", 0)
ORIENTATIONS = ((0, False), (90, False), (180, False), (270, True))


def launch_us(ctx, fn, launches):
    """us per k_frontend-class launch of fn(), which makes `launches` of them"""
    ctx.profile_read()
    fn()
    n, ms = ctx.profile_read()["k_frontend"]
    assert n == launches, (n, launches)
    return ms * 1e3 / n


def report(out, rec):
    rec["tag"] = ARGS.tag
    print(json.dumps(rec), flush=True)
    out.append(rec)


def stats(v):
    v = np.asarray(v)
    return {"median_us": round(float(np.median(v)), 3), "min_us": round(float(v.min()), 3), "max_us": round(float(v.max()), 3)}


def plain(reps, out):
    g = torch.Generator(device=DEV).manual_seed(1)
    rng = np.random.default_rng(2)
    n = 64
    ctx = _capi.Context(256, 256, max_batch=1, frame_slots=n)
    ctx.profile_enable(["k_frontend"])
    bgr = rng.integers(0, 256, (1080, 1920, 3), dtype=np.uint8)
    nv12 = rng.integers(0, 256, (1620, 1920), dtype=np.uint8)
    d_bgr = torch.randint(0, 256, (n, 2160, 3840, 3), dtype=torch.uint8, device=DEV, generator=g)
    d_nv12 = torch.randint(0, 256, (n, 1620, 1920), dtype=torch.uint8, device=DEV, generator=g)
    cases = {"k_frontend 1080p bgr": (lambda: ctx.upload_frames_raw(0, [bgr], (256, 256)), 1),
             "k_frontend 1080p nv12": (lambda: ctx.upload_frames_yuv(0, [nv12], "nv12", (256, 256)), 1),
             "k_frontend_dev 64 x 4K bgr": (lambda: ctx.upload_frames_device(0, d_bgr, "bgr", (256, 256)), 1),
             "k_frontend_dev 64 x 1080p nv12": (lambda: ctx.upload_frames_device(0, d_nv12, "nv12", (256, 256)), 1)}
    us = {k: [] for k in cases}
    for r in range(reps + 2):
        for k, (fn, launches) in cases.items():
            t = launch_us(ctx, fn, launches)
            if r >= 2:
                us[k].append(t)
    for k, v in us.items():
        report(out, {"what": "plain", "launch": k, "reps": reps, **stats(v)})
    ctx.close()


def rotated(reps, out):
    g = torch.Generator(device=DEV).manual_seed(1)
    n = 64
    ctx = _capi.Context(256, 256, max_batch=1, frame_slots=n)
    ctx.profile_enable(["k_frontend"])
    d_nv12 = torch.randint(0, 256, (n, 1620, 1920), dtype=torch.uint8, device=DEV, generator=g)
    pin = ctx.pinned_frames(n, size=(1920, 1080), yuv=True)
    pin[:] = np.random.default_rng(3).integers(0, 256, pin.shape, dtype=np.uint8)
    frames = list(pin)
    us = {o: [] for o in ORIENTATIONS}
    fps = {o: [] for o in ORIENTATIONS}
    for r in range(reps + 2):
        for rot, mir in ORIENTATIONS:
            t = launch_us(ctx, lambda: ctx.upload_frames_device(0, d_nv12, "nv12", (256, 256), rotate=rot, mirror=mir), 1)
            ctx.sync()
            t0 = time.perf_counter()
            ctx.upload_frames_yuv(0, frames, "nv12", (256, 256), rotate=rot, mirror=mir)
            ctx.sync()
            dt = time.perf_counter() - t0
            if r >= 2:
                us[(rot, mir)].append(t)
                fps[(rot, mir)].append(n / dt)
    base_us, base_fps = np.median(us[ORIENTATIONS[0]]), np.median(fps[ORIENTATIONS[0]])
    for rot, mir in ORIENTATIONS:
        win, nbytes = _capi.frontend_yuv_window((1920, 1080), "nv12", (256, 256), (0, 0), (256, 256), rotate=rot, mirror=mir)
        f = np.asarray(fps[(rot, mir)])
        report(out, {"what": "rotated", "rotate": rot, "mirror": mir, "reps": reps, "k_frontend_dev 64 x 1080p nv12": stats(us[(rot, mir)]),
                     "launch_ratio_to_unrotated": round(float(np.median(us[(rot, mir)]) / base_us), 3),
                     "host_nv12_pinned_frames_per_s": round(float(np.median(f)), 1),
                     "host_frames_per_s_min_max": [round(float(f.min()), 1), round(float(f.max()), 1)],
                     "host_ratio_to_unrotated": round(float(np.median(f) / base_fps), 3), "window": list(win),
                     "window_bytes": nbytes})
    ctx.close()


def main():
    out = []
    (plain if ARGS.mode == "plain" else rotated)(ARGS.reps, out)
    if ARGS.out:
        with open(ARGS.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
