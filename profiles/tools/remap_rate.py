"""Measurements of the map-driven front-end.

  kernels  for `rocprofv3 --kernel-trace`: one k_frontend_dev launch in generic mode and one k_frontend_remap_dev launch at
           supersample 1, 2, 4 of the same 64 device NV12 frames into 256x256, alternated --reps times, for 1080p frames (a 90
           degree view of the whole frame as one equirectangular eye) and 5760x2880 frames (the crop path in vr_mode, FF:1076-
           1079; the map a 90 degree view of the left eye).  Writes the launch plan (--plan): dispatch i of a k_frontend* kernel
           in the trace is entry i of the plan.
  summary  the kernel trace CSV + the plan -> one line per case: median / min / max us, bytes per output pixel
  rate     frames/s, H2D included, of 5760x2880 NV12 host frames out of ffl_host_alloc memory into 256x256: the 90 degree
           view of the left eye at supersample 2 against the vr_mode crop path, alternated in one process (host clock around
           the upload calls and ctx.sync()); reports the bytes each transfers per frame.  One JSON line per round.

    python profiles/tools/remap_rate.py kernels --plan P.json [--reps 10]
    python profiles/tools/remap_rate.py summary --plan P.json --trace T_kernel_trace.csv
    python profiles/tools/remap_rate.py rate [--rounds 7] [--frames 8] [--out file.jsonl]
"""
import argparse
import csv
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["kernels", "summary", "rate"])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--plan", default=None)
ap.add_argument("--trace", default=None)
ap.add_argument("--out", default=None)
ARGS = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

OUT = (256, 256)
# bytes an output pixel loads: generic mode 4 taps x (Y + U + V); a map entry (8) + 4 taps x 3 per sample; 1 byte stored
BYTES = {"generic": 12 + 1, 1: 20 + 1, 2: 80 + 1, 4: 320 + 1}


def kernels():
    import torch
    from funscript_flow_amd import _capi, frontend
    dev, n = torch.device("cuda", 0), 64
    g = torch.Generator(device=dev).manual_seed(1)
    plan = []
    ctx = _capi.Context(*OUT, max_batch=1, frame_slots=n)
    for name, (w, h), vr, stereo in (("1080p", (1920, 1080), False, None), ("5760x2880", (5760, 2880), True, "sbs")):
        frames = torch.randint(0, 256, (n, h * 3 // 2, w), dtype=torch.uint8, device=dev, generator=g)
        resize, crop = frontend.geometry(*OUT, vr)
        maps = {S: ctx.remap_create(frontend.view_map((w, h), OUT, "equirect", 90, rect=frontend.eye_rect((w, h), stereo, "left"),
                                                      supersample=S), (w, h), S) for S in (1, 2, 4)}
        for r in range(ARGS.reps + 2):                       # the first two rounds are warm-up
            ctx.upload_frames_device(0, frames, "nv12", resize, crop)
            plan.append((f"{name} k_frontend_dev generic", "generic", r >= 2))
            for S, m in maps.items():
                ctx.upload_frames_device_remap(0, frames, "nv12", m)
                plan.append((f"{name} k_frontend_remap_dev S={S}", S, r >= 2))
        ctx.sync()
        for m in maps.values():
            ctx.remap_destroy(m)
        del frames
    ctx.close()
    json.dump(plan, open(ARGS.plan, "w"))


def summary():
    plan = json.load(open(ARGS.plan))
    rows = [r for r in csv.DictReader(open(ARGS.trace)) if "k_frontend" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == len(plan), (len(rows), len(plan))
    us = {}
    for (label, key, timed), r in zip(plan, rows):
        assert ("remap" in r["Kernel_Name"]) == (key != "generic"), (label, r["Kernel_Name"])
        if timed:
            us.setdefault((label, key), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    for (label, key), v in us.items():
        v = np.asarray(v)
        b = BYTES["generic" if key == "generic" else int(key)]
        print(f"{label:40s} 64 frames  median {np.median(v):8.2f} us  min {v.min():8.2f}  max {v.max():8.2f}  n {len(v):3d}  "
              f"{b:4d} B/output px  {b * OUT[0] * OUT[1] * 64 / np.median(v) / 1e3:7.1f} GB/s")


def rate():
    from funscript_flow_amd import _capi, frontend
    src, n = (5760, 2880), ARGS.frames
    ctx = _capi.Context(*OUT, max_batch=1, frame_slots=n)
    pin = ctx.pinned_frames(n, size=src, yuv=True)
    pin[:] = np.random.default_rng(3).integers(0, 256, pin.shape[1:], dtype=np.uint8)[None]
    frames = [pin[i] for i in range(n)]
    S = 2
    m = frontend.view_map(src, OUT, "equirect", 90, rect=frontend.eye_rect(src, "sbs", "left"), supersample=S)
    remap = ctx.remap_create(m, src, S)
    resize, crop = frontend.geometry(*OUT, True)
    win_v = _capi.remap_check(m, OUT, src, S)[1]
    win_c, bytes_c = _capi.frontend_yuv_window(src, "nv12", resize, crop, OUT)
    cases = {"view 90 deg left eye S=2 (ffl_upload_frames_remap)": (lambda: ctx.upload_frames_remap(0, frames, remap, "nv12"),
                                                                  win_v, win_v[2] * win_v[3] * 3 // 2),
             "vr_mode crop (ffl_upload_frames_yuv)": (lambda: ctx.upload_frames_yuv(0, frames, "nv12", resize, crop), win_c, bytes_c)}
    out = open(ARGS.out, "a") if ARGS.out else None
    for r in range(ARGS.rounds + 1):                         # round 0 is warm-up
        for name, (fn, win, nbytes) in cases.items():
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(4):
                fn()
            ctx.sync()
            dt = (time.perf_counter() - t0) / (4 * n)
            if r:
                rec = {"what": "remap_frontend_rate", "case": name, "round": r, "source": "5760x2880 nv12, ffl_host_alloc", "out": "256x256",
                       "frames_per_s": round(1 / dt, 1), "window": list(win), "bytes_per_frame": int(nbytes),
                       "full_frame_bytes": src[0] * src[1] * 3 // 2, "h2d_GBps": round(nbytes / dt / 1e9, 2)}
                print(json.dumps(rec), flush=True)
                if out:
                    out.write(json.dumps(rec) + "\n")
    ctx.close()


{"kernels": kernels, "summary": summary, "rate": rate}[ARGS.mode]()
