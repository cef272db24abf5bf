"""Rates of device-memory I/O, timed with HIP events in one process, repetitions interleaved:

  ingest  frames/s of ffl_upload_frames_device from torch tensors into a 256x256 context, 64 frames per call: 1080p BGR,
          4K BGR, 5760x2880 NV12 VR, and that VR source as P010 (uint16, depth 10: ffl_upload_frames_device16) (event on the caller's stream before the call, and after it -- the call makes that
          stream wait for the ingest, so the interval ends when the frames are in their slots)
  export  GB/s of ffl_export_flows (bytes read + written) for 256 flows at 256x256 and 32 at 1080p, NHWC and NCHW
  chain   pairs/s of PairEngine.process_chunk at 256x256, B = 256, from device-resident gray frames (DeviceUploader)
          against the same frames uploaded from host memory (host clock; process_chunk returns its results)

    python profiles/tools/device_io_rate.py [--reps 5] [--chain-frames 2049] [--out file.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from funscript_flow_amd import _capi, frontend, pipeline  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

DEV = torch.device("cuda", 0)


def timed(fn):
    """ms between an event before fn() and one after it on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def ingest(reps, out):
    n = 64
    g = torch.Generator(device=DEV).manual_seed(1)
    srcs = [("1920x1080 bgr", "bgr", (n, 1080, 1920, 3), False), ("3840x2160 bgr", "bgr", (n, 2160, 3840, 3), False),
            ("5760x2880 nv12 vr", "nv12", (n, 4320, 5760), True), ("5760x2880 p010 vr", "nv12", (n, 4320, 5760), True)]
    ctx = _capi.Context(256, 256, max_batch=1, frame_slots=n)
    data = {name: torch.randint(0, 256, shape, dtype=torch.uint8, device=DEV, generator=g) for name, _, shape, _ in srcs}
    deep = {"5760x2880 p010 vr": {"depth": 10}}
    for name in deep:   # ten random bits, high in the 16
        data[name] = torch.randint(-32768, 32768, data[name].shape, dtype=torch.int16, device=DEV, generator=g).bitwise_and_(-64).view(torch.uint16)
    ms = {name: [] for name, *_ in srcs}
    for r in range(reps + 1):
        for name, fmt, shape, vr in srcs:
            resize, crop = frontend.geometry(256, 256, vr)
            t = timed(lambda: ctx.upload_frames_device(0, data[name], fmt, resize, crop, **deep.get(name, {})))
            if r:
                ms[name].append(t)
    for name, *_ in srcs:
        med = float(np.median(ms[name]))
        rec = {"what": "ingest", "source": name, "frames_per_call": n, "median_ms_per_call": round(med, 4),
               "frames_per_s": round(n / med * 1e3, 1), "us_per_frame": round(med * 1e3 / n, 3), "reps": reps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()


def export(reps, out):
    cases = [(256, 256, 256), (1920, 1080, 32)]
    ctxs = {}
    for w, h, n in cases:
        ctx = _capi.Context(w, h, max_batch=n, frame_slots=n + 1, flow_slots=n)
        ctx.upload_frames(0, list(sine_translate_frames(n + 1, w, h, seed=2)))
        ctx.flow_pairs(list(range(n)), list(range(1, n + 1)), list(range(n)))
        ctx.sync()
        ctxs[(w, h)] = ctx
    bufs = {(w, h, lay): torch.empty((n, h, w, 2) if lay == "nhwc" else (n, 2, h, w), dtype=torch.float32, device=DEV)
            for w, h, n in cases for lay in ("nhwc", "nchw")}
    ms = {k: [] for k in bufs}
    for r in range(reps + 1):
        for (w, h, lay), buf in bufs.items():
            n = buf.shape[0]
            t = timed(lambda: ctxs[(w, h)].export_flows(list(range(n)), buf, lay))
            if r:
                ms[(w, h, lay)].append(t)
    for (w, h, lay), v in ms.items():
        n = bufs[(w, h, lay)].shape[0]
        med = float(np.median(v))
        moved = 2 * n * w * h * 8
        rec = {"what": "export", "size": f"{w}x{h}", "flows": n, "layout": lay, "median_ms": round(med, 4),
               "GBps_read_plus_write": round(moved / med / 1e6, 1), "reps": reps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    for c in ctxs.values():
        c.close()


def chain(reps, n_frames, out):
    B = 256
    fr = sine_translate_frames(n_frames, 256, 256, seed=5)
    host = list(fr)
    dev = torch.from_numpy(fr).to(DEV)
    fs, fl = pipeline.min_frame_slots(B, 2), pipeline.min_flow_slots(B, 2)
    ctx = _capi.Context(256, 256, max_batch=B, frame_slots=fs, flow_slots=fl)
    eng = {"device": pipeline.PairEngine(ctx, frontend.DeviceUploader(ctx, "gray")), "host": pipeline.PairEngine(ctx)}
    frames = {"device": dev, "host": host}
    dt = {k: [] for k in eng}
    ref = None
    for r in range(reps + 1):
        for k in ("device", "host"):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dots, recs = eng[k].process_chunk(frames[k])
            dt[k].append(time.perf_counter() - t0)
            if ref is None:
                ref = (dots, recs)
            assert recs == ref[1] and np.array_equal(dots, ref[0]), "device and host chains differ"
    for k, v in dt.items():
        med = float(np.median(v[1:]))
        rec = {"what": "chain", "frames": k, "size": "256x256", "batch": B, "pairs": n_frames - 1,
               "pairs_per_s": round((n_frames - 1) / med, 1), "median_s": round(med, 5), "reps": reps,
               "capture_failures": ctx.graph_stats()["capture_failures"]}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain-frames", type=int, default=2049)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    ingest(a.reps, out)
    export(a.reps, out)
    chain(a.reps, a.chain_frames, out)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
