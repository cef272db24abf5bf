"""Rates of ffl_import_flows, timed with HIP events on the caller's stream in one process, after a
warm-up, as the median of interleaved repetitions:

  import  ms per Context.import_flows call for 256 fields at 256x256 and 32 at 1080p, float32 NHWC, float32 NCHW and
          float16 NHWC (k_import_pass1: conversion + pass 1 in one read).  The call makes the caller's stream wait for
          the import, so the interval ends when the slots and records are complete.  Bytes moved: the source once + the
          slot written; the share is of the 6.3 TB/s copy ceiling of DESIGN.md section 12.
  host    the route without the import for the same float32 NHWC fields: download to host memory, one upload_flow per
          field, then the records (host clock around work that ends in a device synchronise)

    python profiles/tools/flow_import_rate.py [--reps 5] [--out file.json]
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
from funscript_flow_amd import _capi  # noqa: E402

DEV = torch.device("cuda", 0)
CEILING = 6.3e12   # bytes/s, DESIGN.md section 12


def timed(fn):
    """ms between an event before fn() and one after it on torch's current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    g = torch.Generator(device=DEV).manual_seed(3)
    for w, h, n in [(256, 256, 256), (1920, 1080, 32)]:
        ctx = _capi.Context(w, h, max_batch=n, frame_slots=2, flow_slots=n)
        f32 = torch.randn((n, h, w, 2), device=DEV, generator=g) * 3
        srcs = {"f32_nhwc": f32, "f32_nchw": f32.permute(0, 3, 1, 2).contiguous(), "f16_nhwc": f32.half()}
        slots = list(range(n))
        want = None
        ms = {k: [] for k in srcs}
        for r in range(a.reps + 1):           # repetition 0 is the warm-up
            for k, v in ms.items():
                t = timed(lambda: ctx.import_flows(srcs[k], slots))
                if k == "f32_nhwc":
                    recs = ctx.pass1_results(slots)
                    want = want or recs
                    assert recs == want, "imports differ"
                if r:
                    v.append(t)
        for k, v in ms.items():
            med = float(np.median(v))
            src_b = 4 if k.startswith("f16") else 8
            moved = n * w * h * (src_b + 8)
            rec = {"what": "import", "size": f"{w}x{h}", "fields": n, "source": k,
                   "form": "fused", "median_ms": round(med, 4),
                   "bytes_moved": moved, "GBps": round(moved / med / 1e6, 1),
                   "share_of_copy_ceiling": round(moved / med * 1e3 / CEILING, 3), "reps": a.reps}
            print(json.dumps(rec), flush=True)
            out.append(rec)
        host_s = []
        for r in range(a.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fields = f32.cpu().numpy()
            for j in slots:
                ctx.upload_flow(j, fields[j])
            recs = ctx.pass1_results(slots)
            dt = time.perf_counter() - t0
            assert recs == want, "upload_flow records differ from the import's"
            if r:
                host_s.append(dt)
        med = float(np.median(host_s)) * 1e3
        rec = {"what": "host_route", "size": f"{w}x{h}", "fields": n, "source": "f32_nhwc",
               "median_ms": round(med, 3), "reps": a.reps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
        ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
