"""Cost of the global-motion fit and compensation.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python profiles/motion_rate.py --kernels W H N [--calls 20]
    python profiles/motion_rate.py --stats DIR            # the kernels' mean durations out of rocprofv3's *_kernel_stats.csv
    python profiles/motion_rate.py --chunk W H B [--reps 3] [--rounds 20] [--out profiles/motion_chunk_rate.json]

--kernels is the workload of a profiler run of its own: N resident random fields of W x H, then `--calls` calls each of
motion_fit with one pass in its four forms ({no map, map} x {no prior, prior}), of the four-component radial_window_axes on
the same slots (k_strip_sums<RadialSums<4, 2, NoWeights>>, the yardstick of the fit), of motion_subtract in place and of
export_flows (the yardstick of the subtraction).  Every kernel form has a name of its own in the trace.  --chunk times
PairEngine.process_chunk() on a synthetic clip of 3 * B pairs against the same call with compensate="translation" at one and
three passes, alternating `--reps` times; a timed sample is `--rounds` runs of the chunk back to back and a device
synchronise, and the rate is pairs per second of that wall time.  Nothing runs on import."""
import argparse
import csv
import glob
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)

KERNELS = ("k_strip_sums", "k_motion_solve", "k_motion_subtract", "k_radial_final", "k_export_flows", "k_pass1")


def kernels(w, h, n, calls):
    import numpy as np
    import torch
    from funscript_flow_amd import _capi
    _capi.set_option("lanes", 1)
    rng = np.random.default_rng(7)
    dev = torch.device("cuda", 0)
    with _capi.Context(w, h, frame_slots=2, flow_slots=n, max_batch=n) as ctx:
        step = 8 if w * h > 256 * 256 else n
        for i0 in range(0, n, step):
            f = torch.from_numpy((rng.standard_normal((min(step, n - i0), h, w, 2)) * 2.5).astype(np.float32)).to(dev)
            ctx.import_flows(f, list(range(i0, min(i0 + step, n))))
        slots = list(range(n))
        maps = torch.from_numpy(rng.integers(0, 256, (n, h, w)).astype(np.uint8)).to(dev)
        prior = torch.from_numpy(np.tile([0.1, 0.0, 0.0, -0.1, 0.0, 0.0], (n, 1))).to(dev)
        models = torch.zeros((n, 6), dtype=torch.float64, device=dev)
        out = torch.empty(n * _capi.MOTION_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        recs = torch.empty(n * _capi.PASS2_AXES_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        dst = torch.empty((n, h, w, 2), dtype=torch.float32, device=dev)
        for _ in range(calls):
            for wts in (None, maps):
                for pr in (None, prior):
                    ctx.motion_fit(slots, "translation", 1, 1.0, weights=wts, prior=pr, out=out)
            ctx.radial_window_axes(slots, 0, n, recs, 6, 1e30, False)
            ctx.motion_subtract(slots, slots, models)
            ctx.export_flows(slots, dst)
        ctx.sync()
        torch.cuda.synchronize()


def stats(directory):
    """{kernel name: (calls, mean us)} of every kernel of KERNELS in the run's kernel-stats CSV"""
    rows = {}
    for path in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in KERNELS):
                rows[name] = (int(r["Calls"]), float(r["AverageNs"]) / 1e3)
    return rows


def chunk(w, h, B, reps, rounds, out):
    import numpy as np
    import torch  # noqa: F401  (first: its HIP runtime, same SONAME, is the one libffl_hip.so binds to)
    from funscript_flow_amd import _capi, pipeline
    from funscript_flow_amd.synth import sine_translate_frames
    n = 3 * B
    frames = list(sine_translate_frames(n + 1, w, h, seed=1))
    forms = [("plain", {}), ("translation_1", {"compensate": {"model": "translation", "iterations": 1}}),
             ("translation_3", {"compensate": {"model": "translation", "iterations": 3}})]
    rows = []
    with _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2)) as ctx:
        eng = pipeline.PairEngine(ctx)
        for _, kw in forms:   # warm-up: graphs captured, scratch allocated
            eng.process_chunk(frames, **kw)
        ctx.sync()
        for rep in range(reps):
            for name, kw in forms:
                t0 = time.perf_counter()
                for _ in range(rounds):
                    eng.process_chunk(frames, **kw)
                ctx.sync()
                dt = time.perf_counter() - t0
                rows.append({"form": name, "rep": rep, "w": w, "h": h, "B": B, "pairs": n * rounds, "seconds": dt,
                             "pairs_per_s": n * rounds / dt})
                print(json.dumps(rows[-1]), flush=True)
    med = {name: float(np.median([r["pairs_per_s"] for r in rows if r["form"] == name])) for name, _ in forms}
    summary = {"w": w, "h": h, "B": B, "pairs_per_chunk": n, "rounds": rounds, "median_pairs_per_s": med,
               "relative_to_plain": {k: v / med["plain"] for k, v in med.items()}}
    print(json.dumps(summary))
    if out:
        prev = json.load(open(out)) if os.path.exists(out) else []
        with open(out, "w") as f:
            json.dump(prev + [{"summary": summary, "runs": rows}], f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", nargs=3, type=int, metavar=("W", "H", "N"))
    ap.add_argument("--chunk", nargs=3, type=int, metavar=("W", "H", "B"))
    ap.add_argument("--stats", metavar="DIR")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.kernels:
        kernels(*a.kernels, a.calls)
    if a.stats:
        for name, (calls, us) in sorted(stats(a.stats).items()):
            print(f"{us:10.1f} us  x{calls:<5d} {name}")
    if a.chunk:
        chunk(*a.chunk, a.reps, a.rounds, a.out)


if __name__ == "__main__":
    main()
