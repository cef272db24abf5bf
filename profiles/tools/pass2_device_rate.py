"""Rate of one chunk through PairEngine.process_chunk with pass 2 on the host (the default: pass1_results, the +-6 window in
Python, ffl_radial per batch) and on the device (post_out=: ffl_radial_window behind every batch, one read per chunk;
DESIGN.md section 14), in one process, alternating, as the median of the repetitions after a warm-up:

  host      gray frames in host memory (Context.upload_frames)
  resident  the same frames as torch tensors on the device (frontend.DeviceUploader, "gray")

The interval is the host clock from the call to the moment the chunk's (dots, records) are in host memory, so the device
form includes its one device-to-host copy.  Both forms must give the same bits.

    python profiles/tools/pass2_device_rate.py [--size 256x256] [--batch 256] [--frames 3000] [--reps 3] [--out file.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="256x256")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--frames", type=int, default=3000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    w, h = (int(v) for v in a.size.split("x"))
    B, n = a.batch, a.frames - 1
    base = list(sine_translate_frames(min(a.frames, 64), w, h, seed=7))
    host = [base[i % len(base)] if (i // len(base)) % 2 == 0 else base[len(base) - 1 - i % len(base)] for i in range(a.frames)]
    resident = list(torch.from_numpy(np.stack(host)).to(DEV))
    ctx = _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2))
    engines = {"host": (pipeline.PairEngine(ctx), host),
               "resident": (pipeline.PairEngine(ctx, frontend.DeviceUploader(ctx, "gray")), resident)}

    def run(source, device_pass2):
        eng, frames = engines[source]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if device_pass2:
            dots, recs = pipeline.post_records(eng.process_chunk(frames, post_out=pipeline.post_buffer(ctx, n)), n)
        else:
            dots, recs = eng.process_chunk(frames)
        return time.perf_counter() - t0, np.asarray(dots, np.float64).tobytes(), recs

    out, want = [], None
    times = {(s, d): [] for s in engines for d in (False, True)}
    for r in range(a.reps + 1):                    # repetition 0 is the warm-up
        for key, v in times.items():
            dt, dots, recs = run(*key)
            want = want or (dots, recs)
            assert (dots, recs) == want, f"{key}: the chunk's scalars differ"
            if r:
                v.append(dt)
    for (source, device_pass2), v in times.items():
        med = float(np.median(v))
        rec = {"what": "process_chunk", "size": f"{w}x{h}", "batch": B, "pairs": n, "frames_from": source,
               "pass2": "device" if device_pass2 else "host", "median_s": round(med, 5), "pairs_per_s": round(n / med, 1),
               "all_s": [round(t, 5) for t in v], "reps": a.reps}
        print(json.dumps(rec), flush=True)
        out.append(rec)
    assert ctx.graph_stats()["capture_failures"] == 0
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
