"""Rate of the radial pair of kernels with one and with four components.

    python profiles/axes_rate.py --out profiles/axes_rate.json [--parent-tree DIR] [--reps 3]

times ffl_radial and ffl_radial_axes on resident fields at 1920x1080 with n = 32 and at 256x256 with n = 256, each in a
process of its own (`--one`), with ffl_profile_read(FFL_K_RADIAL): device events around the pair of launches of every
call, after warm-up calls that are not counted.  The runs alternate, `--reps` times over, so that the spread of the same
measurement on the same box stands next to the differences.  `--parent-tree DIR` names a built checkout of another commit
(its funscript_flow_amd package is imported instead of this one): its ffl_radial is the yardstick for this tree's.
Nothing runs on import.
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1920, 1080, 32), (256, 256, 256)]


def one(tree, call, w, h, n, calls, warmup):
    """a single measurement in this process: ms per call of the FFL_K_RADIAL class"""
    sys.path.insert(0, tree)
    import numpy as np
    import torch
    from funscript_flow_amd import _capi
    _capi.set_option("lanes", 1)
    rng = np.random.default_rng(7)
    with _capi.Context(w, h, frame_slots=2, flow_slots=n, max_batch=n) as ctx:
        step = 8 if w * h > 256 * 256 else n
        for i0 in range(0, n, step):
            f = torch.from_numpy((rng.standard_normal((min(step, n - i0), h, w, 2)) * 2.5).astype(np.float32)).to(f"cuda:{ctx.device}")
            ctx.import_flows(f, list(range(i0, min(i0 + step, n))))
        ctx.sync()
        slots, cen, cut = list(range(n)), [(0.47 * w + 0.3, 0.46 * h + 0.7)] * n, [False] * n
        fn = getattr(ctx, call)
        for _ in range(warmup):
            fn(slots, cen, cut, False)
        ctx.profile_enable(["k_radial"])
        for _ in range(calls):
            out = fn(slots, cen, cut, False)
        launches, ms = ctx.profile_read()["k_radial"]
        assert launches == calls, (launches, calls)
        return {"call": call, "w": w, "h": h, "n": n, "calls": calls, "ms_per_call": ms / launches,
                "GB_per_s": 8.0 * w * h * n / (ms / launches * 1e-3) / 1e9, "first": float(np.asarray(out).ravel()[0])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--one", nargs=5, metavar=("TREE", "CALL", "W", "H", "N"))
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--parent-tree")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.one:
        tree, call, w, h, n = a.one
        print(json.dumps(one(tree, call, int(w), int(h), int(n), a.calls, a.warmup)))
        return
    runs = [("parent", a.parent_tree, "radial")] if a.parent_tree else []
    runs += [("this", HERE, "radial"), ("this", HERE, "radial_axes")]
    rows = []
    for w, h, n in SHAPES:
        for rep in range(a.reps):
            for who, tree, call in runs:   # alternating: parent, this, four components, parent, ...
                cmd = [sys.executable, os.path.abspath(__file__), "--one", tree, call, str(w), str(h), str(n), "--calls", str(a.calls),
                       "--warmup", str(a.warmup)]
                p = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:      # nothing more is started after a failure
                    sys.stderr.write(p.stdout + p.stderr)
                    sys.exit(f"axes_rate: {who} {call} {w}x{h} n={n} ended with status {p.returncode}")
                row = dict(json.loads(p.stdout.strip().splitlines()[-1]), tree=who, rep=rep)
                rows.append(row)
                print(json.dumps(row), flush=True)
    summary = []
    for w, h, n in SHAPES:
        s = {"w": w, "h": h, "n": n}
        for who, _, call in runs:
            v = sorted(r["ms_per_call"] for r in rows if (r["tree"], r["call"], r["w"], r["n"]) == (who, call, w, n))
            s[f"{who}_{call}_ms"] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1], "spread_pct": 100.0 * (v[-1] - v[0]) / v[len(v) // 2]}
        s["axes_over_radial"] = s["this_radial_axes_ms"]["median"] / s["this_radial_ms"]["median"]
        if a.parent_tree:
            s["this_over_parent_radial"] = s["this_radial_ms"]["median"] / s["parent_radial_ms"]["median"]
        summary.append(s)
    result = {"calls_per_run": a.calls, "warmup_calls": a.warmup, "reps": a.reps, "summary": summary, "runs": rows}
    print(json.dumps(result["summary"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
