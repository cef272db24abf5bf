"""Writes tests/golden/param_sweep_golden.npz: fixtures of the two parameterised flow paths at the corners of their declared
domain (tests/param_domain.py), computed by the plain-C restatements (tests/dis_ref, tests/fb_general_ref), so that the
appendix-D and appendix-F arithmetic is pinned there independently of the restatements and the kernels (a change made to
both alike still fails against these numbers).

One DIS entry per DIS_SIZES size at PRESET_FAST, one general-Farneback entry per FB_PARAMS set at 130x66.  Per entry: the
case name, the parameter overrides as JSON, SHA-256 of the input frames and of the full (H, W, 2) float32 flow, the pass-1
record (argmax x, y, its divergence, mean magnitude) and the radial scalar about a fixed centre with pov off and on.  Data
only: the inputs are regenerated from funscript_flow_amd.synth.

    python tests/gen_param_sweep_golden.py          (run from the repository root)
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import dis_ref  # noqa: E402
import fb_general_ref  # noqa: E402
import gen_dis_golden  # noqa: E402
import param_domain as pd  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

OUT = os.path.join(HERE, "golden", "param_sweep_golden.npz")
FB_SIZE = (130, 66)

sha = gen_dis_golden.sha
record = gen_dis_golden.record   # pass-1 record + radial (pov off, on) about gen_dis_golden.center()


def dis_frames(w, h):
    """a translating, 3 % zooming textured pair, seeded from the size"""
    f = sine_translate_frames(2, w, h, seed=w * 31 + h, amp=(3.0, 2.0), zoom=0.03)
    return np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])


def cases():
    """(case name, algorithm, width, height, overrides)"""
    out = [(f"dis_{w}x{h}", "dis", w, h, {}) for w, h in pd.DIS_SIZES]
    out += [(f"fb_{name}", "farneback", *FB_SIZE, over) for name, over in pd.FB_PARAMS]
    return out


def compute(algo, w, h, over):
    """(f0, f1, the restatement's flow)"""
    if algo == "dis":
        f0, f1 = dis_frames(w, h)
        return f0, f1, dis_ref.flow(f0, f1, dis_ref.fast_params(**over))
    f0, f1 = pd.fb_frames(w, h, 2)
    return f0, f1, fb_general_ref.flow(f0, f1, over)


def entries():
    """the fixture's arrays, recomputed"""
    names, params, fsha, insha, xy, div, mag, rad = [], [], [], [], [], [], [], []
    for name, algo, w, h, over in cases():
        f0, f1, flow = compute(algo, w, h, over)
        x, y, v, m, r = record(flow)
        names.append(name)
        params.append(json.dumps(over, sort_keys=True))
        fsha.append(sha(flow))
        insha.append(sha(f0) + sha(f1))
        xy.append((x, y))
        div.append(v)
        mag.append(m)
        rad.append(r)
    return dict(names=np.array(names), params=np.array(params), flow_sha256=np.array(fsha), frames_sha256=np.array(insha),
                pass1_xy=np.array(xy, np.int32), pass1_div=np.array(div, np.float32), pass1_mean_mag=np.array(mag, np.float32),
                radial=np.array(rad, np.float64))


def main():
    e = entries()
    for i, n in enumerate(e["names"]):
        print(f"{n:36s} {e['params'][i]:70s} argmax ({e['pass1_xy'][i][0]:4d},{e['pass1_xy'][i][1]:4d}) "
              f"mean_mag {float(e['pass1_mean_mag'][i]):.6f} radial {e['radial'][i][0]:+.6e}")
    np.savez_compressed(OUT, **e)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
