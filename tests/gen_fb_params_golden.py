"""Writes tests/golden/fb_params_golden.npz: fixtures of Farneback with caller-chosen parameters computed by the plain-C
restatement (tests/fb_general_ref), so that the appendix-F arithmetic is pinned independently of the
restatement and the kernels (a change made to both alike still fails against these numbers).

Per case: SHA-256 of the input frames and of the full (H, W, 2) float32 flow, the pass-1 record (argmax x, y, its
divergence, mean magnitude) and the radial scalar about a fixed centre with pov off and on.  Data only: the inputs are
regenerated from funscript_flow_amd.synth.

    python tests/gen_fb_params_golden.py          (run from the repository root)
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fb_general_ref  # noqa: E402
import gen_dis_golden  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

OUT = os.path.join(HERE, "golden", "fb_params_golden.npz")

# (case name, width, height, parameter overrides with cv2's keyword names)
CASES = [
    ("defaults_256", 256, 256, {}),
    ("defaults_640", 640, 360, {}),
    ("levels5_1080p", 1920, 1080, {"levels": 5}),
    ("pyr07_levels6", 640, 360, {"pyr_scale": 0.7, "levels": 6}),
    ("winsize3", 256, 256, {"winsize": 3}),
    ("winsize31", 640, 360, {"winsize": 31}),
    ("polyn7_sigma15", 256, 256, {"poly_n": 7, "poly_sigma": 1.5}),
    ("iters1", 256, 256, {"iterations": 1}),
    ("iters6", 640, 360, {"iterations": 6}),
]


def frames(w, h, seed=11):
    """the case's pair: a textured frame and its translated, slightly zoomed successor"""
    f = sine_translate_frames(2, w, h, seed=seed, amp=(2.5, 1.5), period=7, zoom=0.02)
    return np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1])


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


record = gen_dis_golden.record   # pass-1 record + radial (pov off, on) about gen_dis_golden.center()


def main():
    names, params, fsha, insha, xy, div, mag, rad = [], [], [], [], [], [], [], []
    for name, w, h, over in CASES:
        f0, f1 = frames(w, h)
        flow = fb_general_ref.flow(f0, f1, over)
        x, y, v, m, r = record(flow)
        names.append(name)
        params.append(json.dumps(over, sort_keys=True))
        fsha.append(sha(flow))
        insha.append(sha(f0) + sha(f1))
        xy.append((x, y))
        div.append(v)
        mag.append(m)
        rad.append(r)
        print(f"{name:16s} {w}x{h} {json.dumps(over):36s} argmax ({x:4d},{y:4d}) mean_mag {float(m):.6f} radial {r[0]:+.6e}")
    np.savez_compressed(OUT, names=np.array(names), params=np.array(params), flow_sha256=np.array(fsha),
                        frames_sha256=np.array(insha), pass1_xy=np.array(xy, np.int32), pass1_div=np.array(div, np.float32),
                        pass1_mean_mag=np.array(mag, np.float32), radial=np.array(rad, np.float64))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
