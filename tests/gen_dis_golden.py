"""Writes tests/golden/dis_golden.npz: fixtures of the DIS path computed by the plain-C restatement (tests/dis_ref,
DESIGN.md appendix D), so that the appendix-D arithmetic is pinned independently of the restatement and the kernels
(a change that edits both identically still fails against these numbers).

Per case: SHA-256 of the input frames and of the full (H, W, 2) float32 flow, the pass-1 record (argmax x, y, its
divergence, mean magnitude), the radial scalar about a fixed centre (pov off / on), and for two cases the 64x64
finest-scale field after refinement.  Data only: the inputs are regenerated from funscript_flow_amd.synth.

    python tests/gen_dis_golden.py          (run from the repository root)
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

import dis_ref  # noqa: E402
import oracle as orc  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402

OUT = os.path.join(HERE, "golden", "dis_golden.npz")
FINEST = ("zoom", "blocks")   # cases whose finest-scale refined field is stored


def block_motion(w, h, seed):
    """frame 1 = frame 0 with every 8x8 block moved by its own integer offset (piecewise motion)"""
    rng = np.random.default_rng(seed)
    f0 = sine_translate_frames(1, w + 16, h + 16, seed=seed, amp=(0.0, 0.0))[0]
    f1 = np.empty((h, w), np.uint8)
    for by in range(0, h, 8):
        for bx in range(0, w, 8):
            dx, dy = rng.integers(-3, 4, 2)
            f1[by:by + 8, bx:bx + 8] = f0[8 + by + dy:16 + by + dy, 8 + bx + dx:16 + bx + dx]
    return f0[8:8 + h, 8:8 + w], f1


def contents(w, h):
    """(name, f0, f1): translation, 5 % zoom, 8x8 block motion, noise, constant, identical frames"""
    out = []
    t = sine_translate_frames(2, w, h, seed=1, amp=(3.0, 2.0))
    out.append(("translate", t[0], t[1]))
    z = sine_translate_frames(5, w, h, seed=2, amp=(0.0, 0.0), zoom=0.05, period=16)
    out.append(("zoom", z[0], z[4]))
    out.append(("blocks",) + block_motion(w, h, 3))
    rng = np.random.default_rng(4)
    out.append(("noise", rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)))
    c = np.full((h, w), 117, np.uint8)
    out.append(("constant", c, c.copy()))
    out.append(("identical", t[0], t[0].copy()))
    return [(n, np.ascontiguousarray(a), np.ascontiguousarray(b)) for n, a, b in out]


def cases():
    """(case name, f0, f1, parameter overrides): every 256x256 content with PRESET_FAST, the zoom pair with stripes 8 / 1
    and without refinement, and one 512x512 pair"""
    out = [(n, a, b, {}) for n, a, b in contents(256, 256)]
    z = dict((n, (a, b)) for n, a, b in contents(256, 256))["zoom"]
    out += [("zoom_stripes8", z[0], z[1], {"stripes": 8}), ("zoom_stripes1", z[0], z[1], {"stripes": 1}),
            ("zoom_novr", z[0], z[1], {"var_refine_iters": 0})]
    f = sine_translate_frames(2, 512, 512, seed=9, amp=(4.0, 3.0), zoom=0.03)
    out.append(("zoom512", np.ascontiguousarray(f[0]), np.ascontiguousarray(f[1]), {}))
    return out


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def center(w, h):
    return np.array([w * 0.51, h * 0.47])


def record(flow):
    """pass-1 record, radial (pov off, on) about center() -- the numbers the device must reproduce"""
    h, w, _ = flow.shape
    x, y, v = orc.max_divergence_np(flow)
    c = center(w, h)
    return (int(x), int(y), np.float32(v), np.float32(orc.mean_mag_np(flow)),
            [float(orc.radial_np(flow, c, False, pov)) for pov in (False, True)])


def main():
    names, params, fsha, insha, xy, div, mag, rad = [], [], [], [], [], [], [], []
    extra = {}
    for name, f0, f1, over in cases():
        p = dis_ref.fast_params(**over)
        if name in FINEST:
            flow, fin = dis_ref.flow(f0, f1, p, dbg=(2, dis_ref.STAGE_VR))
            extra["finest_" + name] = fin
        else:
            flow = dis_ref.flow(f0, f1, p)
        x, y, v, m, r = record(flow)
        names.append(name)
        params.append(json.dumps(over, sort_keys=True))
        fsha.append(sha(flow))
        insha.append(sha(f0) + sha(f1))
        xy.append((x, y))
        div.append(v)
        mag.append(m)
        rad.append(r)
        print(f"{name:14s} {json.dumps(over):24s} argmax ({x:3d},{y:3d}) mean_mag {float(m):.6f} radial {r[0]:+.6e}")
    np.savez_compressed(OUT, names=np.array(names), params=np.array(params), flow_sha256=np.array(fsha),
                        frames_sha256=np.array(insha), pass1_xy=np.array(xy, np.int32), pass1_div=np.array(div, np.float32),
                        pass1_mean_mag=np.array(mag, np.float32), radial=np.array(rad, np.float64), **extra)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
