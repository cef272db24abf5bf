"""Stripe sensitivity of the DIS path, measured on the C restatement (tests/dis_ref; no GPU).  The reference's DNN output
depends on the host's OpenCV thread count through DIS's stripes; this bounds how much.  For stripes
8 and 1 against the default 0 (one patch row per stripe, any host with >= 15 threads at 256x256), per clip:
  * argmax moved: pairs whose max_divergence position differs
  * radial change: |r_k - r_0| per pair through the reference's chain (each variant's own argmax centres smoothed over
    +-6 pairs, cut = mean magnitude > 7), as a fraction of the clip's median non-zero |r_0|: median and max over the pairs
python profiles/tools/dis_stripe_sensitivity.py > profiles/r05_dis_stripe_sensitivity.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import dis_ref  # noqa: E402
import gen_dis_golden  # noqa: E402
import oracle as orc  # noqa: E402
from funscript_flow_amd import pipeline  # noqa: E402
from funscript_flow_amd.synth import sine_translate_frames  # noqa: E402


def clips():
    out = [("6 test contents, 256x256 (unrelated pairs: own argmax centre, no smoothing)",
            [(a, b) for _, a, b in gen_dis_golden.contents(256, 256)], False)]
    z = sine_translate_frames(600, 256, 256, seed=13, amp=(2.0, 1.5), zoom=0.04, period=24)
    out.append(("zoom clip, 600 frames 256x256", list(zip(z[:-1], z[1:])), True))
    t = sine_translate_frames(200, 256, 256, seed=14, amp=(4.0, 3.0), period=32)
    out.append(("translate clip, 200 frames 256x256", list(zip(t[:-1], t[1:])), True))
    return out


def chain(pairs, stripes, smooth):
    xy, dots = [], []
    flows = [dis_ref.flow(a, b, dis_ref.fast_params(stripes=stripes)) for a, b in pairs]
    recs = [(orc.max_divergence_np(f)[:2], float(orc.mean_mag_np(f)) > 7.0) for f in flows]
    pos = np.array([r[0] for r in recs])
    cen = pipeline.smooth_centers(pos) if smooth else pos.astype(np.float64)
    for f, (pos, cut), c in zip(flows, recs, cen):
        xy.append(pos)
        dots.append(0.0 if cut else float(orc.radial_np(f, c, False, False)))
    return xy, np.array(dots)


def main():
    print("| clip | stripes | argmax moved | radial change / median non-zero abs(r0): median | max |")
    print("|---|---|---|---|---|")
    for name, pairs, smooth in clips():
        xy0, r0 = chain(pairs, 0, smooth)
        nz = np.abs(r0[r0 != 0])   # constant / identical pairs have r = 0 under every stripe count
        scale = float(np.median(nz)) if len(nz) else 1.0
        for k in (8, 1):
            xy, r = chain(pairs, k, smooth)
            moved = sum(a != b for a, b in zip(xy, xy0))
            d = np.abs(r - r0) / scale
            print(f"| {name} | {k} | {moved} / {len(pairs)} | {np.median(d):.2e} | {d.max():.2e} |", flush=True)


if __name__ == "__main__":
    main()
