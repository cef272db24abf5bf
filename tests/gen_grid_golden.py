"""Writes tests/golden/grid_golden.npz: the centres the reference's own center_of_mass_variance (FF:721-746, imported
through oracle/ref_loader.py) returns on the closed-form fields of tests/grid_ref.py, so that rules G2-G5 (DESIGN.md
section 17) are pinned against the real function and not against their own restatement.

Per case of grid_ref.GOLDEN_CASES: the (cx, cy) of the real function.  One constant field: the (w // 2, h // 2) default.
And the largest distance between the restatement's centre and the real function's over the cases, as measured when the
file was written.  Outputs only: the fields are regenerated from grid_ref.field, so the file is a few hundred bytes.

    python tests/gen_grid_golden.py          (run from the repository root, where the reference exists)
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import grid_ref as gr  # noqa: E402
from ref_loader import load_reference  # noqa: E402

OUT = os.path.join(HERE, "golden", "grid_golden.npz")
CONSTANT = (80, 48, 8)   # (w, h, G) of the constant field


def main():
    ref = load_reference()
    cases = np.array(gr.GOLDEN_CASES, np.int32)
    centres = np.empty((len(cases), 2), np.float64)
    worst = 0.0
    for k, (w, h, G) in enumerate(gr.GOLDEN_CASES):
        f = gr.field(w, h, seed=k)
        cx, cy = ref.center_of_mass_variance(f, num_cells=G)
        centres[k] = (float(cx), float(cy))
        mx, my, _, empty = gr.centre(f, G)
        dist = float(np.hypot(mx - centres[k, 0], my - centres[k, 1]))
        worst = max(worst, dist)
        print(f"{w}x{h} G={G}: reference ({centres[k, 0]!r}, {centres[k, 1]!r})  restatement distance {dist:.3e} px  empty={empty}")
    w, h, G = CONSTANT
    const = np.empty((h, w, 2), np.float32)
    const[..., 0], const[..., 1] = np.float32(1.25), np.float32(-0.75)
    cc = ref.center_of_mass_variance(const, num_cells=G)
    print(f"constant {w}x{h} G={G}: reference {cc}, restatement {gr.centre(const, G)}")
    np.savez(OUT, cases=cases, centres=centres, constant_case=np.array(CONSTANT, np.int32),
             constant_centre=np.array([float(cc[0]), float(cc[1])], np.float64), max_distance=np.float64(worst))
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); largest distance {worst:.3e} px (bound {gr.CENTRE_BOUND})")


if __name__ == "__main__":
    main()
