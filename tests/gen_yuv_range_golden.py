"""Writes tests/golden/yuv_range_golden.npz: recorded answers of rule Y7 (full-range 4:2:0), so that
a change made alike in the numpy restatement (tests/front_orient.py) and in the kernel still fails a test.

    corners_yuv, corners_bgr        the eight (Y, U, V) in {0, 255}^3 and their B, G, R
    <layout>_frame / _bgr / _operand    one 8x8 ramp frame per layout, its (8, 8, 3) BGR and the 16x16 operand of its
                                        resize to 16x16

Run from the repository root:  python tests/gen_yuv_range_golden.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

import front_orient as fo   # noqa: E402
import front_sweep as fs    # noqa: E402

PATH = os.path.join(HERE, "golden", "yuv_range_golden.npz")


def golden():
    c = np.array([[(k & 1) * 255, (k >> 1 & 1) * 255, (k >> 2 & 1) * 255] for k in range(8)], np.uint8)
    d = {"corners_yuv": c, "corners_bgr": fo.yuv_to_bgr_full_pixels(c[:, 0], c[:, 1], c[:, 2])}
    for layout in ("i420", "nv12"):
        f = fs.yuv_frame("ramp", 8, 8, layout, 7)
        d[layout + "_frame"] = f
        d[layout + "_bgr"] = fo.yuv_to_bgr_full(f, layout)
        d[layout + "_operand"] = fo.full_operand(f, layout, (16, 16), (0, 0), (16, 16))
    return d


if __name__ == "__main__":
    np.savez(PATH, **golden())
    print(PATH, os.path.getsize(PATH), "bytes")
