"""Writes tests/golden/yuv_frontend_golden.npz: fixtures of the 4:2:0 front-end
computed by the numpy restatement tests/yuv_ref.py composed with the oracle's resize and luma, so that the appendix-Y
arithmetic is pinned independently of the restatement and the kernel (a change made to both alike still fails here).

Holds the known-answer table (Y, U, V) -> (B, G, R) and, per case, SHA-256 of the input frame and of the (h, w) gray
operand.  Data only: the inputs are regenerated from a seeded generator (yuv_ref.random_frame).

    python tests/gen_yuv_golden.py          (run from the repository root)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, os.path.join(ROOT, "oracle"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import yuv_ref  # noqa: E402

OUT = os.path.join(HERE, "golden", "yuv_frontend_golden.npz")

# (Y, U, V) -> (B, G, R): the answers appendix Y must give
KNOWN = [((16, 128, 128), (0, 0, 0)), ((0, 128, 128), (0, 0, 0)), ((235, 128, 128), (255, 255, 255)),
         ((126, 128, 128), (128, 128, 128)), ((81, 90, 240), (0, 0, 254)), ((145, 54, 34), (1, 255, 0)),
         ((41, 240, 110), (255, 0, 0)), ((255, 0, 255), (20, 225, 255))]

# (case name, layout, source w, h, row pitch (None: w), resize (w, h), crop (x, y), operand (w, h), seed)
CASES = [
    ("i420_640x360_256", "i420", 640, 360, None, (256, 256), (0, 0), (256, 256), 1),
    ("nv12_640x360_256", "nv12", 640, 360, None, (256, 256), (0, 0), (256, 256), 2),
    ("nv12_640x360_oddcrop", "nv12", 640, 360, None, (301, 283), (37, 19), (200, 160), 3),
    ("i420_512_area2", "i420", 512, 512, None, (256, 256), (0, 0), (256, 256), 4),
    ("nv12_256_identity", "nv12", 256, 256, None, (256, 256), (0, 0), (256, 256), 5),
    ("nv12_640x360_pitch704", "nv12", 640, 360, 704, (256, 256), (0, 0), (256, 256), 6),
    ("i420_1920x1080_vr", "i420", 1920, 1080, None, (512, 512), (0, 256), (256, 256), 7),
    ("i420_160x90_upscale", "i420", 160, 90, None, (256, 256), (0, 0), (256, 256), 8),
]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def case_frame(case):
    _, layout, w, h, pitch, _, _, _, seed = case
    return yuv_ref.random_frame(w, h, layout, seed, pitch)


def case_operand(case):
    _, layout, _, _, _, resize, crop, out, _ = case
    return yuv_ref.operand(case_frame(case), layout, resize, crop, out)


def main():
    names = np.array([c[0] for c in CASES])
    in_sha = np.array([sha(case_frame(c)) for c in CASES])
    op_sha = np.array([sha(case_operand(c)) for c in CASES])
    yuv = np.array([k[0] for k in KNOWN], np.uint8)
    bgr = np.array([k[1] for k in KNOWN], np.uint8)
    np.savez(OUT, names=names, input_sha256=in_sha, operand_sha256=op_sha, known_yuv=yuv, known_bgr=bgr)
    for n, a, b in zip(names, in_sha, op_sha):
        print(f"{n:28s} in {a[:16]}  operand {b[:16]}")
    print("wrote", OUT)


if __name__ == "__main__":
    main()
