"""numpy restatement of DESIGN.md appendix Y, rule Y5: a 4:2:0 frame of uint16 samples (9 to 16 significant bits, low- or
high-aligned) is reduced to 8 bits sample by sample -- round half up with saturation, defined for every 16-bit pattern --

    s  = raw >> (16 - depth) if msb_aligned else raw
    v8 = min(255, (s + (1 << (depth - 9))) >> (depth - 8))

and is then the uint8 frame of the same layout: operand() is yuv_ref.operand() of it."""
import numpy as np

import yuv_ref


def default_msb(layout):
    """where decoders put the bits: high in P010 / P016 ("nv12"), low in yuv420p10le ("i420")"""
    return layout == "nv12"


def reduce8(raw, depth, msb_aligned):
    """rule Y5 on an integer array of 16-bit patterns -> uint8"""
    if not 9 <= depth <= 16:
        raise ValueError(depth)
    s = np.asarray(raw).astype(np.int64)
    if s.min(initial=0) < 0 or s.max(initial=0) > 0xFFFF:
        raise ValueError("not 16-bit patterns")
    if msb_aligned:
        s = s >> (16 - depth)
    return np.minimum(255, (s + (1 << (depth - 9))) >> (depth - 8)).astype(np.uint8)


def operand(frame, layout, depth, msb_aligned, resize, crop=(0, 0), out_size=(256, 256)):
    """the gray operand of ffl_upload_frames_yuv16(frame, layout, depth, msb_aligned, resize, crop) on an out_size context"""
    return yuv_ref.operand(reduce8(frame, depth, msb_aligned), layout, resize, crop, out_size)


def widen(frame8, depth, msb_aligned):
    """a uint8 frame as the depth-bit frame whose samples are v << (depth - 8): rule Y5 takes it back to frame8"""
    f = frame8.astype(np.uint16) << (depth - 8)
    return (f << (16 - depth)).astype(np.uint16) if msb_aligned else f


def random_frame(w, h, depth, msb_aligned, seed, pitch=None, junk=False):
    """a random (3h/2, w) uint16 4:2:0 frame of depth-bit samples; pitch > w (samples; NV12 only): a view of a wider
    buffer.  junk=True: every 16-bit pattern -- low-aligned samples beyond 2^depth (which saturate), high-aligned ones
    with random bits below the sample (which are ignored)."""
    rng = np.random.default_rng(seed)
    shape = (h * 3 // 2, pitch or w)
    if junk:
        f = rng.integers(0, 1 << 16, shape, dtype=np.uint16)
    else:
        f = rng.integers(0, 1 << depth, shape, dtype=np.uint16)
        if msb_aligned:
            f = (f << (16 - depth)).astype(np.uint16)
    return f[:, :w]
