"""GPU sweep of the 8-bit front-end at small shapes (k_frontend behind ffl_upload_frames_raw / ffl_upload_frames_yuv,
k_frontend_dev behind ffl_upload_frames_device; DESIGN.md sections 8, 11, 12) over the table of tests/front_sweep.py:
every resize mode, clamp and crop on contexts of 16x16, 17x19, 65x21 and 130x16 -- partial x- and y-tiles, odd sizes --
through every host path and, on the device path, one launch of five frames whose descriptors all differ.  Each operand
must equal the two-pass oracle AND the per-pixel restatement, bit for bit, and every slot a call does not write must keep
what it held.  One context per test; the references are computed once per output size (front_sweep's caches)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                      # before the library initialises the device: torch's HIP runtime comes first (as in test_gpu_device_io)
    import torch
except ImportError:
    torch = None

import front_sweep as fs
import yuv_ref
from funscript_flow_amd import _capi

OUT_IDS = [f"{w}x{h}" for w, h in fs.OUTS]
HOST_PATHS = ("raw_bgr_staged", "raw_bgr_pinned", "raw_rgb_order", "raw_wider_buffer", "i420_staged", "i420_zero_copy",
              "nv12_staged", "nv12_zero_copy", "nv12_padded_pitch")


class Slots:
    """what every frame slot of a context must hold: the pattern it was filled with, or the operand written since"""

    def __init__(self, ctx, out):
        self.ctx = ctx
        self.want = [fs.slot_pattern(s, out) for s in range(ctx.frame_slots)]
        ctx.upload_frames(0, self.want)

    def wrote(self, first, operands):
        for i, op in enumerate(operands):
            self.want[first + i] = op

    def check(self, what):
        for s, w in enumerate(self.want):
            got = self.ctx.download_frame(s)
            assert np.array_equal(got, w), (what, "slot", s, "first difference at", tuple(np.argwhere(got != w)[0]))


def pinned_copy(ctx, frames, size, pitch=None, channels=1, yuv=False):
    """the frames copied into one page-locked array of the context (the zero-copy placement of front_sweep)"""
    pin = ctx.pinned_frames(len(frames), channels=channels, size=(pitch or size[0], size[1]), yuv=yuv)
    assert pin.ctypes.data % 4 == 0                       # what front_sweep.yuv_direct's address arithmetic assumes
    pin[:, :, :size[0]] = np.stack(frames)
    return [pin[i, :, :size[0]] for i in range(len(frames))]


def wider(frames, pad):
    """the frames as views of buffers whose rows are `pad` elements longer, filled with other bytes"""
    out = []
    for f in frames:
        big = np.full((f.shape[0], f.shape[1] + pad) + f.shape[2:], 0x5A, np.uint8)
        lead = pad // 2 if f.ndim == 3 else 0              # a 4:2:0 array's rows start at its first column
        big[:, lead:lead + f.shape[1]] = f
        out.append(big[:, lead:lead + f.shape[1]])
    return out


@pytest.mark.parametrize("path", HOST_PATHS)
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_host_paths_bit_exact_and_neighbours_untouched(out, path):
    layout = path[:4] if path[:4] in yuv_ref.LAYOUTS else None
    rows = fs.yuv_cases(out, layout) if layout else fs.bgr_cases(out)
    took = {True: 0, False: 0}                            # zero-copy rows by the transfer path the rule gives them
    with _capi.Context(*out, max_batch=1, frame_slots=2 * len(rows) + 2) as ctx:
        slots = Slots(ctx, out)
        slots.check("the pattern itself")
        for k, row in enumerate(rows):
            name, src, rs, crop, frames = row[:5]
            first = 1 + 2 * k                             # slots 0 and the last one are never written
            if layout is None:
                want = row[6] if path == "raw_rgb_order" else row[5]
                if path == "raw_bgr_pinned":
                    frames = pinned_copy(ctx, frames, src, channels=3)
                elif path == "raw_wider_buffer":
                    frames = wider(frames, 5)
                    assert frames[0].strides[0] != 3 * src[0]
                ctx.upload_frames_raw(first, frames, rs, crop, rgb_order=path == "raw_rgb_order")
            else:
                want = row[5]
                if path.endswith("zero_copy"):
                    frames = pinned_copy(ctx, frames, src, yuv=True)
                    win = _capi.frontend_yuv_window(src, layout, rs, crop, out)[0]
                    d = [fs.yuv_direct(f.ctypes.data, src, layout, src[0], win) for f in frames]
                    assert d == [fs.yuv_direct(a, src, layout, src[0], win) for a in fs.zero_copy_addresses(src)]
                    took[all(d)] += 1
                elif path == "nv12_padded_pitch":
                    frames = wider(frames, 6)
                ctx.upload_frames_yuv(first, frames, layout, rs, crop)
            slots.wrote(first, want)
            if k + 1 == len(rows) or rows[k + 1][0] != name:
                slots.check((name, path))
        if path.endswith("zero_copy"):
            assert took[True] >= 1 and took[False] >= 1, took   # per size; test_front_sweep_host counts the whole table


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def junk(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def bgr_tensors(frames, seed):
    """five device views of five (h, w, 3) frames, no two described alike (a view keeps its tensor alive)"""
    h, w = frames[0].shape[:2]
    big = junk((h + 5, w + 7, 3), seed)
    big[2:2 + h, 3:3 + w] = frames[1]
    bgra = junk((h, w, 4), seed + 1)
    bgra[..., :3] = frames[2]
    batch = junk((3, h, w, 3), seed + 2)
    batch[1] = frames[4]
    t = [dev(frames[0]),                                  # contiguous
         dev(big)[2:2 + h, 3:3 + w],                      # a view of a wider and taller tensor
         dev(bgra),                                       # pixel stride 4
         dev(frames[3].transpose(2, 0, 1)),               # planar (3, h, w): channel stride = pitch * h
         dev(batch)[1]]                                   # a slice of a batched tensor
    rows, size = _capi.Context._device_rows(t, _capi.DEV_FORMATS["bgr"])
    assert size == (w, h) and len({(r[3], r[6], r[7]) for r in rows}) >= 4 and rows[3][7] == rows[3][3] * h
    assert rows[2][6] == 4 and rows[1][3] == 3 * (w + 7)
    return t


def yuv_rows(frames, layout, seed):
    """ffl_dev_frame rows of five 4:2:0 frames whose planes lie in separate allocations with pitches of their own: I420
    with pitch[1] != pitch[2] and the V pitch the larger, NV12 with a UV pitch that is not the Y pitch"""
    keep, rows = [], []
    for i, f in enumerate(frames):
        Y, U, V = yuv_ref.planes(f, layout)
        h, w = Y.shape
        yp = w + (0, 3, 16, 1, 7)[i]
        if layout == "nv12":
            planes, pitches = [Y, f[h:]], [yp, w + (5, 0, 2, 32, 1)[i]]
        else:
            up = w // 2 + (0, 1, 5, 2, 0)[i]
            planes, pitches = [Y, U, V], [yp, up, up + (4, 1, 3, 9, 2)[i]]
        t = []
        for p, pitch in zip(planes, pitches):
            buf = junk((p.shape[0], pitch), seed + 10 * i + len(t))
            buf[:, :p.shape[1]] = p
            t.append(dev(buf))
        keep += t
        ptrs = [x.data_ptr() for x in t] + [0] * (3 - len(t))
        rows.append(ptrs + pitches + [0] * (3 - len(t)) + [1, 0])
    return rows, keep


@pytest.mark.parametrize("fmt", ["bgr", "rgb", "i420", "nv12"])
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_device_path_five_descriptors_in_one_launch(out, fmt):
    if torch is None:
        pytest.skip("needs torch")
    yuv = fmt in yuv_ref.LAYOUTS
    rows = fs.yuv_cases(out, fmt, 5) if yuv else fs.bgr_cases(out, 5)
    with _capi.Context(*out, max_batch=1, frame_slots=13) as ctx:
        slots = Slots(ctx, out)
        for k, row in enumerate(rows):
            name, src, rs, crop, frames = row[:5]
            want = row[6] if fmt == "rgb" else row[5]
            assert len({w.tobytes() for w in want}) == 5      # no two operands alike: a launch that misplaces one shows
            d_first, h_first = (1, 7) if k % 2 == 0 else (7, 1)   # slots 0, 6 and 12 keep the pattern
            if yuv:
                desc, keep = yuv_rows(frames, fmt, 1000 * k)
                d = np.ascontiguousarray(desc, np.int64)
                ctx._chk(ctx.L.ffl_upload_frames_device(ctx._h, d_first, 5, d.ctypes.data, _capi.dev_format(fmt), src[0], src[1],
                                                        rs[0], rs[1], crop[0], crop[1], _capi.stream_handle(None, ctx.device)))
                ctx.upload_frames_yuv(h_first, frames, fmt, rs, crop)
            else:
                keep = bgr_tensors(frames, 1000 * k)
                ctx.upload_frames_device(d_first, keep, fmt, rs, crop)
                ctx.upload_frames_raw(h_first, frames, rs, crop, rgb_order=fmt == "rgb")
            for i in range(5):                                # the host path's slots hold the same bytes ...
                assert np.array_equal(ctx.download_frame(d_first + i), ctx.download_frame(h_first + i)), (name, crop, i)
            slots.wrote(d_first, want)
            slots.wrote(h_first, want)
            slots.check((name, crop, fmt))                    # ... and both hold the two restatements' operand, in order
            del keep


@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_device_gray_frames_pitch_and_pixel_stride(out):
    """gray frames of the context's size are copied as they are: contiguous, pitch-padded, and one channel of a packed
    tensor (pixel stride 3), all in one launch"""
    if torch is None:
        pytest.skip("needs torch")
    ow, oh = out
    with _capi.Context(*out, max_batch=1, frame_slots=9) as ctx:
        slots = Slots(ctx, out)
        for rnd in range(2):
            g = [junk((oh, ow), 10 * rnd + i) for i in range(3)]
            padded = junk((oh, ow + 9), 50 + rnd)
            padded[:, 4:4 + ow] = g[1]
            packed = junk((oh, ow, 3), 60 + rnd)
            packed[..., 1] = g[2]
            t = [dev(g[0]), dev(padded)[:, 4:4 + ow], dev(packed)[..., 1]]
            rows, _ = _capi.Context._device_rows(t, _capi.DEV_FORMATS["gray"])
            assert [(r[3], r[6]) for r in rows] == [(ow, 1), (ow + 9, 1), (3 * ow, 3)]
            order = [t[i] for i in ((0, 1, 2), (2, 0, 1))[rnd]]
            want = [g[i] for i in ((0, 1, 2), (2, 0, 1))[rnd]]
            d_first, h_first = ((1, 5), (5, 1))[rnd]          # slots 0, 4 and 8 keep the pattern
            ctx.upload_frames_device(d_first, order, "gray")
            ctx.upload_frames(h_first, want)
            slots.wrote(d_first, want)
            slots.wrote(h_first, want)
            slots.check(("gray", rnd))
