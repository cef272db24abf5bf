"""Host side of the high-bit-depth 4:2:0 front-end (DESIGN.md section 11, appendix Y rule Y5; no GPU): the rule's known
answers, `v << (depth - 8)` reducing to v, the source window of ffl_frontend_yuv16_window against the 8-bit window and
every sample the restatement reads, every refusal with its rule's words, the prefetch ring with uint16 slots against a
fake capture, and the Python refusals."""
import ctypes as C
import time

import numpy as np
import pytest

import yuv16_ref
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline, prefetch
from test_frontend_yuv_host import GEOMS


def test_rule_known_answers():
    for raw, v8 in [(64, 16), (65, 16), (66, 17), (940, 235), (942, 236), (1021, 255), (1023, 255)]:
        assert int(yuv16_ref.reduce8(np.array([raw]), 10, False)[0]) == v8, raw
    for raw, v8 in [(64 << 6, 16), ((66 << 6) | 63, 17)]:                     # P010
        assert int(yuv16_ref.reduce8(np.array([raw]), 10, True)[0]) == v8, raw
    # a low-aligned sample at or above 2^depth saturates; the bits below a high-aligned sample are ignored
    assert list(yuv16_ref.reduce8(np.array([1024, 4096, 65535]), 10, False)) == [255, 255, 255]
    assert list(yuv16_ref.reduce8(np.array([(65 << 6) | 63, 65 << 6]), 10, True)) == [16, 16]


@pytest.mark.parametrize("msb", [False, True], ids=["low", "high"])
@pytest.mark.parametrize("depth", [9, 10, 12, 16])
def test_widened_bytes_reduce_to_themselves(depth, msb):
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(yuv16_ref.reduce8(yuv16_ref.widen(v, depth, msb), depth, msb), v)
    # and the operands equal the 8-bit path's
    f = yuv_ref.random_frame(16, 16, "nv12", depth)
    assert np.array_equal(yuv16_ref.operand(yuv16_ref.widen(f, depth, msb), "nv12", depth, msb, (16, 16), (0, 0), (16, 16)),
                          yuv_ref.operand(f, "nv12", (16, 16), (0, 0), (16, 16)))


def test_rounding_differs_from_truncation_on_random_content():
    """a kernel that truncates (raw >> 2) instead of rounding fails the operand comparison: the restated 16x16 operand of
    random 10-bit content differs from the truncated one at a large share of its pixels"""
    f = yuv16_ref.random_frame(16, 16, 10, False, 5)
    a = yuv16_ref.operand(f, "i420", 10, False, (16, 16), (0, 0), (16, 16))
    b = yuv_ref.operand((f >> 2).astype(np.uint8), "i420", (16, 16), (0, 0), (16, 16))
    assert np.count_nonzero(a != b) > 256 // 5


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("sw,sh,resize,crop,out", GEOMS)
def test_window_equals_the_8bit_window_at_twice_the_bytes(sw, sh, resize, crop, out, layout):
    win8, bytes8 = _capi.frontend_yuv_window((sw, sh), layout, resize, crop, out)
    win16, bytes16 = _capi.frontend_yuv_window((sw, sh), layout, resize, crop, out, depth=10)
    assert win16 == win8 and bytes16 == 2 * bytes8
    x, y, w, h = win16
    assert bytes16 == w * h * 3
    assert x % 16 == 0 and ((x + w) % 16 == 0 or x + w == sw) and y % 2 == 0 and h % 2 == 0 and w % 2 == 0
    xs = yuv_ref.source_span(crop[0], crop[0] + out[0] - 1, sw, resize[0])
    ys = yuv_ref.source_span(crop[1], crop[1] + out[1] - 1, sh, resize[1])
    assert xs.min() >= x and xs.max() < x + w
    assert ys.min() >= y and ys.max() < y + h


def test_window_with_a_padded_semi_planar_pitch_and_every_depth():
    want = _capi.frontend_yuv_window((640, 360), "nv12", (256, 256), (0, 0), (256, 256), depth=10)
    assert _capi.frontend_yuv_window((640, 360), "nv12", (256, 256), (0, 0), (256, 256), stride=1408, depth=10) == want
    for depth in range(9, 17):
        assert _capi.frontend_yuv_window((640, 360), "i420", (256, 256), (0, 0), (256, 256), depth=depth) == want


@pytest.mark.parametrize("args,rule", [
    (dict(depth=7), "depth 7 outside 9..16"),
    (dict(depth=17), "depth 17 outside 9..16"),
    (dict(layout=1, stride=1281), "odd stride 1281"),
    (dict(stride=640), r"I420 needs stride == 2 \* width"),
    (dict(stride=1408), r"I420 needs stride == 2 \* width"),
    (dict(layout=1, stride=1278), r"NV12 needs stride >= 2 \* width"),
    (dict(src_size=(641, 360)), "even width and height"),
    (dict(src_size=(640, 361)), "even width and height"),
    (dict(layout=2), "unknown layout"),
    (dict(resize=(200, 300)), "does not fit"),
    (dict(crop=(1, 0)), "does not fit"),
    (dict(resize=(0, 256)), "unsupported source"),
])
def test_every_refusal_names_its_rule(args, rule):
    a = dict(src_size=(640, 360), layout=0, resize=(256, 256), crop=(0, 0), out_size=(256, 256), stride=None, depth=10)
    a.update(args)
    with pytest.raises(ValueError, match=rule) as e:
        _capi.frontend_yuv_window(**a)
    assert "ffl_frontend_yuv16_window" in str(e.value)


class Cai:
    """an object with __cuda_array_interface__ over an invented device address (nothing is read)"""

    def __init__(self, shape, strides=None, typestr="<u2", ptr=1 << 33):
        self.__cuda_array_interface__ = {"version": 3, "data": (ptr, False), "shape": tuple(shape),
                                         "strides": None if strides is None else tuple(strides), "typestr": typestr}


def refused16(fmt, frame, depth=10, resize=(256, 256), crop=(0, 0), out=(256, 256)):
    with pytest.raises(ValueError) as e:
        _capi.dev_frame_check(fmt, frame, resize, crop, out, depth=depth)
    assert "ffl_dev_frame_check16" in str(e.value)
    return str(e.value)


def test_device_frame_rows_and_refusals():
    """_frame_row with "<u2": pitches in bytes, planes counted in bytes; ffl_dev_frame_check16's rules by name"""
    f = _capi.device_frame(Cai((540, 640)), "i420", depth=10)
    base = 1 << 33
    assert (f.width, f.height) == (640, 360)
    assert list(f.plane) == [base, base + 360 * 1280, base + 360 * 1280 + 180 * 640] and list(f.pitch) == [1280, 640, 640]
    n = _capi.device_frame(Cai((540, 640), strides=(1408, 2)), "nv12", depth=16)
    assert list(n.plane)[:2] == [base, base + 360 * 1408] and list(n.pitch)[:2] == [1408, 1408]
    _capi.dev_frame_check("i420", f, (256, 256), (0, 0), (256, 256), depth=10)
    _capi.dev_frame_check("nv12", n, (256, 256), (0, 0), (256, 256), depth=16)
    L = _capi.load()
    assert L.ffl_dev_frame_check16(4, 8, 640, 360, C.byref(n), 256, 256, 0, 0, 256, 256) == _capi.FFL_ERR_INVALID
    assert "depth 8 outside 9..16" in L.ffl_last_error(None).decode()
    assert "depth 17 outside 9..16" in refused16("nv12", n, depth=17)
    assert "16-bit frames are 4:2:0 only" in refused16("bgr", n)
    n.pitch[1] = 1409
    assert "odd pitch" in refused16("nv12", n)
    n.pitch[1] = 1278
    assert "chroma pitch 1278 / 1278 too small for a row of 1280 bytes" in refused16("nv12", n)
    n.pitch[1], n.pitch[0] = 1408, 1278
    assert "Y pitch 1278 too small" in refused16("nv12", n)
    n.pitch[0] = 1408
    n.plane[1] = n.plane[1] + 1
    assert "not 2-byte aligned" in refused16("nv12", n)
    f.pitch[2] = 638
    assert "chroma pitch 640 / 638 too small for a row of 640 bytes" in refused16("i420", f)
    odd = _capi.device_frame(Cai((543, 642)), "nv12", depth=10)
    odd.height = 361
    assert "even width and height" in refused16("nv12", odd)
    assert "does not fit" in refused16("i420", _capi.device_frame(Cai((540, 640)), "i420", depth=10), crop=(1, 0))
    # Python's own words
    with pytest.raises(ValueError, match="depth=10 needs uint16 frames"):
        _capi.device_frame(Cai((540, 640), typestr="|u1"), "nv12", depth=10)
    with pytest.raises(ValueError, match="pass depth=9..16"):
        _capi.device_frame(Cai((540, 640)), "nv12")
    with pytest.raises(ValueError, match="4:2:0 frames"):
        _capi.device_frame(Cai((256, 256, 3)), "bgr", depth=10)
    with pytest.raises(ValueError, match="column stride 2"):
        _capi.device_frame(Cai((540, 640), strides=(2560, 4)), "nv12", depth=10)
    with pytest.raises(ValueError, match="I420 needs contiguous rows"):
        _capi.device_frame(Cai((540, 640), strides=(1408, 2)), "i420", depth=10)


def test_the_abi_exports_and_declares_the_new_entry_points():
    import os
    L = _capi.load()
    header = open(os.path.join(os.path.dirname(_capi._HERE), "include", "ffl.h")).read()
    for name in ("ffl_upload_frames_yuv16", "ffl_frontend_yuv16_window", "ffl_dev_frame_check16", "ffl_upload_frames_device16"):
        assert hasattr(L, name) and name in _capi.EXPORTS and f"int {name}(" in header
    win, b = (C.c_int * 4)(), C.c_size_t()
    assert L.ffl_frontend_yuv16_window(640, 360, 1, 1280, 10, 256, 256, 0, 0, 256, 256, win, C.byref(b)) == 0
    assert tuple(win) == (0, 0, 640, 360) and b.value == 640 * 360 * 3
    assert L.ffl_frontend_yuv16_window(640, 360, 1, 1280, 10, 256, 256, 0, 0, 256, 256, None, None) == 0
    assert L.ffl_upload_frames_yuv16(None, 0, 1, None, 640, 360, 1280, 1, 10, 1, 256, 256, 0, 0) == _capi.FFL_ERR_INVALID


def test_depth_and_alignment_defaults():
    assert _capi.yuv_depth(10, "nv12") == (10, 1) and _capi.yuv_depth(10, "i420") == (10, 0)
    assert _capi.yuv_depth(10, 1) == (10, 1) and _capi.yuv_depth(10, 0) == (10, 0)
    assert _capi.yuv_depth(12, "nv12", False) == (12, 0) and _capi.yuv_depth(12, "i420", True) == (12, 1)
    assert _capi.yuv_depth(8, "nv12") == (8, 1)
    for bad in (7, 17, 10.0, "10", None, True):
        with pytest.raises(ValueError, match="depth must be 8"):
            _capi.yuv_depth(bad)


def test_python_layer_refusals():
    with pytest.raises(ValueError, match=r'yuv="nv12", depth=10'):
        frontend.DecodedUploader(object(), yuv="p010")
    with pytest.raises(ValueError, match="layout.*depth=10"):
        frontend.upload_decoded(object(), 0, [], yuv="yuv420p10le")
    with pytest.raises(ValueError, match=r'yuv="nv12", depth=10'):
        frontend.DeviceUploader(object(), fmt="p010")
    with pytest.raises(ValueError, match="depth must be 8"):
        frontend.DecodedUploader(object(), yuv="nv12", depth=17)
    with pytest.raises(ValueError, match="need yuv="):
        frontend.DecodedUploader(object(), depth=10)
    with pytest.raises(ValueError, match="needs depth=9..16"):
        frontend.DecodedUploader(object(), yuv="nv12", msb=True)
    with pytest.raises(ValueError, match="rgb_order"):
        frontend.DecodedUploader(object(), rgb_order=True, yuv="i420", depth=10)
    with pytest.raises(ValueError, match="4:2:0 frames"):
        frontend.DeviceUploader(object(), fmt="bgr", depth=10)
    with pytest.raises(TypeError):
        frontend.upload_decoded(object(), 0, [np.zeros((6, 4), np.uint16)], yuv="nv12", depth=10)
    with pytest.raises(TypeError):
        frontend.DeviceUploader(object(), fmt="nv12", depth=10)
    up = frontend.DecodedUploader(object(), yuv="nv12", depth=10)
    assert up.deep == {"depth": 10}                                   # msb travels only when the caller set it
    assert frontend.DecodedUploader(object(), yuv="i420", depth=12, msb=True).deep == {"depth": 12, "msb": True}
    assert frontend.DecodedUploader(object(), yuv="i420").deep == {} and frontend.DecodedUploader(object(), yuv="i420", depth=8).deep == {}


def test_params_carry_the_depth_only_when_set():
    assert prefetch.yuv_params({"hip_yuv": "i420"}) == ("i420", {})
    assert prefetch.yuv_params({"hip_yuv": "i420", "hip_yuv_depth": 10}) == ("i420", {"depth": 10})
    assert prefetch.yuv_params({"hip_yuv": "nv12", "hip_yuv_depth": 12.0, "hip_yuv_msb": 0}) == ("nv12", {"depth": 12, "msb": False})
    assert prefetch.yuv_params({}) == (None, {})
    assert prefetch.ring_depth({"depth": 10, "msb": True}) == {"depth": 10} and prefetch.ring_depth({"depth": 8}) == {}


# ---- prefetch ring with uint16 4:2:0 slots ---------------------------------------------------------------------------
class Yuv16Capture:
    """cv2.VideoCapture look-alike whose read() yields (3h/2, w) uint16 4:2:0 frames: frame i carries i in sample (0, 0)"""

    def __init__(self, n_frames, fps=30.0, size=(8, 6)):
        self.n, self.fps, self.size = n_frames, fps, size
        self.pos, self.seeks, self.grabs, self.reads = 0, 0, 0, 0

    def get(self, prop):
        return {prefetch.CAP_PROP_FRAME_COUNT: self.n, prefetch.CAP_PROP_FPS: self.fps,
                prefetch.CAP_PROP_FRAME_WIDTH: self.size[0], prefetch.CAP_PROP_FRAME_HEIGHT: self.size[1]}[prop]

    def set(self, prop, value):
        self.seeks += 1
        return True

    def grab(self):
        if self.pos >= self.n:
            return False
        self.pos += 1
        self.grabs += 1
        return True

    def read(self, image=None):
        if self.pos >= self.n:
            return False, None
        w, h = self.size
        assert image is None or (image.shape == (h * 3 // 2, w) and image.dtype == np.uint16)
        frame = image if image is not None else np.empty((h * 3 // 2, w), np.uint16)
        frame[...] = 1023 - self.pos % 251
        frame[0, 0] = self.pos
        self.pos += 1
        self.reads += 1
        return True, frame


class Yuv16Ctx:
    """Device stand-in (as in test_prefetch_host): an upload only remembers the host array, whose samples are read when
    the first batch that uses the slot returns its results -- a ring that recycles a frame early shows a wrong pair."""

    def __init__(self, max_batch, delay=0.0):
        self.max_batch, self.frame_slots, self.flow_slots, self.delay = max_batch, 2 * max_batch + 2, pipeline.min_flow_slots(max_batch), delay
        self.slot_upload, self.pending, self.pinned = {}, [], []

    def pinned_frames(self, n, channels=1, size=None, yuv=False, depth=8):
        self.pinned.append((n, channels, size, yuv, depth))
        w, h = size
        return np.zeros((n, h * 3 // 2, w), np.uint16 if depth > 8 else np.uint8)

    def upload_frames(self, first, frames):
        for k, f in enumerate(frames):
            self.slot_upload[first + k] = {"host": f, "device": None}

    def flow_pairs(self, f0, f1, slots, pov):
        self.pending.append([(self.slot_upload[a], self.slot_upload[b], s) for a, b, s in zip(f0, f1, slots)])

    def pass1_results(self, slots, thr):
        time.sleep(self.delay)
        out = []
        for (a, b, s), want in zip(self.pending.pop(0), slots):
            for up in (a, b):
                if up["device"] is None:
                    up["device"] = int(up["host"][0, 0])
            out.append((a["device"], b["device"], np.float32(0), np.float32(0), False))
        return out

    def radial(self, slots, centers, cuts, pov):
        return [0.0] * len(slots)


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_prefetch_ring_uint16_slots_order_no_seek_and_back_pressure(layout):
    B, n = 4, 90
    cap = Yuv16Capture(n, 30.0, size=(10, 6))
    ctx = Yuv16Ctx(B, delay=0.003)
    ring = prefetch.PrefetchRing(ctx, cap, list(range(n)), 45, 3 * B + 2, yuv=layout, depth=10)
    assert ctx.pinned == [(3 * B + 2, 1, (10, 6), True, 10)]
    assert ring.slots.shape == (3 * B + 2, 9, 10) and ring.slots.dtype == np.uint16
    eng = pipeline.PairEngine(ctx)
    got = []
    try:
        for view, fidx in ring.chunks():
            _, recs = eng.process_chunk(view)
            got += [(r[0], r[1]) for r in recs]
    finally:
        ring.close()
    assert got == [(i, i + 1) for i in range(0, 44)] + [(i, i + 1) for i in range(45, 89)]
    assert ring.max_outstanding <= 3 * B + 2
    assert cap.seeks == 0 and cap.reads == n


def test_prefetch_ring_depth_refusals_and_the_8bit_call_shape():
    with pytest.raises(ValueError, match="depth must be 8"):
        prefetch.PrefetchRing(Yuv16Ctx(2), Yuv16Capture(10), list(range(10)), 10, 8, yuv="i420", depth=20)
    with pytest.raises(ValueError, match="needs yuv="):
        prefetch.PrefetchRing(Yuv16Ctx(2), Yuv16Capture(10), list(range(10)), 10, 8, depth=10)
    with pytest.raises(ValueError, match="even"):
        prefetch.PrefetchRing(Yuv16Ctx(2), Yuv16Capture(10, size=(9, 6)), list(range(10)), 10, 8, yuv="i420", depth=10)

    class OldCtx:                         # a context whose pinned_frames knows no depth keyword: depth 8 never passes one
        def pinned_frames(self, n, channels=1, size=None, yuv=False):
            return np.zeros((n, size[1] * 3 // 2, size[0]), np.uint8)

    class Cap8(Yuv16Capture):
        def read(self, image=None):
            self.pos += 1
            image[...] = 0
            return True, image

    ring = prefetch.PrefetchRing(OldCtx(), Cap8(4), list(range(4)), 4, 8, yuv="i420", depth=8)
    ring.close()
    assert ring.slots.dtype == np.uint8
