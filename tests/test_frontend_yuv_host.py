"""Host side of the 4:2:0 front-end (no GPU): the restatement's known answers and its
committed golden, the source window of ffl_frontend_yuv_window against every pixel the restatement reads, the refusals,
and the prefetch ring with 4:2:0 slots against a fake capture."""
import threading
import time

import numpy as np
import pytest

import gen_yuv_golden
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline, prefetch


def test_restatement_known_answers():
    for (y, u, v), bgr in gen_yuv_golden.KNOWN:
        assert tuple(int(t) for t in yuv_ref.yuv_to_bgr_pixels(y, u, v)) == bgr, (y, u, v)


def test_restatement_layouts_agree_and_chroma_is_nearest():
    """The same planes as I420 and as NV12 give the same BGR image; every 2x2 block shares one chroma sample."""
    rng = np.random.default_rng(11)
    h, w = 6, 8
    Y = rng.integers(0, 256, (h, w), dtype=np.uint8)
    U, V = (rng.integers(0, 256, (h // 2, w // 2), dtype=np.uint8) for _ in range(2))
    i420 = np.concatenate([Y.reshape(-1), U.reshape(-1), V.reshape(-1)]).reshape(h * 3 // 2, w)
    uv = np.empty((h // 2, w), np.uint8)
    uv[:, 0::2], uv[:, 1::2] = U, V
    nv12 = np.concatenate([Y, uv])
    a, b = yuv_ref.yuv_to_bgr(i420, "i420"), yuv_ref.yuv_to_bgr(nv12, "nv12")
    assert np.array_equal(a, b)
    for y in range(h):
        for x in range(w):
            assert tuple(a[y, x]) == tuple(yuv_ref.yuv_to_bgr_pixels(Y[y, x], U[y // 2, x // 2], V[y // 2, x // 2]))


def test_restatement_reproduces_committed_golden(golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "yuv_frontend_golden.npz"))
    assert [tuple(k) for k in g["known_yuv"].tolist()] == [k[0] for k in gen_yuv_golden.KNOWN]
    assert np.array_equal(yuv_ref.yuv_to_bgr_pixels(g["known_yuv"][:, 0], g["known_yuv"][:, 1], g["known_yuv"][:, 2]),
                          g["known_bgr"])
    assert list(g["names"]) == [c[0] for c in gen_yuv_golden.CASES]
    for case, s_in, s_op in zip(gen_yuv_golden.CASES, g["input_sha256"], g["operand_sha256"]):
        assert gen_yuv_golden.sha(gen_yuv_golden.case_frame(case)) == s_in, case[0]
        assert gen_yuv_golden.sha(gen_yuv_golden.case_operand(case)) == s_op, case[0]


# (source w, h, resize, crop, operand size): the reference's two geometries over common sources, odd crops, exact x2,
# identity and up-scaling
GEOMS = [(sw, sh, (256, 256), (0, 0), (256, 256)) for sw, sh in
         [(1920, 1080), (3840, 2160), (5760, 2880), (640, 360), (1280, 720), (512, 512), (256, 256), (160, 90), (2, 2)]] + \
        [(sw, sh, (512, 512), (0, 256), (256, 256)) for sw, sh in
         [(1920, 1080), (3840, 2160), (5760, 2880), (640, 360), (1024, 1024), (512, 512), (200, 100)]] + [
    (640, 360, (301, 283), (37, 19), (200, 160)),
    (640, 360, (301, 283), (101, 123), (200, 160)),
    (1920, 1080, (1920, 1080), (333, 211), (256, 256)),         # identity with an odd crop
    (1920, 1080, (960, 540), (101, 77), (320, 180)),            # exact x2 with an odd crop
    (3840, 2160, (1000, 700), (999 - 255, 699 - 255), (256, 256)),
    (5760, 2880, (777, 555), (13, 7), (256, 256)),
    (130, 66, (1000, 900), (511, 333), (256, 256)),             # up-scaling far beyond the source
    (6, 4, (300, 300), (1, 1), (17, 19)),
]


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("sw,sh,resize,crop,out", GEOMS)
def test_window_covers_every_pixel_the_restatement_reads(sw, sh, resize, crop, out, layout):
    (x, y, w, h), nbytes = _capi.frontend_yuv_window((sw, sh), layout, resize, crop, out)
    assert x % 16 == 0 and ((x + w) % 16 == 0 or x + w == sw) and y % 2 == 0 and h % 2 == 0 and w % 2 == 0
    assert 0 <= x and x + w <= sw and 0 <= y and y + h <= sh and w > 0 and h > 0
    assert nbytes == w * h * 3 // 2
    xs = yuv_ref.source_span(crop[0], crop[0] + out[0] - 1, sw, resize[0])
    ys = yuv_ref.source_span(crop[1], crop[1] + out[1] - 1, sh, resize[1])
    assert xs.min() >= x and xs.max() < x + w
    assert ys.min() >= y and ys.max() < y + h
    # not a full-frame fallback where the window is a small part of the frame: one pixel of widening, then columns
    # rounded out to multiples of 16 and rows to even
    assert x >= max(0, xs.min() - 17) and x + w <= min(sw, xs.max() + 18)
    assert y >= max(0, ys.min() - 3) and y + h <= min(sh, ys.max() + 4)


def test_vr_window_is_the_issue_arithmetic():
    """5760x2880 VR onto 256x256: columns 5..2874 are read (widened and rounded out to 0..2879), rows 1442..2877
    (1440..2879); about 1/8 of the frame's BGR bytes."""
    (x, y, w, h), nbytes = _capi.frontend_yuv_window((5760, 2880), "i420", (512, 512), (0, 256), (256, 256))
    assert (x, y, x + w, y + h) == (0, 1440, 2880, 2880)
    assert nbytes * 7 < 5760 * 2880 * 3          # the BGR path sends 3 bytes per source pixel


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("sw,sh,resize,crop,out", [(640, 360, (301, 283), (37, 19), (200, 160)),
                                                   (640, 360, (512, 512), (0, 256), (256, 256)),
                                                   (512, 288, (256, 144), (31, 17), (96, 80)),
                                                   (320, 180, (320, 180), (41, 23), (100, 60))])
def test_pixels_outside_the_window_do_not_matter(sw, sh, resize, crop, out, layout):
    """Brute force: replacing every byte outside the window (luma and chroma) leaves the restated operand unchanged."""
    (x, y, w, h), _ = _capi.frontend_yuv_window((sw, sh), layout, resize, crop, out)
    f = yuv_ref.random_frame(sw, sh, layout, 21)
    g = yuv_ref.random_frame(sw, sh, layout, 22)
    Yf, Uf, Vf = yuv_ref.planes(f, layout)
    Yg, Ug, Vg = yuv_ref.planes(g, layout)
    Yg[y:y + h, x:x + w] = Yf[y:y + h, x:x + w]
    if layout == "nv12":
        g[sh + y // 2:sh + (y + h) // 2, x:x + w] = f[sh + y // 2:sh + (y + h) // 2, x:x + w]
    else:                                        # planes() returns copies for I420: rebuild g from its planes
        Ug[y // 2:(y + h) // 2, x // 2:(x + w) // 2] = Uf[y // 2:(y + h) // 2, x // 2:(x + w) // 2]
        Vg[y // 2:(y + h) // 2, x // 2:(x + w) // 2] = Vf[y // 2:(y + h) // 2, x // 2:(x + w) // 2]
        g = np.concatenate([Yg.reshape(-1), Ug.reshape(-1), Vg.reshape(-1)]).reshape(g.shape)
    assert not np.array_equal(f, g)
    assert np.array_equal(yuv_ref.operand(f, layout, resize, crop, out), yuv_ref.operand(g, layout, resize, crop, out))


@pytest.mark.parametrize("args,rule", [
    (dict(src_size=(641, 360)), "even width and height"),
    (dict(src_size=(640, 361)), "even width and height"),
    (dict(layout=2), "unknown layout"),
    (dict(stride=704), "I420 needs stride == width"),
    (dict(layout=1, stride=600), "NV12 needs stride >= width"),
    (dict(resize=(200, 300)), "does not fit"),
    (dict(crop=(1, 0)), "does not fit"),
    (dict(resize=(0, 256)), "unsupported source"),
])
def test_every_refusal_names_its_rule(args, rule):
    a = dict(src_size=(640, 360), layout=0, resize=(256, 256), crop=(0, 0), out_size=(256, 256), stride=None)
    a.update(args)
    with pytest.raises(ValueError, match=rule):
        _capi.frontend_yuv_window(**a)


def test_nv12_padded_stride_is_accepted():
    assert _capi.frontend_yuv_window((640, 360), "nv12", (256, 256), (0, 0), (256, 256), stride=704)[0] == \
        _capi.frontend_yuv_window((640, 360), "nv12", (256, 256), (0, 0), (256, 256))[0]


def test_python_layer_refusals():
    with pytest.raises(ValueError, match="layout"):
        _capi.yuv_layout("yv12")
    with pytest.raises(ValueError, match="rgb_order"):
        frontend.DecodedUploader(object(), rgb_order=True, yuv="i420")
    with pytest.raises(ValueError, match="layout"):
        frontend.DecodedUploader(object(), yuv="p010")
    with pytest.raises(ValueError, match="rgb_order"):
        frontend.upload_decoded(object(), 0, [], rgb_order=True, yuv="nv12")
    with pytest.raises(TypeError):
        frontend.upload_decoded(object(), 0, [np.zeros((6, 4), np.uint8)], yuv="nv12")


# ---- prefetch ring with 4:2:0 slots --------------------------------------------------------------------------------
class YuvCapture:
    """cv2.VideoCapture look-alike whose read() yields (3h/2, w) 4:2:0 frames: frame i carries i in its first two bytes."""

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
        assert image is None or image.shape == (h * 3 // 2, w)
        frame = image if image is not None else np.empty((h * 3 // 2, w), np.uint8)
        frame[...] = self.pos % 251
        frame[0, 0], frame[0, 1] = self.pos & 255, (self.pos >> 8) & 255
        self.pos += 1
        self.reads += 1
        return True, frame


def frame_id(a):
    return int(a[0, 0]) | (int(a[0, 1]) << 8)


class YuvCtx:
    """Device stand-in (as in test_prefetch_host): an upload only remembers the host array, whose pixels are read when
    the first batch that uses the slot returns its results -- a ring that recycles a frame early shows a wrong pair."""

    def __init__(self, max_batch, delay=0.0):
        self.max_batch, self.frame_slots, self.flow_slots, self.delay = max_batch, 2 * max_batch + 2, pipeline.min_flow_slots(max_batch), delay
        self.slot_upload, self.pending, self.pinned = {}, [], []

    def pinned_frames(self, n, channels=1, size=None, yuv=False):
        self.pinned.append((n, channels, size, yuv))
        w, h = size
        return np.zeros((n, h * 3 // 2, w) if yuv else (n, h, w, 3), np.uint8)

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
                    up["device"] = frame_id(up["host"])
            out.append((a["device"], b["device"], np.float32(0), np.float32(0), False))
        return out

    def radial(self, slots, centers, cuts, pov):
        return [0.0] * len(slots)


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_prefetch_ring_yuv_slots_no_seek_and_back_pressure(layout):
    B, n = 4, 90
    cap = YuvCapture(n, 30.0, size=(10, 6))
    ctx = YuvCtx(B, delay=0.003)
    ring = prefetch.PrefetchRing(ctx, cap, list(range(n)), 45, 3 * B + 2, yuv=layout)
    assert ctx.pinned == [(3 * B + 2, 1, (10, 6), True)]
    assert ring.slots.shape == (3 * B + 2, 9, 10)
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


def test_prefetch_ring_yuv_sampling_grabs_instead_of_seeking():
    cap = YuvCapture(71, 60.0, size=(8, 4))
    ctx = YuvCtx(3)
    from funscript_flow_amd import postchain
    _, _, indices = postchain.sampling(60.0, 71)
    ring = prefetch.PrefetchRing(ctx, cap, indices, 10, 11, yuv="nv12")
    try:
        for view, _ in ring.chunks():
            pipeline.PairEngine(ctx).process_chunk(view)
    finally:
        ring.close()
    assert cap.seeks == 0 and cap.reads == 36 and cap.grabs == 35


def test_prefetch_ring_yuv_refuses_odd_frames():
    with pytest.raises(ValueError, match="even"):
        prefetch.PrefetchRing(YuvCtx(2), YuvCapture(10, size=(9, 6)), list(range(10)), 10, 8, yuv="i420")
    with pytest.raises(ValueError, match="layout"):
        prefetch.PrefetchRing(YuvCtx(2), YuvCapture(10), list(range(10)), 10, 8, yuv="yuyv")
