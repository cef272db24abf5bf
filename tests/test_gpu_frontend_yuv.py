"""GPU parity of the 4:2:0 front-end (k_frontend behind ffl_upload_frames_yuv) against the numpy
restatement of appendix Y composed with the oracle's resize and luma (tests/yuv_ref.py).  Integer work: bit-exact.  Both
transfer paths (a staging copy out of pageable arrays; 2-D copies straight out of ffl_host_alloc memory) are covered."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline, prefetch


def frames_for(sw, sh, layout, n, seed, pitch=None, ctx=None):
    """n random 4:2:0 frames; with ctx, they sit in the context's page-locked memory (the zero-copy path)"""
    fr = [yuv_ref.random_frame(sw, sh, layout, seed + i, pitch) for i in range(n)]
    if ctx is None:
        return fr
    pin = ctx.pinned_frames(n, size=(pitch or sw, sh), yuv=True)
    pin[:, :, :sw] = np.stack(fr)
    return [pin[i, :, :sw] for i in range(n)]


# (layout, source w, h, row pitch, resize, crop, context w, h)
CASES = [(lay, sw, sh, None, (256, 256), (0, 0), 256, 256) for lay in ("i420", "nv12")
         for sw, sh in [(1920, 1080), (3840, 2160)]] + \
        [(lay, 5760, 2880, None, (512, 512), (0, 256), 256, 256) for lay in ("i420", "nv12")] + [
    ("i420", 640, 360, None, (301, 283), (37, 19), 200, 160),     # odd crop of an arbitrary resize
    ("nv12", 640, 360, None, (301, 283), (101, 123), 200, 160),
    ("i420", 512, 512, None, (256, 256), (0, 0), 256, 256),       # exact x2 -> 2x2 mean
    ("nv12", 1920, 1080, None, (960, 540), (101, 77), 320, 180),  # exact x2 with a crop
    ("nv12", 1920, 1080, None, (1920, 1080), (0, 0), 1920, 1080), # identity on a 1080p context
    ("i420", 1920, 1080, None, (1920, 1080), (0, 0), 1920, 1080),
    ("nv12", 640, 360, 704, (256, 256), (0, 0), 256, 256),        # NV12 with a padded row pitch
    ("nv12", 1280, 720, 1536, (512, 512), (0, 256), 256, 256),
    ("i420", 160, 90, None, (256, 256), (0, 0), 256, 256),        # up-scaling
]


@pytest.mark.parametrize("zero_copy", [False, True], ids=["staged", "zero_copy"])
@pytest.mark.parametrize("layout,sw,sh,pitch,resize,crop,cw,ch", CASES)
def test_yuv_frontend_bit_exact(layout, sw, sh, pitch, resize, crop, cw, ch, zero_copy):
    with _capi.Context(cw, ch, max_batch=1, frame_slots=4) as ctx:
        fr = frames_for(sw, sh, layout, 2, 31, pitch, ctx if zero_copy else None)
        ctx.upload_frames_yuv(0, fr, layout, resize, crop)
        for i, f in enumerate(fr):
            assert np.array_equal(ctx.download_frame(i), yuv_ref.operand(f, layout, resize, crop, (cw, ch))), i


def test_ring_reuse_and_growing_sources():
    """More frames than ring buffers, both layouts, a later and larger source, then a smaller one again."""
    with _capi.Context(256, 256, max_batch=1, frame_slots=16) as ctx:
        small = frames_for(320, 180, "i420", 7, 50)
        large = frames_for(1920, 1080, "nv12", 5, 60)
        again = frames_for(640, 360, "i420", 3, 70, ctx=ctx)
        frontend.upload_decoded(ctx, 0, small, yuv="i420")
        frontend.upload_decoded(ctx, 7, large, yuv="nv12")
        frontend.upload_decoded(ctx, 12, again, vr_mode=True, yuv="i420")
        for i, (f, lay, vr) in enumerate([(f, "i420", False) for f in small] + [(f, "nv12", False) for f in large] +
                                         [(f, "i420", True) for f in again]):
            resize, crop = frontend.geometry(256, 256, vr)
            assert np.array_equal(ctx.download_frame(i), yuv_ref.operand(f, lay, resize, crop)), i


def yuv_clip(n, sw, sh, layout, seed):
    """smooth moving content as 4:2:0 frames: luma from synth, chroma from the luma's 2x2 means"""
    from funscript_flow_amd.synth import sine_translate_frames
    g = sine_translate_frames(n, sw, sh, seed=seed, amp=(5.0, 3.0), period=7)
    out = []
    for f in g:
        c = f.reshape(sh // 2, 2, sw // 2, 2).astype(np.int32).mean(axis=(1, 3)).astype(np.uint8)
        u, v = (c // 2 + 64).astype(np.uint8), (255 - c).astype(np.uint8)
        if layout == "i420":
            out.append(np.concatenate([f.reshape(-1), u.reshape(-1), v.reshape(-1)]).reshape(sh * 3 // 2, sw))
        else:
            uv = np.empty((sh // 2, sw), np.uint8)
            uv[:, 0::2], uv[:, 1::2] = u, v
            out.append(np.concatenate([f, uv]))
    return out


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_chunk_from_yuv_frames_equals_chunk_from_restated_operands(layout):
    dec = yuv_clip(12, 640, 360, layout, 9)
    for vr in (False, True):
        resize, crop = frontend.geometry(256, 256, vr)
        with _capi.Context(256, 256, max_batch=4, frame_slots=10, flow_slots=25) as ctx:
            d_yuv, r_yuv = pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, vr_mode=vr, yuv=layout)).process_chunk(dec)
        with _capi.Context(256, 256, max_batch=4, frame_slots=10, flow_slots=25) as ctx:
            d_ref, r_ref = pipeline.PairEngine(ctx).process_chunk([yuv_ref.operand(f, layout, resize, crop) for f in dec])
        assert np.array_equal(d_yuv, d_ref) and [tuple(r) for r in r_yuv] == [tuple(r) for r in r_ref]


def test_video_to_actions_with_an_i420_capture():
    """params["hip_yuv"] = "i420": a (fake) capture whose read() yields (3h/2, w) I420 frames is read sequentially into the
    context's page-locked 4:2:0 ring, uploaded zero-copy, and gives exactly frames_to_actions on the restated operands.
    60 fps source (every second frame is grabbed), 3 chunks incl. a ragged one."""
    sw, sh, n, fps = 320, 240, 101, 60.0
    src = yuv_clip(n, sw, sh, "i420", 6)

    class Cap:
        def __init__(self):
            self.pos, self.seeks = 0, 0

        def get(self, prop):
            return {prefetch.CAP_PROP_FRAME_COUNT: n, prefetch.CAP_PROP_FPS: fps, prefetch.CAP_PROP_FRAME_WIDTH: sw,
                    prefetch.CAP_PROP_FRAME_HEIGHT: sh}[prop]

        def set(self, *a):
            self.seeks += 1
            return True

        def grab(self):
            self.pos += 1
            return self.pos <= n

        def read(self, image=None):
            if self.pos >= n:
                return False, None
            np.copyto(image, src[self.pos])
            self.pos += 1
            return True, image

    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False,
              "hip_yuv": "i420"}
    cap = Cap()
    with _capi.Context(128, 96, max_batch=4, frame_slots=10, flow_slots=pipeline.min_flow_slots(4)) as ctx:
        got = prefetch.video_to_actions(ctx, cap, params)
        ops = [yuv_ref.operand(f, "i420", (128, 96), (0, 0), (128, 96)) for f in src]
        want = pipeline.frames_to_actions(pipeline.PairEngine(ctx), ops, fps, {k: v for k, v in params.items() if k != "hip_yuv"})
    assert cap.seeks == 0
    assert got == want and len(got) == 48


def test_yuv_refusals_are_loud():
    f = yuv_ref.random_frame(640, 360, "i420", 1)
    with _capi.Context(256, 256, max_batch=1) as ctx:
        def refused(rule, *a, **k):
            with pytest.raises(_capi.FFLError, match=rule):
                ctx.upload_frames_yuv(*a, **k)
        refused("bad frame slot range", 5, [f], "i420", (256, 256))
        refused("does not fit", 0, [f], "i420", (200, 300))
        refused("does not fit", 0, [f], "nv12", (256, 256), (1, 0))
        refused("even width and height", 0, [yuv_ref.random_frame(640, 360, "i420", 2)[:, :639]], "nv12", (256, 256))
        refused("3h/2 rows", 0, [f[:-1]], "i420", (256, 256))
        wide = np.zeros((540, 704), np.uint8)[:, :640]
        refused("I420 needs stride == width", 0, [wide], "i420", (256, 256))
        with pytest.raises(ValueError, match="layout"):
            ctx.upload_frames_yuv(0, [f], "yv12", (256, 256))
        L, vp = ctx.L, C.c_void_p
        ptrs = (vp * 2)(f.ctypes.data, None)
        assert L.ffl_upload_frames_yuv(ctx._h, 0, 2, ptrs, 640, 360, 640, 0, 256, 256, 0, 0) == 1
        assert b"frame 1 is NULL" in L.ffl_last_error(ctx._h)
        assert L.ffl_upload_frames_yuv(ctx._h, 0, 1, ptrs, 640, 360, 640, 7, 256, 256, 0, 0) == 1
        assert b"unknown layout" in L.ffl_last_error(ctx._h)
        assert L.ffl_upload_frames_yuv(ctx._h, 0, 1, ptrs, 640, 360, 600, 1, 256, 256, 0, 0) == 1
        assert b"NV12 needs stride >= width" in L.ffl_last_error(ctx._h)
        assert L.ffl_upload_frames_yuv(ctx._h, 0, 1, None, 640, 360, 640, 0, 256, 256, 0, 0) == 1
        with pytest.raises(_capi.FFLError):
            ctx.download_frame(0)                                      # nothing was uploaded by the refused calls
        with pytest.raises(ValueError, match="rgb_order"):
            frontend.upload_decoded(ctx, 0, [f], rgb_order=True, yuv="i420")
