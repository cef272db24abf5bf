"""GPU parity of the high-bit-depth 4:2:0 front-end (k_frontend behind ffl_upload_frames_yuv16, k_frontend_dev behind
ffl_upload_frames_device16; DESIGN.md sections 11 and 12) against the numpy restatement of appendix Y's rule Y5 composed
with the 8-bit restatement (tests/yuv16_ref.py).  Integer work: bit-exact.  Contexts are 16x16 and sources tens of pixels:
every path of the kernel (generic, exact x2, identity; windows smaller than the frame; both layouts; both alignments;
saturating and junk-carrying samples) at the smallest sizes that take it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                      # before the library initialises the device: torch's HIP runtime comes first (as in test_gpu_device_io)
    import torch
except ImportError:
    torch = None

import yuv16_ref
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline, prefetch

OUT = (16, 16)

# (source w, h, row pitch in samples or None, resize, crop, layouts): the issue's table
GEOMS = {
    "generic_48x32": (48, 32, None, (16, 16), (0, 0), ("i420", "nv12")),
    "x2_32x32": (32, 32, None, (16, 16), (0, 0), ("i420", "nv12")),
    "identity_16x16": (16, 16, None, (16, 16), (0, 0), ("i420", "nv12")),
    "vr_48x32": (48, 32, None, (32, 32), (0, 16), ("i420", "nv12")),              # window smaller than the frame
    "upscale_34x18_odd_crop": (34, 18, None, (40, 36), (7, 5), ("i420", "nv12")),
    "identity_640x64_col320": (640, 64, None, (640, 64), (333, 21), ("i420", "nv12")),   # window starts at column 320
    "nv12_48x32_pitch128": (48, 32, 64, (16, 16), (0, 0), ("nv12",)),             # 128-byte rows of 48 samples
}

# (depth, msb_aligned or None = the layout's default, every 16-bit pattern, layouts)
CONTENTS = {
    "yuv420p10le": (10, False, False, ("i420",)),
    "p010": (10, True, False, ("nv12",)),
    "depth12": (12, None, False, ("i420", "nv12")),
    "depth16": (16, None, False, ("i420", "nv12")),
    "saturating_10bit_low": (10, False, True, ("i420", "nv12")),                 # samples >= 2^10 -> 255
    "p010_junk_low_bits": (10, True, True, ("nv12",)),                           # random bits below the sample
}


def place(frames, ctx, pitch):
    """the frames as they are (the staged path), or copied into the context's page-locked memory (the zero-copy path)"""
    if ctx is None:
        return frames
    h32, w = frames[0].shape
    pin = ctx.pinned_frames(len(frames), size=(pitch or w, h32 * 2 // 3), yuv=True, depth=16)
    assert pin.dtype == np.uint16
    pin[:, :, :w] = np.stack(frames)
    return [pin[i, :, :w] for i in range(len(frames))]


@pytest.mark.parametrize("zero_copy", [False, True], ids=["staged", "zero_copy"])
@pytest.mark.parametrize("geom", list(GEOMS))
def test_yuv16_frontend_bit_exact(geom, zero_copy):
    sw, sh, pitch, resize, crop, layouts = GEOMS[geom]
    runs = [(name, lay) + CONTENTS[name][:3] for name in CONTENTS for lay in CONTENTS[name][3] if lay in layouts]
    with _capi.Context(*OUT, max_batch=1, frame_slots=2 * len(runs)) as ctx:
        want = []
        for k, (name, lay, depth, msb, junk) in enumerate(runs):
            m = yuv16_ref.default_msb(lay) if msb is None else msb
            fr = place([yuv16_ref.random_frame(sw, sh, depth, m, 100 * k + i, pitch, junk) for i in range(2)],
                       ctx if zero_copy else None, pitch)
            ctx.upload_frames_yuv(2 * k, fr, lay, resize, crop, depth=depth, msb=msb)
            want += [(name, lay, yuv16_ref.operand(f, lay, depth, m, resize, crop, OUT)) for f in fr]
        for i, (name, lay, op) in enumerate(want):
            assert np.array_equal(ctx.download_frame(i), op), (name, lay, i)


@pytest.mark.parametrize("msb", [False, True], ids=["low", "high"])
@pytest.mark.parametrize("depth", [10, 16])
def test_widened_bytes_give_the_8bit_operands_on_the_device(depth, msb):
    """metamorphic, the device alone: f.astype(uint16) << (depth - 8) under the new call == f under upload_frames_yuv"""
    with _capi.Context(*OUT, max_batch=1, frame_slots=8) as ctx:
        k = 0
        for lay in ("i420", "nv12"):
            for sw, sh, resize, crop in [(48, 32, (16, 16), (0, 0)), (34, 18, (40, 36), (7, 5))]:
                f = yuv_ref.random_frame(sw, sh, lay, 7 + k)
                ctx.upload_frames_yuv(k, [f], lay, resize, crop)
                ctx.upload_frames_yuv(k + 1, [yuv16_ref.widen(f, depth, msb)], lay, resize, crop, depth=depth, msb=msb)
                assert np.array_equal(ctx.download_frame(k), ctx.download_frame(k + 1)), (lay, sw, sh)
                k += 2


def test_device_tensors_equal_the_host_call():
    """torch.uint16 tensors through ffl_upload_frames_device16: contiguous frames, a padded-pitch view, one batched array"""
    if torch is None:
        pytest.skip("needs torch")
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")   # noqa: E731
    with _capi.Context(*OUT, max_batch=1, frame_slots=16) as ctx:
        def same(first, host, tens, lay, resize, crop, **kw):
            n = len(host)
            ctx.upload_frames_yuv(first, host, lay, resize, crop, **kw)
            ctx.upload_frames_device(first + n, tens, lay, resize, crop, **kw)
            for i in range(n):
                m = kw.get("msb", yuv16_ref.default_msb(lay))
                op = yuv16_ref.operand(host[i], lay, kw["depth"], m, resize, crop, OUT)
                assert np.array_equal(ctx.download_frame(first + i), op), (lay, i)
                assert np.array_equal(ctx.download_frame(first + n + i), op), (lay, i, "device")
        for lay, depth in (("i420", 10), ("nv12", 10), ("nv12", 16)):                # contiguous, the layout's alignment
            f = [yuv16_ref.random_frame(48, 32, depth, lay == "nv12", 3 + i, junk=True) for i in range(2)]
            same(0, f, [dev(x) for x in f], lay, (32, 32), (0, 16), depth=depth)
        wide = yuv16_ref.random_frame(48, 32, 12, False, 9, pitch=64)                # 128-byte rows, low-aligned NV12
        same(4, [wide], [dev(wide.base)[:, :48]], "nv12", (16, 16), (0, 0), depth=12, msb=False)
        batch = np.stack([yuv16_ref.random_frame(34, 18, 10, False, 20 + i) for i in range(3)])   # (n, 3h/2, w)
        same(6, list(batch), dev(batch), "i420", (40, 36), (7, 5), depth=10)
        same(6, list(batch), dev(batch), "nv12", (40, 36), (7, 5), depth=10, msb=False)
        # refusals: an odd pitch, a uint8 tensor with depth=10, a capturing stream -- and the context works afterwards
        t16 = dev(batch[0])
        row = np.array([[t16.data_ptr(), t16.data_ptr() + 18 * 69, 0, 69, 69, 0, 1, 0]], np.int64)
        assert ctx.L.ffl_upload_frames_device16(ctx._h, 0, 1, row.ctypes.data, 4, 10, 0, 34, 18, 40, 36, 7, 5, 0) == _capi.FFL_ERR_INVALID
        assert b"odd pitch" in ctx.L.ffl_last_error(ctx._h)
        with pytest.raises(ValueError, match="depth=10 needs uint16 frames"):
            ctx.upload_frames_device(0, [dev(np.zeros((27, 34), np.uint8))], "i420", (40, 36), (7, 5), depth=10)
        with pytest.raises(ValueError, match="pass depth=9..16"):
            ctx.upload_frames_device(0, [t16], "i420", (40, 36), (7, 5))
        class Huge:   # a frame far beyond the tensor's allocation
            __cuda_array_interface__ = {"version": 2, "data": (t16.data_ptr(), False), "shape": (49152, 32768), "strides": None,
                                        "typestr": "<u2"}
        with pytest.raises(_capi.FFLError, match="more than its allocation holds"):
            ctx.upload_frames_device(0, [Huge()], "nv12", (16, 16), (0, 0), depth=10)
        g, codes = torch.cuda.CUDAGraph(), []
        x = torch.zeros(16, device="cuda:0")
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                ctx.upload_frames_device(0, [t16], "i420", (40, 36), (7, 5), stream=torch.cuda.current_stream(), depth=10)
            except _capi.FFLError as err:
                codes.append(err.code)
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [_capi.FFL_ERR_STATE] and float(x.sum()) == 16.0
        same(6, list(batch), dev(batch), "i420", (40, 36), (7, 5), depth=10)


def test_ring_reuse_across_8bit_and_16bit_uploads():
    """more frames than ring buffers; 8-bit and 16-bit uploads of growing and shrinking sources share the ring"""
    with _capi.Context(*OUT, max_batch=1, frame_slots=24) as ctx:
        plan = [("i420", 48, 32, 8, 7), ("nv12", 96, 64, 10, 5), ("i420", 34, 18, 8, 3), ("i420", 160, 90, 12, 5),
                ("nv12", 32, 32, 8, 2), ("nv12", 48, 32, 16, 2)]
        slot, want = 0, []
        for k, (lay, sw, sh, depth, n) in enumerate(plan):
            if depth == 8:
                fr = [yuv_ref.random_frame(sw, sh, lay, 50 * k + i) for i in range(n)]
                frontend.upload_decoded(ctx, slot, fr, yuv=lay)
                want += [yuv_ref.operand(f, lay, OUT, (0, 0), OUT) for f in fr]
            else:
                m = yuv16_ref.default_msb(lay)
                fr = [yuv16_ref.random_frame(sw, sh, depth, m, 50 * k + i) for i in range(n)]
                frontend.upload_decoded(ctx, slot, fr, yuv=lay, depth=depth)
                want += [yuv16_ref.operand(f, lay, depth, m, OUT, (0, 0), OUT) for f in fr]
            slot += n
        for i, op in enumerate(want):
            assert np.array_equal(ctx.download_frame(i), op), i


def test_every_refusal_leaves_the_context_working():
    f = yuv16_ref.random_frame(48, 32, 10, False, 1)
    nv = yuv16_ref.random_frame(48, 32, 10, True, 2)
    with _capi.Context(*OUT, max_batch=1, frame_slots=2) as ctx:
        def still_works():
            ctx.upload_frames_yuv(1, [nv], "nv12", (16, 16), depth=10)
            assert np.array_equal(ctx.download_frame(1), yuv16_ref.operand(nv, "nv12", 10, True, (16, 16), (0, 0), OUT))

        def refused(rule, *a, exc=_capi.FFLError, **k):
            with pytest.raises(exc, match=rule):
                ctx.upload_frames_yuv(*a, **k)
            with pytest.raises(_capi.FFLError):
                ctx.download_frame(0)                                  # nothing was uploaded by the refused call
            still_works()

        refused("bad frame slot range", 5, [f], "i420", (16, 16), depth=10)
        refused("does not fit", 0, [f], "i420", (12, 20), depth=10)
        refused("does not fit", 0, [f], "nv12", (16, 16), (1, 0), depth=10)
        refused("even width and height", 0, [f[:, :47]], "nv12", (16, 16), depth=10)
        refused("3h/2 rows", 0, [f[:-1]], "i420", (16, 16), depth=10)
        refused(r"I420 needs stride == 2 \* width", 0, [np.zeros((48, 64), np.uint16)[:, :48]], "i420", (16, 16), depth=10)
        refused("depth=10 needs uint16 frames, got uint8", 0, [f.astype(np.uint8)], "i420", (16, 16), depth=10)
        refused("uint16 frames need their bit depth", 0, [f], "i420", (16, 16))
        refused("depth must be 8", 0, [f], "i420", (16, 16), exc=ValueError, depth=17)
        refused("layout", 0, [f], "p010", (16, 16), exc=ValueError, depth=10)
        L, vp = ctx.L, C.c_void_p

        def raw(rule, frames, stride, layout, depth, n=1):
            ptrs = (vp * len(frames))(*frames) if frames is not None else None
            assert L.ffl_upload_frames_yuv16(ctx._h, 0, n, ptrs, 48, 32, stride, layout, depth, 0, 16, 16, 0, 0) == _capi.FFL_ERR_INVALID
            assert rule in L.ffl_last_error(ctx._h), L.ffl_last_error(ctx._h)
            with pytest.raises(_capi.FFLError):
                ctx.download_frame(0)
            still_works()

        p = f.ctypes.data
        raw(b"depth 8 outside 9..16", [p], 96, 0, 8)
        raw(b"depth 17 outside 9..16", [p], 96, 0, 17)
        raw(b"odd stride 97", [p], 97, 1, 10)
        raw(b"frame 0 is not 2-byte aligned", [p + 1], 96, 0, 10)
        raw(b"NV12 needs stride >= 2 * width", [p], 94, 1, 10)
        raw(b"unknown layout 2", [p], 96, 2, 10)
        raw(b"frame 1 is NULL", [p, None], 96, 0, 10, n=2)
        raw(b"bad frame slot range", None, 96, 0, 10)


def yuv10_clip(n, sw, sh, seed):
    """smooth moving content as yuv420p10le frames whose low two bits are random: rounding decides many samples"""
    from funscript_flow_amd.synth import sine_translate_frames
    rng = np.random.default_rng(seed)
    out = []
    for f in sine_translate_frames(n, sw, sh, seed=seed, amp=(3.0, 2.0), period=7):
        c = f.reshape(sh // 2, 2, sw // 2, 2).astype(np.int32).mean(axis=(1, 3)).astype(np.uint8)
        f8 = np.concatenate([f.reshape(-1), (c // 2 + 64).reshape(-1), (255 - c).reshape(-1)]).reshape(sh * 3 // 2, sw)
        out.append(((f8.astype(np.uint16) << 2) | rng.integers(0, 4, f8.shape, dtype=np.uint16)).astype(np.uint16))
    return out


def test_video_to_actions_with_a_yuv420p10le_capture():
    """params["hip_yuv"] = "i420", ["hip_yuv_depth"] = 10: a (fake) capture whose read() yields (3h/2, w) uint16 frames is
    read into the context's page-locked uint16 ring and gives exactly frames_to_actions on the restated operands.  64x48
    clip, 3 chunks incl. a ragged one."""
    sw, sh, n, fps = 64, 48, 50, 30.0
    src = yuv10_clip(n, sw, sh, 6)

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
            assert image.dtype == np.uint16
            np.copyto(image, src[self.pos])
            self.pos += 1
            return True, image

    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False,
              "hip_yuv": "i420", "hip_yuv_depth": 10}
    cap = Cap()
    with _capi.Context(40, 32, max_batch=4, frame_slots=10, flow_slots=pipeline.min_flow_slots(4)) as ctx:
        got = prefetch.video_to_actions(ctx, cap, params)
        ops = [yuv16_ref.operand(f, "i420", 10, False, (40, 32), (0, 0), (40, 32)) for f in src]
        assert any(not np.array_equal(o, yuv_ref.operand((f >> 2).astype(np.uint8), "i420", (40, 32), (0, 0), (40, 32)))
                   for o, f in zip(ops, src))                                     # truncation would give other operands
        want = pipeline.frames_to_actions(pipeline.PairEngine(ctx), ops, fps,
                                          {k: v for k, v in params.items() if not k.startswith("hip_yuv")})
    assert cap.seeks == 0
    assert got == want and len(got) == 47
