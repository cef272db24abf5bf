"""Input front-end of the HIP backend: decoded frames -> gray pair-kernel operands, on the device.

Mirrors what the reference does on the host to every decoded frame (FF = FunscriptFlow.pyw):

    AsyncVideoReader._decode_frame    cv2.cvtColor(BGR2RGB) FF:182, cv2.resize(frame, (256, 256)) FF:185-186
    fetch_frames_optimized, non-VR    cv2.cvtColor(f, COLOR_RGB2GRAY)                               FF:1082
    fetch_frames_optimized, VR        cv2.resize(f, (512, 512)); f[256:, :256]; RGB2GRAY            FF:1076-1079

One `ffl_upload_frames_raw` call does all of it (k_frontend): the frame is sent as decoded and only the
crop window of the resized image is ever computed.  No CPU fallback: without the HIP library this raises.

yuv="i420" | "nv12" takes a decoder's native 4:2:0 output instead -- (3h/2, w) uint8 arrays, as PyAV's yuv420p frames
or an `ffmpeg -pix_fmt yuv420p|nv12` pipe deliver them -- through `ffl_upload_frames_yuv` (k_frontend): the
colour conversion runs on the device and only the source rectangle the crop window reads crosses PCIe (DESIGN.md
section 11, appendix Y).  depth=9..16 beside it takes the same layouts in uint16 samples -- yuv420p10le is yuv="i420",
depth=10; P010 is yuv="nv12", depth=10 -- through `ffl_upload_frames_yuv16`, each sample reduced to 8 bits at its load
(rule Y5).

DeviceUploader takes frames that are already in device memory (torch tensors, a GPU decoder's DLPack surfaces) through
`ffl_upload_frames_device` (k_frontend_dev): the same operands with no host round trip.

rotate=, mirror=, yuv_range= carry the stream metadata cv2.VideoCapture.read applies before the reference sees a pixel
(FF:178) and raw decoder planes lack: the container's display rotation and the colour range (rules
Y6 and Y7).  They describe how the frames are STORED; the operand is that of the upright frame.  Nothing is detected
automatically -- and a cv2.VideoCapture BGR frame is upright already, so rotating it again is the trap.
"""
from . import _capi


def geometry(width, height, vr_mode=False):
    """(resize size, crop origin) that yield a `width` x `height` operand.  The reference's sizes are
    width = height = 256 (FF:1057); VR keeps the bottom-left quadrant of a 2x larger resize (FF:1076-1079)."""
    if vr_mode:
        return (2 * width, 2 * height), (0, height)
    return (width, height), (0, 0)


def _depth_hint(e):
    """the layout refusal, telling where the bit depth goes: it is no part of the layout's name"""
    return ValueError(f"{e}; the bit depth is a keyword of its own: 10-bit NV12 (P010) is yuv=\"nv12\", depth=10, "
                      "yuv420p10le is yuv=\"i420\", depth=10")


def _range_hint(e):
    """the metadata refusal, telling where rotation and range come from: they are properties of the stream"""
    return ValueError(f"{e}; rotate / mirror / yuv_range describe the stream: a portrait phone clip decoded to NV12 is "
                      "yuv=\"nv12\", rotate=90, full-range yuvj420p is yuv=\"i420\", yuv_range=\"full\"")


def _check_source(yuv, rotate=0, mirror=False, yuv_range="limited"):
    """the stream metadata keywords checked -> the keywords that travel (none when they say nothing)"""
    try:
        info = _capi.source_info(rotate, mirror, yuv_range)
    except ValueError as e:
        raise _range_hint(e) from None
    if info is None:
        return {}
    if info.full_range and yuv is None:
        raise _range_hint("yuv_range=\"full\" describes 4:2:0 frames: it needs yuv=\"i420\" | \"nv12\"")
    src = {}
    if info.rotate:
        src["rotate"] = info.rotate
    if info.mirror:
        src["mirror"] = True
    if info.full_range:
        src["yuv_range"] = "full"
    return src


def _check_yuv(yuv, rgb_order, depth=8, msb=None):
    """(yuv, keywords of upload_frames_yuv beyond the 8-bit ones) checked"""
    if yuv is None:
        if depth != 8 or msb is not None:
            raise ValueError("depth / msb describe 4:2:0 frames: they need yuv=\"i420\" | \"nv12\"")
        return None, {}
    if rgb_order:
        raise ValueError("rgb_order applies to 3-channel frames: it cannot be combined with yuv")
    try:
        _capi.yuv_layout(yuv)
    except ValueError as e:
        raise _depth_hint(e) from None
    depth, _ = _capi.yuv_depth(depth, yuv, msb)
    if depth == 8:
        if msb is not None:
            raise ValueError("msb describes uint16 frames: it needs depth=9..16")
        return yuv, {}
    return yuv, ({"depth": depth} if msb is None else {"depth": depth, "msb": bool(msb)})


def upload_decoded(ctx, first_slot, frames, vr_mode=False, rgb_order=False, yuv=None, depth=8, msb=None, rotate=0,
                   mirror=False, yuv_range="limited"):
    """frames: (h, w, 3) uint8 arrays as cv2.VideoCapture.read returns them (BGR; pass rgb_order=True for
    frames that already went through FF:182), or with yuv="i420" | "nv12" (3h/2, w) uint8 4:2:0 arrays -- uint16
    ones with depth=9..16 (msb: see Context.upload_frames_yuv) -- -> frame slots first_slot.. of `ctx`.
    rotate (0, 90, 180, 270: the clockwise rotation that makes the stored frame upright), mirror and yuv_range
    ("limited" | "full") are the stream's metadata (see _capi.source_info).  They are never read from a capture: frames
    out of cv2.VideoCapture.read are upright and range-expanded already, and rotating those again is the trap."""
    yuv, deep = _check_yuv(yuv, rgb_order, depth, msb)
    src = _check_source(yuv, rotate, mirror, yuv_range)
    if not isinstance(ctx, _capi.Context):
        raise TypeError("upload_decoded needs a funscript_flow_amd._capi.Context")
    resize, crop = geometry(ctx.width, ctx.height, vr_mode)
    if yuv is not None:
        ctx.upload_frames_yuv(first_slot, list(frames), yuv, resize, crop, **deep, **src)
    elif src:
        ctx.upload_frames_raw(first_slot, list(frames), resize, crop, rgb_order, **src)
    else:
        ctx.upload_frames_raw(first_slot, list(frames), resize, crop, rgb_order)


class DecodedUploader:
    """`upload` hook for pipeline.PairEngine: feeds it decoded frames instead of gray operands (yuv, depth, msb, rotate,
    mirror, yuv_range: see upload_decoded; all are checked here, at construction)."""

    def __init__(self, ctx, vr_mode=False, rgb_order=False, yuv=None, depth=8, msb=None, rotate=0, mirror=False,
                 yuv_range="limited"):
        self.ctx, self.vr_mode, self.rgb_order = ctx, bool(vr_mode), bool(rgb_order)
        self.yuv, self.deep = _check_yuv(yuv, self.rgb_order, depth, msb)
        self.src = _check_source(self.yuv, rotate, mirror, yuv_range)

    def __call__(self, first_slot, frames):
        upload_decoded(self.ctx, first_slot, frames, self.vr_mode, self.rgb_order, self.yuv, **self.deep, **self.src)


class DeviceUploader:
    """`upload` hook for pipeline.PairEngine taking device-resident frames: a sequence of device
    arrays, or one (n, h, w[, c]) array, in format `fmt` ("gray", "bgr", "rgb", "i420", "nv12"; see _capi.device_frame)
    with geometry()'s resize and crop.  `stream`: see _capi.stream_handle (None: torch's current stream at each call).
    depth=9..16, msb: "i420" / "nv12" frames of uint16 samples (see Context.upload_frames_device).  rotate, mirror,
    yuv_range: the stream's metadata, which a GPU decoder's surfaces do not carry (see upload_decoded); checked here."""

    def __init__(self, ctx, fmt="bgr", vr_mode=False, stream=None, depth=8, msb=None, rotate=0, mirror=False,
                 yuv_range="limited"):
        try:
            _capi.dev_format(fmt)
        except ValueError as e:
            raise _depth_hint(e) from None
        depth, _ = _capi.yuv_depth(depth, fmt, msb)
        if depth > 8 and str(fmt).lower() not in _capi.YUV_LAYOUTS:
            raise ValueError("depth > 8 applies to 4:2:0 frames (\"i420\", \"nv12\") only")
        if depth == 8 and msb is not None:
            raise ValueError("msb describes uint16 frames: it needs depth=9..16")
        self.deep = {} if depth == 8 else ({"depth": depth} if msb is None else {"depth": depth, "msb": bool(msb)})
        self.src = _check_source(fmt if str(fmt).lower() in _capi.YUV_LAYOUTS else None, rotate, mirror, yuv_range)
        if not isinstance(ctx, _capi.Context):
            raise TypeError("DeviceUploader needs a funscript_flow_amd._capi.Context")
        self.ctx, self.fmt, self.vr_mode, self.stream = ctx, fmt, bool(vr_mode), stream
        self.resize, self.crop = geometry(ctx.width, ctx.height, self.vr_mode)

    def __call__(self, first_slot, frames):
        resize = None if self.fmt == "gray" and not self.vr_mode else self.resize   # gray: the context size, as it is
        self.ctx.upload_frames_device(first_slot, frames, self.fmt, resize, self.crop, self.stream, **self.deep, **self.src)
