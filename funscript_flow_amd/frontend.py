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

remap= replaces the one geometry of all of the above (resize, axis-aligned crop) by a per-output-pixel source map, applied by
a gather kernel where the operand is formed (`ffl_upload_frames_remap`, `ffl_upload_frames_device_remap`; DESIGN.md section
20, appendix R).  The reference's VR mode keeps a quadrant of the resized side-by-side equirectangular frame (FF:1076-1079),
which is not a rectilinear image; view_map() builds the map of a pinhole view of one eye instead, identity_map() the map that
ties the mechanism to the crop paths, map_valid_mask() the static weight map of the pixels a map covers.  The view parameters
are not tuned on footage, and the sampling rule's parity with cv2.remap is unpinned.
"""
import numpy as np

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


def _check_remap(remap, vr_mode):
    """remap= of the uploaders: a _capi.Remap of the context (Context.remap_create), never together with vr_mode"""
    if remap is None:
        return None
    if vr_mode:
        raise ValueError("remap= and vr_mode are two answers to one question: vr_mode keeps a quadrant of the resized frame "
                         "(FF:1076-1079), a source map (view_map) replaces resize and crop altogether -- pass one of them")
    if not isinstance(remap, _capi.Remap):
        raise TypeError("remap= takes the handle Context.remap_create returns")
    return remap


class DecodedUploader:
    """`upload` hook for pipeline.PairEngine: feeds it decoded frames instead of gray operands (yuv, depth, msb, rotate,
    mirror, yuv_range: see upload_decoded; all are checked here, at construction).  remap=: a source map of the context
    (Context.remap_create, view_map) forms the operand instead of resize and crop; refused together with vr_mode."""

    def __init__(self, ctx, vr_mode=False, rgb_order=False, yuv=None, depth=8, msb=None, rotate=0, mirror=False,
                 yuv_range="limited", remap=None):
        self.ctx, self.vr_mode, self.rgb_order = ctx, bool(vr_mode), bool(rgb_order)
        self.yuv, self.deep = _check_yuv(yuv, self.rgb_order, depth, msb)
        self.src = _check_source(self.yuv, rotate, mirror, yuv_range)
        self.remap = _check_remap(remap, self.vr_mode)

    def __call__(self, first_slot, frames):
        if self.remap is not None:
            fmt = self.yuv if self.yuv is not None else ("rgb" if self.rgb_order else "bgr")
            self.ctx.upload_frames_remap(first_slot, list(frames), self.remap, fmt, **self.deep, **self.src)
            return
        upload_decoded(self.ctx, first_slot, frames, self.vr_mode, self.rgb_order, self.yuv, **self.deep, **self.src)


class DeviceUploader:
    """`upload` hook for pipeline.PairEngine taking device-resident frames: a sequence of device
    arrays, or one (n, h, w[, c]) array, in format `fmt` ("gray", "bgr", "rgb", "i420", "nv12"; see _capi.device_frame)
    with geometry()'s resize and crop.  `stream`: see _capi.stream_handle (None: torch's current stream at each call).
    depth=9..16, msb: "i420" / "nv12" frames of uint16 samples (see Context.upload_frames_device).  rotate, mirror,
    yuv_range: the stream's metadata, which a GPU decoder's surfaces do not carry (see upload_decoded); checked here.
    remap=: as DecodedUploader's (one k_frontend_remap_dev launch per call)."""

    def __init__(self, ctx, fmt="bgr", vr_mode=False, stream=None, depth=8, msb=None, rotate=0, mirror=False,
                 yuv_range="limited", remap=None):
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
        self.remap = _check_remap(remap, bool(vr_mode))
        if not isinstance(ctx, _capi.Context):
            raise TypeError("DeviceUploader needs a funscript_flow_amd._capi.Context")
        self.ctx, self.fmt, self.vr_mode, self.stream = ctx, fmt, bool(vr_mode), stream
        self.resize, self.crop = geometry(ctx.width, ctx.height, self.vr_mode)

    def __call__(self, first_slot, frames):
        if self.remap is not None:
            self.ctx.upload_frames_device_remap(first_slot, frames, self.fmt, self.remap, self.stream, **self.deep, **self.src)
            return
        resize = None if self.fmt == "gray" and not self.vr_mode else self.resize   # gray: the context size, as it is
        self.ctx.upload_frames_device(first_slot, frames, self.fmt, resize, self.crop, self.stream, **self.deep, **self.src)


# ---- source maps ---------------------------------------------------------------------------
NO_SOURCE = _capi.REMAP_NO_SOURCE


def _supersample(supersample):
    if isinstance(supersample, bool) or supersample not in _capi.REMAP_SUPERSAMPLES:
        raise ValueError(f"supersample must be one of {_capi.REMAP_SUPERSAMPLES}, got {supersample!r}")
    return int(supersample)


def identity_map(out, origin=(0, 0), supersample=1):
    """The map whose sample (i, j) of the (S*oh, S*ow) grid reads source pixel (origin_x + j, origin_y + i) exactly (fraction
    0).  S = 1: output pixel (x, y) is source pixel origin + (x, y) -- the identity-mode operand of the crop paths at crop =
    origin; S = 2: output pixel (x, y) is the 2x2 mean of the source pixels 2 * (x, y) + origin .. + 1 -- their exact-half
    operand for an even origin."""
    S = _supersample(supersample)
    ow, oh = int(out[0]), int(out[1])
    m = np.empty((S * oh, S * ow, 2), np.int32)
    m[..., 0] = (32 * (int(origin[0]) + np.arange(S * ow, dtype=np.int64)))[None, :]
    m[..., 1] = (32 * (int(origin[1]) + np.arange(S * oh, dtype=np.int64)))[:, None]
    return m


def map_valid_mask(map, supersample=1):
    """(oh, ow) uint8: 255 where all S*S samples of the output pixel have a source, else 0 -- a static weight map
    (params["hip_weights"]) that keeps the pixels a view does not fully cover out of pass 1 and 2."""
    S = _supersample(supersample)
    m = np.asarray(map)
    if m.ndim != 3 or m.shape[2] != 2 or m.shape[0] % S or m.shape[1] % S:
        raise ValueError(f"a source map at supersample={S} is (S*oh, S*ow, 2), got shape {m.shape}")
    ok = (m[..., 0] != NO_SOURCE).reshape(m.shape[0] // S, S, m.shape[1] // S, S)
    return np.where(ok.all(axis=(1, 3)), 255, 0).astype(np.uint8)


def eye_rect(src_size, stereo=None, eye="left"):
    """(x, y, w, h) of one eye inside an upright src_size = (w, h) frame: stereo None (the whole frame), "sbs" (side by side:
    left eye in the left half) or "tb" (top-bottom: left eye in the top half); eye "left" | "right"."""
    w, h = int(src_size[0]), int(src_size[1])
    if eye not in ("left", "right"):
        raise ValueError(f"eye must be \"left\" or \"right\", got {eye!r}")
    second = eye == "right"
    if stereo is None:
        return (0, 0, w, h)
    if stereo == "sbs":
        return (w // 2 if second else 0, 0, w // 2, h)
    if stereo == "tb":
        return (0, h // 2 if second else 0, w, h // 2)
    raise ValueError(f"stereo must be None, \"sbs\" or \"tb\", got {stereo!r}")


PROJECTIONS = ("equirect", "fisheye")


def view_map(src_size, out, projection, fov, yaw=0, pitch=0, roll=0, src_hfov=180, src_vfov=180, rect=None, supersample=1):
    """The source map of a pinhole view into an equirectangular or equidistant-fisheye image (all angles in degrees), in
    float64 numpy.  The sample grid is H x W = (S*oh, S*ow) with focal length f = (W/2) / tan(fov/2); sample (i, j) looks
    along ((j + .5 - W/2) / f, (i + .5 - H/2) / f, 1), x right, y down, turned by Ry(yaw) Rx(pitch) Rz(roll): yaw > 0 looks
    right, pitch > 0 looks up, roll turns the view about its axis.  With (X, Y, Z) the turned ray and (x0, y0, w, h) = rect
    (None: the whole src_size frame; eye_rect() gives one eye):
      "equirect"  lon = atan2(X, Z), lat = atan2(Y, hypot(X, Z)); sx = x0 + (lon / hfov + .5) w - .5, sy = y0 + (lat / vfov
                  + .5) h - .5; no source outside +-src_hfov/2 or +-src_vfov/2.
      "fisheye"   theta = atan2(hypot(X, Y), Z), radius theta / (src_hfov/2) * min(w, h)/2 about the centre of rect along
                  (X, Y); no source beyond src_hfov/2 (src_vfov is not used).
    q = rint(32 s), clamped to the rectangle -- a clamped coordinate has fraction 0, so the neighbouring eye never blends in
    -- and samples without a source get NO_SOURCE.  Nothing here is tuned on footage: fov and the angles are the caller's."""
    S = _supersample(supersample)
    if projection not in PROJECTIONS:
        raise ValueError(f"projection must be one of {PROJECTIONS}, got {projection!r}")
    if not 0 < float(fov) < 180:
        raise ValueError(f"fov must be inside (0, 180) degrees for a pinhole view, got {fov!r}")
    if not (0 < float(src_hfov) <= 360 and 0 < float(src_vfov) <= 180):
        raise ValueError(f"src_hfov must be inside (0, 360] and src_vfov inside (0, 180], got {src_hfov!r}, {src_vfov!r}")
    x0, y0, w, h = (0, 0, int(src_size[0]), int(src_size[1])) if rect is None else (int(v) for v in rect)
    if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > src_size[0] or y0 + h > src_size[1]:
        raise ValueError(f"rect {(x0, y0, w, h)} does not lie inside the {src_size[0]}x{src_size[1]} source")
    W, H = S * int(out[0]), S * int(out[1])
    f = (W / 2.) / np.tan(np.radians(float(fov)) / 2.)
    rx = ((np.arange(W, dtype=np.float64) + .5 - W / 2.) / f)[None, :] + np.zeros((H, 1))
    ry = ((np.arange(H, dtype=np.float64) + .5 - H / 2.) / f)[:, None] + np.zeros((1, W))
    ray = np.stack([rx, ry, np.ones((H, W))], -1)
    a, b, c = np.radians(float(yaw)), np.radians(float(pitch)), np.radians(float(roll))
    Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])       # +yaw: the axis turns towards +x
    Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])       # +pitch: the axis turns towards -y
    Rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    X, Y, Z = np.moveaxis(ray @ (Ry @ Rx @ Rz).T, -1, 0)
    hf, vf = np.radians(float(src_hfov)), np.radians(float(src_vfov))
    if projection == "equirect":
        lon, lat = np.arctan2(X, Z), np.arctan2(Y, np.hypot(X, Z))
        sx = x0 + (lon / hf + .5) * w - .5
        sy = y0 + (lat / vf + .5) * h - .5
        valid = (np.abs(lon) <= hf / 2) & (np.abs(lat) <= vf / 2)
    else:
        rho = np.hypot(X, Y)
        theta = np.arctan2(rho, Z)
        rad = theta / (hf / 2) * (min(w, h) / 2.)
        ux, uy = np.divide(X, rho, out=np.zeros_like(X), where=rho > 0), np.divide(Y, rho, out=np.zeros_like(Y), where=rho > 0)
        sx = x0 + w / 2. - .5 + rad * ux
        sy = y0 + h / 2. - .5 + rad * uy
        valid = theta <= hf / 2
    qx = np.clip(np.rint(32. * sx), 32 * x0, 32 * (x0 + w - 1)).astype(np.int64)
    qy = np.clip(np.rint(32. * sy), 32 * y0, 32 * (y0 + h - 1)).astype(np.int64)
    m = np.empty((H, W, 2), np.int32)
    m[..., 0] = np.where(valid, qx, NO_SOURCE)
    m[..., 1] = np.where(valid, qy, 0)
    return m
