"""ctypes binding of libffl_hip.so (include/ffl.h).  No fallback: if the HIP library is missing or no
device is usable, loading / context creation raises."""
import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libffl_hip.so")

FFL_OK = 0
FFL_MAX_BATCH = 256
# kernel classes of ffl_profile_read
KERNEL_CLASSES = ["k_gray", "k_pyr_level", "k_polyexp", "k_frontend", "k_update_matrices", "k_blur_solve",
                  "k_pass1", "k_radial"]
FFL_PROFILE_ALL = 0xFF

# The records the library writes are numpy dtypes in the header's field order.  None of them has padding, so the packed
# dtype is the C layout; tests/test_abi_host.py compares every offset and size with the compiled header.
# the per-cell statistics grid and the variance centre: ffl_cell_record, ffl_grid_centre, FFL_MAX_CELLS
FFL_MAX_CELLS = 64
CELL_DTYPE = np.dtype([(k, "<f8") for k in ("mean_u", "mean_v", "mean_mag", "var_mag")])
GRID_CENTRE_DTYPE = np.dtype([("cx", "<f8"), ("cy", "<f8"), ("total_var", "<f8"), ("cells", "<i4"), ("empty", "<i4")])
CENTERS = ("variance", "track")   # params["hip_center"] / center=: estimators beside the default |div| argmax
# region tracking and ROI maps (appendices Q and E): the header's enums, ffl_track_state, ffl_track_record
FFL_MAX_TRACKS, FFL_MAX_TRACK_RADIUS = 8, 32
TRACK_ON_CUT = ("hold", "home")                            # FFL_TRACK_HOLD, FFL_TRACK_HOME
TRACK_OK, TRACK_CUT, TRACK_LOST, TRACK_CLAMPED = 0, 1, 2, 4   # status bits of a record
TRACK_STATE_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("home_x", "<f8"), ("home_y", "<f8"), ("steps", "<i8"),
                              ("lost_run", "<i4"), ("pad", "<i4")])
TRACK_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("du", "<f8"), ("dv", "<f8"), ("sw", "<f8"), ("count", "<i4"), ("status", "<i4")])
# template matching about tracked centres: the header's enums and ffl_match_record
FFL_MAX_MATCH_P, FFL_MAX_MATCH_S = 16, 16
MATCH_MODES = ("ssd", "zssd")                                 # FFL_MATCH_SSD, FFL_MATCH_ZSSD
MATCH_FLAT, MATCH_POOR, MATCH_AMBIGUOUS = 1, 2, 4             # status bits of a record; 0: accepted
# whole-frame re-detection: its records are MATCH_DTYPE
FFL_MAX_REDETECT_EXCLUDE, REDETECT_SKIPPED = 32, 8            # rule L5's square at most; the status of a search that did not run
MATCH_STATUS_OFFSET = 40                                      # a record's int32 `status`: rule L1's intended trigger word
MATCH_DTYPE = np.dtype([("x", "<f8"), ("y", "<f8"), ("dx", "<i4"), ("dy", "<i4"), ("cost", "<i8"), ("second", "<i8"),
                        ("status", "<i4"), ("pad", "<i4")])

# 4:2:0 layouts of ffl_upload_frames_yuv (FFL_YUV_I420, FFL_YUV_NV12): cv2's single-array (3h/2, w) uint8 frames
YUV_LAYOUTS = {"i420": 0, "nv12": 1}
# rule Y5: 9- to 16-bit samples in uint16 containers are a keyword of their own, depth=, beside the
# layout -- "nv12" with depth=10 is P010, "i420" with depth=10 is yuv420p10le
YUV_DEPTHS = range(8, 17)

# stream metadata (ffl_source_info; DESIGN.md appendix Y, rules Y6 and Y7): the keywords rotate=, mirror=, yuv_range=
ROTATIONS = (0, 90, 180, 270)
YUV_RANGES = {"limited": 0, "full": 1}

# device-memory I/O (ffl_upload_frames_device / ffl_export_flows): FFL_DEV_* and FFL_FLOW_* codes
DEV_FORMATS = {"gray": 0, "bgr": 1, "rgb": 2, "i420": 3, "nv12": 4}
# source maps of the front-end: the header's enum
FFL_MAX_REMAPS = 8
REMAP_NO_SOURCE = -2 ** 31   # FFL_REMAP_NO_SOURCE: qx of a sample with no source (rule R1)
REMAP_SUPERSAMPLES = (1, 2, 4)
FLOW_LAYOUTS = {"nhwc": 0, "nchw": 1}
FFL_ERR_INVALID, FFL_ERR_STATE = 1, 4
# flow import (ffl_import_flows): FFL_F32, FFL_F16, FFL_BF16 by __cuda_array_interface__ typestr
FLOW_DTYPES = {"<f4": 0, "<f2": 1, "bfloat16": 2}

# ffl_radial_window: ffl_pass2_record as a numpy structured dtype, and FFL_MAX_RADIUS
PASS2_DTYPE = np.dtype([("dot", "<f8"), ("cx", "<f8"), ("cy", "<f8"), ("mean_mag", "<f4"), ("div_val", "<f4"), ("x", "<i4"),
                        ("y", "<i4"), ("cut", "<i4"), ("pad", "<i4")])
FFL_MAX_RADIUS = 32
# the four motion components about the centre: FFL_AXIS_* in order, and ffl_axes_record -- a
# PASS2_DTYPE record, then components 1..3 and `reserved`
AXES = ("radial", "tangential", "shift_x", "shift_y")
PASS2_AXES_DTYPE = np.dtype(PASS2_DTYPE.descr + [(k, "<f8") for k in AXES[1:] + ("reserved",)])

# global-motion fit and compensation: FFL_MOTION_* models in order, the statuses, the
# twelve sums of rule C4 in order, and ffl_motion_record
MOTION_MODELS = ("translation", "rigid", "similarity", "affine")
MOTION_STATUS = ("ok", "empty", "degenerate")
MOTION_SUMS = ("S", "Sx", "Sy", "Sxx", "Sxy", "Syy", "Su", "Sux", "Suy", "Sv", "Svx", "Svy")
MOTION_DTYPE = np.dtype([(k, "<f8") for k in ("a0", "a1", "a2", "b0", "b1", "b2", "sw")] + [("model", "<i4"), ("status", "<i4")])

FLOWS = ("farneback", "dis")   # params["hip_flow"]: the reference's CPU/CUDA/OpenCL branch, or its "DNN" branch (FF:948-980)
DIS_STAGES = {"pass1": 0, "pass2": 1, "dense": 2, "refined": 3, "images": 4}   # ffl_debug_dis_pair stages


class DisParams(C.Structure):
    """ffl_dis_params; the defaults are PRESET_FAST."""
    _fields_ = [("finest_scale", C.c_int), ("patch_size", C.c_int), ("patch_stride", C.c_int),
                ("grad_descent_iters", C.c_int), ("var_refine_iters", C.c_int), ("vr_alpha", C.c_float),
                ("vr_gamma", C.c_float), ("vr_delta", C.c_float), ("use_mean_norm", C.c_int),
                ("use_spatial_prop", C.c_int), ("stripes", C.c_int)]
    FAST = dict(finest_scale=2, patch_size=8, patch_stride=4, grad_descent_iters=16, var_refine_iters=5, vr_alpha=20.0,
                vr_gamma=10.0, vr_delta=5.0, use_mean_norm=1, use_spatial_prop=1, stripes=0)

    def __init__(self, **over):
        unknown = set(over) - set(self.FAST)
        if unknown:
            raise ValueError(f"unknown DIS parameter(s) {sorted(unknown)}; known: {sorted(self.FAST)}")
        super().__init__(**{**self.FAST, **over})

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


def flow_choice(params):
    """("farneback", None) or ("dis", DisParams) from a reference params dict: "hip_flow" picks the algorithm
    (default "farneback"), "hip_dis" = {field: value} overrides single DIS parameters.  Unknown values raise ValueError, and so
    does "hip_dis" without "hip_flow": "dis" (it would otherwise be ignored)."""
    flow = params.get("hip_flow", "farneback")
    if flow not in FLOWS:
        raise ValueError(f"hip_flow must be one of {FLOWS}, got {flow!r}")
    if flow == "farneback":
        if params.get("hip_dis"):
            raise ValueError('"hip_dis" overrides DIS parameters: it needs "hip_flow": "dis"')
        return flow, None
    return flow, DisParams(**dict(params.get("hip_dis") or {}))


class FarnebackParams(C.Structure):
    """ffl_farneback_params with cv2.calcOpticalFlowFarneback's keyword names; the defaults are the reference's call
    (0.5, 3, 15, 3, 5, 1.2, 0), FF:878-879.  The rules are DESIGN.md appendix F."""
    _fields_ = [("pyr_scale", C.c_float), ("levels", C.c_int), ("winsize", C.c_int), ("iterations", C.c_int),
                ("poly_n", C.c_int), ("poly_sigma", C.c_float), ("flags", C.c_int)]
    DEFAULTS = dict(pyr_scale=0.5, levels=3, winsize=15, iterations=3, poly_n=5, poly_sigma=1.2, flags=0)
    INTS = ("levels", "winsize", "iterations", "poly_n", "flags")

    def __init__(self, **over):
        unknown = set(over) - set(self.DEFAULTS)
        if unknown:
            raise ValueError(f"unknown Farneback parameter(s) {sorted(unknown)}; known: {sorted(self.DEFAULTS)}")
        super().__init__(**{**self.DEFAULTS, **over})

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}

    def is_default(self):
        return bytes(self) == bytes(FarnebackParams())


class FFLError(RuntimeError):
    """A refused or failed library call; `code` is the FFL_ERR_* status (None where Python refused it)."""
    code = None


def _check(rc, ctx=None, exc=None, prefix=""):
    """The one place a non-zero status becomes an exception, with the message the library recorded for `ctx` (None: the
    calling thread's).  exc None: FFLError "ffl error <rc>: <message>" carrying `.code`; else exc(prefix + message)."""
    if rc == FFL_OK:
        return
    msg = load().ffl_last_error(ctx)
    msg = msg.decode() if msg else "refused"
    if exc is not None:
        raise exc(prefix + msg)
    err = FFLError(f"ffl error {rc}: {msg}")
    err.code = rc
    raise err


def _sizes(name, *args, outs=1):
    """the size_t results of a sizing call `name(ints..., size_t *...)`; FFLError "<name> failed: ..." when it refuses"""
    out = [C.c_size_t() for _ in range(outs)]
    _check(getattr(load(), name)(*map(int, args), *map(C.byref, out)), exc=FFLError, prefix=f"{name} failed: ")
    return out[0].value if outs == 1 else tuple(o.value for o in out)


def _src_call(L, name, info, *args):
    """name(*args), or its _src sibling with the SourceInfo appended when the stream has metadata (source_info)"""
    if info is None:
        return getattr(L, name)(*args)
    return getattr(L, name + "_src")(*args, C.byref(info))


def farneback_geometry(width, height, params=None):
    """(scales, working-set bytes per pair) of the general Farneback kernels; ValueError (with the library's reason) when
    the parameters or the size are refused."""
    p = params if params is not None else FarnebackParams()
    n, b = C.c_int(), C.c_size_t()
    _check(load().ffl_farneback_geometry(int(width), int(height), C.byref(p), C.byref(n), C.byref(b)), exc=ValueError,
           prefix=f"Farneback at {width}x{height} with {p.as_dict()}: ")
    return n.value, b.value


def farneback_extra_bytes(width, height, max_batch, params):
    """device bytes ffl_flow_pairs_farneback(params) may add to ffl_estimate_bytes (0 when the lane buffers suffice)"""
    b = C.c_size_t()
    _check(load().ffl_farneback_extra_bytes(int(width), int(height), int(max_batch), C.byref(params), C.byref(b)),
           exc=ValueError, prefix=f"Farneback at {width}x{height} with {params.as_dict()}: ")
    return b.value


def farneback_choice(params):
    """FarnebackParams from params["hip_farneback"] = {cv2 keyword: value}, or None for the reference's values (the tuned
    path).  ValueError for unknown names, values the rules refuse, or "hip_farneback" together with "hip_flow": "dis"."""
    over = params.get("hip_farneback")
    if not over:
        return None
    if params.get("hip_flow", "farneback") == "dis":
        raise ValueError('"hip_farneback" sets Farneback parameters: it cannot be combined with "hip_flow": "dis"')
    over = dict(over)
    for name, v in over.items():   # integer fields must be given whole numbers (no silent truncation)
        if name in FarnebackParams.INTS:
            if float(v) != int(v):
                raise ValueError(f"Farneback parameter {name} must be an integer, got {v!r}")
            over[name] = int(v)
    p = FarnebackParams(**over)
    _check(load().ffl_farneback_geometry(64, 64, C.byref(p), None, None), exc=ValueError, prefix=f"hip_farneback {dict(over)}: ")
    return None if p.is_default() else p


# the mode bits of ffl_flow_pairs_farneback_ex and the window names of params["hip_farneback_window"]
FFL_FB_USE_INITIAL_FLOW, FFL_FB_GAUSSIAN_WINDOW = 4, 256
FARNEBACK_WINDOWS = {"box": 0, "gaussian": FFL_FB_GAUSSIAN_WINDOW}


def farneback_window(window):
    """the mode bit of a window name; ValueError names the ones known"""
    if window not in FARNEBACK_WINDOWS:
        raise ValueError(f"Farneback window must be one of {tuple(FARNEBACK_WINDOWS)}, got {window!r}")
    return FARNEBACK_WINDOWS[window]


def farneback_mode(params):
    """"box" (the default) or "gaussian" from params["hip_farneback_window"]: the window of the Farneback batches
    (cv2.OPTFLOW_FARNEBACK_GAUSSIAN; "gaussian" always runs the general kernels, with "hip_farneback"'s numbers or the
    reference's).  ValueError for any other name, or for the key together with "hip_flow": "dis"."""
    if "hip_farneback_window" not in params:
        return "box"
    window = params["hip_farneback_window"]
    farneback_window(window)
    if params.get("hip_flow", "farneback") == "dis":
        raise ValueError('"hip_farneback_window" sets the Farneback window: it cannot be combined with "hip_flow": "dis"')
    return window


def dis_geometry(width, height, params=None):
    """(coarsest, finest) DIS scales of a frame size; ValueError when the size or the parameters are not supported."""
    c, f = C.c_int(), C.c_int()
    p = params if params is not None else DisParams()
    _check(load().ffl_dis_geometry(int(width), int(height), C.byref(p), C.byref(c), C.byref(f)), exc=ValueError,
           prefix=f"DIS does not support {width}x{height} with {p.as_dict()} (DESIGN.md appendix D2: patch_size 8, "
                  "sides divisible by 2^coarsest): ")
    return c.value, f.value


class DevFrame(C.Structure):
    """ffl_dev_frame: one frame in device memory, described by its planes (include/ffl.h).  device_frame() builds it;
    width / height are the frame's size."""
    _fields_ = [("plane", C.c_void_p * 3), ("pitch", C.c_ssize_t * 3), ("pixel_stride", C.c_ssize_t),
                ("channel_stride", C.c_ssize_t)]


def dev_format(fmt):
    """FFL_DEV_* code of "gray" / "bgr" / "rgb" / "i420" / "nv12"; ValueError for anything else"""
    if isinstance(fmt, str) and fmt.lower() in DEV_FORMATS:
        return DEV_FORMATS[fmt.lower()]
    raise ValueError(f"unknown device frame format {fmt!r}; known: {sorted(DEV_FORMATS)}")


def flow_layout(layout):
    """FFL_FLOW_* code of "nhwc" / "nchw"; ValueError for anything else"""
    if isinstance(layout, str) and layout.lower() in FLOW_LAYOUTS:
        return FLOW_LAYOUTS[layout.lower()]
    raise ValueError(f"unknown flow layout {layout!r}; known: {sorted(FLOW_LAYOUTS)}")


def _array_view(obj):
    """(data pointer, shape, byte strides, typestr) of a device array.  torch tensors are read directly (the per-frame
    cost of a batch of hundreds of views); anything else through __cuda_array_interface__ (v2 / v3), and DLPack producers
    on a GPU through torch.from_dlpack.  Host arrays are refused: they go through the host upload calls."""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(obj, torch.Tensor):
        if not obj.is_cuda:
            raise ValueError("not device memory: a CPU tensor (host frames go through upload_frames / upload_frames_raw / "
                             "upload_frames_yuv)")
        es = obj.element_size()
        ts = {torch.uint8: "|u1", torch.uint16: "<u2", torch.float32: "<f4"}.get(obj.dtype, str(obj.dtype))
        return obj.data_ptr(), tuple(obj.shape), tuple(st * es for st in obj.stride()), ts
    try:
        cai = obj.__cuda_array_interface__
    except AttributeError:
        cai = None
    if cai is None:
        dev = getattr(obj, "__dlpack_device__", None)
        if dev is not None and dev()[0] in (2, 10):   # kDLCUDA, kDLROCM
            import torch
            return _array_view(torch.from_dlpack(obj))
        raise ValueError(f"not device memory: {type(obj).__name__} has no __cuda_array_interface__ (host frames go through "
                         "upload_frames / upload_frames_raw / upload_frames_yuv)")
    if cai.get("version", 2) not in (2, 3):
        raise ValueError(f"__cuda_array_interface__ version {cai.get('version')} is not supported (2 or 3)")
    if cai.get("mask") is not None:
        raise ValueError("masked device arrays are not supported")
    shape, ts = tuple(int(d) for d in cai["shape"]), cai["typestr"]
    item = int(ts[2:]) if ts[2:].isdigit() else 1
    strides = cai.get("strides")
    if strides is None:   # C-contiguous
        strides, acc = [], item
        for d in reversed(shape):
            strides.insert(0, acc)
            acc *= d
    return int(cai["data"][0]), shape, tuple(int(v) for v in strides), ts


def _device_span(obj):
    """(data pointer, bytes) of a contiguous device array (see _array_view); ValueError for host memory or a strided view"""
    ptr, shp, st, ts = _array_view(obj)
    extent = obj.element_size() if hasattr(obj, "element_size") else int(ts[2:]) if ts[2:].isdigit() else 1
    for d, b in zip(reversed(shp), reversed(st)):
        if d > 1 and b != extent:
            raise ValueError(f"a contiguous device buffer is needed: shape {tuple(shp)} has byte strides {tuple(st)}")
        extent *= d
    return ptr, extent


class _DeviceSpan:
    """`nbytes` bytes of device memory at `ptr` as an object with __cuda_array_interface__ (a piece of a larger buffer)"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": (int(nbytes),), "strides": None,
                                         "typestr": "|u1"}


class SourceInfo(C.Structure):
    """ffl_source_info: display rotation, mirroring and colour range of a stream (include/ffl.h)"""
    _fields_ = [("rotate", C.c_int), ("mirror", C.c_int), ("full_range", C.c_int)]


def source_info(rotate=0, mirror=False, yuv_range="limited"):
    """The stream metadata keywords checked (rules Y6 and Y7) -> a SourceInfo, or None when they
    say nothing (the call then goes through the symbol without the _src suffix).  rotate: the clockwise rotation in
    degrees that makes the stored frame upright (0, 90, 180, 270: what PyAV / ffprobe report as the display rotation);
    mirror: a left-right flip after it; yuv_range: "limited" (16..235) or "full" (0..255, yuvj420p) for 4:2:0 frames.
    There is no auto-detection, and a cv2.VideoCapture BGR frame is upright already: rotating it again is wrong.
    ValueError for anything else; that full range needs a 4:2:0 source is the library's refusal."""
    if isinstance(rotate, bool) or not isinstance(rotate, (int, np.integer)) or rotate not in ROTATIONS:
        raise ValueError(f"rotate must be one of {ROTATIONS} (the clockwise rotation that makes the stored frame upright), "
                         f"got {rotate!r}")
    if not isinstance(mirror, (bool, np.bool_)) and mirror not in (0, 1):
        raise ValueError(f"mirror must be False or True (a left-right flip after the rotation), got {mirror!r}")
    if not isinstance(yuv_range, str) or yuv_range.lower() not in YUV_RANGES:
        raise ValueError(f"yuv_range must be one of {sorted(YUV_RANGES)}, got {yuv_range!r}; the range is a keyword of its "
                         "own: full-range yuvj420p is yuv=\"i420\", yuv_range=\"full\"")
    info = SourceInfo(int(rotate), int(bool(mirror)), YUV_RANGES[yuv_range.lower()])
    return info if (info.rotate or info.mirror or info.full_range) else None


def yuv_depth(depth, layout=None, msb=None):
    """(depth, msb_aligned) of rule Y5 checked: depth 8 (plain uint8 frames) or 9..16; msb None = where decoders put the
    bits -- high for "nv12" (P010 / P016), low for "i420" (yuv420p10le).  ValueError for anything else."""
    if isinstance(depth, bool) or not isinstance(depth, (int, np.integer)) or depth not in YUV_DEPTHS:
        raise ValueError(f"depth must be 8 (uint8 frames) or 9..16 (uint16 frames), got {depth!r}")
    if msb is None:
        msb = layout is not None and (layout == YUV_LAYOUTS["nv12"] or str(layout).lower() == "nv12")
    return int(depth), int(bool(msb))


def _frame_row(obj, code, depth=8):
    """the 8 fields of ffl_dev_frame (plane[3], pitch[3], pixel_stride, channel_stride) and (width, height) of one frame;
    depth > 8: a 4:2:0 frame of uint16 samples (typestr "<u2", strides in bytes as everywhere)"""
    ptr, shape, st, ts = _array_view(obj)
    if depth > 8:
        if code not in (DEV_FORMATS["i420"], DEV_FORMATS["nv12"]):
            raise ValueError("depth > 8 applies to 4:2:0 frames (\"i420\", \"nv12\") only")
        if ts != "<u2":
            raise ValueError(f"depth={depth} needs uint16 frames (typestr '<u2'), got {ts!r}; uint8 frames are depth=8")
    elif ts == "<u2":
        raise ValueError("uint16 frames need their bit depth: pass depth=9..16 (depth=8 means uint8 frames)")
    elif ts[1:] != "u1":
        raise ValueError(f"device frames must be uint8 (typestr '|u1'), got {ts!r}")
    es = 2 if depth > 8 else 1
    if code == DEV_FORMATS["gray"]:
        if len(shape) != 2:
            raise ValueError(f"a gray frame is (h, w), got shape {shape}")
        return (ptr, 0, 0, st[0], 0, 0, st[1], 0), (shape[1], shape[0])
    if code in (DEV_FORMATS["bgr"], DEV_FORMATS["rgb"]):
        if len(shape) == 3 and shape[2] in (3, 4):      # HWC packed (BGRA: channel 3 is never read)
            return (ptr, 0, 0, st[0], 0, 0, st[1], st[2]), (shape[1], shape[0])
        if len(shape) == 3 and shape[0] == 3:           # CHW planar
            return (ptr, 0, 0, st[1], 0, 0, st[2], st[0]), (shape[2], shape[1])
        raise ValueError(f"a 3-channel frame is (h, w, 3|4) or (3, h, w), got shape {shape}")
    if len(shape) != 2 or shape[0] % 3:
        raise ValueError(f"a 4:2:0 frame is one (3h/2, w) array, got shape {shape}")
    if st[1] != es:
        raise ValueError(f"4:2:0 rows must be contiguous (column stride {es}), got {st[1]}")
    w, h, pitch = shape[1], shape[0] * 2 // 3, st[0]
    if code == DEV_FORMATS["nv12"]:
        return (ptr, ptr + h * pitch, 0, pitch, pitch, 0, 1, 0), (w, h)
    if pitch != w * es:
        raise ValueError(f"I420 needs contiguous rows (row pitch == width), got pitch {pitch} for width {w}")
    u, cw = ptr + h * pitch, w // 2 * es
    return (ptr, u, u + (h // 2) * cw, pitch, cw, cw, 1, 0), (w, h)


def device_frame(obj, fmt, depth=8):
    """DevFrame (ffl_dev_frame + .width, .height) of a device array: any object with __cuda_array_interface__ (v2 / v3,
    typestr "|u1", byte strides) -- torch tensors included -- or a GPU DLPack producer.  fmt "gray": (h, w); "bgr" / "rgb":
    (h, w, 3) or (h, w, 4) packed, or (3, h, w) planar, any strides; "i420" / "nv12": cv2's single (3h/2, w) array (an
    NV12 row pitch may exceed w), with depth=9..16 of uint16 samples (typestr "<u2", torch.uint16).  ValueError names what
    is refused."""
    row, (w, h) = _frame_row(obj, dev_format(fmt), yuv_depth(depth)[0])
    f = DevFrame((C.c_void_p * 3)(*row[:3]), (C.c_ssize_t * 3)(*row[3:6]), row[6], row[7])
    f.width, f.height = w, h
    return f


def dev_frame_check(fmt, frame, resize, crop, out_size, depth=8, rotate=0, mirror=False, yuv_range="limited"):
    """ffl_dev_frame_check (depth > 8: ffl_dev_frame_check16) for a DevFrame: ValueError with the library's rule when it
    refuses (pure host check).  rotate, mirror, yuv_range: see source_info (the _src siblings; resize and crop are then in
    upright terms)."""
    info = source_info(rotate, mirror, yuv_range)
    geom = (frame.width, frame.height, C.byref(frame), int(resize[0]), int(resize[1]), int(crop[0]), int(crop[1]),
            int(out_size[0]), int(out_size[1]))
    if depth == 8:
        rc = _src_call(load(), "ffl_dev_frame_check", info, dev_format(fmt), *geom)
    else:
        rc = _src_call(load(), "ffl_dev_frame_check16", info, dev_format(fmt), int(depth), *geom)
    _check(rc, exc=ValueError)


class DevFlow(C.Structure):
    """ffl_dev_flow: n flow fields in device memory; item i, pixel (x, y), component c is at
    base + i * item_stride + y * row_pitch + x * pixel_stride + c * channel_stride (bytes, include/ffl.h)."""
    _fields_ = [("base", C.c_void_p), ("item_stride", C.c_ssize_t), ("row_pitch", C.c_ssize_t), ("pixel_stride", C.c_ssize_t),
                ("channel_stride", C.c_ssize_t)]


def _flow_view(obj):
    """(data pointer, shape, byte strides, typestr) of a device flow array; torch tensors are read directly (the only way
    to pass bfloat16, typestr "bfloat16"), anything else through __cuda_array_interface__."""
    torch = sys.modules.get("torch")
    if torch is not None and isinstance(obj, torch.Tensor):
        if not obj.is_cuda:
            raise ValueError("not device memory: a CPU tensor (host flow fields go through upload_flow)")
        ts = {torch.float32: "<f4", torch.float16: "<f2", torch.bfloat16: "bfloat16"}.get(obj.dtype, str(obj.dtype))
        es = obj.element_size()
        return obj.data_ptr(), tuple(obj.shape), tuple(st * es for st in obj.stride()), ts
    if getattr(obj, "__cuda_array_interface__", None) is None:
        raise ValueError(f"not device memory: {type(obj).__name__} has no __cuda_array_interface__ (host flow fields go "
                         "through upload_flow)")
    return _array_view(obj)


def device_flows(obj, width, height):
    """(DevFlow, dtype code, n) of a device array of flow fields: a torch tensor (float32, float16 or bfloat16) or an
    object with __cuda_array_interface__ ("<f4", "<f2"), shaped (n, H, W, 2), (n, 2, H, W) or a single (H, W, 2), any
    non-negative strides.  ValueError names what is refused: host memory, another dtype, another size or shape."""
    ptr, shape, st, ts = _flow_view(obj)
    if ts not in FLOW_DTYPES:
        raise ValueError(f"dtype {ts!r} is not supported: flow fields are float32, float16 or bfloat16 (float64 is not "
                         "accepted; convert it first)")
    W, H = int(width), int(height)
    if len(shape) == 3 and shape[2] == 2:
        if shape[:2] != (H, W):
            raise ValueError(f"size: a field of {shape[1]}x{shape[0]} does not match the context's {W}x{H} (no resizing)")
        return DevFlow(ptr, 0, st[0], st[1], st[2]), FLOW_DTYPES[ts], 1
    if len(shape) == 4 and shape[3] == 2 and shape[1:3] == (H, W):
        return DevFlow(ptr, st[0], st[1], st[2], st[3]), FLOW_DTYPES[ts], shape[0]
    if len(shape) == 4 and shape[1] == 2 and shape[2:] == (H, W):
        return DevFlow(ptr, st[0], st[2], st[3], st[1]), FLOW_DTYPES[ts], shape[0]
    if len(shape) == 4 and 2 in (shape[1], shape[3]):
        raise ValueError(f"size: fields of shape {shape} do not match the context's {W}x{H} (no resizing)")
    raise ValueError(f"shape: flow fields are (n, H, W, 2), (n, 2, H, W) or (H, W, 2), got {shape}")


def dev_flow_check(dtype, n, width, height, desc):
    """ffl_dev_flow_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_dev_flow_check(int(dtype), int(n), int(width), int(height), C.byref(desc)), exc=ValueError)


class DevWeights(C.Structure):
    """ffl_dev_weights: n weight maps (H, W) uint8 in device memory; item i, pixel (x, y) is at
    base + i * item_stride + y * row_pitch + x (bytes, include/ffl.h); item_stride 0: one map for all items."""
    _fields_ = [("base", C.c_void_p), ("item_stride", C.c_ssize_t), ("row_pitch", C.c_ssize_t)]


def device_weights(obj, width, height):
    """(DevWeights, n) of a torch device tensor of weight maps: uint8 or bool, (H, W) -- the static
    mask, n = 0: one map for however many items a call has -- or (n, H, W) with any item and row strides and unit pixel
    stride.  ValueError names what is refused: host memory, another dtype, another size or shape, a pixel stride."""
    torch = sys.modules.get("torch")
    if torch is None or not isinstance(obj, torch.Tensor):
        raise ValueError(f"not device memory: weight maps are torch device tensors, got {type(obj).__name__}")
    if obj.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"dtype {obj.dtype} is not supported: weight maps are uint8 or bool")
    shape, st = tuple(obj.shape), tuple(obj.stride())   # one byte per element
    W, H = int(width), int(height)
    if len(shape) not in (2, 3):
        raise ValueError(f"shape: weight maps are (H, W) or (n, H, W), got {shape}")
    if shape[-2:] != (H, W):
        raise ValueError(f"size: a map of {shape[-1]}x{shape[-2]} does not match the context's {W}x{H} (no resizing)")
    if st[-1] != 1:
        raise ValueError(f"pixel stride: the pixels of a row must be contiguous, the stride is {st[-1]}")
    if len(shape) == 3 and shape[0] < 1:
        raise ValueError("shape: no maps (n = 0)")
    if not obj.is_cuda:
        raise ValueError("not device memory: a CPU tensor (weight maps live in device memory)")
    if len(shape) == 2:
        return DevWeights(obj.data_ptr(), 0, st[0]), 0
    return DevWeights(obj.data_ptr(), st[0], st[1]), shape[0]


def dev_weights_check(n, width, height, desc):
    """ffl_dev_weights_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_dev_weights_check(int(n), int(width), int(height), None if desc is None else C.byref(desc)), exc=ValueError)


class ConsistencyParams(C.Structure):
    """ffl_consistency_params: thr = alpha * (|F|^2 + |B|^2) + beta, soft 1 (a ramp) or 0 (a
    threshold).  ConsistencyParams() holds the library's defaults; keywords override single fields."""
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("soft", C.c_int)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_consistency_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("alpha", "beta", "soft"):
                raise ValueError(f"unknown consistency parameter {k!r} (alpha, beta, soft)")
            setattr(self, k, v)

    def as_dict(self):
        return {"alpha": self.alpha, "beta": self.beta, "soft": self.soft}


def consistency_params_check(params):
    """ffl_consistency_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_consistency_params_check(None if params is None else C.byref(params)), exc=ValueError)


def consistency_choice(params):
    """a ConsistencyParams out of None (the defaults), a dict of its fields or a ConsistencyParams; checked"""
    if not isinstance(params, ConsistencyParams):
        params = ConsistencyParams(**dict(params or {}))
    consistency_params_check(params)
    return params


class ResidualParams(C.Structure):
    """ffl_residual_params: thr = alpha * (|gx| + |gy|) + beta in grey levels, soft 1 (a ramp) or 0 (a
    threshold).  ResidualParams() holds the library's defaults (the project's own choice, not tuned on footage); keywords
    override single fields."""
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("soft", C.c_int)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_residual_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("alpha", "beta", "soft"):
                raise ValueError(f"unknown residual parameter {k!r} (alpha, beta, soft)")
            setattr(self, k, v)

    def as_dict(self):
        return {"alpha": self.alpha, "beta": self.beta, "soft": self.soft}


def residual_params_check(params):
    """ffl_residual_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_residual_params_check(None if params is None else C.byref(params)), exc=ValueError)


def residual_choice(params):
    """a ResidualParams out of None (the defaults), a dict of its fields or a ResidualParams; checked"""
    if not isinstance(params, ResidualParams):
        params = ResidualParams(**dict(params or {}))
    residual_params_check(params)
    return params


class TextureParams(C.Structure):
    """ffl_texture_params: the window radius r (1..8, the window is (2r+1)^2), tau, the cornerness per
    window pixel at which the weight saturates (soft) or switches (hard), and soft 1 (a ramp) or 0 (a threshold).
    TextureParams() holds the library's defaults (the project's own choice, not tuned on footage); keywords override single
    fields."""
    _fields_ = [("radius", C.c_int), ("tau", C.c_float), ("soft", C.c_int)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_texture_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("radius", "tau", "soft"):
                raise ValueError(f"unknown texture parameter {k!r} (radius, tau, soft)")
            setattr(self, k, v)

    def as_dict(self):
        return {"radius": self.radius, "tau": self.tau, "soft": self.soft}


def texture_params_check(params):
    """ffl_texture_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_texture_params_check(None if params is None else C.byref(params)), exc=ValueError)


def texture_choice(params):
    """a TextureParams out of None or True (the defaults), a dict of its fields or a TextureParams; checked"""
    if not isinstance(params, TextureParams):
        params = TextureParams(**dict({} if params is None or params is True else params))
    texture_params_check(params)
    return params


def track_on_cut(on_cut):
    """FFL_TRACK_HOLD / FFL_TRACK_HOME of a name of TRACK_ON_CUT (or the code itself)"""
    if isinstance(on_cut, str):
        if on_cut not in TRACK_ON_CUT:
            raise ValueError(f"on_cut must be one of {TRACK_ON_CUT}, got {on_cut!r}")
        return TRACK_ON_CUT.index(on_cut)
    return int(on_cut)


class TrackParams(C.Structure):
    """ffl_track_params: the window radius r (1..32, the window is (2r+1)^2, clipped to the image),
    on_cut ("hold": the track stays where it is over a cut, "home": it returns to its home position) and the cut threshold of
    rule Q5.  TrackParams() holds the library's defaults (the radius is the project's own choice, not tuned on footage);
    keywords override single fields."""
    _fields_ = [("radius", C.c_int), ("on_cut", C.c_int), ("cut_threshold", C.c_float)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_track_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("radius", "on_cut", "cut_threshold"):
                raise ValueError(f"unknown track parameter {k!r} (radius, on_cut, cut_threshold)")
            setattr(self, k, track_on_cut(v) if k == "on_cut" else v)

    def as_dict(self):
        return {"radius": self.radius, "on_cut": TRACK_ON_CUT[self.on_cut] if self.on_cut in (0, 1) else self.on_cut,
                "cut_threshold": self.cut_threshold}


def track_params_check(params):
    """ffl_track_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_track_params_check(None if params is None else C.byref(params)), exc=ValueError)


def track_choice(params):
    """a TrackParams out of None (the defaults), a dict of its fields or a TrackParams; checked"""
    if not isinstance(params, TrackParams):
        params = TrackParams(**dict(params or {}))
    track_params_check(params)
    return params


class RoiParams(C.Structure):
    """ffl_roi_params: the ellipse's half-axes ax, ay in pixels (0.5..32768) and soft 1 (a paraboloid
    that falls from 255 at the centre to 0 at the ellipse) or 0 (255 inside, 0 outside).  RoiParams() holds the library's
    defaults (the project's own choice, not tuned on footage); keywords override single fields."""
    _fields_ = [("ax", C.c_float), ("ay", C.c_float), ("soft", C.c_int)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_roi_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("ax", "ay", "soft"):
                raise ValueError(f"unknown ROI parameter {k!r} (ax, ay, soft)")
            setattr(self, k, v)

    def as_dict(self):
        return {"ax": self.ax, "ay": self.ay, "soft": self.soft}


def roi_params_check(params):
    """ffl_roi_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_roi_params_check(None if params is None else C.byref(params)), exc=ValueError)


def roi_choice(params):
    """a RoiParams out of None (the defaults), a dict of its fields or a RoiParams; checked"""
    if not isinstance(params, RoiParams):
        params = RoiParams(**dict(params or {}))
    roi_params_check(params)
    return params


def match_mode(mode):
    """FFL_MATCH_SSD / FFL_MATCH_ZSSD of a name of MATCH_MODES (or the code itself)"""
    if isinstance(mode, str):
        if mode not in MATCH_MODES:
            raise ValueError(f"mode must be one of {MATCH_MODES}, got {mode!r}")
        return MATCH_MODES.index(mode)
    return int(mode)


MATCH_FIELDS = ("p", "s", "mode", "min_var", "max_mse", "ratio")


class MatchParams(C.Structure):
    """ffl_match_params: the template's half-side p (1..16, the template is (2p+1)^2), the search range
    s (1..16, |dx|, |dy| <= s), mode ("ssd" | "zssd": the zero-mean form, invariant to a brightness offset), and the three
    thresholds of rule N6: min_var (the template's own variance below which it is FLAT), max_mse (the mean squared
    difference above which the best match is POOR) and ratio (the best cost above ratio * the runner-up's is AMBIGUOUS).
    MatchParams() holds the library's defaults (the project's own choice, not tuned on footage); keywords override single
    fields."""
    _fields_ = [("p", C.c_int), ("s", C.c_int), ("mode", C.c_int), ("reserved", C.c_int), ("min_var", C.c_double),
                ("max_mse", C.c_double), ("ratio", C.c_double)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_match_default_params(C.byref(self))
        for k, v in over.items():
            if k not in MATCH_FIELDS:
                raise ValueError(f"unknown match parameter {k!r} {MATCH_FIELDS}")
            setattr(self, k, match_mode(v) if k == "mode" else v)

    def as_dict(self):
        return {"p": self.p, "s": self.s, "mode": MATCH_MODES[self.mode] if self.mode in (0, 1) else self.mode,
                "min_var": self.min_var, "max_mse": self.max_mse, "ratio": self.ratio}


def match_params_check(params):
    """ffl_match_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_match_params_check(None if params is None else C.byref(params)), exc=ValueError)


def match_choice(params):
    """a MatchParams out of None (the defaults), a dict of its fields or a MatchParams; checked"""
    if not isinstance(params, MatchParams):
        params = MatchParams(**dict(params or {}))
    match_params_check(params)
    return params


REDETECT_FIELDS = ("p", "mode", "exclude", "reach", "trigger_mask", "min_var", "max_mse", "ratio")


class RedetectParams(C.Structure):
    """ffl_redetect_params: p, mode and the three thresholds as MatchParams has them; exclude (1..32:
    the runner-up is the best candidate further than this, Chebyshev, from the best), reach (0: the whole frame; 1..32768:
    candidates within +-reach of the centre) and trigger_mask (a search runs iff its trigger word & trigger_mask != 0).
    RedetectParams() holds the library's defaults -- the match defaults with exclude = p, reach 0 and trigger_mask =
    MATCH_POOR; the project's own choice, not tuned on footage; keywords override single fields."""
    _fields_ = [("p", C.c_int), ("mode", C.c_int), ("exclude", C.c_int), ("reach", C.c_int), ("trigger_mask", C.c_int),
                ("reserved", C.c_int), ("min_var", C.c_double), ("max_mse", C.c_double), ("ratio", C.c_double)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_redetect_default_params(C.byref(self))
        for k, v in over.items():
            if k not in REDETECT_FIELDS:
                raise ValueError(f"unknown redetect parameter {k!r} {REDETECT_FIELDS}")
            setattr(self, k, match_mode(v) if k == "mode" else v)

    def as_dict(self):
        return {"p": self.p, "mode": MATCH_MODES[self.mode] if self.mode in (0, 1) else self.mode, "exclude": self.exclude,
                "reach": self.reach, "trigger_mask": self.trigger_mask, "min_var": self.min_var, "max_mse": self.max_mse,
                "ratio": self.ratio}


def redetect_params_check(params):
    """ffl_redetect_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_redetect_params_check(None if params is None else C.byref(params)), exc=ValueError)


def redetect_choice(params):
    """a RedetectParams out of None (the defaults), a dict of its fields or a RedetectParams; checked"""
    if not isinstance(params, RedetectParams):
        params = RedetectParams(**dict(params or {}))
    redetect_params_check(params)
    return params


class MotionParams(C.Structure):
    """ffl_motion_params: the sub-model of rule C2 (a name of MOTION_MODELS or its code), the passes of
    rule C7 and the Cauchy scale tau of rule C3 in pixels.  MotionParams() holds the library's defaults (rule C9: translation,
    3 passes, tau 1.0 -- the project's own choice, not tuned on footage); keywords override single fields."""
    _fields_ = [("model", C.c_int), ("iterations", C.c_int), ("tau", C.c_float)]

    def __init__(self, **over):
        super().__init__()
        load().ffl_motion_default_params(C.byref(self))
        for k, v in over.items():
            if k not in ("model", "iterations", "tau"):
                raise ValueError(f"unknown motion parameter {k!r} (model, iterations, tau)")
            setattr(self, k, motion_model(v) if k == "model" else v)

    def as_dict(self):
        return {"model": MOTION_MODELS[self.model], "iterations": self.iterations, "tau": self.tau}


def motion_model(model):
    """FFL_MOTION_* code of a name of MOTION_MODELS (or of the code itself); ValueError for anything else"""
    if isinstance(model, str) and model.lower() in MOTION_MODELS:
        return MOTION_MODELS.index(model.lower())
    if not isinstance(model, (str, bool)) and model in range(len(MOTION_MODELS)):
        return int(model)
    raise ValueError(f"motion model must be one of {MOTION_MODELS}, got {model!r}")


def motion_params_check(params):
    """ffl_motion_params_check: ValueError with the library's rule when it refuses (pure host check)."""
    _check(load().ffl_motion_params_check(None if params is None else C.byref(params)), exc=ValueError)


def motion_choice(compensate):
    """a checked MotionParams out of a model name, a dict of its fields or a MotionParams (compensate= / params["hip_compensate"])"""
    if isinstance(compensate, str):
        compensate = {"model": compensate}
    if not isinstance(compensate, MotionParams):
        compensate = MotionParams(**dict(compensate))
    motion_params_check(compensate)
    return compensate


def motion_solve(sums, model):
    """ffl_motion_solve: rules C5 and C6 on twelve float64 sums in MOTION_SUMS' order -> one MOTION_DTYPE record (a numpy
    array of shape ()).  The host compiles the source of the device's solve, so these are the device's bits.  Needs no device."""
    ps, keep = _darr(sums)
    if keep.shape != (len(MOTION_SUMS),):
        raise ValueError(f"motion_solve: {len(MOTION_SUMS)} sums are needed, got shape {keep.shape}")
    out = np.zeros((), MOTION_DTYPE)
    _check(load().ffl_motion_solve(ps, motion_model(model), out.ctypes.data), exc=ValueError)
    return out


def _model_entries(models, n, name):
    """(pointer, byte stride) of n models in device memory: a float64 (n, 6) array, rows any multiple of 8 bytes apart, or a
    contiguous buffer of n MOTION_DTYPE records"""
    ptr, shp, st, ts = _array_view(models)
    if ts in ("<f8", "torch.float64") and len(shp) == 2:
        if shp != (n, 6) or st[1] != 8:
            raise ValueError(f"{name}: float64 shape {shp} with byte strides {st}, ({n}, 6) with adjacent coefficients is needed")
        return ptr, (st[0] if n > 1 else 48)
    ptr, extent = _device_span(models)
    if extent < n * MOTION_DTYPE.itemsize:
        raise ValueError(f"{name}: {extent} bytes, {n} motion records need {n * MOTION_DTYPE.itemsize}")
    return ptr, MOTION_DTYPE.itemsize


def stream_handle(stream, device=0):
    """hipStream_t of `stream` as an int: None = torch's current stream on `device` when torch is already imported (else
    0, the null stream); a torch.cuda.Stream; or an int as it is."""
    if stream is None:
        torch = sys.modules.get("torch")
        return int(torch.cuda.current_stream(device).cuda_stream) if torch is not None else 0
    if isinstance(stream, int):
        return stream
    handle = getattr(stream, "cuda_stream", None)
    if handle is None:
        raise TypeError(f"stream must be None, an int or a torch.cuda.Stream, got {type(stream).__name__}")
    return int(handle)


def yuv_layout(layout):
    """FFL_YUV_* code of "i420" / "nv12" (or of the code itself); ValueError for anything else"""
    if isinstance(layout, str) and layout.lower() in YUV_LAYOUTS:
        return YUV_LAYOUTS[layout.lower()]
    if not isinstance(layout, str) and layout in YUV_LAYOUTS.values():
        return int(layout)
    raise ValueError(f"YUV layout must be one of {sorted(YUV_LAYOUTS)}, got {layout!r}")


def frontend_yuv_window(src_size, layout, resize, crop, out_size, stride=None, depth=8, rotate=0, mirror=False,
                        yuv_range="limited"):
    """((x, y, w, h), bytes per frame) of the source rectangle ffl_upload_frames_yuv transfers for a src_size = (w, h)
    4:2:0 frame, resized to `resize` = (w, h) and cropped at `crop` = (x, y) to out_size = (w, h).
    ValueError with the library's reason for what it refuses.  stride (bytes) defaults to a packed row; an int layout is
    passed to the library as it is.  depth != 8: ffl_frontend_yuv16_window for uint16 samples, to which the depth goes
    as it is -- the same rectangle in samples, twice the bytes.  rotate, mirror, yuv_range: see source_info (the _src
    siblings): src_size and the rectangle stay in stored terms, resize and crop are in upright ones."""
    sw, sh = int(src_size[0]), int(src_size[1])
    win, b = (C.c_int * 4)(), C.c_size_t()
    code = layout if isinstance(layout, int) else yuv_layout(layout)
    info = source_info(rotate, mirror, yuv_range)
    geom = (int(resize[0]), int(resize[1]), int(crop[0]), int(crop[1]), int(out_size[0]), int(out_size[1]), win, C.byref(b))
    if depth == 8:
        rc = _src_call(load(), "ffl_frontend_yuv_window", info, sw, sh, code, int(sw if stride is None else stride), *geom)
    else:
        rc = _src_call(load(), "ffl_frontend_yuv16_window", info, sw, sh, code, int(2 * sw if stride is None else stride),
                       int(depth), *geom)
    _check(rc, exc=ValueError)
    return tuple(win), b.value


def _map_array(map, out_size, supersample):
    """a source map as the C-contiguous (S*oh, S*ow, 2) int32 array the library reads; ValueError for another shape or S"""
    if supersample not in REMAP_SUPERSAMPLES or isinstance(supersample, bool):
        raise ValueError(f"supersample must be one of {REMAP_SUPERSAMPLES}, got {supersample!r}")
    m = np.asarray(map)
    want = (supersample * int(out_size[1]), supersample * int(out_size[0]), 2)
    if m.dtype != np.int32 or m.shape != want:
        raise ValueError(f"a source map for a {out_size[0]}x{out_size[1]} operand at supersample={supersample} is an int32 array of "
                         f"shape {want} holding (qx, qy) in 1/32 px, got {m.dtype} {m.shape}")
    return np.ascontiguousarray(m)


def remap_check(map, out_size, src_size, supersample=1, rotate=0, mirror=False, yuv_range="limited"):
    """ffl_remap_check: rules R1 and R6 of DESIGN.md appendix R for `map` (see Context.remap_create) over a STORED
    src_size = (w, h) source with the stream metadata of source_info -> (upright tap window (x, y, w, h), the stored window
    a host 4:2:0 frame transfers, number of valid entries).  Pure host check; ValueError with the library's rule."""
    info = source_info(rotate, mirror, yuv_range)
    m = _map_array(map, out_size, supersample)
    up, st, valid = (C.c_int * 4)(), (C.c_int * 4)(), C.c_size_t()
    _check(load().ffl_remap_check(m.ctypes.data, int(out_size[0]), int(out_size[1]), int(supersample), int(src_size[0]),
                                  int(src_size[1]), C.byref(info) if info is not None else None, up, st, C.byref(valid)),
           exc=ValueError)
    return tuple(up), tuple(st), valid.value


def remap_bytes(out_size, supersample=1):
    """device bytes one source map adds to a context of out_size (ffl_remap_bytes)"""
    return _sizes("ffl_remap_bytes", out_size[0], out_size[1], supersample)


class Remap:
    """A source map resident in a context (Context.remap_create): `id`, the upright `src_size` = (w, h) it addresses, its
    `supersample`, `window` = the upright bounding box (x, y, w, h) of every tap (rule R6) and `valid`, its valid entries."""

    def __init__(self, id, src_size, supersample, window, valid):
        self.id, self.src_size, self.supersample, self.window, self.valid = id, tuple(src_size), supersample, window, valid

    def __repr__(self):
        return f"Remap(id={self.id}, src_size={self.src_size}, supersample={self.supersample}, window={self.window})"


# ---- the C ABI, stated once --------------------------------------------------------------------------------------------------
# SIGNATURES holds every entry point of include/ffl.h, in the header's order, as (return type, parameter types).  load()
# applies it, EXPORTS is its keys, and tests/test_abi_host.py holds it against the prototypes parsed from the header, parameter
# by parameter.  A new entry point is added to the header and here, nowhere else.  Structs that Python passes with byref() are
# typed pointers; integer addresses (device pointers, numpy's .ctypes.data, descriptor rows) stay c_void_p.
_i, _u, _f, _pd, _sz, _u64, _vp, _str = C.c_int, C.c_uint, C.c_float, C.c_ssize_t, C.c_size_t, C.c_uint64, C.c_void_p, C.c_char_p
_ip, _i32p, _fp, _dp, _szp, _vpp = (C.POINTER(t) for t in (C.c_int, C.c_int32, C.c_float, C.c_double, C.c_size_t, C.c_void_p))
_P = C.POINTER
_ctx = _vp                                        # ffl_ctx *
_FRAMES = (_ctx, _i, _i, _vpp, _i, _i, _pd)       # ctx, first_slot, n, frames, src_width, src_height, stride_bytes
_DEVICE = (_ctx, _i, _i, _vp, _i)                 # ctx, first_slot, n, frames (rows of ffl_dev_frame), format
_YUV_WIN = (_i, _i, _i, _pd)                      # src_w, src_h, layout, stride_bytes
_PAIRS = (_ctx, _i, _ip, _ip, _ip, _i)            # ctx, n, fslot0, fslot1, flow_slots, pov_mode
_RADIAL = (_ctx, _i, _ip, _dp, _dp, _ip, _i, _dp)   # ctx, n, flow_slots, cx, cy, is_cut, pov_mode, out
_WINDOW = (_ctx, _i, _ip, _i, _i, _i, _f, _i)     # ctx, n_seq, seq_slots, first, n, radius, cut_threshold, pov_mode
_SRC = "_src"   # a front-end call's sibling: the parameters of the name without the suffix, then const ffl_source_info *
SIGNATURES = {
    "ffl_device_count": (_i, ()),
    "ffl_create": (_i, (_i,) * 6 + (_vpp,)),
    "ffl_destroy": (None, (_ctx,)),
    "ffl_last_error": (_str, (_ctx,)),
    "ffl_device_mem_info": (_i, (_i, _szp, _szp)),
    "ffl_estimate_bytes": (_i, (_i,) * 5 + (_szp, _szp)),
    "ffl_upload_frame": (_i, (_ctx, _i, _vp, _i, _i, _i, _pd)),
    "ffl_upload_frames": (_i, (_ctx, _i, _i, _vpp, _i, _i, _i, _pd)),
    "ffl_upload_frames_raw": (_i, _FRAMES + (_i,) * 5),
    "ffl_upload_frames_raw_src": _SRC,
    "ffl_upload_frames_yuv": (_i, _FRAMES + (_i,) * 5),
    "ffl_frontend_yuv_window": (_i, _YUV_WIN + (_i,) * 6 + (_ip, _szp)),
    "ffl_upload_frames_yuv_src": _SRC,
    "ffl_frontend_yuv_window_src": _SRC,
    "ffl_upload_frames_yuv16": (_i, _FRAMES + (_i,) * 7),
    "ffl_frontend_yuv16_window": (_i, _YUV_WIN + (_i,) * 7 + (_ip, _szp)),
    "ffl_upload_frames_yuv16_src": _SRC,
    "ffl_frontend_yuv16_window_src": _SRC,
    "ffl_dev_frame_check": (_i, (_i,) * 3 + (_P(DevFrame),) + (_i,) * 6),
    "ffl_upload_frames_device": (_i, _DEVICE + (_i,) * 6 + (_u64,)),
    "ffl_dev_frame_check16": (_i, (_i,) * 4 + (_P(DevFrame),) + (_i,) * 6),
    "ffl_upload_frames_device16": (_i, _DEVICE + (_i,) * 8 + (_u64,)),
    "ffl_dev_frame_check_src": _SRC,
    "ffl_dev_frame_check16_src": _SRC,
    "ffl_upload_frames_device_src": _SRC,
    "ffl_upload_frames_device16_src": _SRC,
    "ffl_remap_check": (_i, (_vp,) + (_i,) * 5 + (_P(SourceInfo), _ip, _ip, _szp)),
    "ffl_remap_bytes": (_i, (_i,) * 3 + (_szp,)),
    "ffl_remap_create": (_i, (_ctx, _vp, _i, _i, _i, _ip)),
    "ffl_remap_destroy": (_i, (_ctx, _i)),
    "ffl_upload_frames_remap": (_i, (_ctx, _i, _i, _vpp, _i, _i, _i, _pd, _i, _i, _i, _P(SourceInfo))),
    "ffl_upload_frames_device_remap": (_i, _DEVICE + (_i,) * 5 + (_u64, _P(SourceInfo))),
    "ffl_export_flows": (_i, (_ctx, _i, _ip, _vp, _i, _pd, _u64)),
    "ffl_dev_flow_check": (_i, (_i,) * 4 + (_P(DevFlow),)),
    "ffl_import_flows": (_i, (_ctx, _i, _ip, _P(DevFlow), _i, _i, _u64)),
    "ffl_host_alloc": (_i, (_ctx, _sz, _vpp)),
    "ffl_host_free": (_i, (_ctx, _vp)),
    "ffl_flow_pairs": (_i, _PAIRS),
    "ffl_pass1_result": (_i, (_ctx, _i, _f, _i32p, _i32p, _fp, _fp, _ip)),
    "ffl_pass1_results": (_i, (_ctx, _i, _ip, _f, _i32p, _i32p, _fp, _fp, _ip)),
    "ffl_radial": (_i, _RADIAL),
    "ffl_radial_window": (_i, _WINDOW + (_vp, _u64)),
    "ffl_radial_axes": (_i, _RADIAL),
    "ffl_radial_window_axes": (_i, _WINDOW + (_vp, _u64)),
    "ffl_axes_extra_bytes": (_i, (_i, _i, _szp)),
    "ffl_dev_weights_check": (_i, (_i,) * 3 + (_P(DevWeights),)),
    "ffl_pass1_weighted": (_i, (_ctx, _i, _ip, _P(DevWeights), _i, _u64)),
    "ffl_radial_window_axes_weighted": (_i, _WINDOW + (_P(DevWeights), _vp, _u64)),
    "ffl_weights_extra_bytes": (_i, (_i, _i, _szp)),
    "ffl_consistency_default_params": (_i, (_P(ConsistencyParams),)),
    "ffl_consistency_params_check": (_i, (_P(ConsistencyParams),)),
    "ffl_consistency_weights": (_i, (_ctx, _i, _ip, _ip, _P(ConsistencyParams), _P(DevWeights), _P(DevWeights), _u64)),
    "ffl_residual_default_params": (_i, (_P(ResidualParams),)),
    "ffl_residual_params_check": (_i, (_P(ResidualParams),)),
    "ffl_residual_weights": (_i, (_ctx, _i, _ip, _ip, _ip, _P(ResidualParams), _P(DevWeights), _P(DevWeights), _u64)),
    "ffl_texture_default_params": (_i, (_P(TextureParams),)),
    "ffl_texture_params_check": (_i, (_P(TextureParams),)),
    "ffl_texture_weights": (_i, (_ctx, _i, _ip, _P(TextureParams), _P(DevWeights), _P(DevWeights), _u64)),
    "ffl_cell_grid_check": (_i, (_i,) * 3 + (_ip, _ip)),
    "ffl_cell_stats": (_i, (_ctx, _i, _ip, _i, _vp, _vp, _u64)),
    "ffl_radial_window_axes_centres": (_i, _WINDOW + (_vp, _pd, _vp, _u64)),
    "ffl_cells_extra_bytes": (_i, (_i,) * 3 + (_szp,)),
    "ffl_track_default_params": (_i, (_P(TrackParams),)),
    "ffl_track_params_check": (_i, (_P(TrackParams),)),
    "ffl_track_advance": (_i, (_ctx, _i, _ip, _i, _P(TrackParams), _P(DevWeights), _vp, _vp, _u64)),
    "ffl_roi_default_params": (_i, (_P(RoiParams),)),
    "ffl_roi_params_check": (_i, (_P(RoiParams),)),
    "ffl_roi_weights": (_i, (_ctx, _i, _vp, _pd, _P(RoiParams), _P(DevWeights), _P(DevWeights), _u64)),
    "ffl_radial_window_axes_weighted_centres": (_i, _WINDOW + (_P(DevWeights), _vp, _pd, _vp, _u64)),
    "ffl_match_default_params": (_i, (_P(MatchParams),)),
    "ffl_match_params_check": (_i, (_P(MatchParams),)),
    "ffl_track_template": (_i, (_ctx, _i, _i, _vp, _i, _vp, _u64)),
    "ffl_track_match": (_i, (_ctx, _i, _ip, _i, _P(MatchParams), _vp, _vp, _pd, _i, _vp, _u64)),
    "ffl_redetect_default_params": (_i, (_P(RedetectParams),)),
    "ffl_redetect_params_check": (_i, (_P(RedetectParams),)),
    "ffl_redetect_extra_bytes": (_i, (_i,) * 3 + (_szp,)),
    "ffl_track_redetect": (_i, (_ctx, _i, _ip, _i, _P(RedetectParams), _vp, _vp, _pd, _vp, _pd, _i, _vp, _u64)),
    "ffl_motion_default_params": (_i, (_P(MotionParams),)),
    "ffl_motion_params_check": (_i, (_P(MotionParams),)),
    "ffl_motion_solve": (_i, (_dp, _i, _vp)),
    "ffl_motion_extra_bytes": (_i, (_i, _i, _szp)),
    "ffl_motion_fit": (_i, (_ctx, _i, _ip, _P(MotionParams), _P(DevWeights), _vp, _pd, _vp, _vp, _u64)),
    "ffl_motion_subtract": (_i, (_ctx, _i, _ip, _ip, _vp, _pd, _i, _u64)),
    "ffl_download_flow": (_i, (_ctx, _i, _vp)),
    "ffl_upload_flow": (_i, (_ctx, _i, _vp, _i)),
    "ffl_submit_pair": (_i, (_ctx, _i, _vp, _vp, _i, _i, _i, _pd, _i)),
    "ffl_sync": (_i, (_ctx,)),
    "ffl_dis_default_params": (_i, (_P(DisParams),)),
    "ffl_dis_geometry": (_i, (_i, _i, _P(DisParams), _ip, _ip)),
    "ffl_flow_pairs_dis": (_i, _PAIRS + (_P(DisParams),)),
    "ffl_debug_dis_pair": (_i, (_ctx, _i, _i, _P(DisParams), _i, _i, _vp)),
    "ffl_farneback_default_params": (_i, (_P(FarnebackParams),)),
    "ffl_farneback_geometry": (_i, (_i, _i, _P(FarnebackParams), _ip, _szp)),
    "ffl_farneback_extra_bytes": (_i, (_i,) * 3 + (_P(FarnebackParams), _szp)),
    "ffl_flow_pairs_farneback": (_i, _PAIRS + (_P(FarnebackParams),)),
    "ffl_flow_pairs_farneback_ex": (_i, _PAIRS + (_P(FarnebackParams), _u)),
    "ffl_num_levels": (_i, (_ctx,)),
    "ffl_level_size": (_i, (_ctx, _i, _ip)),
    "ffl_download_frame": (_i, (_ctx, _i, _vp)),
    "ffl_debug_pair": (_i, (_ctx,) + (_i,) * 4 + (_vp,) * 6),
    "ffl_debug_blur_plan": (_i, (_i,) * 9 + (_ip, _ip, _ip, _ip, _i)),
    "ffl_set_option": (_i, (_str, _i)),
    "ffl_ctx_set_option": (_i, (_ctx, _str, _i)),
    "ffl_ctx_get_option": (_i, (_ctx, _str, _ip)),
    "ffl_graph_stats": (_i, (_ctx, _ip, _ip, _ip)),
    "ffl_profile_enable": (_i, (_ctx, _u)),
    "ffl_profile_read": (_i, (_ctx, _i, _ip, _dp)),
    "ffl_kernel_name": (_str, (_i,)),
}
for _name, _sig in SIGNATURES.items():
    if _sig is _SRC:
        SIGNATURES[_name] = (SIGNATURES[_name[:-4]][0], SIGNATURES[_name[:-4]][1] + (_P(SourceInfo),))
EXPORTS = list(SIGNATURES)   # every symbol include/ffl.h declares
# the header's records and their Python statements (the test takes the struct names from the header: none can be forgotten)
RECORDS = {"ffl_source_info": SourceInfo, "ffl_dev_frame": DevFrame, "ffl_dev_flow": DevFlow, "ffl_pass2_record": PASS2_DTYPE,
           "ffl_axes_record": PASS2_AXES_DTYPE, "ffl_dev_weights": DevWeights, "ffl_consistency_params": ConsistencyParams,
           "ffl_residual_params": ResidualParams, "ffl_texture_params": TextureParams,
           "ffl_cell_record": CELL_DTYPE, "ffl_grid_centre": GRID_CENTRE_DTYPE, "ffl_motion_params": MotionParams,
           "ffl_motion_record": MOTION_DTYPE, "ffl_dis_params": DisParams, "ffl_track_params": TrackParams,
           "ffl_track_state": TRACK_STATE_DTYPE, "ffl_track_record": TRACK_DTYPE, "ffl_roi_params": RoiParams,
           "ffl_match_params": MatchParams, "ffl_match_record": MATCH_DTYPE, "ffl_redetect_params": RedetectParams,
           "ffl_farneback_params": FarnebackParams}

_lib = None


def load():
    """Load libffl_hip.so; raises FFLError if it has not been built (see __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FFLError(f"{LIB_PATH} is missing: build it with `make -C funscript_flow_amd/csrc` "
                       "(there is no CPU fallback for the HIP backend)")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def set_option(name, value):
    """Process-wide DEFAULT of a tuning knob (ffl_set_option): contexts created afterwards start from it; live contexts
    keep their own copy (Context.set_option).  Results do not depend on options."""
    if load().ffl_set_option(name.encode(), int(value)) != FFL_OK:
        raise FFLError(f"ffl_set_option({name!r}, {value}) rejected")


def get_option(name):
    """The process-wide default of a knob (ffl_ctx_get_option with no context)."""
    v = C.c_int()
    if load().ffl_ctx_get_option(None, name.encode(), C.byref(v)) != FFL_OK:
        raise FFLError(f"unknown option {name!r}")
    return v.value


def blur_plan(tiles_x, tiles_y, n_pairs, slots, blur_rows=0, blur_min_wgs=3500, blur_taper=0, blur_taper_pairs=0,
              tile_order=0, blocks=True):
    """ffl_debug_blur_plan: the launch plan of k_blur_solve for a level of tiles_x x tiles_y tiles and n_pairs pairs on
    `slots` workgroup slots -> (segments, grid, blocks).  segments: rows of (first workgroup, first pair, pairs, tiles per
    strip, strips per column); blocks: int32 (grid, 4) of (pair, tile column, first tile row, tiles) with pair -1 for padding
    workgroups, enumerated on the host with the kernel's own mapping (None with blocks=False).  Needs no device."""
    L = load()
    args = [int(v) for v in (tiles_x, tiles_y, n_pairs, slots, blur_rows, blur_min_wgs, blur_taper, blur_taper_pairs, tile_order)]
    seg, n, grid = (C.c_int * 15)(), C.c_int(), C.c_int()
    _check(L.ffl_debug_blur_plan(*args, seg, C.byref(n), C.byref(grid), None, 0), exc=ValueError)
    segments = [tuple(seg[5 * i:5 * i + 5]) for i in range(n.value)]
    if not blocks:
        return segments, grid.value, None
    out = np.zeros((grid.value, 4), np.int32)
    _check(L.ffl_debug_blur_plan(*args, seg, C.byref(n), C.byref(grid), out.ctypes.data_as(_ip), grid.value), exc=ValueError)
    return segments, grid.value, out


def device_count():
    return load().ffl_device_count()


def device_mem_info(device=0):
    """(free, total) bytes of device memory (hipMemGetInfo)."""
    return _sizes("ffl_device_mem_info", device, outs=2)


def estimate_bytes(width, height, frame_slots, flow_slots, max_batch):
    """(device, pinned host) bytes a Context with these arguments allocates under the current "lanes" option."""
    return _sizes("ffl_estimate_bytes", width, height, frame_slots, flow_slots, max_batch, outs=2)


def axes_extra_bytes(width, height):
    """Device bytes the first radial_axes / radial_window_axes call of a Context of this size allocates (estimate_bytes does
    not count them)."""
    return _sizes("ffl_axes_extra_bytes", width, height)


def weights_extra_bytes(width, height):
    """Device bytes the first pass1_weighted / radial_window_axes_weighted call of a Context of this size allocates
    (estimate_bytes does not count them)."""
    return _sizes("ffl_weights_extra_bytes", width, height)


def cells_extra_bytes(width, height, cells):
    """Device bytes the first cell_stats call of a Context allocates (estimate_bytes does not count them)."""
    return _sizes("ffl_cells_extra_bytes", width, height, cells)


def motion_extra_bytes(width, height):
    """Device bytes the first motion_fit call of a Context of this size allocates (estimate_bytes does not count them)."""
    return _sizes("ffl_motion_extra_bytes", width, height)


def redetect_extra_bytes(width, height, max_batch):
    """Device bytes the first track_redetect call of a Context of this size and max_batch allocates (estimate_bytes does not
    count them).  Needs no device."""
    return _sizes("ffl_redetect_extra_bytes", width, height, max_batch)


def cell_grid(width, height, cells):
    """(cell_w, cell_h) of a cells x cells grid on a width x height field (ffl_cell_grid_check; rule G1 of DESIGN.md section
    17); FFLError with the rule where the grid is refused.  Needs no device."""
    gw, gh = C.c_int(), C.c_int()
    _check(load().ffl_cell_grid_check(int(width), int(height), int(cells), C.byref(gw), C.byref(gh)))
    return gw.value, gh.value


def _centre_entries(centres, n_seq):
    """(pointer, byte stride) of n_seq centres in device memory: a float64 (n_seq, 2) array, rows any multiple of 8 bytes
    apart, a contiguous buffer of n_seq GRID_CENTRE_DTYPE records, or an explicit span (pointer or device buffer, byte
    stride) -- (track_buffer, 48 * tracks) reads track 0 of ffl_track_advance's records; the library checks such a span"""
    if isinstance(centres, tuple) and len(centres) == 2 and isinstance(centres[1], (int, np.integer)):
        base, stride = centres
        return (int(base) if isinstance(base, (int, np.integer)) else _array_view(base)[0]), int(stride)
    ptr, shp, st, ts = _array_view(centres)
    if ts in ("<f8", "torch.float64") and len(shp) == 2:
        if shp != (n_seq, 2) or st[1] != 8:
            raise ValueError(f"centres: float64 shape {shp} with byte strides {st}, ({n_seq}, 2) with adjacent (cx, cy) is needed")
        return ptr, (st[0] if n_seq > 1 else 16)
    ptr, extent = _device_span(centres)
    if extent < n_seq * GRID_CENTRE_DTYPE.itemsize:
        raise ValueError(f"centres: {extent} bytes, {n_seq} centre records need {n_seq * GRID_CENTRE_DTYPE.itemsize}")
    return ptr, GRID_CENTRE_DTYPE.itemsize


def _iarr(v):
    """int array argument: a C int pointer plus the object that keeps the memory alive (numpy does the conversion of a list
    or an array in C; element-by-element ctypes construction cost 30 us per 256 entries, three times per batch)"""
    a = np.ascontiguousarray(v, dtype=np.intc)
    return a.ctypes.data_as(C.POINTER(C.c_int)), a


def _darr(v):
    a = np.ascontiguousarray(v, dtype=np.float64)
    return a.ctypes.data_as(C.POINTER(C.c_double)), a


class Context:
    """One device context for frames of a fixed size (ffl_create / ffl_destroy)."""

    def __init__(self, width, height, device=0, frame_slots=None, flow_slots=None, max_batch=8):
        self.L = load()
        self.width, self.height, self.device, self.max_batch = int(width), int(height), int(device), int(max_batch)
        self.frame_slots = int(frame_slots if frame_slots is not None else 2 * max_batch + 2)
        self.flow_slots = int(flow_slots if flow_slots is not None else 13 + 2 * max_batch)
        h = C.c_void_p()
        rc = self.L.ffl_create(self.device, self.width, self.height, self.frame_slots, self.flow_slots, self.max_batch,
                               C.byref(h))
        if rc != FFL_OK:
            raise FFLError(f"ffl_create failed ({rc}): {self.L.ffl_last_error(None).decode()}")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self.L.ffl_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc != FFL_OK:   # tested here: the per-batch calls pay one comparison
            _check(rc, self._h)

    # ---- frames -------------------------------------------------------------------------------
    def upload_frame(self, fslot, frame):
        """frame: C-contiguous-rows uint8 (H,W) gray or (H,W,3) BGR, exactly what cv2 hands Python."""
        if frame.dtype != np.uint8 or frame.ndim not in (2, 3):
            raise FFLError("frame must be uint8 (H,W) or (H,W,3)")
        ch = 1 if frame.ndim == 2 else frame.shape[2]
        if frame.strides[-1] != 1 or (frame.ndim == 3 and frame.strides[1] != ch):
            frame = np.ascontiguousarray(frame)
        self._chk(self.L.ffl_upload_frame(self._h, fslot, frame.ctypes.data, frame.shape[1], frame.shape[0], ch,
                                          frame.strides[0]))

    def upload_frames(self, first_slot, frames):
        """frames: sequence of equally shaped uint8 frames -> consecutive slots, one H2D transfer."""
        f0 = frames[0]
        shape, strides = f0.shape, f0.strides
        if f0.dtype == np.uint8 and f0.ndim in (2, 3) and strides[-1] == 1 and (f0.ndim == 2 or strides[1] == shape[2]):
            # the common case -- every frame an ndarray of frame 0's shape and strides -- in one pass: at 256x256 a batch is
            # 257 frames, and what is done per frame in Python here is what the upload call costs the host
            n = len(frames)
            ptrs = np.empty(n, np.uintp)
            uniform = True
            for i, f in enumerate(frames):
                if f.shape != shape or f.strides != strides or f.dtype != np.uint8:
                    uniform = False          # the general path below converts or refuses it
                    break
                ptrs[i] = f.__array_interface__["data"][0]
            if uniform:
                ch = 1 if f0.ndim == 2 else shape[2]
                self._chk(self.L.ffl_upload_frames(self._h, first_slot, n, ptrs.ctypes.data_as(C.POINTER(C.c_void_p)), shape[1], shape[0],
                                                   ch, strides[0]))
                return
        fr = [f if (f.strides[-1] == 1 and (f.ndim == 2 or f.strides[1] == f.shape[2])) else np.ascontiguousarray(f)
              for f in frames]
        f0 = fr[0]
        ch = 1 if f0.ndim == 2 else f0.shape[2]
        if any(f.dtype != np.uint8 or f.shape != f0.shape or f.strides[0] != f0.strides[0] for f in fr):
            raise FFLError("upload_frames needs uint8 frames of one shape and row stride")
        ptrs = (C.c_void_p * len(fr))(*[f.ctypes.data for f in fr])
        self._chk(self.L.ffl_upload_frames(self._h, first_slot, len(fr), ptrs, f0.shape[1], f0.shape[0], ch,
                                           f0.strides[0]))

    def pinned_frames(self, n, channels=1, size=None, yuv=False, depth=8):
        """(n, height, width[, 3]) uint8 array in page-locked memory of this context (ffl_host_alloc): frames a
        decoder writes into consecutive entries go to the device without the staging copy.  Do not overwrite an
        entry before the batch that uses it has returned results (or ctx.sync()).  `size=(w, h)`: decoded source
        frames of another size, for upload_frames_raw.  yuv=True: (n, 3h/2, w) 4:2:0 frames for upload_frames_yuv
        (channels is ignored), uint16 ones with depth=9..16.  The memory belongs to the context: the array (and every
        view of it) must not be touched after ctx.close()."""
        w, h = size if size is not None else (self.width, self.height)
        shape = (n, h * 3 // 2, w) if yuv else (n, h, w) + ((channels,) if channels != 1 else ())
        dtype = np.uint8
        if depth != 8:
            if not yuv:
                raise FFLError("pinned_frames: depth applies to 4:2:0 frames (yuv=True)")
            dtype = np.uint16 if yuv_depth(depth)[0] > 8 else np.uint8
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self._chk(self.L.ffl_host_alloc(self._h, nbytes, C.byref(p)))
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        return np.frombuffer(buf, dtype).reshape(shape)

    def upload_frames_raw(self, first_slot, frames, resize, crop=(0, 0), rgb_order=False, rotate=0, mirror=False,
                          yuv_range="limited"):
        """Decoded (h, w, 3) uint8 frames -> gray(resize(frame, resize)[crop window]) in consecutive slots
        (cv2.resize / cv2.cvtColor 8-bit rules on the device; FF:182-186, FF:1076-1082).  rotate, mirror: the frames are
        stored unrotated (see source_info); resize and crop then describe the upright frame.  Frames out of
        cv2.VideoCapture.read are upright already.  yuv_range other than "limited" is the library's refusal here."""
        info = source_info(rotate, mirror, yuv_range)
        fr = [f if (f.ndim == 3 and f.strides[2] == 1 and f.strides[1] == 3) else np.ascontiguousarray(f) for f in frames]
        f0 = fr[0]
        if any(f.dtype != np.uint8 or f.ndim != 3 or f.shape != f0.shape or f.shape[2] != 3 or
               f.strides[0] != f0.strides[0] for f in fr):
            raise FFLError("upload_frames_raw needs (h, w, 3) uint8 frames of one shape and row stride")
        ptrs = (C.c_void_p * len(fr))(*[f.ctypes.data for f in fr])
        self._chk(_src_call(self.L, "ffl_upload_frames_raw", info, self._h, first_slot, len(fr), ptrs, f0.shape[1], f0.shape[0],
                            f0.strides[0], int(bool(rgb_order)), int(resize[0]), int(resize[1]), int(crop[0]), int(crop[1])))

    def upload_frames_yuv(self, first_slot, frames, layout, resize, crop=(0, 0), depth=8, msb=None, rotate=0, mirror=False,
                          yuv_range="limited"):
        """Decoded 4:2:0 frames -- (3h/2, w) uint8 arrays, cv2's single-array I420 / NV12 layout, layout "i420" or "nv12"
        -- -> gray(resize(YUV2BGR(frame), resize)[crop window]) in consecutive slots.  Only the
        source rectangle the window reads is transferred.  Rows must be contiguous (an NV12 row pitch may exceed w).
        depth=9..16: uint16 frames (yuv420p10le, P010, ...; ffl_upload_frames_yuv16), each sample reduced to 8 bits by
        rule Y5; msb: whether the bits sit high in the 16 (None: high for "nv12", low for "i420").  rotate, mirror,
        yuv_range: the stream's display rotation, mirroring and colour range (see source_info; rules Y6 and Y7); resize
        and crop then describe the upright frame, and the rectangle that travels is still one of the stored frame."""
        code = yuv_layout(layout)
        info = source_info(rotate, mirror, yuv_range)
        depth, msb = yuv_depth(depth, code, msb)
        dt, es = (np.uint16, 2) if depth > 8 else (np.uint8, 1)
        fr = [f if (f.ndim == 2 and f.strides[1] == f.itemsize) else np.ascontiguousarray(f) for f in frames]
        f0 = fr[0]
        if any(f.dtype == np.uint8 for f in fr) and depth > 8:
            raise FFLError(f"upload_frames_yuv: depth={depth} needs uint16 frames, got uint8 (uint8 frames are depth=8)")
        if any(f.dtype == np.uint16 for f in fr) and depth == 8:
            raise FFLError("upload_frames_yuv: uint16 frames need their bit depth: pass depth=9..16 (depth=8 means uint8 frames)")
        if any(f.dtype != dt or f.ndim != 2 or f.shape != f0.shape or f.strides[0] != f0.strides[0] for f in fr):
            raise FFLError(f"upload_frames_yuv needs (3h/2, w) {np.dtype(dt).name} frames of one shape and row stride")
        if f0.shape[0] % 3:
            raise FFLError(f"upload_frames_yuv: a 4:2:0 frame has 3h/2 rows, got {f0.shape[0]}")
        ptrs = (C.c_void_p * len(fr))(*[f.ctypes.data for f in fr])
        head = (self._h, first_slot, len(fr), ptrs, f0.shape[1], f0.shape[0] * 2 // 3, f0.strides[0], code)
        geom = (int(resize[0]), int(resize[1]), int(crop[0]), int(crop[1]))
        if es == 2:
            self._chk(_src_call(self.L, "ffl_upload_frames_yuv16", info, *head, depth, msb, *geom))
        else:
            self._chk(_src_call(self.L, "ffl_upload_frames_yuv", info, *head, *geom))

    def upload_frames_device(self, first_slot, frames, fmt, resize=None, crop=(0, 0), stream=None, depth=8, msb=None,
                             rotate=0, mirror=False, yuv_range="limited"):
        """Device-resident frames -> gray(resize(frame, resize)[crop window]) in consecutive slots without a host round
        trip (ffl_upload_frames_device): the bytes upload_frames_raw / upload_frames_yuv /
        upload_frames give for the same pixels.  `frames`: a sequence of device arrays (see device_frame) or one array with
        a leading frame axis, all of one size; fmt one of DEV_FORMATS; resize None = the source size.  The frames are read
        after the work queued on `stream` (stream_handle) and `stream` waits for the read: the caller may overwrite or free
        them in its order on that stream, with no host synchronisation.  depth=9..16, msb: "i420" / "nv12" frames of
        uint16 samples (torch.uint16, typestr "<u2"; ffl_upload_frames_device16), as upload_frames_yuv takes them.
        rotate, mirror, yuv_range: see source_info -- a GPU decoder's surfaces are stored unrotated; resize (None = the
        upright source size) and crop then describe the upright frame."""
        code = dev_format(fmt)
        depth, msb = yuv_depth(depth, fmt, msb)
        info = source_info(rotate, mirror, yuv_range)
        rows, size = self._device_rows(frames, code, depth)
        descs = np.ascontiguousarray(rows, np.int64)
        rw, rh = ((size[::-1] if info is not None and info.rotate in (90, 270) else size) if resize is None else resize)
        head = (self._h, int(first_slot), len(descs), descs.ctypes.data, code)
        geom = (size[0], size[1], int(rw), int(rh), int(crop[0]), int(crop[1]), stream_handle(stream, self.device))
        if depth > 8:
            self._chk(_src_call(self.L, "ffl_upload_frames_device16", info, *head, depth, msb, *geom))
        else:
            self._chk(_src_call(self.L, "ffl_upload_frames_device", info, *head, *geom))

    # ---- source maps -----------------------------------------------------
    def remap_create(self, map, src_size, supersample=1):
        """A source map for this context: an (S*height, S*width, 2) int32 array of (qx, qy), upright source coordinates in
        1/32 px of an upright src_size = (w, h) source, REMAP_NO_SOURCE in qx where a sample has none (frontend.view_map,
        frontend.identity_map build them).  Checked (rule R1), copied to the device; the array is not needed afterwards.
        Returns a Remap; at most FFL_MAX_REMAPS are alive per context."""
        m = _map_array(map, (self.width, self.height), supersample)
        window, _, valid = remap_check(m, (self.width, self.height), src_size, supersample)
        rid = C.c_int(-1)
        self._chk(self.L.ffl_remap_create(self._h, m.ctypes.data, int(supersample), int(src_size[0]), int(src_size[1]), C.byref(rid)))
        return Remap(rid.value, (int(src_size[0]), int(src_size[1])), int(supersample), window, valid)

    def remap_destroy(self, remap):
        """frees the map (a Remap or its id); safe straight after an upload call that used it"""
        self._chk(self.L.ffl_remap_destroy(self._h, int(getattr(remap, "id", remap))))

    def upload_frames_remap(self, first_slot, frames, remap, fmt="bgr", depth=8, msb=None, rotate=0, mirror=False,
                            yuv_range="limited"):
        """Host frames -> the operand `remap` gathers from them, in consecutive slots (ffl_upload_frames_remap; rules R2 to R6):
        fmt "bgr" / "rgb": (h, w, 3) uint8 frames, which travel whole; "i420" / "nv12": (3h/2, w) 4:2:0 arrays of uint8, or
        of uint16 with depth=9..16 and msb as upload_frames_yuv takes them -- only the rectangle the map's taps touch is
        transferred.  rotate, mirror, yuv_range: how the frames are STORED (see source_info); the map is in upright terms."""
        code = dev_format(fmt)
        info = source_info(rotate, mirror, yuv_range)
        yuv = code in (DEV_FORMATS["i420"], DEV_FORMATS["nv12"])
        depth, msb = yuv_depth(depth, fmt if yuv else None, msb)
        if yuv:
            dt = np.uint16 if depth > 8 else np.uint8
            fr = [f if (f.ndim == 2 and f.strides[1] == f.itemsize) else np.ascontiguousarray(f) for f in frames]
            f0 = fr[0]
            if any(f.dtype != dt or f.ndim != 2 or f.shape != f0.shape or f.strides[0] != f0.strides[0] for f in fr) or f0.shape[0] % 3:
                raise FFLError(f"upload_frames_remap needs (3h/2, w) {np.dtype(dt).name} frames of one shape and row stride for "
                               f"fmt={fmt!r}, depth={depth}")
            size = (f0.shape[1], f0.shape[0] * 2 // 3)
        else:
            fr = [f if (f.ndim == 3 and f.strides[2] == 1 and f.strides[1] == 3) else np.ascontiguousarray(f) for f in frames]
            f0 = fr[0]
            if any(f.dtype != np.uint8 or f.ndim != 3 or f.shape != f0.shape or f.shape[2] != 3 or f.strides[0] != f0.strides[0]
                   for f in fr):
                raise FFLError(f"upload_frames_remap needs (h, w, 3) uint8 frames of one shape and row stride for fmt={fmt!r}")
            size = (f0.shape[1], f0.shape[0])
        ptrs = (C.c_void_p * len(fr))(*[f.ctypes.data for f in fr])
        self._chk(self.L.ffl_upload_frames_remap(self._h, int(first_slot), len(fr), ptrs, code, size[0], size[1], f0.strides[0], depth,
                                                 msb, int(getattr(remap, "id", remap)), C.byref(info) if info is not None else None))

    def upload_frames_device_remap(self, first_slot, frames, fmt, remap, stream=None, depth=8, msb=None, rotate=0, mirror=False,
                                   yuv_range="limited"):
        """upload_frames_device through a source map (ffl_upload_frames_device_remap): device frames of any DEV_FORMATS
        format -- a "gray" frame of any size is gathered like a channel -- in one launch, under the stream contract of
        upload_frames_device."""
        code = dev_format(fmt)
        depth, msb = yuv_depth(depth, fmt, msb)
        info = source_info(rotate, mirror, yuv_range)
        rows, size = self._device_rows(frames, code, depth)
        descs = np.ascontiguousarray(rows, np.int64)
        self._chk(self.L.ffl_upload_frames_device_remap(self._h, int(first_slot), len(descs), descs.ctypes.data, code, depth, msb,
                                                        size[0], size[1], int(getattr(remap, "id", remap)),
                                                        stream_handle(stream, self.device),
                                                        C.byref(info) if info is not None else None))

    @staticmethod
    def _device_rows(frames, code, depth=8):
        """ffl_dev_frame rows of a frame sequence or of one batched array, and the common (width, height)"""
        nd = 3 if code in (DEV_FORMATS["bgr"], DEV_FORMATS["rgb"]) else 2
        view = None
        if not isinstance(frames, (list, tuple)):
            try:
                view = _array_view(frames)
            except ValueError:
                view = None                                  # another kind of sequence: frame by frame below
        if view is not None and len(view[1]) == nd + 1:     # one (n, ...) array: frame i starts i * stride[0] bytes in
            ptr, shp, st, ts = view
            class _One:   # frame 0's view; the others are offsets of it
                __cuda_array_interface__ = {"version": 2, "data": (ptr, False), "shape": shp[1:], "strides": st[1:], "typestr": ts}
            row, size = _frame_row(_One(), code, depth)
            rows = np.tile(np.asarray(row, np.int64), (shp[0], 1))
            for k in range(3):
                if row[k]:
                    rows[:, k] += np.arange(shp[0], dtype=np.int64) * st[0]
            return rows, size
        rows, size = [], None
        for f in frames:
            row, sz = _frame_row(f, code, depth)
            if size is not None and sz != size:
                raise ValueError(f"upload_frames_device needs frames of one size, got {size} and {sz}")
            rows.append(row)
            size = sz
        if not rows:
            raise ValueError("upload_frames_device: no frames")
        return rows, size

    def export_flows(self, flow_slots, out=None, layout="nhwc", stream=None):
        """The flow fields of flow_slots into device memory without a host round trip (ffl_export_flows): `out` a float32
        device array of (n, H, W, 2) ("nhwc", cv2's layout) or (n, 2, H, W) ("nchw"), each item contiguous, items any
        stride apart -- or None for a new torch tensor.  Bit for bit what download_flow returns.  Ordered after the batches
        that produced the slots and the work queued on `stream`; `stream` waits for the export.  Returns `out`."""
        code = flow_layout(layout)
        (ps, slots) = _iarr(flow_slots)
        n, H, W = len(slots), self.height, self.width
        shape = (n, H, W, 2) if code == 0 else (n, 2, H, W)
        handle = stream_handle(stream, self.device)
        if out is None:
            import torch
            dev = torch.device("cuda", self.device)
            if handle == torch.cuda.current_stream(dev).cuda_stream:
                out = torch.empty(shape, dtype=torch.float32, device=dev)
            else:   # allocated in the order of the stream that writes it
                with torch.cuda.stream(torch.cuda.ExternalStream(handle, device=dev)):
                    out = torch.empty(shape, dtype=torch.float32, device=dev)
        ptr, shp, st, ts = _array_view(out)
        if ts[1:] != "f4":
            raise ValueError(f"export_flows needs a float32 output, got typestr {ts!r}")
        if tuple(shp) != shape:
            raise ValueError(f"export_flows: output shape {tuple(shp)} is not {shape} ({layout})")
        inner = [4 * int(np.prod(shape[k + 1:])) for k in range(1, 4)]
        if any(st[k] != inner[k - 1] for k in range(1, 4) if shape[k] > 1):
            raise ValueError(f"export_flows: every item of the output must be contiguous, strides are {st}")
        self._chk(self.L.ffl_export_flows(self._h, n, ps, ptr, code, st[0], handle))
        return out

    def import_flows(self, flows, flow_slots, pov_mode=False, stream=None):
        """Caller flow fields in device memory -> flow_slots, with their pass-1 records (ffl_import_flows, DESIGN.md section
        13): upload_flow for every field in one launch, without the host.  `flows`: see device_flows (one field per slot).
        Each record equals upload_flow's for the float32 widening of the field.  The fields are read after the work queued
        on `stream` (None: torch's current stream) and `stream` waits for the read: the caller may overwrite or free them in
        its order on that stream.  Results are read with pass1_results; radial, export_flows and download_flow work on
        the slots as on any other."""
        desc, dt, n = device_flows(flows, self.width, self.height)
        if len(flow_slots) != n:
            raise ValueError(f"import_flows: {n} fields for {len(flow_slots)} flow slots")
        self.import_flows_desc(desc, dt, flow_slots, pov_mode, stream)

    def import_flows_desc(self, desc, dtype, flow_slots, pov_mode=False, stream=None):
        """import_flows for a DevFlow descriptor and FLOW_DTYPES code as device_flows returns them (one field per slot)."""
        ps, slots = _iarr(flow_slots)
        self._chk(self.L.ffl_import_flows(self._h, len(slots), ps, C.byref(desc), int(dtype), int(bool(pov_mode)),
                                          stream_handle(stream, self.device)))

    def flow_pairs(self, fslot0, fslot1, flow_slots, pov_mode=False):
        n = len(flow_slots)
        (p0, k0), (p1, k1), (ps, ks) = _iarr(fslot0), _iarr(fslot1), _iarr(flow_slots)
        if len(k0) != n or len(k1) != n:
            raise FFLError("flow_pairs: the three slot lists must have one entry per pair")
        self._chk(self.L.ffl_flow_pairs(self._h, n, p0, p1, ps, int(bool(pov_mode))))

    def flow_pairs_dis(self, fslot0, fslot1, flow_slots, pov_mode=False, params=None):
        """ffl_flow_pairs_dis: DIS flow (params: DisParams, None = PRESET_FAST) + pass 1 for a batch of pairs."""
        n = len(flow_slots)
        (p0, k0), (p1, k1), (ps, ks) = _iarr(fslot0), _iarr(fslot1), _iarr(flow_slots)
        if len(k0) != n or len(k1) != n:
            raise FFLError("flow_pairs_dis: the three slot lists must have one entry per pair")
        self._chk(self.L.ffl_flow_pairs_dis(self._h, n, p0, p1, ps, int(bool(pov_mode)),
                                            None if params is None else C.byref(params)))

    def flow_pairs_farneback(self, fslot0, fslot1, flow_slots, pov_mode=False, params=None, window="box",
                             initial_flow=False):
        """ffl_flow_pairs_farneback: Farneback with caller-chosen parameters (FarnebackParams; None or the defaults = the
        tuned path of flow_pairs) + pass 1 for a batch of pairs.  window "gaussian" and initial_flow (each pair starts from
        the flow its flow slot already holds, then overwrites it) are the modes of ffl_flow_pairs_farneback_ex, which is
        called only when one of them is set; either runs the general kernels."""
        n = len(flow_slots)
        (p0, k0), (p1, k1), (ps, ks) = _iarr(fslot0), _iarr(fslot1), _iarr(flow_slots)
        if len(k0) != n or len(k1) != n:
            raise FFLError("flow_pairs_farneback: the three slot lists must have one entry per pair")
        mode = farneback_window(window) | (FFL_FB_USE_INITIAL_FLOW if initial_flow else 0)
        pp = None if params is None else C.byref(params)
        if mode:
            self._chk(self.L.ffl_flow_pairs_farneback_ex(self._h, n, p0, p1, ps, int(bool(pov_mode)), pp, mode))
        else:
            self._chk(self.L.ffl_flow_pairs_farneback(self._h, n, p0, p1, ps, int(bool(pov_mode)), pp))

    def submit_pair(self, slot, prev, nxt, pov_mode=False):
        prev, nxt = np.ascontiguousarray(prev), np.ascontiguousarray(nxt)
        ch = 1 if prev.ndim == 2 else prev.shape[2]
        self._chk(self.L.ffl_submit_pair(self._h, slot, prev.ctypes.data, nxt.ctypes.data, prev.shape[1], prev.shape[0],
                                         ch, prev.strides[0], int(bool(pov_mode))))

    def pass1_result(self, flow_slot, cut_threshold=7.0):
        x, y, c = C.c_int32(), C.c_int32(), C.c_int()
        v, mm = C.c_float(), C.c_float()
        self._chk(self.L.ffl_pass1_result(self._h, flow_slot, float(cut_threshold), C.byref(x), C.byref(y), C.byref(v),
                                          C.byref(mm), C.byref(c)))
        return x.value, y.value, np.float32(v.value), np.float32(mm.value), bool(c.value)

    def pass1_results(self, flow_slots, cut_threshold=7.0):
        """ffl_pass1_results: the records of many slots with one call (list of pass1_result tuples)."""
        n = len(flow_slots)
        x, y, c = np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n, np.intc)
        v, mm = np.empty(n, np.float32), np.empty(n, np.float32)
        i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
        ps, ks = _iarr(flow_slots)
        self._chk(self.L.ffl_pass1_results(self._h, n, ps, float(cut_threshold), x.ctypes.data_as(i32), y.ctypes.data_as(i32),
                                           v.ctypes.data_as(f32), mm.ctypes.data_as(f32), c.ctypes.data_as(C.POINTER(C.c_int))))
        return list(zip(x.tolist(), y.tolist(), list(v), list(mm), (c != 0).tolist()))

    def _radial(self, call, out, flow_slots, centers, is_cut, pov_mode):
        n = len(flow_slots)
        cen = np.asarray(centers, np.float64).reshape(n, 2)
        (ps, ks), (px, kx), (py, ky) = _iarr(flow_slots), _darr(cen[:, 0]), _darr(cen[:, 1])
        pc, kc = _iarr(np.asarray(is_cut, bool))
        self._chk(call(self._h, n, ps, px, py, pc, int(bool(pov_mode)), out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def radial(self, flow_slots, centers, is_cut, pov_mode=False):
        return self._radial(self.L.ffl_radial, np.empty(len(flow_slots), np.float64), flow_slots, centers, is_cut, pov_mode).tolist()

    def radial_axes(self, flow_slots, centers, is_cut, pov_mode=False):
        """radial with the four components of AXES per item (ffl_radial_axes): float64[n, 4]; column 0
        has the bits of radial()."""
        return self._radial(self.L.ffl_radial_axes, np.empty((len(flow_slots), len(AXES)), np.float64), flow_slots, centers,
                            is_cut, pov_mode)

    def radial_window_axes(self, seq_slots, first, n, out, radius=6, cut_threshold=7.0, pov_mode=False, stream=None):
        """radial_window with PASS2_AXES_DTYPE records (ffl_radial_window_axes): `out` is device memory of at least n * 80
        bytes; a record's first 48 bytes are radial_window's, its further components the bits of radial_axes."""
        return self._radial_window(self.L.ffl_radial_window_axes, "radial_window_axes", PASS2_AXES_DTYPE, seq_slots, first, n,
                                   out, radius, cut_threshold, pov_mode, stream)

    def radial_window(self, seq_slots, first, n, out, radius=6, cut_threshold=7.0, pov_mode=False, stream=None):
        """The centre window, the cut test and pass 2 on the device without a host round trip (ffl_radial_window, DESIGN.md
        section 14): seq_slots are the flow slots of consecutive pairs in time order, items first .. first+n-1 of them go
        to out[0..n) as PASS2_DTYPE records -- pass1_results, smooth_centers over the window clipped to seq_slots, and
        radial, bit for bit.  `out`: device memory of at least n * 48 bytes (anything with __cuda_array_interface__, a
        torch tensor included).  Ordered after the batches that produced the slots and the work queued on `stream` (None:
        torch's current stream); `stream` waits for the records.  The host does not wait.  Returns `out`."""
        return self._radial_window(self.L.ffl_radial_window, "radial_window", PASS2_DTYPE, seq_slots, first, n, out, radius,
                                   cut_threshold, pov_mode, stream)

    def _radial_window(self, call, name, dtype, seq_slots, first, n, out, radius, cut_threshold, pov_mode, stream, weights=()):
        ptr, extent = _device_span(out)   # the records are written back to back
        if extent < int(n) * dtype.itemsize:
            raise ValueError(f"{name}: out holds {extent} bytes, {int(n)} records need {int(n) * dtype.itemsize}")
        ps, ks = _iarr(seq_slots)
        self._chk(call(self._h, len(ks), ps, int(first), int(n), int(radius), float(cut_threshold), int(bool(pov_mode)), *weights,
                       ptr, stream_handle(stream, self.device)))
        return out

    def _weights(self, name, weights, n):
        """the DevWeights of a call with n items: a descriptor as it is, or a tensor through device_weights"""
        if isinstance(weights, DevWeights):
            return weights
        desc, m = device_weights(weights, self.width, self.height)
        if m not in (0, int(n)):
            raise ValueError(f"{name}: {m} weight maps for {int(n)} items")
        return desc

    def pass1_weighted(self, flow_slots, weights, pov_mode=False, stream=None):
        """The pass-1 records of flow_slots recomputed under per-pixel weight maps (ffl_pass1_weighted, DESIGN.md section
        16): `weights` is a uint8 / bool device tensor, (H, W) for every slot or (n, H, W), one map per slot (or a
        DevWeights).  The flow is only read; the records stay until the slot is written again.  Queued behind the work on
        `stream` (None: torch's current stream), which waits for it; the host does not wait."""
        ps, slots = _iarr(flow_slots)
        desc = self._weights("pass1_weighted", weights, len(slots))
        self._chk(self.L.ffl_pass1_weighted(self._h, len(slots), ps, C.byref(desc), int(bool(pov_mode)),
                                            stream_handle(stream, self.device)))

    def radial_window_axes_weighted(self, seq_slots, first, n, weights, out, radius=6, cut_threshold=7.0, pov_mode=False,
                                    stream=None):
        """radial_window_axes with every term weighted by the maps of the n computed items (ffl_radial_window_axes_weighted):
        `weights` as in pass1_weighted, (H, W) or (n, H, W).  Windows, centres and the cut test come from the records the seq
        slots hold.  An all-ones map gives the bytes of radial_window_axes."""
        desc = self._weights("radial_window_axes_weighted", weights, n)
        return self._radial_window(self.L.ffl_radial_window_axes_weighted, "radial_window_axes_weighted", PASS2_AXES_DTYPE,
                                   seq_slots, first, n, out, radius, cut_threshold, pov_mode, stream, weights=(C.byref(desc),))

    def consistency_weights(self, fwd_slots, bwd_slots, out, params=None, gate=None, stream=None):
        """Forward-backward consistency maps (ffl_consistency_weights): item i from the forward field in
        flow slot fwd_slots[i] and the backward field in bwd_slots[i], written into `out`, a uint8 device tensor (n, H, W)
        (or a DevWeights; (H, W) for one item).  `params`: a ConsistencyParams, a dict of its fields or None (the defaults);
        `gate`: maps S of rule K6 as pass1_weighted takes maps, (H, W) or (n, H, W).  Queued behind the work on `stream` and
        the slots' last users; `stream` waits for it.  Returns `out`."""
        pf, fs = _iarr(fwd_slots)
        pb, bs = _iarr(bwd_slots)
        if len(fs) != len(bs):
            raise ValueError(f"consistency_weights: {len(fs)} forward slots for {len(bs)} backward slots")
        prm = params if isinstance(params, ConsistencyParams) else ConsistencyParams(**dict(params or {}))
        odesc = self._weights("consistency_weights", out, len(fs))
        gdesc = None if gate is None else self._weights("consistency_weights", gate, len(fs))
        self._chk(self.L.ffl_consistency_weights(self._h, len(fs), pf, pb, C.byref(prm), None if gdesc is None else C.byref(gdesc),
                                                 C.byref(odesc), stream_handle(stream, self.device)))
        return out

    def residual_weights(self, fslot0, fslot1, flow_slots, out, params=None, gate=None, stream=None):
        """Photometric-residual maps (ffl_residual_weights): item i from the gray frames in frame slots
        fslot0[i] and fslot1[i] (which may repeat between items) and the forward field in flow slot flow_slots[i], written into
        `out`, a uint8 device tensor (n, H, W) (or a DevWeights; (H, W) for one item).  `params`: a ResidualParams, a dict of
        its fields or None (the defaults, which are not tuned on footage); `gate`: maps S of rule P6 as pass1_weighted takes
        maps, (H, W) or (n, H, W).  Queued behind the work on `stream`, the frames' uploads and the flow slots' last users;
        `stream` waits for it, and a later upload into one of the frame slots runs behind it.  Returns `out`."""
        p0, f0 = _iarr(fslot0)
        p1, f1 = _iarr(fslot1)
        pf, fl = _iarr(flow_slots)
        if not len(f0) == len(f1) == len(fl):
            raise ValueError(f"residual_weights: {len(f0)} and {len(f1)} frame slots for {len(fl)} flow slots")
        prm = params if isinstance(params, ResidualParams) else ResidualParams(**dict(params or {}))
        odesc = self._weights("residual_weights", out, len(fl))
        gdesc = None if gate is None else self._weights("residual_weights", gate, len(fl))
        self._chk(self.L.ffl_residual_weights(self._h, len(fl), p0, p1, pf, C.byref(prm), None if gdesc is None else C.byref(gdesc),
                                              C.byref(odesc), stream_handle(stream, self.device)))
        return out

    def texture_weights(self, fslots, out, params=None, gate=None, stream=None):
        """Texture (structure-tensor) maps (ffl_texture_weights): item i from the gray frame in frame slot
        fslots[i] (slots may repeat between items; for a pair, its frame 0), written into `out`, a uint8 device tensor
        (n, H, W) (or a DevWeights; (H, W) for one item).  `params`: a TextureParams, a dict of its fields or None (the
        defaults, which are not tuned on footage); `gate`: maps S of rule T6 as pass1_weighted takes maps, (H, W) or (n, H, W)
        -- or `out` itself, which min-combines the texture into the maps that are already there, in place.  Queued behind the
        work on `stream` and the frames' uploads; `stream` waits for it, and a later upload into one of the frame slots runs
        behind it.  Returns `out`."""
        pf, fs = _iarr(fslots)
        prm = params if isinstance(params, TextureParams) else TextureParams(**dict({} if params is None or params is True else params))
        odesc = self._weights("texture_weights", out, len(fs))
        gdesc = None if gate is None else odesc if gate is out else self._weights("texture_weights", gate, len(fs))
        self._chk(self.L.ffl_texture_weights(self._h, len(fs), pf, C.byref(prm), None if gdesc is None else C.byref(gdesc),
                                             C.byref(odesc), stream_handle(stream, self.device)))
        return out

    def cell_stats(self, flow_slots, cells=32, cells_out=None, centres_out=None, stream=None):
        """The cells x cells grid of regional mean flow, mean magnitude and magnitude variance of every slot and / or its
        centre of mass, the reference's center_of_mass_variance (ffl_cell_stats).  cells_out: device
        memory for n * cells * cells CELL_DTYPE records (item-major, then row-major); centres_out: for n GRID_CENTRE_DTYPE
        records; one of them at least.  The flow is only read.  Queued behind the work on `stream` (None: torch's current
        stream), which waits for it; the host does not wait."""
        ps, slots = _iarr(flow_slots)
        n, ptrs = len(slots), []
        for name, out, need in (("cells_out", cells_out, n * int(cells) * int(cells) * CELL_DTYPE.itemsize),
                                ("centres_out", centres_out, n * GRID_CENTRE_DTYPE.itemsize)):
            if out is None:
                ptrs.append(None)
                continue
            ptr, extent = _device_span(out)
            if extent < need:
                raise ValueError(f"cell_stats: {name} holds {extent} bytes, the call's records need {need}")
            ptrs.append(ptr)
        self._chk(self.L.ffl_cell_stats(self._h, n, ps, int(cells), ptrs[0], ptrs[1], stream_handle(stream, self.device)))

    def radial_window_axes_centres(self, seq_slots, first, n, centres, out, radius=6, cut_threshold=7.0, pov_mode=False,
                                   stream=None):
        """radial_window_axes about caller centres (ffl_radial_window_axes_centres): `centres` holds one centre per seq slot in
        device memory, a float64 (n_seq, 2) tensor of (cx, cy) or a buffer of GRID_CENTRE_DTYPE records as cell_stats wrote
        them; the window mean over them is rule G6 of DESIGN.md section 17.  Everything else of a record is
        radial_window_axes'."""
        ptr, stride = _centre_entries(centres, len(seq_slots))
        return self._radial_window(self.L.ffl_radial_window_axes_centres, "radial_window_axes_centres", PASS2_AXES_DTYPE,
                                   seq_slots, first, n, out, radius, cut_threshold, pov_mode, stream, weights=(ptr, stride))

    def radial_window_axes_weighted_centres(self, seq_slots, first, n, weights, centres, out, radius=6, cut_threshold=7.0,
                                            pov_mode=False, stream=None):
        """The fifth window form (ffl_radial_window_axes_weighted_centres): radial_window_axes_weighted's terms about
        radial_window_axes_centres' centres.  `weights` as in pass1_weighted, (H, W) or (n, H, W); `centres` as in
        radial_window_axes_centres, or a (buffer, byte stride) span such as (track_buffer, 48 * tracks)."""
        desc = self._weights("radial_window_axes_weighted_centres", weights, n)
        ptr, stride = _centre_entries(centres, len(seq_slots))
        return self._radial_window(self.L.ffl_radial_window_axes_weighted_centres, "radial_window_axes_weighted_centres",
                                   PASS2_AXES_DTYPE, seq_slots, first, n, out, radius, cut_threshold, pov_mode, stream,
                                   weights=(C.byref(desc), ptr, stride))

    def track_advance(self, seq_slots, state, out, params=None, weights=None, stream=None):
        """Advect the tracks of `state` through the fields in flow slots seq_slots, in that order (ffl_track_advance, DESIGN.md
        section 23): `state` is device memory of T TRACK_STATE_DTYPE records (pipeline.track_state makes one), read and
        written; `out` device memory for at least len(seq_slots) * T TRACK_DTYPE records, record (i, t) at index i * T + t
        (a slice of a longer buffer serves a batch of a chunk).  `params`: a TrackParams, a dict of its fields or None
        (the defaults); `weights`: maps of the items as pass1_weighted takes them, or None.  Queued behind the work on
        `stream` (None: torch's current stream) and the slots' last writers; `stream` waits for it; the host does not wait.
        Returns `out`."""
        ps, slots = _iarr(seq_slots)
        n = len(slots)
        prm = params if isinstance(params, TrackParams) else TrackParams(**dict(params or {}))
        sptr, sbytes = _device_span(state)
        tracks = sbytes // TRACK_STATE_DTYPE.itemsize
        if tracks < 1 or sbytes % TRACK_STATE_DTYPE.itemsize:
            raise ValueError(f"track_advance: state holds {sbytes} bytes, no whole number of {TRACK_STATE_DTYPE.itemsize}-byte records")
        optr, extent = _device_span(out)
        if extent < n * tracks * TRACK_DTYPE.itemsize:
            raise ValueError(f"track_advance: out holds {extent} bytes, {n} x {tracks} records need {n * tracks * TRACK_DTYPE.itemsize}")
        wdesc = None if weights is None else self._weights("track_advance", weights, n)
        self._chk(self.L.ffl_track_advance(self._h, n, ps, tracks, C.byref(prm), None if wdesc is None else C.byref(wdesc), sptr, optr,
                                           stream_handle(stream, self.device)))
        return out

    def roi_weights(self, n, centres, out, params=None, gate=None, stream=None):
        """Elliptical ROI maps (ffl_roi_weights): item i about the centre `centres` holds for it, as
        radial_window_axes_centres takes centres (n of them) or a (buffer, byte stride) span, written into `out`, a uint8
        device tensor (n, H, W) (or a DevWeights; (H, W) for one item).  `params`: a RoiParams, a dict of its fields or None
        (the defaults, which are not tuned on footage); `gate`: maps S of rule E5 as pass1_weighted takes maps -- or `out`
        itself, which min-combines the ellipse into the maps that are already there, in place.  Queued behind the work on
        `stream`, which waits for it.  Returns `out`."""
        n = int(n)
        prm = params if isinstance(params, RoiParams) else RoiParams(**dict(params or {}))
        ptr, stride = _centre_entries(centres, n)
        odesc = self._weights("roi_weights", out, n)
        gdesc = None if gate is None else odesc if gate is out else self._weights("roi_weights", gate, n)
        self._chk(self.L.ffl_roi_weights(self._h, n, ptr, stride, C.byref(prm), None if gdesc is None else C.byref(gdesc),
                                         C.byref(odesc), stream_handle(stream, self.device)))
        return out

    def track_template(self, fslot, centres, templates, p=None, tracks=None, stream=None):
        """Capture the tracks' templates out of frame slot `fslot` (ffl_track_template, DESIGN.md section 24, rule N10):
        `centres` is device memory that holds track t's centre as two doubles at byte 48 * t -- a track_state tensor, or one
        item's track records; `templates` device memory for T * (2p+1)^2 bytes (pipeline.match_templates makes one).  `p`:
        the half-side (None: the default of MatchParams); `tracks`: T (None: the 48-byte records `centres` holds).  Queued
        behind the work on `stream` (None: torch's current stream) and the upload that filled the slot; `stream` waits for
        it.  Returns `templates`."""
        p = MatchParams().p if p is None else int(p)
        cptr, cbytes = _device_span(centres)
        T = (cbytes + 32) // 48 if tracks is None else int(tracks)
        tptr, tbytes = _device_span(templates)
        if 1 <= p <= FFL_MAX_MATCH_P and tbytes < T * (2 * p + 1) ** 2:
            raise ValueError(f"track_template: templates holds {tbytes} bytes, {T} templates of {(2 * p + 1) ** 2} are needed")
        self._chk(self.L.ffl_track_template(self._h, int(fslot), T, cptr, p, tptr, stream_handle(stream, self.device)))
        return templates

    def track_match(self, fslots, templates, centres, out, params=None, tracks=1, write_back=True, stream=None):
        """Search frame slot fslots[i] for every track's template about item i's centres and correct them in place
        (ffl_track_match): `templates` as track_template filled it; `centres` a (buffer, byte stride)
        span -- (track records of the batch, 48 * tracks), (a track_state tensor, 48 * tracks) with one item -- or a float64
        (n, 2) device array for one track; `out` device memory for len(fslots) * tracks MATCH_DTYPE records, record (i, t) at
        index i * tracks + t.  `params`: a MatchParams, a dict of its fields or None (the defaults, which are not tuned on
        footage); `write_back`: an accepted match overwrites its centre (rule N8).  Queued behind the work on `stream` and
        the uploads that filled the slots; `stream` waits for it; the host does not wait.  Returns `out`."""
        ps, slots = _iarr(fslots)
        n, T = len(slots), int(tracks)
        prm = params if isinstance(params, MatchParams) else MatchParams(**dict(params or {}))
        cptr, stride = _centre_entries(centres, n)
        tptr, _ = _device_span(templates)
        optr, extent = _device_span(out)
        if extent < n * T * MATCH_DTYPE.itemsize:
            raise ValueError(f"track_match: out holds {extent} bytes, {n} x {T} records need {n * T * MATCH_DTYPE.itemsize}")
        wb = int(write_back) if isinstance(write_back, (bool, int, np.integer)) else -1
        self._chk(self.L.ffl_track_match(self._h, n, ps, T, C.byref(prm), tptr, cptr, stride, wb, optr,
                                         stream_handle(stream, self.device)))
        return out

    def track_redetect(self, fslots, templates, centres, out, params=None, tracks=1, trigger=None, write_back=True, stream=None):
        """Search frame slot fslots[i] as a whole (or within params' reach) for every track's template and put item i's
        centres onto it (ffl_track_redetect): `templates`, `centres`, `out`, `tracks` and `write_back`
        as track_match takes them; the records are MATCH_DTYPE, with status REDETECT_SKIPPED for a search that did not run.
        `trigger`: None (every search runs), a buffer of len(fslots) * tracks match records -- a search runs iff its record's
        status & params.trigger_mask != 0 -- or an explicit (pointer or device buffer, byte stride) span of int32 words, track
        t's at + 48 t.  `params`: a RedetectParams, a dict of its fields or None (the defaults, which are not tuned on
        footage).  Queued behind the work on `stream` and the uploads that filled the slots; `stream` waits for it; the host
        does not wait.  Returns `out`."""
        ps, slots = _iarr(fslots)
        n, T = len(slots), int(tracks)
        prm = params if isinstance(params, RedetectParams) else RedetectParams(**dict(params or {}))
        cptr, stride = _centre_entries(centres, n)
        tptr, _ = _device_span(templates)
        optr, extent = _device_span(out)
        if extent < n * T * MATCH_DTYPE.itemsize:
            raise ValueError(f"track_redetect: out holds {extent} bytes, {n} x {T} records need {n * T * MATCH_DTYPE.itemsize}")
        gptr, gstride = None, 0
        if isinstance(trigger, tuple) and len(trigger) == 2 and isinstance(trigger[1], (int, np.integer)):
            gptr, gstride = trigger
            gptr = int(gptr) if isinstance(gptr, (int, np.integer)) else _array_view(gptr)[0]
        elif trigger is not None:
            gptr, gbytes = _device_span(trigger)
            if gbytes < n * T * MATCH_DTYPE.itemsize:
                raise ValueError(f"track_redetect: trigger holds {gbytes} bytes, {n} x {T} match records need "
                                 f"{n * T * MATCH_DTYPE.itemsize}")
            gptr, gstride = gptr + MATCH_STATUS_OFFSET, T * MATCH_DTYPE.itemsize
        wb = int(write_back) if isinstance(write_back, (bool, int, np.integer)) else -1
        self._chk(self.L.ffl_track_redetect(self._h, n, ps, T, C.byref(prm), tptr, cptr, stride, gptr, int(gstride), wb, optr,
                                            stream_handle(stream, self.device)))
        return out

    def motion_fit(self, slots, model="translation", iterations=3, tau=1.0, weights=None, prior=None, out=None, sums_out=None,
                   stream=None):
        """Fit a camera model to the field of every slot (ffl_motion_fit): `model` a name of
        MOTION_MODELS -- or a MotionParams, which then also gives iterations and tau -- fitted by `iterations` passes of
        Cauchy-weighted least squares with scale `tau` px.  "similarity" and "affine" contain a zoom term, which is the radial
        signal itself (rule C9).  `weights`: maps as pass1_weighted takes them, (H, W) or (n, H, W), which also weight the fit;
        `prior`: the first pass's prior per slot in device memory, a float64 (n, 6) tensor or a buffer of MOTION_DTYPE records;
        `out`: device memory for n MOTION_DTYPE records (None: a new torch buffer); `sums_out`: device memory for n * 12
        float64, the last pass's sums.  The flow is only read.  Queued behind the work on `stream` (None: torch's current
        stream), which waits for it; the host does not wait.  Returns `out`."""
        ps, ks = _iarr(slots)
        n = len(ks)
        prm = model if isinstance(model, MotionParams) else MotionParams(model=model, iterations=int(iterations), tau=float(tau))
        wdesc = None if weights is None else self._weights("motion_fit", weights, n)
        pptr, pstride = (None, 0) if prior is None else _model_entries(prior, n, "motion_fit: prior")
        if out is None:
            import torch
            out = torch.empty(n * MOTION_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", self.device))
        optr, extent = _device_span(out)
        if extent < n * MOTION_DTYPE.itemsize:
            raise ValueError(f"motion_fit: out holds {extent} bytes, {n} records need {n * MOTION_DTYPE.itemsize}")
        sptr = None
        if sums_out is not None:
            sptr, extent = _device_span(sums_out)
            if extent < n * len(MOTION_SUMS) * 8:
                raise ValueError(f"motion_fit: sums_out holds {extent} bytes, {n} items need {n * len(MOTION_SUMS) * 8}")
        self._chk(self.L.ffl_motion_fit(self._h, n, ps, C.byref(prm), None if wdesc is None else C.byref(wdesc), pptr, pstride,
                                        optr, sptr, stream_handle(stream, self.device)))
        return out

    def motion_subtract(self, src, dst, models, pov_mode=False, stream=None):
        """Subtract item i's model from the field of slot src[i] into slot dst[i] (ffl_motion_subtract, rule C8), then the
        pass-1 reductions of the dst slots: their records are upload_flow's for the compensated field.  dst[i] == src[i] is in
        place.  `models`: device memory, motion_fit's records or a float64 (n, 6) tensor.  Queued behind the work on `stream`
        (None: torch's current stream), which waits for it; the host does not wait."""
        (ps, ks), (pd, kd) = _iarr(src), _iarr(dst)
        if len(ks) != len(kd):
            raise ValueError(f"motion_subtract: {len(ks)} src slots for {len(kd)} dst slots")
        mptr, mstride = _model_entries(models, len(ks), "motion_subtract: models")
        self._chk(self.L.ffl_motion_subtract(self._h, len(ks), ps, pd, mptr, mstride, int(bool(pov_mode)),
                                             stream_handle(stream, self.device)))

    def download_frame(self, fslot):
        out = np.empty((self.height, self.width), np.uint8)
        self._chk(self.L.ffl_download_frame(self._h, fslot, out.ctypes.data))
        return out

    def download_flow(self, flow_slot):
        out = np.empty((self.height, self.width, 2), np.float32)
        self._chk(self.L.ffl_download_flow(self._h, flow_slot, out.ctypes.data))
        return out

    def upload_flow(self, flow_slot, flow, pov_mode=False):
        flow = np.ascontiguousarray(flow, np.float32)
        if flow.shape != (self.height, self.width, 2):
            raise FFLError(f"flow shape {flow.shape} does not match context {(self.height, self.width, 2)}")
        self._chk(self.L.ffl_upload_flow(self._h, flow_slot, flow.ctypes.data, int(bool(pov_mode))))

    def sync(self):
        self._chk(self.L.ffl_sync(self._h))

    def set_option(self, name, value):
        """A knob of THIS context only (ffl_ctx_set_option); "lanes" is fixed at creation."""
        self._chk(self.L.ffl_ctx_set_option(self._h, name.encode(), int(value)))

    def get_option(self, name):
        v = C.c_int()
        self._chk(self.L.ffl_ctx_get_option(self._h, name.encode(), C.byref(v)))
        return v.value

    def graph_stats(self):
        """{"captured", "replayed", "capture_failures"} of this context's hipGraph path (ffl_graph_stats)."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.ffl_graph_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"captured": a.value, "replayed": b.value, "capture_failures": c.value}

    # ---- test / measurement hooks --------------------------------------------------------------
    def num_levels(self):
        return self.L.ffl_num_levels(self._h)

    def level_size(self, level):
        wh = (C.c_int * 2)()
        self._chk(self.L.ffl_level_size(self._h, level, wh))
        return wh[0], wh[1]

    def debug_pair(self, f0, f1, level, it):
        lw, lh = self.level_size(level)
        d = dict(I0=np.empty((lh, lw), np.float32), I1=np.empty((lh, lw), np.float32),
                 R0=np.empty((5, lh, lw), np.float32), R1=np.empty((5, lh, lw), np.float32),
                 M=np.empty((5, lh, lw), np.float32), flow=np.empty((lh, lw, 2), np.float32))
        self._chk(self.L.ffl_debug_pair(self._h, f0, f1, level, it, d["I0"].ctypes.data, d["I1"].ctypes.data,
                                        d["R0"].ctypes.data, d["R1"].ctypes.data, d["M"].ctypes.data,
                                        d["flow"].ctypes.data))
        d["out"] = self.download_flow(0)
        return d

    def debug_dis_pair(self, f0, f1, scale, stage, params=None):
        """ffl_debug_dis_pair: one DIS pair, the field of (scale, stage) -- stage a DIS_STAGES name or number.  Patch
        stages come back as (hs, ws, 2), dense ones as (lh, lw, 2), "images" as (2, lh, lw)."""
        p = params if params is not None else DisParams()
        st = DIS_STAGES.get(stage, stage)
        lw, lh = self.width >> scale, self.height >> scale
        if st in (0, 1):
            shape = (1 + (lh - p.patch_size) // p.patch_stride, 1 + (lw - p.patch_size) // p.patch_stride, 2)
        elif st == 4:
            shape = (2, lh, lw)
        else:
            shape = (lh, lw, 2)
        out = np.empty(shape, np.float32)
        self._chk(self.L.ffl_debug_dis_pair(self._h, int(f0), int(f1), C.byref(p), int(scale), int(st), out.ctypes.data))
        return out

    def profile_enable(self, classes=True):
        """classes: True (all), False/None (off) or an iterable of kernel-class names."""
        if classes is True:
            mask = FFL_PROFILE_ALL
        elif not classes:
            mask = 0
        else:
            mask = sum(1 << KERNEL_CLASSES.index(c) for c in classes)
        self._chk(self.L.ffl_profile_enable(self._h, mask))

    def profile_read(self):
        out = {}
        for k, name in enumerate(KERNEL_CLASSES):
            n, ms = C.c_int(), C.c_double()
            self._chk(self.L.ffl_profile_read(self._h, k, C.byref(n), C.byref(ms)))
            out[name] = (n.value, ms.value)
        return out
