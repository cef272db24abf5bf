"""Host tests of the map-driven front-end: ffl_remap_check against the numpy restatement
(tests/remap_ref.py), its refusals, the map builders of frontend.py, and params["hip_view"] through the prefetch ring to a
.funscript with stand-ins for the capture and the device.  No device is needed."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import front_orient as fo
import front_sweep as fs
import remap_ref as rr
from funscript_flow_amd import _capi, frontend, pipeline, prefetch

SUPER = (1, 2, 4)


# ---- ffl_remap_check ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rot, mir", fo.ORIENTATIONS, ids=fo.ORI_IDS)
def test_remap_check_agrees_with_the_restatement(rot, mir):
    for k, (out, S) in enumerate((o, s) for o in fs.OUTS[:2] for s in SUPER):
        for stored in ((2, 2), (34, 18), (33, 17), (320, 180)):
            up = stored[::-1] if rot in (90, 270) else stored
            rects = [None]
            if min(up) > 40:   # an odd interior rectangle: no side on a multiple of 16 or 2
                rects.append((37, 11, up[0] - 37 - 23, up[1] - 11 - 9))
            for rect in rects:
                m = rr.hostile_map(out, S, up, 7 * k + rot, rect)
                want_up, want_st = rr.windows(m, S, stored, rot, mir)
                got_up, got_st, valid = _capi.remap_check(m, out, stored, S, rotate=rot, mirror=mir)
                assert (got_up, got_st) == (want_up, want_st), (out, S, stored, rect)
                assert valid == int(rr.check(m, S, up).sum()) < m.shape[0] * m.shape[1]
                if rect is not None and stored == (320, 180):
                    assert got_st[2] * got_st[3] < 320 * 180 and (got_st[0] > 0 or got_st[1] > 0)


def test_a_single_valid_entry():
    out, S, stored = (17, 19), 2, (34, 18)
    for q, rot, mir in (((32 * 33, 32 * 17), 0, False), ((0, 0), 180, True), ((5 * 32 + 3, 9 * 32), 90, False),
                        ((17 * 32, 33 * 32), 270, True)):
        up = stored[::-1] if rot in (90, 270) else stored
        m = np.full((S * out[1], S * out[0], 2), rr.NONE, np.int32)
        m[11, 5] = q
        got_up, got_st, valid = _capi.remap_check(m, out, stored, S, rotate=rot, mirror=mir)
        assert valid == 1 and (got_up, got_st) == rr.windows(m, S, stored, rot, mir)
        x0, y0 = q[0] >> 5, q[1] >> 5
        assert got_up == (x0, y0, min(x0 + 1, up[0] - 1) - x0 + 1, min(y0 + 1, up[1] - 1) - y0 + 1)


def test_remap_check_refusals():
    out, src = (16, 16), (34, 18)
    good = rr.hostile_map(out, 1, src, 3)
    for (i, j, q), S in ((((5, 7, (32 * 33 + 1, 0))), 1), ((0, 0, (-1, 5)), 1), ((15, 15, (0, 32 * 17 + 1)), 1),
                         ((20, 31, (4, -2 ** 31)), 2)):
        m = rr.hostile_map(out, S, src, 4, sentinels=False)
        m[i, j] = q
        index = i * m.shape[1] + j
        with pytest.raises(ValueError, match=rf"map entry {index} \(sample row {i}, column {j}\) is \({q[0]}, {q[1]}\)"):
            _capi.remap_check(m, out, src, S)
        with pytest.raises(ValueError, match=f"entry {index}$"):
            rr.check(m, S, src)
    m = good.copy()
    m[3, 3], m[9, 2] = (0, -7), (-5, 0)                     # the first offender in row-major order is the one named
    with pytest.raises(ValueError, match=r"map entry 51 "):
        _capi.remap_check(m, out, src)
    none = np.full((16, 16, 2), rr.NONE, np.int32)
    with pytest.raises(ValueError, match="no valid entry"):
        _capi.remap_check(none, out, src)
    L = _capi.load()
    for S in (0, 3, 8, -1):
        assert L.ffl_remap_check(good.ctypes.data, 16, 16, S, 34, 18, None, None, None, None) == _capi.FFL_ERR_INVALID
        assert b"supersample" in L.ffl_last_error(None) and b"1, 2, 4" in L.ffl_last_error(None)
        with pytest.raises(ValueError, match="supersample"):
            _capi.remap_check(good, out, src, S)
    assert L.ffl_remap_check(None, 16, 16, 1, 34, 18, None, None, None, None) == _capi.FFL_ERR_INVALID
    info = _capi.SourceInfo(45, 0, 0)
    assert L.ffl_remap_check(good.ctypes.data, 16, 16, 1, 34, 18, C.byref(info), None, None, None) == _capi.FFL_ERR_INVALID
    assert b"rotate 45" in L.ffl_last_error(None)
    # a quarter turn makes the upright source 18 wide: the entries beyond it are refused
    with pytest.raises(ValueError, match="upright 18x34 source"):
        _capi.remap_check(good, out, src, rotate=90)
    assert _capi.remap_check(good, out, src)[2] == int(rr.check(good, 1, src).sum())
    with pytest.raises(ValueError, match="shape"):
        _capi.remap_check(good[:, :15], out, src)


def test_remap_bytes_and_the_constants():
    assert [_capi.remap_bytes((130, 16), S) for S in SUPER] == [8 * S * S * 130 * 16 for S in SUPER]
    with pytest.raises(_capi.FFLError, match="supersample"):
        _capi.remap_bytes((16, 16), 3)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ffl.h")).read()
    assert f"FFL_MAX_REMAPS = {_capi.FFL_MAX_REMAPS}," in header and "FFL_REMAP_NO_SOURCE = -2147483647 - 1" in header
    assert _capi.REMAP_NO_SOURCE == rr.NONE == frontend.NO_SOURCE == -2147483648


# ---- builders -------------------------------------------------------------------------------------------------------------
def test_identity_map_known_answers():
    m = frontend.identity_map((3, 2), origin=(5, 7))
    assert m.dtype == np.int32 and m.shape == (2, 3, 2)
    assert m[..., 0].tolist() == [[160, 192, 224]] * 2 and m[..., 1].tolist() == [[224] * 3, [256] * 3]
    m = frontend.identity_map((2, 1), origin=(4, 6), supersample=2)
    assert m[..., 0].tolist() == [[128, 160, 192, 224]] * 2 and m[..., 1].tolist() == [[192] * 4, [224] * 4]
    img = fs.bgr_frame("noise", 40, 30, 1)
    assert np.array_equal(rr.operand(img, frontend.identity_map((17, 19), (3, 2)), 1),
                          fs.direct_operand(img, (40, 30), (3, 2), (17, 19), False))
    img = fs.bgr_frame("ramp", 48, 48, 2)
    assert np.array_equal(rr.operand(img, frontend.identity_map((17, 19), (4, 6), 2), 2, rgb=True),
                          fs.direct_operand(img, (24, 24), (2, 3), (17, 19), True))
    with pytest.raises(ValueError, match="supersample"):
        frontend.identity_map((4, 4), supersample=3)


def test_map_valid_mask():
    m = frontend.identity_map((4, 3), supersample=2)
    m[2, 5, 0] = frontend.NO_SOURCE                        # one of pixel (2, 1)'s four samples
    m[0, 0] = (frontend.NO_SOURCE, 99)
    mask = frontend.map_valid_mask(m, 2)
    want = np.full((3, 4), 255, np.uint8)
    want[1, 2] = want[0, 0] = 0
    assert mask.dtype == np.uint8 and np.array_equal(mask, want)
    assert np.array_equal(frontend.map_valid_mask(m[::2, ::2], 1) == 0, m[::2, ::2, 0] == frontend.NO_SOURCE)
    with pytest.raises(ValueError, match="shape"):
        frontend.map_valid_mask(m[:5], 2)


def test_eye_rect():
    assert frontend.eye_rect((400, 200)) == (0, 0, 400, 200)
    assert frontend.eye_rect((400, 200), "sbs", "left") == (0, 0, 200, 200)
    assert frontend.eye_rect((400, 200), "sbs", "right") == (200, 0, 200, 200)
    assert frontend.eye_rect((400, 200), "tb", "left") == (0, 0, 400, 100)
    assert frontend.eye_rect((400, 200), "tb", "right") == (0, 100, 400, 100)
    for bad in ({"stereo": "lr"}, {"eye": "both"}):
        with pytest.raises(ValueError):
            frontend.eye_rect((400, 200), **{"stereo": "sbs", "eye": "left", **bad})


def centre(m):
    """mean of the four samples about the optical axis, in px"""
    H, W = m.shape[:2]
    return m[H // 2 - 1:H // 2 + 1, W // 2 - 1:W // 2 + 1].reshape(4, 2).astype(np.float64).mean(0) / 32


@pytest.mark.parametrize("projection", frontend.PROJECTIONS)
def test_view_map_geometry(projection):
    """every comparison within 1 unit of 1/32 px: the freedom a correctly rounded float64 chain leaves at an exact half"""
    src, out = (800, 400), (32, 24)
    for stereo, eye in ((None, "left"), ("sbs", "left"), ("sbs", "right"), ("tb", "right")):
        x0, y0, w, h = rect = frontend.eye_rect(src, stereo, eye)
        m = frontend.view_map(src, out, projection, 80, rect=rect)
        assert m.dtype == np.int32 and m.shape == (24, 32, 2) and (m[..., 0] != frontend.NO_SOURCE).all()
        # left-right (and up-down) symmetry about the rectangle's centre line at zero angles
        assert np.abs((m[:, ::-1, 0] + m[..., 0]) - 32 * (2 * x0 + w - 1)).max() <= 1
        assert np.abs(m[:, ::-1, 1] - m[..., 1]).max() <= 1
        assert np.abs((m[::-1, :, 1] + m[..., 1]) - 32 * (2 * y0 + h - 1)).max() <= 1
        # the centre ray lands on the centre of the eye rectangle
        assert np.abs(centre(m) - (x0 + w / 2 - .5, y0 + h / 2 - .5)).max() <= 1 / 32
        assert m[..., 0].min() >= 32 * x0 and m[..., 0].max() <= 32 * (x0 + w - 1)
        assert m[..., 1].min() >= 32 * y0 and m[..., 1].max() <= 32 * (y0 + h - 1)
    # yaw = hfov / 4 moves the centre by w / 4 to the right; pitch moves it up by the matching fraction of h
    x0, y0, w, h = rect = frontend.eye_rect(src, "sbs", "left")
    c0 = centre(frontend.view_map(src, out, projection, 80, rect=rect))
    cy = centre(frontend.view_map(src, out, projection, 80, yaw=45, rect=rect))
    cp = centre(frontend.view_map(src, out, projection, 80, pitch=30, rect=rect))
    if projection == "equirect":
        assert np.abs(cy - c0 - (w / 4, 0)).max() <= 1 / 32 + 1e-9
        assert np.abs(cp - c0 - (0, -h * 30 / 180)).max() <= 1 / 32 + 1e-9
    else:                                                   # equidistant: the radius is linear in the angle off the axis
        r = min(w, h) / 2
        assert np.abs(cy - c0 - (r * 45 / 90, 0)).max() <= 1 / 32 + 1e-9 and np.abs(cp - c0 - (0, -r * 30 / 90)).max() <= 1 / 32 + 1e-9
    # roll by 180 turns the sample grid about its centre
    turned = frontend.view_map(src, out, projection, 80, roll=180, rect=rect)
    assert np.abs(turned[::-1, ::-1].astype(np.int64) - frontend.view_map(src, out, projection, 80, rect=rect)).max() <= 1


@pytest.mark.parametrize("projection", frontend.PROJECTIONS)
def test_view_map_validity_clamps_and_supersampling(projection):
    src, out = (800, 400), (32, 24)
    rect = frontend.eye_rect(src, "sbs", "right")
    # a 150 degree view into a 120 degree source: the rim has no source, the middle has
    m = frontend.view_map(src, out, projection, 150, src_hfov=120, src_vfov=120, rect=rect)
    gone = m[..., 0] == frontend.NO_SOURCE
    assert gone[:, 0].all() and gone[:, -1].all() and not gone[10:14, 14:18].any() and 0.1 < gone.mean() < 0.9
    assert (m[gone][:, 1] == 0).all()
    f = 16 / np.tan(np.radians(150) / 2)                     # the rule, restated: which rays leave the source's field
    rx, ry = np.meshgrid((np.arange(32) + .5 - 16) / f, (np.arange(24) + .5 - 12) / f)
    if projection == "equirect":
        beyond = (np.abs(np.degrees(np.arctan(rx))) > 60) | (np.abs(np.degrees(np.arctan2(ry, np.hypot(rx, 1)))) > 60)
    else:
        beyond = np.degrees(np.arctan(np.hypot(rx, ry))) > 60
    assert np.array_equal(gone, beyond)
    rr.check(m, 1, src)
    # looking far to the side of a 180 degree eye: coordinates that leave the rectangle are clamped, with fraction 0
    m = frontend.view_map(src, out, "equirect", 100, yaw=60, pitch=50, rect=rect)
    ok = m[..., 0] != frontend.NO_SOURCE
    qx, qy = m[..., 0][ok], m[..., 1][ok]
    lo, hi = 32 * rect[0], 32 * (rect[0] + rect[2] - 1)
    assert qx.min() >= lo and qx.max() <= hi and qy.min() >= 0 and qy.max() <= 32 * 399
    assert ((qx == hi) | (qy == 0)).any()                   # some are clamped ...
    assert (qx[qx >= hi] & 31 == 0).all() and (qy[qy <= 0] & 31 == 0).all()   # ... and those sit on a pixel
    # supersample = 2: the four sub-samples of a pixel bracket its S = 1 sample
    one = frontend.view_map(src, out, projection, 80, yaw=10, pitch=-5, rect=rect).astype(np.int64)
    two = frontend.view_map(src, out, projection, 80, yaw=10, pitch=-5, rect=rect, supersample=2).astype(np.int64)
    assert two.shape == (48, 64, 2)
    sub = two.reshape(24, 2, 32, 2, 2)
    assert (sub.min(axis=(1, 3)) <= one + 1).all() and (sub.max(axis=(1, 3)) >= one - 1).all()
    for bad in ({"projection": "mercator"}, {"fov": 180}, {"supersample": 3}, {"rect": (700, 0, 200, 400)}, {"src_hfov": 0}):
        with pytest.raises(ValueError):
            frontend.view_map(**{"src_size": src, "out": out, "projection": "equirect", "fov": 90, **bad})


def test_uploaders_refuse_remap_with_vr_mode_in_words():
    handle = _capi.Remap(0, (8, 6), 1, (0, 0, 8, 6), 48)
    with pytest.raises(ValueError, match="remap= and vr_mode are two answers to one question"):
        frontend.DecodedUploader(object(), vr_mode=True, remap=handle)
    with pytest.raises(TypeError, match="remap_create"):
        frontend.DecodedUploader(object(), remap=3)
    assert frontend.DecodedUploader(object(), remap=handle).remap is handle
    assert frontend.DecodedUploader(object()).remap is None


# ---- params["hip_view"] through the prefetch ring ----------------------------------------------------------------------------
class Capture:
    """cv2.VideoCapture look-alike: frame i is filled with i"""

    def __init__(self, n, size):
        self.n, self.size, self.pos, self.released = n, size, 0, False

    def isOpened(self):
        return True

    def get(self, prop):
        return {prefetch.CAP_PROP_FRAME_COUNT: self.n, prefetch.CAP_PROP_FPS: 30.0, prefetch.CAP_PROP_FRAME_WIDTH: self.size[0],
                prefetch.CAP_PROP_FRAME_HEIGHT: self.size[1]}[prop]

    def grab(self):
        self.pos += 1
        return self.pos <= self.n

    def read(self, image=None):
        if self.pos >= self.n:
            return False, None
        image[...] = self.pos
        self.pos += 1
        return True, image

    def release(self):
        self.released = True


class Ctx:
    """device stand-in that records what the map-driven path asks of a context"""
    width, height = 16, 16

    def __init__(self, B=4):
        self.max_batch, self.frame_slots, self.flow_slots = B, 2 * B + 2, pipeline.min_flow_slots(B)
        self.maps, self.uploads, self.alive, self.destroyed_after_uploads = [], [], set(), []

    def pinned_frames(self, n, channels=1, size=None, yuv=False):
        return np.zeros((n, size[1] * 3 // 2, size[0]) if yuv else (n, size[1], size[0], 3), np.uint8)

    def remap_create(self, map, src_size, supersample=1):
        if len(self.alive) >= _capi.FFL_MAX_REMAPS:          # the library's refusal of a ninth map
            raise _capi.FFLError(f"ffl_remap_create: {_capi.FFL_MAX_REMAPS} maps are alive already (FFL_MAX_REMAPS); destroy one first")
        self.maps.append((np.array(map), tuple(src_size), supersample))
        self.alive.add(len(self.maps) - 1)
        return _capi.Remap(len(self.maps) - 1, src_size, supersample, None, None)

    def remap_destroy(self, remap):
        self.alive.remove(remap.id)                          # KeyError: destroyed twice, or never created
        self.destroyed_after_uploads.append(len(self.uploads))

    def upload_frames_remap(self, first, frames, remap, fmt="bgr", **kw):
        assert remap.id in self.alive, "an upload through a destroyed map"
        self.uploads.append((first, [int(f.flat[0]) for f in frames], remap.id, fmt, kw))

    def flow_pairs(self, f0, f1, slots, pov):
        self.last = list(slots)

    def pass1_results(self, slots, thr):
        return [(8, 8, np.float32(1), np.float32(1), False) for _ in slots]

    def radial(self, slots, centers, cuts, pov):
        return [float(s % 5) - 2 for s in slots]


def test_hip_view_from_the_ring_to_a_funscript(tmp_path):
    view = {"projection": "equirect", "fov": 90, "yaw": 10, "stereo": "sbs", "eye": "right", "supersample": 2}
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "overwrite": True,
              "hip_view": view, "hip_yuv": "nv12", "hip_rotate": 90}
    ctx, logs, caps = Ctx(), [], []

    def open_capture(path):
        caps.append(Capture(30, (40, 80)))                  # stored 40 x 80, upright 80 x 40
        return caps[-1]

    video = str(tmp_path / "clip.mp4")
    assert prefetch.process_video(video, params, logs.append, open_capture, lambda cap: ctx) is False, logs
    assert caps[0].released and json.load(open(str(tmp_path / "clip.funscript")))["actions"]
    (m, src, S), = ctx.maps                                 # built once, for the upright size, for the right eye
    assert not ctx.alive and ctx.destroyed_after_uploads == [len(ctx.uploads)]   # and freed after the last upload
    assert src == (80, 40) and S == 2
    assert np.array_equal(m, frontend.view_map((80, 40), (16, 16), "equirect", 90, yaw=10, rect=(40, 0, 40, 40), supersample=2))
    assert ctx.uploads and all(u[2:] == (0, "nv12", {"rotate": 90}) for u in ctx.uploads)
    assert sorted(i for u in ctx.uploads for i in u[1]) == list(range(30))
    # refused together with vr_mode, in words, and reported the way process_video reports every error
    logs.clear()
    assert prefetch.process_video(video, {**params, "vr_mode": True}, logs.append, open_capture, lambda cap: Ctx()) is True
    assert any("two answers to one question" in line for line in logs)
    with pytest.raises(ValueError, match="two answers to one question"):
        prefetch.view_remap(Ctx(), Capture(4, (40, 80)), {"hip_view": view, "vr_mode": True})
    with pytest.raises(ValueError, match="knows"):
        prefetch.view_remap(Ctx(), Capture(4, (40, 80)), {"hip_view": {"projection": "equirect", "fov": 90, "zoom": 2}})
    # without the key nothing changes
    plain = Ctx()
    assert prefetch.view_remap(plain, Capture(4, (40, 80)), {"vr_mode": True}) == {} and not plain.maps


def test_a_reused_context_does_not_run_out_of_maps(tmp_path):
    """the context is the caller's and outlives a video: every map a hip_view call creates is destroyed by that call -- after
    its last upload, on success and on failure -- so more than FFL_MAX_REMAPS videos run on one context"""
    view = {"projection": "fisheye", "fov": 100, "stereo": "tb", "eye": "left"}
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "overwrite": True,
              "hip_view": view}
    ctx, logs = Ctx(), []
    n = _capi.FFL_MAX_REMAPS + 3
    for k in range(n):
        video = str(tmp_path / f"clip{k}.mp4")
        assert prefetch.process_video(video, params, logs.append, lambda p: Capture(12, (48, 64)), lambda cap: ctx) is False, logs
        assert not ctx.alive and len(ctx.maps) == k + 1
    for k in range(n):
        assert prefetch.video_to_actions(ctx, Capture(12, (48, 64)), params)
        assert not ctx.alive and len(ctx.maps) == n + k + 1
    assert ctx.destroyed_after_uploads == sorted(ctx.destroyed_after_uploads) and len(ctx.destroyed_after_uploads) == 2 * n
    # a video that fails half-way frees its map too

    class Broken(Capture):
        def read(self, image=None):
            if self.pos == 7:
                return False, None
            return super().read(image)

    assert prefetch.process_video(str(tmp_path / "bad.mp4"), params, logs.append, lambda p: Broken(12, (48, 64)), lambda cap: ctx) is True
    assert not ctx.alive and len(ctx.maps) == 2 * n + 1
    with pytest.raises(prefetch.DecodeError):
        prefetch.video_to_actions(ctx, Broken(12, (48, 64)), params)
    assert not ctx.alive and len(ctx.maps) == 2 * n + 2
    # a caller's engine carries the caller's map: the call creates and destroys nothing
    mine = ctx.remap_create(ctx.maps[0][0], (48, 64))
    eng = pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, remap=mine))
    assert prefetch.video_to_actions(ctx, Capture(12, (48, 64)), params, engine=eng)
    assert ctx.alive == {mine.id} and len(ctx.maps) == 2 * n + 3


def test_device_uploader_refuses_remap_with_vr_mode_in_words():
    handle = _capi.Remap(0, (8, 6), 1, (0, 0, 8, 6), 48)
    with pytest.raises(ValueError, match="remap= and vr_mode are two answers to one question"):
        frontend.DeviceUploader(object(), "nv12", vr_mode=True, remap=handle)
    with pytest.raises(TypeError, match="remap_create"):
        frontend.DeviceUploader(object(), "nv12", remap=3)
