"""GPU tests of the map-driven front-end (ffl_upload_frames_remap, ffl_upload_frames_device_remap; DESIGN.md section 20,
appendix R) at the small shapes of tests/front_sweep.py, bit for bit: the ties to the crop paths (an identity map is the
identity-mode operand, a 2x supersampled one the 2x2-mean operand), hostile maps through every source kind, orientation and
supersampling against the numpy restatement (tests/remap_ref.py), the transfer window, map lifetime and the refusals.  Every
written slot is first filled with front_sweep.slot_pattern; slot 0 and the last slot must keep theirs."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

try:                      # before the library initialises the device: torch's HIP runtime comes first (as in test_gpu_device_io)
    import torch
except ImportError:
    torch = None

import front_orient as fo
import front_sweep as fs
import remap_ref as rr
import yuv16_ref
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline

OUT_IDS = [f"{w}x{h}" for w, h in fs.OUTS]
SUPER = (1, 2, 4)
HOST_KINDS = ("host_bgr", "host_rgb", "host_i420", "host_nv12_padded", "host_yuv420p10le", "host_p010")
DEV_KINDS = ("dev_bgr_padded", "dev_planar_rgb", "dev_bgra", "dev_i420_pitches", "dev_nv12", "dev_p010", "dev_gray")
ORIENTS = ((0, False), (90, False), (270, True))
INTERIOR = (37, 11, 260, 160)   # of 320 x 180: the window starts at x0 = 32 > 0, so chroma rows start inside their planes


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def junk(shape, seed, dtype=np.uint8):
    return np.random.default_rng(seed).integers(0, np.iinfo(dtype).max + 1, shape, dtype=dtype)


def padded(f, pad, seed):
    """the frame as a view of a buffer whose rows are `pad` elements longer, filled with other values"""
    big = junk((f.shape[0], f.shape[1] + pad) + f.shape[2:], seed, f.dtype.type)
    big[:, :f.shape[1]] = f
    return big[:, :f.shape[1]]


def prefill(ctx, first, n, out):
    ctx.upload_frames(first, [fs.slot_pattern(first + i, out) for i in range(n)])


def check(ctx, first, want, out, what):
    """slots first.. hold `want`; slot 0 and the last one still hold their pattern"""
    for i, w in enumerate(want):
        got = ctx.download_frame(first + i)
        assert np.array_equal(got, w), (what, "frame", i, "first difference at", tuple(np.argwhere(got != w)[0]))
    for s in (0, ctx.frame_slots - 1):
        assert np.array_equal(ctx.download_frame(s), fs.slot_pattern(s, out)), (what, "slot", s, "was written")


def layout_of(kind):
    return "i420" if ("i420" in kind or "yuv420p" in kind) else "nv12"


def is_yuv(kind):
    return not any(k in kind for k in ("bgr", "rgb", "gray"))


def i420_rows(frames, seed):
    """ffl_dev_frame rows of I420 frames whose planes lie in separate allocations with three different pitches"""
    keep, rows = [], []
    for i, f in enumerate(frames):
        planes = yuv_ref.planes(f, "i420")
        w = planes[0].shape[1]
        pitches = [w + 3 + i, w // 2 + 1, w // 2 + 6 + i]
        t = [dev(padded(np.ascontiguousarray(p), pitch - p.shape[1], seed + 10 * i + k).base)
             for k, (p, pitch) in enumerate(zip(planes, pitches))]
        keep += t
        rows.append([x.data_ptr() for x in t] + pitches + [1, 0])
    return rows, keep


def upright_frames(kind, src, seed, n=2):
    """n upright frames of source kind `kind` and the images their taps yield (limited range)"""
    w, h = src
    if kind == "dev_gray":
        fr = [junk((h, w), seed + i) for i in range(n)]
        return fr, fr
    if not is_yuv(kind):
        fr = [fs.bgr_frame(k, w, h, seed + i) for i, k in enumerate(("noise", "ramp")[:n])]
        return fr, fr
    fr = [fs.yuv_frame(k, w, h, layout_of(kind), seed + i) for i, k in enumerate(("noise", "corners")[:n])]
    return fr, None


def upload_kind(ctx, kind, first, upright, remap, rot, mir, seed, **more):
    """uploads the stored forms of the upright frames through source kind `kind` and the map; returns what must stay alive"""
    src = dict(rotate=rot, mirror=mir, **more)
    layout = layout_of(kind)
    if kind in ("host_bgr", "host_rgb"):
        st = [np.ascontiguousarray(fo.inverse_orient(f, rot, mir)) for f in upright]
        ctx.upload_frames_remap(first, st, remap, "rgb" if kind == "host_rgb" else "bgr", **src)
        return st
    if kind in ("dev_bgr_padded", "dev_planar_rgb", "dev_bgra", "dev_gray"):
        st = [np.ascontiguousarray(fo.inverse_orient(f, rot, mir)) for f in upright]
        if kind == "dev_bgr_padded":
            t = [dev(padded(f, 5, seed + i).base)[:, :f.shape[1]] for i, f in enumerate(st)]
        elif kind == "dev_planar_rgb":
            t = [dev(f.transpose(2, 0, 1)) for f in st]
        elif kind == "dev_bgra":
            t = [dev(np.concatenate([f, junk(f.shape[:2] + (1,), seed + i)], 2)) for i, f in enumerate(st)]
        else:
            t = [dev(padded(st[0], 7, seed).base)[:, :st[0].shape[1]], dev(np.stack([st[1]] * 3, -1))[..., 1]]
        fmt = {"dev_planar_rgb": "rgb", "dev_gray": "gray"}.get(kind, "bgr")
        ctx.upload_frames_device_remap(first, t, fmt, remap, **src)
        return t
    st = [fo.inverse_orient420(f, layout, rot, mir) for f in upright]
    if kind in ("host_i420", "host_nv12_padded"):
        st = [padded(f, 6, seed + i) for i, f in enumerate(st)] if kind == "host_nv12_padded" else st
        ctx.upload_frames_remap(first, st, remap, layout, **src)
        return st
    if kind in ("host_yuv420p10le", "host_p010"):
        st = [yuv16_ref.widen(f, 10, layout == "nv12") for f in st]
        ctx.upload_frames_remap(first, st, remap, layout, depth=10, **src)
        return st
    if kind == "dev_i420_pitches":
        size = (st[0].shape[1], st[0].shape[0] * 2 // 3)
        rows, keep = i420_rows(st, seed)
        d = np.ascontiguousarray(rows, np.int64)
        info = _capi.source_info(**src)
        ctx._chk(ctx.L.ffl_upload_frames_device_remap(ctx._h, first, len(st), d.ctypes.data, _capi.dev_format("i420"), 8, 0, size[0],
                                                      size[1], remap.id, _capi.stream_handle(None, ctx.device),
                                                      C.byref(info) if info is not None else None))
        return keep
    if kind == "dev_nv12":
        t = [dev(padded(f, 9, seed + i).base)[:, :f.shape[1]] for i, f in enumerate(st)]
        ctx.upload_frames_device_remap(first, t, "nv12", remap, **src)
        return t
    if kind == "dev_p010":
        t = [dev(yuv16_ref.widen(f, 10, True)) for f in st]
        ctx.upload_frames_device_remap(first, t, "nv12", remap, depth=10, **src)
        return t
    raise ValueError(kind)


# ---- ties to the crop paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host_bgr", "dev_nv12"])
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_identity_maps_equal_the_crop_paths(out, kind):
    """S = 1, a shifted identity map == upload_frames_raw(resize=src, crop=shift); S = 2, the integer map over a 2(ow+7) x
    2(oh+5) source == the AREA2 operand: against the cached expectations and against the crop path's own slots"""
    if kind.startswith("dev") and torch is None:
        pytest.skip("needs torch")
    cases = fs.bgr_cases(out) if kind == "host_bgr" else fs.yuv_cases(out, "nv12")
    seen = set()
    with _capi.Context(*out, max_batch=1, frame_slots=6) as ctx:
        for row in cases:
            name, src, rs, crop, frames, want = row[:6]
            if name not in ("identity", "identity_wide", "area2"):
                continue
            S = 2 if name == "area2" else 1
            assert src == ((2 * (out[0] + 7), 2 * (out[1] + 5)) if S == 2 else rs)
            seen.add(name)
            remap = ctx.remap_create(frontend.identity_map(out, (S * crop[0], S * crop[1]), S), src, S)
            assert remap.window == (S * crop[0], S * crop[1], min(S * out[0] + 1, src[0] - S * crop[0]),
                                    min(S * out[1] + 1, src[1] - S * crop[1]))
            prefill(ctx, 0, 6, out)
            if kind == "host_bgr":
                ctx.upload_frames_raw(3, frames, rs, crop)
                ctx.upload_frames_remap(1, frames, remap)
            else:
                t = [dev(f) for f in frames]
                ctx.upload_frames_device(3, t, "nv12", rs, crop)
                ctx.upload_frames_device_remap(1, t, "nv12", remap)
            check(ctx, 1, want, out, (kind, name, crop, "against the restatement"))
            check(ctx, 1, [ctx.download_frame(3 + i) for i in range(2)], out, (kind, name, crop, "against the crop path"))
            ctx.remap_destroy(remap)
    assert seen == {"identity", "identity_wide", "area2"}


# ---- hostile maps -------------------------------------------------------------------------------------------------------
def sources(kind):
    s = [((2, 2), None), ((34, 18), None), ((320, 180), INTERIOR)]
    return s + [((33, 17), None)] if kind in ("host_bgr", "host_rgb", "dev_bgr_padded") else s


@pytest.mark.parametrize("kind", HOST_KINDS + DEV_KINDS)
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_hostile_maps_bit_exact(out, kind):
    if kind.startswith("dev") and torch is None:
        pytest.skip("needs torch")
    layout, yuv = layout_of(kind), is_yuv(kind)
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        for k, (src, rect) in enumerate(sources(kind)):
            upright, images = upright_frames(kind, src, 40 * k)
            if yuv:
                images = [yuv_ref.yuv_to_bgr(f, layout) for f in upright]
                full = [fo.yuv_to_bgr_full(f, layout) for f in upright]
            for S in SUPER:
                m = rr.hostile_map(out, S, src, 1000 * k + S, rect)
                remap = ctx.remap_create(m, src, S)
                assert remap.window == rr.windows(m, S, src)[0] and remap.valid == int(rr.check(m, S, src).sum())
                want = [rr.operand(img, m, S, rgb="rgb" in kind) for img in images]
                runs = [(rot, mir, {}, want) for rot, mir in ORIENTS]
                if yuv:
                    wf = [rr.operand(img, m, S) for img in full]
                    assert not np.array_equal(wf[0], want[0])
                    runs += [(0, False, {"yuv_range": "full"}, wf), (90, False, {"yuv_range": "full"}, wf)]
                for rot, mir, more, w in runs:
                    prefill(ctx, 1, 2, out)
                    keep = upload_kind(ctx, kind, 1, upright, remap, rot, mir, 7 * k + S, **more)
                    check(ctx, 1, w, out, (kind, src, S, rot, mir, more))
                    del keep
                ctx.remap_destroy(remap)


# ---- the transfer window ------------------------------------------------------------------------------------------------
def poisoned(frame, stored, layout, window):
    """the frame with every byte outside the window's planes inverted"""
    keep = np.zeros(frame.size, bool)
    for off, pitch, row, rows in fs.yuv_planes(stored, layout, stored[0], window):
        for r in range(rows):
            keep[off + r * pitch: off + r * pitch + row] = True
    flat = frame.reshape(-1).copy()
    flat[~keep] ^= 0xFF
    return flat.reshape(frame.shape)


@pytest.mark.parametrize("pinned", [False, True], ids=["staged", "pinned_frames"])
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_only_the_window_of_a_host_nv12_frame_is_read(out, pinned):
    """a map confined to an interior rectangle of a 320 x 180 NV12 frame: the operand is the full frame's although every
    byte outside the R6 window is inverted -- out of ffl_host_alloc memory (one 2-D copy per plane) and out of pageable
    memory (the staging copy)"""
    up, layout = (320, 180), "nv12"
    frames = [fs.yuv_frame(k, up[0], up[1], layout, 5 + i) for i, k in enumerate(("noise", "ramp"))]
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        for S, (rot, mir) in zip(SUPER, ORIENTS):
            m = rr.hostile_map(out, S, up, 77 + S, INTERIOR)
            want = [rr.operand(yuv_ref.yuv_to_bgr(f, layout), m, S) for f in frames]
            stored = up[::-1] if rot in (90, 270) else up
            _, win, _ = _capi.remap_check(m, out, stored, S, rotate=rot, mirror=mir)
            assert win == rr.windows(m, S, stored, rot, mir)[1] and win[2] * win[3] < up[0] * up[1] and (win[0] > 0 or win[1] > 0)
            st = [poisoned(fo.inverse_orient420(f, layout, rot, mir), stored, layout, win) for f in frames]
            assert not np.array_equal(st[0], fo.inverse_orient420(frames[0], layout, rot, mir))
            if pinned:
                pin = ctx.pinned_frames(2, size=stored, yuv=True)
                pin[:] = np.stack(st)
                st = [pin[0], pin[1]]
            remap = ctx.remap_create(m, up, S)
            prefill(ctx, 1, 2, out)
            ctx.upload_frames_remap(1, st, remap, layout, rotate=rot, mirror=mir)
            check(ctx, 1, want, out, (S, rot, mir))
            ctx.remap_destroy(remap)


# ---- lifetime -----------------------------------------------------------------------------------------------------------
def test_map_lifetime():
    out, src = fs.OUTS[1], (34, 18)
    frames = [fs.bgr_frame(k, src[0], src[1], 3 + i) for i, k in enumerate(("noise", "ramp"))]
    maps = [rr.hostile_map(out, S, src, 60 + S) for S in (1, 2)]
    want = [[rr.operand(f, m, S) for f in frames] for m, S in zip(maps, (1, 2))]
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        a, b = (ctx.remap_create(m, src, S) for m, S in zip(maps, (1, 2)))
        assert (a.id, b.id) == (0, 1) and (a.supersample, b.supersample) == (1, 2) and a.src_size == b.src_size == src
        for r in (a, b, a, b):                                 # two maps alive and alternated
            prefill(ctx, 1, 2, out)
            ctx.upload_frames_remap(1, frames, r)
            check(ctx, 1, want[r.id], out, ("alternated", r.id))
        prefill(ctx, 1, 2, out)                                # create -> upload -> destroy -> download
        c = ctx.remap_create(maps[1], src, 2)
        ctx.upload_frames_remap(1, frames, c)
        ctx.remap_destroy(c)
        check(ctx, 1, want[1], out, "destroyed straight after the upload")
        more = [ctx.remap_create(maps[0], src, 1) for _ in range(_capi.FFL_MAX_REMAPS - 2)]
        assert sorted(r.id for r in [a, b] + more) == list(range(_capi.FFL_MAX_REMAPS))
        with pytest.raises(_capi.FFLError, match="8 maps are alive already") as e:     # the ninth
            ctx.remap_create(maps[0], src, 1)
        assert e.value.code == _capi.FFL_ERR_INVALID
        ctx.remap_destroy(more[3])
        again = ctx.remap_create(maps[1], src, 2)              # after one destroy a create succeeds again, in the freed place
        assert again.id == more[3].id
        prefill(ctx, 1, 2, out)
        ctx.upload_frames_remap(1, frames, again)
        check(ctx, 1, want[1], out, "the map created after the refusal")
        ctx.remap_destroy(more[0])
        bad = maps[0].copy()
        bad[0, 0] = (32 * src[0], 0)
        with pytest.raises(ValueError, match="map entry 0 "):                           # an invalid map creates nothing ...
            ctx.remap_create(bad, src, 1)
        rid = C.c_int(-1)                                                               # ... the library's own check included
        assert ctx.L.ffl_remap_create(ctx._h, bad.ctypes.data, 1, src[0], src[1], C.byref(rid)) == _capi.FFL_ERR_INVALID
        assert b"map entry 0 " in ctx.L.ffl_last_error(ctx._h) and rid.value == -1
        assert ctx.remap_create(maps[0], src, 1).id == more[0].id
    # maps left alive are freed with the context


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_happen_before_any_device_work():
    out, src = fs.OUTS[0], (34, 18)
    frames = [fs.bgr_frame("noise", src[0], src[1], i) for i in range(2)]
    nv12 = [fs.yuv_frame("noise", src[0], src[1], "nv12", i) for i in range(2)]
    m = rr.hostile_map(out, 1, src, 9)
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        remap = ctx.remap_create(m, src, 1)
        gone = ctx.remap_create(m, src, 1)
        ctx.remap_destroy(gone)
        with pytest.raises(_capi.FFLError, match="names no map"):
            ctx.remap_destroy(gone)
        for call, words in (
                (lambda: ctx.upload_frames_remap(1, [f[:, :32] for f in frames], remap), "the upright source is 32x18, map 0 was created for 34x18"),
                (lambda: ctx.upload_frames_remap(1, frames, remap, rotate=90), "the upright source is 18x34"),
                (lambda: ctx.upload_frames_remap(1, frames, gone), "remap id 1 names no map"),
                (lambda: ctx.upload_frames_remap(1, frames, 99), "remap id 99 names no map"),
                (lambda: ctx.upload_frames_remap(1, frames, remap, yuv_range="full"), "full_range describes 4:2:0 sources"),
                (lambda: ctx.upload_frames_remap(3, frames, remap), "bad frame slot range"),
                (lambda: ctx.upload_frames_remap(1, nv12, remap, "nv12", depth=8, rotate=45), "rotate")):
            with pytest.raises((_capi.FFLError, ValueError), match=words):
                call()
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        gray = (ctx._h, 1, 2, ptrs, _capi.DEV_FORMATS["gray"], src[0], src[1], src[0], 8, 0, remap.id, None)
        assert ctx.L.ffl_upload_frames_remap(*gray) == _capi.FFL_ERR_INVALID           # gray on the host call
        assert b"host gray frames have no map path" in ctx.L.ffl_last_error(ctx._h)
        rid = C.c_int(-1)
        assert ctx.L.ffl_remap_create(ctx._h, m.ctypes.data, 3, src[0], src[1], C.byref(rid)) == _capi.FFL_ERR_INVALID
        assert b"supersample 3 is not one of 1, 2, 4" in ctx.L.ffl_last_error(ctx._h) and rid.value == -1
        with pytest.raises(ValueError, match="supersample"):
            ctx.remap_create(m, src, 3)
        if torch is not None:
            t = [dev(f) for f in nv12]
            with pytest.raises(_capi.FFLError, match="remap id 1 names no map"):
                ctx.upload_frames_device_remap(1, t, "nv12", gone)
            with pytest.raises(_capi.FFLError, match="map 0 was created for 34x18"):
                ctx.upload_frames_device_remap(1, [x[:, :32] for x in t], "nv12", remap)
            pin = ctx.pinned_frames(1, size=src, yuv=True)     # page-locked host memory belongs to the host call, and is sent there

            class Host:
                __cuda_array_interface__ = {"version": 2, "data": (pin.ctypes.data, False), "shape": pin[0].shape, "strides": None,
                                            "typestr": "|u1"}
            with pytest.raises(_capi.FFLError, match="page-locked host memory.*host frames go through ffl_upload_frames_remap$"):
                ctx.upload_frames_device_remap(1, [Host()], "nv12", remap)
            x = torch.zeros(16, device="cuda:0")               # a capturing stream
            g = torch.cuda.CUDAGraph()
            codes = []
            torch.cuda.synchronize()
            with torch.cuda.graph(g):
                try:
                    ctx.upload_frames_device_remap(1, t, "nv12", remap, stream=torch.cuda.current_stream())
                except _capi.FFLError as err:
                    codes.append((err.code, "capturing" in str(err), "ffl_upload_frames_device_remap" in str(err)))
                x += 1
            g.replay()
            torch.cuda.synchronize()
            assert codes == [(_capi.FFL_ERR_STATE, True, True)] and float(x.sum()) == 16.0
        check(ctx, 1, [fs.slot_pattern(1, out), fs.slot_pattern(2, out)], out, "refused calls wrote nothing")
        ctx.upload_frames_remap(1, frames, remap)
        check(ctx, 1, [rr.operand(f, m, 1) for f in frames], out, "the upload after the refusals")


# ---- end to end ---------------------------------------------------------------------------------------------------------
def test_chunk_through_a_view_map_equals_the_restated_operands():
    """process_chunk on 8 NV12 frames through DecodedUploader(remap=), and through DeviceUploader(remap=) from device
    memory, == the same chunk fed remap_ref's operands"""
    from funscript_flow_amd.synth import sine_translate_frames
    src, out, S = (160, 80), (48, 32), 2
    g = sine_translate_frames(8, src[0], src[1], seed=4, amp=(3.0, 2.0), period=13)
    c = np.full((src[1] // 2, src[0] // 2), 128, np.uint8)
    clip = [fs.pack420(f, c, c, "nv12") for f in g]
    m = frontend.view_map(src, out, "equirect", 70, yaw=-8, pitch=5, rect=frontend.eye_rect(src, "sbs", "left"), supersample=S)
    operands = [rr.operand(yuv_ref.yuv_to_bgr(f, "nv12"), m, S) for f in clip]
    assert len({o.tobytes() for o in operands}) == 8
    res = []
    runs = [(clip, lambda ctx: frontend.DecodedUploader(ctx, yuv="nv12", remap=ctx.remap_create(m, src, S))),
            (operands, lambda ctx: None)]
    if torch is not None:
        runs.append(([dev(f) for f in clip], lambda ctx: frontend.DeviceUploader(ctx, "nv12", remap=ctx.remap_create(m, src, S))))
    for frames, upload in runs:
        with _capi.Context(*out, max_batch=4, frame_slots=10, flow_slots=pipeline.min_flow_slots(4)) as ctx:
            res.append(pipeline.PairEngine(ctx, upload(ctx)).process_chunk(frames))
    (d1, r1) = res[1]
    assert len(d1) == 7
    for d, r in res[:1] + res[2:]:
        assert np.array_equal(np.asarray(d), np.asarray(d1)) and [tuple(x) for x in r] == [tuple(x) for x in r1]


def test_hip_view_through_the_prefetch_ring():
    """params["hip_view"]: frames of a (fake) side-by-side capture go from the page-locked ring through a view map to the
    actions of the same engine fed the decoded list through DecodedUploader(remap=)"""
    from funscript_flow_amd import prefetch
    from funscript_flow_amd.synth import gray_to_bgr, sine_translate_frames
    sw, sh, n, fps = 192, 96, 41, 30.0
    srcf = gray_to_bgr(sine_translate_frames(n, sw, sh, seed=6, amp=(3.0, 2.0), period=12, zoom=0.03))

    class Cap:
        pos = 0

        def get(self, prop):
            return {prefetch.CAP_PROP_FRAME_COUNT: n, prefetch.CAP_PROP_FPS: fps, prefetch.CAP_PROP_FRAME_WIDTH: sw,
                    prefetch.CAP_PROP_FRAME_HEIGHT: sh}[prop]

        def grab(self):
            self.pos += 1
            return self.pos <= n

        def read(self, image=None):
            if self.pos >= n:
                return False, None
            np.copyto(image, srcf[self.pos])
            self.pos += 1
            return True, image

    view = {"projection": "equirect", "fov": 80, "stereo": "sbs", "eye": "left", "supersample": 2}
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False}
    with _capi.Context(64, 48, max_batch=4, frame_slots=10, flow_slots=pipeline.min_flow_slots(4)) as ctx:
        got = prefetch.video_to_actions(ctx, Cap(), {**params, "hip_view": view})
        for _ in range(_capi.FFL_MAX_REMAPS):                  # every call frees the map it made: the context does not run out
            assert prefetch.video_to_actions(ctx, Cap(), {**params, "hip_view": view}) == got
        assert [ctx.remap_create(frontend.identity_map((64, 48)), (64, 48)).id for _ in range(2)] == [0, 1]
        plain = prefetch.video_to_actions(ctx, Cap(), params)
        m = frontend.view_map((sw, sh), (64, 48), "equirect", 80, rect=(0, 0, sw // 2, sh), supersample=2)
        eng = pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, remap=ctx.remap_create(m, (sw, sh), 2)))   # id 2
        want = pipeline.frames_to_actions(eng, [srcf[i] for i in range(n)], fps, params)
    assert got == want and len(got) == 38 and got != plain   # 41 frames -> chunks of 20, 20, 1 (skipped) -> 19 + 19 pairs
