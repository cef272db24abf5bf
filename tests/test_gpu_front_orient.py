"""GPU tests of the front-end's stream metadata (ffl_source_info; DESIGN.md appendix Y, rules Y6 and Y7) at the small shapes
of tests/front_sweep.py.  Orientation is an index permutation, so every expectation is an existing one: a table row's frame
is taken as the UPRIGHT frame, inverse_orient() of it is what gets uploaded, and the slot must hold the row's cached operand
bit for bit -- through every source kind of k_frontend and k_frontend_dev.  Full range is checked against the numpy
restatement of rule Y7 (tests/front_orient.py).  Every written slot is first filled with front_sweep.slot_pattern."""
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
import yuv16_ref
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline

OUT_IDS = [f"{w}x{h}" for w, h in fs.OUTS]
QUARTERS = ((90, False), (270, True))
HOST_KINDS = ("host_bgr", "host_rgb", "host_i420", "host_nv12_padded", "host_yuv420p10le", "host_p010")
DEV_KINDS = ("dev_bgr_padded", "dev_planar_rgb", "dev_bgra", "dev_i420_pitches", "dev_nv12", "dev_p010", "dev_gray")


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


def i420_rows(frames, seed, dtype=np.uint8):
    """ffl_dev_frame rows of I420 frames whose planes lie in separate allocations with three different pitches"""
    keep, rows = [], []
    es = np.dtype(dtype).itemsize
    for i, f in enumerate(frames):
        planes = yuv_ref.planes(f, "i420")
        w = planes[0].shape[1]
        pitches = [w + 3 + i, w // 2 + 1, w // 2 + 6 + i]
        t = [dev(padded(np.ascontiguousarray(p), pitch - p.shape[1], seed + 10 * i + k).base)
             for k, (p, pitch) in enumerate(zip(planes, pitches))]
        keep += t
        rows.append([x.data_ptr() for x in t] + [p * es for p in pitches] + [1, 0])
    return rows, keep


def upload_kind(ctx, kind, first, upright_bgr, upright_yuv, layout, rs, crop, rot, mir, seed, **more):
    """uploads the stored forms of the upright frames through source kind `kind` with rotate=rot, mirror=mir; returns what
    must stay alive until the slots have been read"""
    src = dict(rotate=rot, mirror=mir, **more)
    if kind in ("host_bgr", "host_rgb"):
        st = [np.ascontiguousarray(fo.inverse_orient(f, rot, mir)) for f in upright_bgr]
        ctx.upload_frames_raw(first, st, rs, crop, rgb_order=kind == "host_rgb", **src)
        return st
    if kind in ("dev_bgr_padded", "dev_planar_rgb", "dev_bgra"):
        st = [np.ascontiguousarray(fo.inverse_orient(f, rot, mir)) for f in upright_bgr]
        if kind == "dev_bgr_padded":
            t = [dev(padded(f, 5, seed + i).base)[:, :f.shape[1]] for i, f in enumerate(st)]
        elif kind == "dev_planar_rgb":
            t = [dev(f.transpose(2, 0, 1)) for f in st]
        else:
            t = [dev(np.concatenate([f, junk(f.shape[:2] + (1,), seed + i)], 2)) for i, f in enumerate(st)]
        ctx.upload_frames_device(first, t, "rgb" if kind == "dev_planar_rgb" else "bgr", rs, crop, **src)
        return t
    st = [fo.inverse_orient420(f, layout, rot, mir) for f in upright_yuv]
    if kind in ("host_i420", "host_nv12_padded"):
        st = [padded(f, 6, seed + i) for i, f in enumerate(st)] if kind == "host_nv12_padded" else st
        ctx.upload_frames_yuv(first, st, layout, rs, crop, **src)
        return st
    if kind in ("host_yuv420p10le", "host_p010"):
        st = [yuv16_ref.widen(f, 10, layout == "nv12") for f in st]
        ctx.upload_frames_yuv(first, st, layout, rs, crop, depth=10, **src)
        return st
    if kind == "dev_i420_pitches":
        size = (st[0].shape[1], st[0].shape[0] * 2 // 3)
        rows, keep = i420_rows(st, seed)
        d = np.ascontiguousarray(rows, np.int64)
        info = _capi.source_info(**src)
        args = (ctx._h, first, len(st), d.ctypes.data, _capi.dev_format("i420"), size[0], size[1], rs[0], rs[1], crop[0], crop[1],
                _capi.stream_handle(None, ctx.device))
        ctx._chk(ctx.L.ffl_upload_frames_device_src(*args, C.byref(info)) if info is not None else
                 ctx.L.ffl_upload_frames_device(*args))
        return keep
    if kind == "dev_nv12":
        t = [dev(padded(f, 9, seed + i).base)[:, :f.shape[1]] for i, f in enumerate(st)]
        ctx.upload_frames_device(first, t, "nv12", rs, crop, **src)
        return t
    if kind == "dev_p010":
        t = [dev(yuv16_ref.widen(f, 10, True)) for f in st]
        ctx.upload_frames_device(first, t, "nv12", rs, crop, depth=10, **src)
        return t
    raise ValueError(kind)


FULL_KINDS = {"i420": ("host_i420", "host_yuv420p10le", "dev_i420_pitches"),       # host and device, 8 and 10 bits
              "nv12": ("host_nv12_padded", "host_p010", "dev_nv12", "dev_p010")}


def layout_of(kind):
    return "i420" if ("i420" in kind or "yuv420p" in kind) else "nv12"


def orientations(out):
    """all eight at the two smallest sizes; at the sizes with two and three x-tiles the two quarter turns"""
    return fo.ORIENTATIONS if out in fs.OUTS[:2] else QUARTERS


@pytest.mark.parametrize("kind", HOST_KINDS + DEV_KINDS)
@pytest.mark.parametrize("out", fs.OUTS, ids=OUT_IDS)
def test_orientation_sweep_bit_exact(out, kind):
    if kind.startswith("dev") and torch is None:
        pytest.skip("needs torch")
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        if kind == "dev_gray":                               # the stored size is the context's, transposed by a quarter turn
            for k, (rot, mir) in enumerate(orientations(out)):
                up = [junk((out[1], out[0]), 10 * k + i) for i in range(2)]
                st = [np.ascontiguousarray(fo.inverse_orient(g, rot, mir)) for g in up]
                assert st[0].shape == ((out[0], out[1]) if rot in (90, 270) else (out[1], out[0]))
                t = [dev(padded(st[0], 7, k).base)[:, :st[0].shape[1]], dev(np.stack([st[1]] * 3, -1))[..., 1]]
                prefill(ctx, 1, 2, out)
                ctx.upload_frames_device(1, t, "gray", rotate=rot, mirror=mir)
                check(ctx, 1, up, out, (kind, rot, mir))
            return
        layout = layout_of(kind)
        bgr, yuv = fs.bgr_cases(out), fs.yuv_cases(out, layout)
        for k, (b, y) in enumerate(zip(bgr, yuv)):
            name, usrc, rs, crop = b[:4]
            assert y[:4] == b[:4]
            is_yuv = "bgr" not in kind and "rgb" not in kind
            want = y[5] if is_yuv else b[6] if "rgb" in kind else b[5]
            for rot, mir in orientations(out):
                prefill(ctx, 1, 2, out)
                keep = upload_kind(ctx, kind, 1, b[4], y[4], layout, rs, crop, rot, mir, 1000 * k)
                check(ctx, 1, want, out, (kind, name, crop, rot, mir))
                del keep


@pytest.mark.parametrize("kind", ["host_bgr", "host_nv12_padded", "dev_bgr_padded", "dev_nv12"])
def test_src_call_equals_the_plain_call_on_the_upright_frame(kind):
    """device against device: for one row per resize mode, the _src call on inverse_orient(f) == the plain call on f"""
    if kind.startswith("dev") and torch is None:
        pytest.skip("needs torch")
    out, layout = fs.OUTS[1], "nv12"
    bgr, yuv = fs.bgr_cases(out), fs.yuv_cases(out, layout)
    picked = {}
    for k, b in enumerate(bgr):
        picked.setdefault(fs.mode(b[1], b[2]), k)
    assert sorted(picked) == sorted(fs.MODES)
    with _capi.Context(*out, max_batch=1, frame_slots=6) as ctx:
        for mode, k in picked.items():
            b, y = bgr[k], yuv[k]
            rs, crop = b[2], b[3]
            prefill(ctx, 0, 6, out)
            if kind == "host_bgr":
                ctx.upload_frames_raw(3, b[4], rs, crop)
            elif kind == "host_nv12_padded":
                ctx.upload_frames_yuv(3, y[4], layout, rs, crop)
            elif kind == "dev_bgr_padded":
                keep0 = [dev(f) for f in b[4]]
                ctx.upload_frames_device(3, keep0, "bgr", rs, crop)
            else:
                keep0 = [dev(f) for f in y[4]]
                ctx.upload_frames_device(3, keep0, "nv12", rs, crop)
            plain = [ctx.download_frame(3 + i) for i in range(2)]
            for rot, mir in fo.ORIENTATIONS[1:]:
                prefill(ctx, 1, 2, out)
                keep = upload_kind(ctx, kind, 1, b[4], y[4], layout, rs, crop, rot, mir, k)
                check(ctx, 1, plain, out, (kind, mode, rot, mir))
                del keep


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
@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("out", fs.OUTS[:2], ids=OUT_IDS[:2])
def test_only_the_stored_window_is_read(out, layout, pinned):
    rows = [r for r in fs.yuv_cases(out, layout) if r[0] in ("identity_wide", "down_5p3")]
    assert {r[0] for r in rows} == {"identity_wide", "down_5p3"}
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        for name, usrc, rs, crop, frames, want in rows:
            for rot, mir in QUARTERS:
                stored = usrc[::-1]
                win, nbytes = _capi.frontend_yuv_window(stored, layout, rs, crop, out, rotate=rot, mirror=mir)
                assert nbytes == win[2] * win[3] * 3 // 2 < stored[0] * stored[1] * 3 // 2, (name, crop, rot, mir)
                st = [poisoned(fo.inverse_orient420(f, layout, rot, mir), stored, layout, win) for f in frames]
                assert not np.array_equal(st[0], fo.inverse_orient420(frames[0], layout, rot, mir))
                if pinned:
                    pin = ctx.pinned_frames(2, size=stored, yuv=True)
                    pin[:] = np.stack(st)
                    st = [pin[0], pin[1]]
                prefill(ctx, 1, 2, out)
                ctx.upload_frames_yuv(1, st, layout, rs, crop, rotate=rot, mirror=mir)
                check(ctx, 1, want, out, (name, crop, rot, mir))


@pytest.mark.parametrize("layout", ["i420", "nv12"])
@pytest.mark.parametrize("out", fs.OUTS[:2], ids=OUT_IDS[:2])
def test_full_range(out, layout):
    if torch is None:
        pytest.skip("needs torch")
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        differ = 0
        for k, (name, usrc, rs, crop) in enumerate(fs.geoms(*out)):
            up = [fs.yuv_frame(kind, usrc[0], usrc[1], layout, 50 * k + i) for i, kind in enumerate(("corners", "ramp"))]
            full = [fo.full_operand(f, layout, rs, crop, out) for f in up]
            lim = [fs.yuv_direct_operand(f, layout, rs, crop, out) for f in up]
            differ += not np.array_equal(full[1], lim[1])
            for kind in FULL_KINDS[layout]:
                for rot, rng, want in ((0, "full", full), (90, "full", full), (90, "limited", lim)):
                    prefill(ctx, 1, 2, out)
                    keep = upload_kind(ctx, kind, 1, None, up, layout, rs, crop, rot, False, k, yuv_range=rng)
                    check(ctx, 1, want, out, (kind, name, crop, rot, rng))
                    del keep
            prefill(ctx, 1, 2, out)                            # the same frames, limited, through the plain symbols
            ctx.upload_frames_yuv(1, up, layout, rs, crop, yuv_range="limited")
            check(ctx, 1, lim, out, (name, crop, "limited, plain"))
        assert differ > len(fs.geoms(*out)) // 2               # the two ranges are told apart by the ramp


def test_refusals_leave_the_context_usable():
    out, layout = fs.OUTS[0], "nv12"
    name, usrc, rs, crop, frames, want = fs.yuv_cases(out, layout)[0]
    with _capi.Context(*out, max_batch=1, frame_slots=4) as ctx:
        prefill(ctx, 0, 4, out)
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        args = (ctx._h, 1, 2, ptrs, usrc[0], usrc[1], frames[0].strides[0], 1, rs[0], rs[1], crop[0], crop[1])
        for info, words in ((_capi.SourceInfo(45, 0, 0), b"rotate 45 is not one of 0, 90, 180, 270"),
                            (_capi.SourceInfo(90, 3, 0), b"mirror 3 is neither 0 nor 1"),
                            (_capi.SourceInfo(0, 0, 7), b"full_range 7 is neither 0 nor 1")):
            assert ctx.L.ffl_upload_frames_yuv_src(*args, C.byref(info)) == _capi.FFL_ERR_INVALID
            assert words in ctx.L.ffl_last_error(ctx._h)
        bgr = [np.zeros((usrc[1], usrc[0], 3), np.uint8)] * 2
        with pytest.raises(_capi.FFLError, match="full_range describes 4:2:0 sources"):
            ctx.upload_frames_raw(1, bgr, rs, crop, yuv_range="full")
        with pytest.raises(_capi.FFLError, match="does not fit"):     # upright is usrc transposed: the resize no longer fits
            ctx.upload_frames_yuv(1, frames, layout, (usrc[0], 15), (0, 0), rotate=90)
        check(ctx, 1, [fs.slot_pattern(1, out), fs.slot_pattern(2, out)], out, "refused calls wrote nothing")
        st = [fo.inverse_orient420(f, layout, 270, True) for f in frames]
        ctx.upload_frames_yuv(1, st, layout, rs, crop, rotate=270, mirror=True)
        check(ctx, 1, want, out, "the upload after the refusals")


def test_rotated_clip_end_to_end():
    """a 20-frame 64x48 NV12 clip stored rotated by 90 gives the records and pass-2 scalars of the upright clip, bit for bit"""
    from funscript_flow_amd.synth import sine_translate_frames
    g = sine_translate_frames(20, 64, 48, seed=5, amp=(3.0, 2.0), period=7)
    c = np.full((24, 32), 128, np.uint8)
    clip = [fs.pack420(f, c, c, "nv12") for f in g]
    stored = [fo.inverse_orient420(f, "nv12", 90, False) for f in clip]
    assert stored[0].shape == (96, 48)
    res = []
    for frames, kw in ((clip, {}), (stored, {"rotate": 90})):
        with _capi.Context(64, 48, max_batch=4, frame_slots=10, flow_slots=pipeline.min_flow_slots(4)) as ctx:
            res.append(pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, yuv="nv12", **kw)).process_chunk(frames))
    (d0, r0), (d1, r1) = res
    assert len(d0) == 19 and np.array_equal(np.asarray(d0), np.asarray(d1))
    assert [tuple(r) for r in r0] == [tuple(r) for r in r1]
