"""Host side of the front-end's stream metadata (ffl_source_info; DESIGN.md appendix Y, rules Y6 and Y7; no GPU): that
orientation commutes with the colour conversion, the stored-frame window of the _src helpers against a numpy restatement,
the identity of a NULL / zero struct with the plain calls, every refusal by its words, and rule Y7's known answers."""
import ctypes as C
import os

import numpy as np
import pytest

import front_orient as fo
import front_sweep as fs
import gen_yuv_range_golden as gen
import yuv16_ref
import yuv_ref
from funscript_flow_amd import _capi, frontend, prefetch

LAYOUTS = ("i420", "nv12")


def flipped(size, rotate):
    return size[::-1] if rotate in (90, 270) else size


# ---- Y6 -------------------------------------------------------------------------------------------------------------------
def test_orient_restates_the_table_and_inverts():
    for sw, sh in ((6, 4), (4, 6)):
        S = np.arange(sw * sh).reshape(sh, sw)
        for r, m in fo.ORIENTATIONS:
            U = fo.orient(S, r, m)
            assert U.shape == flipped((sh, sw), r)
            uy, ux = np.mgrid[0:U.shape[0], 0:U.shape[1]]
            px, py = fo.stored_xy(ux, uy, (sw, sh), r, m)
            assert np.array_equal(U, S[py, px]), (r, m)
            assert np.array_equal(fo.inverse_orient(U, r, m), S)
            assert np.array_equal(fo.orient(fo.inverse_orient(S, r, m), r, m), S)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("size", [(6, 4), (4, 6)])
def test_orientation_commutes_with_the_colour_conversion(size, layout):
    """cvtColor(orient(planes)) == orient(cvtColor(planes)): 2x2 chroma blocks map to 2x2 chroma blocks"""
    for seed, dtype in ((1, np.uint8), (2, np.uint16)):
        f = yuv_ref.random_frame(size[0], size[1], layout, seed)
        f = f if dtype is np.uint8 else yuv16_ref.widen(f, 10, False)
        for r, m in fo.ORIENTATIONS:
            o = fo.orient420(f, layout, r, m)
            assert o.dtype == f.dtype and o.shape == (flipped(size, r)[1] * 3 // 2, flipped(size, r)[0])
            assert np.array_equal(fo.inverse_orient420(o, layout, r, m), f)
            if dtype is np.uint8:
                assert np.array_equal(fo.orient(yuv_ref.yuv_to_bgr(f, layout), r, m), yuv_ref.yuv_to_bgr(o, layout)), (r, m)
                assert np.array_equal(fo.orient(fo.yuv_to_bgr_full(f, layout), r, m), fo.yuv_to_bgr_full(o, layout)), (r, m)


# ---- the window -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("out", fs.OUTS[:2], ids=lambda o: f"{o[0]}x{o[1]}")
def test_window_equals_the_restatement_and_holds_every_mapped_tap(out, layout):
    seen = set()
    for name, usrc, rs, crop in fs.geoms(*out):
        for r, m in fo.ORIENTATIONS:
            stored = flipped(usrc, r)
            want, (xs, ys) = fo.stored_window(stored, rs, crop, out, r, m)
            for depth in (8, 10):
                win, nbytes = _capi.frontend_yuv_window(stored, layout, rs, crop, out, depth=depth, rotate=r, mirror=m)
                assert win == want, (name, crop, r, m, depth)
                assert nbytes == win[2] * win[3] * 3 // 2 * (2 if depth > 8 else 1)
            x, y, w, h = want
            assert x % 16 == 0 and y % 2 == 0 and h % 2 == 0 and w % 2 == 0 and w > 0 and h > 0
            assert 0 <= x and x + w <= stored[0] and 0 <= y and y + h <= stored[1]
            assert xs.min() >= x and xs.max() < x + w and ys.min() >= y and ys.max() < y + h, (name, crop, r, m)
            seen.add((w < stored[0], h < stored[1]))
    assert (True, True) in seen          # some window is a proper part of its frame on both stored axes


def _window_call(L, name, stored, code, depth, geom, info):
    win, b = (C.c_int * 4)(), C.c_size_t()
    args = (stored[0], stored[1], code, stored[0] * (2 if depth > 8 else 1)) + ((depth,) if depth > 8 else ()) + geom
    rc = getattr(L, name)(*args, win, C.byref(b), *info)
    return rc, tuple(win), b.value


@pytest.mark.parametrize("depth", [8, 10])
def test_null_and_zero_info_are_the_plain_helpers(depth):
    L = _capi.load()
    plain = "ffl_frontend_yuv_window" if depth == 8 else "ffl_frontend_yuv16_window"
    zero = _capi.SourceInfo(0, 0, 0)
    for out in fs.OUTS[:2]:
        for name, src, rs, crop in fs.geoms(*out):
            for code in (0, 1):
                geom = (rs[0], rs[1], crop[0], crop[1], out[0], out[1])
                want = _window_call(L, plain, src, code, depth, geom, ())
                assert want[0] == 0
                assert _window_call(L, plain + "_src", src, code, depth, geom, (None,)) == want
                assert _window_call(L, plain + "_src", src, code, depth, geom, (C.byref(zero),)) == want
    # the same messages: a refusal of the plain call, word for word
    geom = (40, 40, 30, 30, 16, 16)
    for info in ((), (None,), (C.byref(zero),)):
        assert _window_call(L, plain + ("_src" if info else ""), (32, 32), 0, depth, geom, info)[0] == _capi.FFL_ERR_INVALID
        msg = L.ffl_last_error(None).decode()
        assert msg.startswith(plain + ": crop window (30, 30) + 16x16 does not fit the 40x40 resized frame"), msg
    assert _capi.source_info() is None and _capi.source_info(0, False, "limited") is None


def test_dev_frame_check_null_and_zero_info():
    L = _capi.load()
    f = _capi.DevFrame((C.c_void_p * 3)(4096, 0, 0), (C.c_ssize_t * 3)(96, 0, 0), 3, 1)
    zero = _capi.SourceInfo(0, 0, 0)
    for args, rc in (((1, 32, 20, C.byref(f), 32, 20, 0, 0, 16, 16), 0), ((1, 32, 20, C.byref(f), 32, 20, 20, 0, 16, 16), 1)):
        assert L.ffl_dev_frame_check(*args) == rc
        msg = L.ffl_last_error(None).decode()
        for info in (None, C.byref(zero)):
            assert L.ffl_dev_frame_check_src(*args, info) == rc
            assert L.ffl_last_error(None).decode() == msg


# ---- refusals -------------------------------------------------------------------------------------------------------------
def _raw_info(L, rotate, mirror, full):
    win, b = (C.c_int * 4)(), C.c_size_t()
    info = _capi.SourceInfo(rotate, mirror, full)
    rc = L.ffl_frontend_yuv_window_src(32, 32, 0, 32, 32, 32, 0, 0, 16, 16, win, C.byref(b), C.byref(info))
    return rc, L.ffl_last_error(None).decode()


def test_library_refusals_by_their_words():
    L = _capi.load()
    for rot in (45, -90, 360, 1):
        rc, msg = _raw_info(L, rot, 0, 0)
        assert rc == _capi.FFL_ERR_INVALID and f"rotate {rot} is not one of 0, 90, 180, 270" in msg, msg
    for mir in (2, -1):
        rc, msg = _raw_info(L, 0, mir, 0)
        assert rc == _capi.FFL_ERR_INVALID and f"mirror {mir} is neither 0 nor 1" in msg, msg
    for full in (2, -1):
        rc, msg = _raw_info(L, 0, 0, full)
        assert rc == _capi.FFL_ERR_INVALID and f"full_range {full} is neither 0 nor 1" in msg, msg
    assert _raw_info(L, 270, 1, 1)[0] == 0
    # full range on sources that are not 4:2:0
    bgr = _capi.DevFrame((C.c_void_p * 3)(4096, 0, 0), (C.c_ssize_t * 3)(96, 0, 0), 3, 1)
    bgr.width, bgr.height = 32, 20
    gray = _capi.DevFrame((C.c_void_p * 3)(4096, 0, 0), (C.c_ssize_t * 3)(16, 0, 0), 1, 0)
    gray.width, gray.height = 16, 20
    for fmt, fr, rs in (("bgr", bgr, (32, 20)), ("rgb", bgr, (32, 20)), ("gray", gray, (16, 20))):
        with pytest.raises(ValueError, match="full_range describes 4:2:0 sources"):
            _capi.dev_frame_check(fmt, fr, rs, (0, 0), (16, 20), yuv_range="full")
    # existing refusals, in upright terms: a 32x20 stored frame is 20x32 upright
    _capi.dev_frame_check("bgr", bgr, (20, 32), (4, 12), (16, 20), rotate=90)
    with pytest.raises(ValueError, match=r"crop window \(5, 12\) \+ 16x20 does not fit the 20x32 resized frame"):
        _capi.dev_frame_check("bgr", bgr, (20, 32), (5, 12), (16, 20), rotate=90)
    _capi.dev_frame_check("gray", gray, (20, 16), (0, 0), (20, 16), rotate=270, mirror=True)
    with pytest.raises(ValueError, match="a gray frame must be the context size 16x20, got 20x16"):
        _capi.dev_frame_check("gray", gray, (20, 16), (0, 0), (16, 20), rotate=90)
    with pytest.raises(ValueError, match=r"gray frames are copied as they are: a resize \(20x16 -> 16x20\)"):
        _capi.dev_frame_check("gray", gray, (16, 20), (0, 0), (16, 20), rotate=90)
    # the identity mode is chosen in upright terms: 32x20 stored, rotated, resized to 20x32 transfers as identity does
    win, _ = _capi.frontend_yuv_window((32, 20), "nv12", (20, 32), (2, 6), (16, 20), rotate=90)
    assert win == fo.stored_window((32, 20), (20, 32), (2, 6), (16, 20), 90, False)[0]
    with pytest.raises(ValueError, match=r"crop window \(0, 0\) \+ 16x24 does not fit the 32x20 resized frame"):
        _capi.frontend_yuv_window((32, 20), "nv12", (32, 20), (0, 0), (16, 24), rotate=90)
    with pytest.raises(ValueError, match="4:2:0 needs an even width and height"):
        _capi.frontend_yuv_window((31, 20), "nv12", (20, 31), (0, 0), (16, 20), rotate=90)


def test_python_keywords_are_checked_at_construction():
    for bad in (45, "90", 90.0, True, None):
        with pytest.raises(ValueError, match="rotate must be one of"):
            _capi.source_info(rotate=bad)
    with pytest.raises(ValueError, match="mirror must be False or True"):
        _capi.source_info(mirror=2)
    for bad in ("jpeg", 1, None, "pc"):
        with pytest.raises(ValueError, match="yuv_range must be one of"):
            _capi.source_info(yuv_range=bad)
    info = _capi.source_info(270, True, "FULL")
    assert (info.rotate, info.mirror, info.full_range) == (270, 1, 1)

    class NoContext:
        width = height = 16

    with pytest.raises(ValueError, match="rotate must be one of .* describe the stream"):
        frontend.DecodedUploader(NoContext(), yuv="nv12", rotate=91)
    with pytest.raises(ValueError, match="yuv_range must be one of .* describe the stream"):
        frontend.DecodedUploader(NoContext(), yuv="nv12", yuv_range="tv")
    with pytest.raises(ValueError, match="yuv_range=\"full\" describes 4:2:0 frames"):
        frontend.DecodedUploader(NoContext(), yuv_range="full")
    with pytest.raises(ValueError, match="yuv_range=\"full\" describes 4:2:0 frames"):
        frontend.DeviceUploader(NoContext(), "bgr", yuv_range="full")
    with pytest.raises(ValueError, match="rotate must be one of"):
        frontend.DeviceUploader(NoContext(), "nv12", rotate=-90)
    with pytest.raises(ValueError, match="mirror must be False or True"):
        frontend.upload_decoded(NoContext(), 0, [], yuv="i420", mirror="yes")
    up = frontend.DecodedUploader(NoContext(), yuv="nv12", rotate=90, yuv_range="full")
    assert up.src == {"rotate": 90, "yuv_range": "full"}
    assert frontend.DecodedUploader(NoContext(), yuv="nv12").src == {}
    assert frontend.DecodedUploader(NoContext(), rotate=180, mirror=True).src == {"rotate": 180, "mirror": True}


def test_prefetch_params_carry_the_metadata_only_when_set():
    assert prefetch.yuv_params({"hip_yuv": "nv12"}) == ("nv12", {})
    p = {"hip_yuv": "nv12", "hip_yuv_depth": 10, "hip_rotate": 90, "hip_mirror": 1, "hip_yuv_range": "full"}
    assert prefetch.yuv_params(p) == ("nv12", {"depth": 10, "rotate": 90, "mirror": True, "yuv_range": "full"})
    assert prefetch.ring_depth(prefetch.yuv_params(p)[1]) == {"depth": 10}      # the ring is sized by the stored frame
    assert prefetch.yuv_params({"hip_rotate": 270}) == (None, {"rotate": 270})


# ---- Y7 -------------------------------------------------------------------------------------------------------------------
def test_full_range_integers():
    want = [round(c * 2 ** 20) for c in (1.772, 0.714136, 0.344136, 1.402)]
    assert [fo.CB, fo.CG_V, fo.CG_U, fo.CR] == want == [1858077, 748826, 360853, 1470104]


def test_full_range_known_answers():
    Y = np.arange(256)
    gray = fo.yuv_to_bgr_full_pixels(Y, np.full(256, 128), np.full(256, 128))
    assert np.array_equal(gray, np.repeat(Y[:, None], 3, 1))             # U = V = 128: B = G = R = Y
    corners = {(0, 0, 0): (0, 135, 0), (255, 0, 0): (28, 255, 76), (0, 255, 0): (225, 48, 0), (255, 255, 0): (255, 255, 76),
               (0, 0, 255): (0, 0, 178), (255, 0, 255): (28, 208, 255), (0, 255, 255): (225, 0, 178),
               (255, 255, 255): (255, 121, 255)}
    for (y, u, v), bgr in corners.items():
        # the integers, by hand: floor((y * 2^20 + 2^19 + c * (x - 128)) / 2^20), saturated
        b = (y * 2 ** 20 + 2 ** 19 + 1858077 * (u - 128)) // 2 ** 20
        g = (y * 2 ** 20 + 2 ** 19 - 748826 * (v - 128) - 360853 * (u - 128)) // 2 ** 20
        r = (y * 2 ** 20 + 2 ** 19 + 1470104 * (v - 128)) // 2 ** 20
        assert tuple(min(max(c, 0), 255) for c in (b, g, r)) == bgr, (y, u, v)
        assert tuple(fo.yuv_to_bgr_full_pixels(y, u, v)) == bgr, (y, u, v)
    for y in (16, 235):                                                  # where limited range clips and full range does not
        lim, full = yuv_ref.yuv_to_bgr_pixels(y, 128, 128), fo.yuv_to_bgr_full_pixels(y, 128, 128)
        assert tuple(full) == (y, y, y) and tuple(lim) == ((0, 0, 0) if y == 16 else (255, 255, 255))


def test_golden_file_is_what_the_generator_writes():
    rec = np.load(gen.PATH)
    now = gen.golden()
    assert sorted(rec.files) == sorted(now)
    for k, v in now.items():
        assert rec[k].dtype == v.dtype and np.array_equal(rec[k], v), k
    assert os.path.getsize(gen.PATH) < 16384
    assert rec["i420_operand"].shape == (16, 16) and rec["nv12_bgr"].shape == (8, 8, 3)
