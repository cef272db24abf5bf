"""Host side of the front-end sweep (tests/front_sweep.py; no GPU): the per-pixel restatement against the two-pass oracle
on every table row and content kind, and the self-checks of the table -- conditions on the sweep's INPUTS, so that a later
edit of a constant cannot quietly empty what tests/test_gpu_front_sweep.py covers."""
import numpy as np
import pytest

import front_sweep as fs
import oracle as orc
import yuv_ref
from funscript_flow_amd import _capi

LAYOUTS = ("i420", "nv12")


def window(src, layout, rs, crop, out):
    return _capi.frontend_yuv_window(src, layout, rs, crop, out)[0]


@pytest.mark.parametrize("out", fs.OUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_direct_operand_equals_the_oracle_bgr_and_rgb(out):
    for k, (name, src, rs, crop) in enumerate(fs.geoms(*out)):
        for kind in fs.BGR_KINDS:
            f = fs.bgr_frame(kind, src[0], src[1], k)
            for rgb in (False, True):
                assert np.array_equal(fs.direct_operand(f, rs, crop, out, rgb), fs.oracle_operand(f, rs, crop, out, rgb)), \
                    (name, crop, kind, rgb)
            if name == "exact_fit":                                      # and the oracle's own composed entry point
                assert rs == out and crop == (0, 0)
                assert np.array_equal(fs.direct_operand(f, rs, crop, out, False), orc.frontend(f, size=out))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("out", fs.OUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_direct_operand_equals_yuv_ref(out, layout):
    for k, (name, src, rs, crop) in enumerate(fs.geoms(*out)):
        for kind in fs.YUV_KINDS:
            f = fs.yuv_frame(kind, src[0], src[1], layout, k)
            assert f.shape == (src[1] * 3 // 2, src[0]) and f.dtype == np.uint8
            assert np.array_equal(fs.yuv_direct_operand(f, layout, rs, crop, out), yuv_ref.operand(f, layout, rs, crop, out)), \
                (name, crop, kind)


def test_content_kinds_are_what_they_claim():
    for kind in fs.YUV_KINDS:                                       # one image, two layouts
        a, b = fs.yuv_frame(kind, 12, 8, "i420", 3), fs.yuv_frame(kind, 12, 8, "nv12", 3)
        assert np.array_equal(yuv_ref.yuv_to_bgr(a, "i420"), yuv_ref.yuv_to_bgr(b, "nv12")), kind
    for lay in LAYOUTS:
        Y, U, V = yuv_ref.planes(fs.yuv_frame("corners", 16, 12, lay, 0), lay)
        got = {(int(Y[2 * j, 2 * i]), int(U[j, i]), int(V[j, i])) for j in range(6) for i in range(8)}
        assert got == {(y, u, v) for y in (0, 255) for u in (0, 255) for v in (0, 255)}
        bgr = yuv_ref.yuv_to_bgr(fs.yuv_frame("corners", 16, 12, lay, 0), lay)
        assert bgr.min() == 0 and bgr.max() == 255                  # both directions of saturation
    r = fs.bgr_frame("ramp", 9, 7, 0).astype(int)
    assert tuple(r[2, 3]) != tuple(r[3, 2])                          # a swapped axis shows
    assert len(set(r[2, 3])) == 3 and set(np.unique(fs.bgr_frame("checker", 6, 4, 0))) == {0, 255}
    assert (fs.bgr_frame("white", 6, 4, 0) == 255).all() and fs.bgr_frame("checker", 6, 4, 0)[0, 0, 0] != fs.bgr_frame("checker", 6, 4, 0)[0, 1, 0]


# ---- the table itself ---------------------------------------------------------------------------------------------------
def test_table_has_every_family_and_the_expected_size():
    names = ["identity", "identity_wide", "area2", "down_1p5", "down_5p3", "up_3p7", "up_from_2x2", "x2_only_in_x",
             "identity_only_in_y", "exact_fit"]
    for out in fs.OUTS:
        g = fs.geoms(*out)
        assert list(dict.fromkeys(n for n, *_ in g)) == names
        assert len(g) == len(set(g)) == 28                          # 9 families x 3 crops, exact_fit has one
        for name, (sw, sh), (rw, rh), (cx, cy) in g:
            assert sw % 2 == 0 and sh % 2 == 0 and 0 <= cx <= rw - out[0] and 0 <= cy <= rh - out[1]
        far = {n for n, s, r, c in g if c == (r[0] - out[0], r[1] - out[1]) and c != (0, 0)}
        odd = {n for n, s, r, c in g if c[0] % 2 and c[1] % 2 and c != (r[0] - out[0], r[1] - out[1])}
        assert far == odd == set(names) - {"exact_fit"}


@pytest.mark.parametrize("out", fs.OUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_every_mode_and_every_clamp_is_taken(out):
    g = {n: (s, r) for n, s, r, c in fs.geoms(*out)}
    assert {fs.mode(s, r) for s, r in g.values()} == set(fs.MODES)
    # exact x2 or identity on ONE axis only stays generic
    (sw, sh), (rw, rh) = g["x2_only_in_x"]
    assert sw == 2 * rw and sh != 2 * rh and sh != rh and fs.mode((sw, sh), (rw, rh)) == "generic"
    (sw, sh), (rw, rh) = g["identity_only_in_y"]
    assert sh == rh and rw < sw and sw != 2 * rw and fs.mode((sw, sh), (rw, rh)) == "generic"
    assert g["up_from_2x2"][0] == (2, 2)
    # sy = -1 at the top row (up-scaling, crop y = 0) in a family that also runs the far-corner crop
    for name in ("up_3p7", "up_from_2x2"):
        (sw, sh), (rw, rh) = g[name]
        sy, _ = fs._coord(np.arange(1), sh, rh)
        sx, _ = fs._coord(np.arange(1), sw, rw)
        assert sy[0] == -1 and sx[0] == -1, name
        last, _ = fs._coord(np.arange(rh - 1, rh), sh, rh)
        assert last[0] >= sh - 1, name                              # and the bottom clamp at the far corner
    # a scale above 2: the two taps of neighbouring outputs are not adjacent, at a crop other than (0, 0)
    (sw, sh), (rw, rh) = g["down_5p3"]
    assert sw > 2 * rw and sh > 2 * rh and any(c != (0, 0) for n, s, r, c in fs.geoms(*out) if n == "down_5p3")


def test_yuv_windows_are_varied_enough():
    x_pos = y_pos = narrow = 0
    for out in fs.OUTS:
        for name, src, rs, crop in fs.geoms(*out):
            x0, y0, w, h = window(src, "i420", rs, crop, out)
            assert window(src, "nv12", rs, crop, out) == (x0, y0, w, h)
            x_pos += x0 > 0
            y_pos += y0 > 0
            narrow += w < src[0] and w % 4 != 0
    assert x_pos >= 4 and y_pos >= 4 and narrow >= 1, (x_pos, y_pos, narrow)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_zero_copy_placement_takes_both_transfer_paths(layout):
    """by the documented rule (front_sweep.yuv_direct), with the frames where the GPU sweep's zero-copy path puts them"""
    direct = staged = direct_x0 = staged_x0 = 0
    for out in fs.OUTS:
        for name, src, rs, crop in fs.geoms(*out):
            win = window(src, layout, rs, crop, out)
            d = [fs.yuv_direct(a, src, layout, src[0], win) for a in fs.zero_copy_addresses(src)]
            direct += all(d)
            staged += not any(d)
            direct_x0 += all(d) and win[0] > 0
            staged_x0 += not any(d) and win[0] > 0
    assert direct >= 6 and staged >= 6, (direct, staged)
    assert direct_x0 >= 1 and staged_x0 >= 1, (direct_x0, staged_x0)   # the offsets x0 (and x0 / 2) on either path


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("out", fs.OUTS, ids=lambda o: f"{o[0]}x{o[1]}")
def test_window_covers_every_pixel_the_restatement_reads(out, layout):
    """test_frontend_yuv_host's property over the sweep's rows, and by brute force: bytes outside the window do not matter"""
    for k, (name, (sw, sh), rs, crop) in enumerate(fs.geoms(*out)):
        (x, y, w, h), nbytes = _capi.frontend_yuv_window((sw, sh), layout, rs, crop, out)
        assert x % 16 == 0 and ((x + w) % 16 == 0 or x + w == sw) and y % 2 == 0 and h % 2 == 0 and w % 2 == 0
        assert 0 <= x and x + w <= sw and 0 <= y and y + h <= sh and w > 0 and h > 0
        assert nbytes == w * h * 3 // 2
        xs = yuv_ref.source_span(crop[0], crop[0] + out[0] - 1, sw, rs[0])
        ys = yuv_ref.source_span(crop[1], crop[1] + out[1] - 1, sh, rs[1])
        assert xs.min() >= x and xs.max() < x + w, (name, crop)
        assert ys.min() >= y and ys.max() < y + h, (name, crop)
        assert x >= max(0, xs.min() - 17) and x + w <= min(sw, xs.max() + 18), (name, crop)
        assert y >= max(0, ys.min() - 3) and y + h <= min(sh, ys.max() + 4), (name, crop)
        # the planes the transfer rule names are exactly those bytes, and nothing else is read
        f = fs.yuv_frame("noise", sw, sh, layout, k)
        g = np.ascontiguousarray(255 - f)
        total = 0
        for off, pitch, row, rows in fs.yuv_planes((sw, sh), layout, sw, (x, y, w, h)):
            for r in range(rows):
                g.reshape(-1)[off + r * pitch:off + r * pitch + row] = f.reshape(-1)[off + r * pitch:off + r * pitch + row]
            total += row * rows
        assert total == nbytes
        assert np.array_equal(yuv_ref.operand(g, layout, rs, crop, out), yuv_ref.operand(f, layout, rs, crop, out)), (name, crop)
