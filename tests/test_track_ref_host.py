"""Known answers of tests/track_ref.py (rules Q1-Q9 and E1-E5 of DESIGN.md section 23), the pure host checks of the library
and the keyword plumbing of center="track".  No device is needed.  Values are dyadic wherever bits are compared, so every sum
and quotient below is exact and the expected value can be written down."""
import numpy as np
import pytest

import track_ref as tk
from funscript_flow_amd import _capi, pipeline


def uniform(n, w, h, d):
    f = np.empty((n, h, w, 2), np.float32)
    f[..., 0], f[..., 1] = d
    return f


def moving_rectangle(n, w, h, origin, size, d):
    """the field is d inside a rectangle that itself moves by d per pair, and 0 outside"""
    f = np.zeros((n, h, w, 2), np.float32)
    for i in range(n):
        x0, y0 = origin[0] + i * d[0], origin[1] + i * d[1]
        f[i, y0:y0 + size[1], x0:x0 + size[0]] = d
    return f


NO_CUT = [False] * 64


# ---- known answers of the restatement -------------------------------------------------------------------------------------
def test_uniform_field_steps_exactly_until_the_border_then_clamps():
    w, h, n, d = 40, 24, 24, (1.25, -0.5)
    rec, st = tk.advance(uniform(n, w, h, d), NO_CUT, tk.state((10.0, 20.0)), radius=7)
    r = rec[:, 0]
    for i in range(n):
        ex = min(10.0 + 1.25 * i, w - 1.0)
        assert r["x"][i] == ex and r["y"][i] == 20.0 - 0.5 * i
        assert (r["du"][i], r["dv"][i]) == d
    first = int(np.flatnonzero(10.0 + 1.25 * (np.arange(n) + 1) > w - 1)[0])   # the step that leaves the image
    assert list(r["status"][:first]) == [tk.OK] * first and list(r["status"][first:]) == [tk.CLAMPED] * (n - first)
    assert st["x"][0] == w - 1.0 and st["y"][0] == 20.0 - 0.5 * n and st["steps"][0] == n and st["lost_run"][0] == 0
    assert r["count"][0] == 15 * 11 and r["sw"][0] == 15.0 * 11.0   # columns 3 .. 17, rows 13 .. 23: clipped at the bottom


def test_a_track_follows_a_moving_rectangle_exactly():
    w, h, n, d = 96, 64, 12, (2, -1)
    f = moving_rectangle(n, w, h, (20, 30), (24, 20), d)
    start = (20 + 12.0, 30 + 10.0)   # the rectangle's centre, r = 7 below half of 24 x 20
    rec, st = tk.advance(f, NO_CUT, tk.state(start), radius=7)
    for i in range(n):
        assert (rec["x"][i, 0], rec["y"][i, 0]) == (start[0] + 2.0 * i, start[1] - 1.0 * i)
        assert (rec["du"][i, 0], rec["dv"][i, 0], rec["count"][i, 0], rec["status"][i, 0]) == (2.0, -1.0, 225, tk.OK)
    # a second track on the background stays where it is
    rec2, _ = tk.advance(f, NO_CUT, tk.state([start, (80.0, 8.0)]), radius=7)
    assert rec2[:, 0].tobytes() == rec[:, 0].tobytes()
    assert set(rec2["x"][:, 1]) == {80.0} and set(rec2["du"][:, 1]) == {0.0}


@pytest.mark.parametrize("corner, r, want", [((0.0, 0.0), 3, 16), ((15.0, 11.0), 3, 16), ((15.0, 0.0), 5, 36), ((0.0, 11.0), 32, 16 * 12),
                                              ((7.0, 5.0), 32, 16 * 12), ((7.0, 5.0), 1, 9)])
def test_count_is_the_clipped_area(corner, r, want):
    rec, _ = tk.advance(uniform(1, 16, 12, (0.0, 0.0)), NO_CUT, tk.state(corner), radius=r)
    assert rec["count"][0, 0] == want and rec["sw"][0, 0] == float(want)


def test_an_anchor_at_exactly_half_rounds_up():
    assert tk.window_of(4.5, 2.5, 1, 16, 16) == (4, 6, 2, 4)          # floor(x + 0.5): 5, 3
    assert tk.window_of(4.49999, 2.0, 1, 16, 16) == (3, 5, 1, 3)
    assert tk.window_of(0.0, 15.0, 2, 16, 16) == (0, 2, 13, 15)
    f = np.zeros((1, 8, 8, 2), np.float32)
    f[0, :, 6, 0] = 4.0                                                # only column 6 moves
    rec, _ = tk.advance(f, NO_CUT, tk.state((4.5, 4.0)), radius=1)     # window columns 4 .. 6
    assert rec["du"][0, 0] == np.float64(12.0) / np.float64(9.0)       # U = 3 * 4, S = 9
    rec, _ = tk.advance(f, NO_CUT, tk.state((4.25, 4.0)), radius=1)    # window columns 3 .. 5
    assert rec["du"][0, 0] == 0.0


def test_specks_are_dropped_and_an_empty_window_is_lost():
    w, h = 16, 16
    f = uniform(4, w, h, (0.5, 0.25))
    f[0, 8, 8] = (np.nan, 1.0)
    f[0, 7, 8] = (1.0, np.inf)
    f[0, 9, 9] = (-np.inf, np.nan)
    f[1] = np.nan                       # an all-NaN field: LOST
    f[2, :, :, 1] = np.inf              # one component is enough: LOST again
    rec, st = tk.advance(f, NO_CUT, tk.state((8.0, 8.0)), radius=2)
    r = rec[:, 0]
    assert (r["count"][0], r["sw"][0], r["du"][0], r["dv"][0], r["status"][0]) == (22, 22.0, 0.5, 0.25, tk.OK)
    assert list(r["status"][1:3]) == [tk.LOST, tk.LOST] and list(r["count"][1:3]) == [0, 0]
    assert (r["du"][1], r["dv"][1], r["sw"][1]) == (0.0, 0.0, 0.0) and not np.signbit(r["du"][1])
    assert r["x"][2] == r["x"][1] == 8.5 and r["status"][3] == tk.OK
    _, s1 = tk.advance(f[:2], NO_CUT, tk.state((8.0, 8.0)), radius=2)
    _, s2 = tk.advance(f[:3], NO_CUT, tk.state((8.0, 8.0)), radius=2)
    assert (s1["lost_run"][0], s2["lost_run"][0], st["lost_run"][0]) == (1, 2, 0)   # counts up, resets on the next good item


def test_a_map_weights_and_a_zero_map_loses():
    w, h = 16, 16
    f = np.zeros((2, h, w, 2), np.float32)
    f[:, :, :8, 0], f[:, :, 8:, 0] = 1.0, 3.0
    W = np.zeros((2, h, w), np.uint8)
    W[0, :, :8], W[0, :, 8:] = 1, 3                       # window columns 6 .. 10: two of weight 1, three of weight 3
    rec, st = tk.advance(f, NO_CUT, tk.state((8.0, 8.0)), radius=2, maps=W)
    assert rec["sw"][0, 0] == 5 * (2 * 1 + 3 * 3) and rec["du"][0, 0] == np.float64(5 * (2 * 1 + 3 * 9)) / np.float64(55)
    assert rec["status"][1, 0] == tk.LOST and rec["count"][1, 0] == 0 and st["lost_run"][0] == 1
    one, _ = tk.advance(f, NO_CUT, tk.state((8.0, 8.0)), radius=2, maps=W[0])   # a static map serves every item
    assert one["sw"][1, 0] > 0


def test_hold_and_home_on_a_cut_and_an_infinite_threshold():
    w, h = 32, 32
    f = uniform(5, w, h, (1.0, 2.0))
    cuts = [False, False, True, False, False]
    hold, sh = tk.advance(f, cuts, tk.state((4.0, 4.0)), radius=3, on_cut=tk.HOLD)
    home, so = tk.advance(f, cuts, tk.state((4.0, 4.0), home=(20.0, 10.0)), radius=3, on_cut=tk.HOME)
    for rec in (hold, home):
        r = rec[2, 0]
        assert (r["x"], r["y"], r["du"], r["dv"], r["sw"], r["count"], r["status"]) == (6.0, 8.0, 0.0, 0.0, 0.0, 0, tk.CUT)
    assert (hold["x"][3, 0], hold["y"][3, 0]) == (6.0, 8.0) and (home["x"][3, 0], home["y"][3, 0]) == (20.0, 10.0)
    assert sh["steps"][0] == so["steps"][0] == 5 and sh["lost_run"][0] == 0
    assert (sh["x"][0], sh["y"][0]) == (8.0, 12.0) and (so["x"][0], so["y"][0]) == (22.0, 14.0)
    mm = [np.float32(3.0), np.float32(7.0), np.float32(7.5), np.float32("nan"), np.float32("inf")]
    assert tk.mean_mag_cut(mm, 7.0) == [False, False, True, False, True]
    assert tk.mean_mag_cut(mm, float("inf")) == [False] * 5


def test_q9_splits_and_independence_of_the_other_tracks():
    rng = np.random.default_rng(5)
    n, w, h = 9, 48, 33
    f = (rng.integers(-64, 65, (n, h, w, 2)) / 16.0).astype(np.float32)
    pts = [(3.0, 4.0), (40.0, 30.0), (24.0, 16.0), (0.0, 32.0), (47.0, 0.0), (10.5, 10.5), (30.25, 2.75), (5.0, 28.0)]
    cuts = [False] * n
    cuts[4] = True
    whole, sw = tk.advance(f, cuts, tk.state(pts), radius=5, on_cut=tk.HOME)
    for k in (1, n - 1):
        a, sa = tk.advance(f[:k], cuts[:k], tk.state(pts), radius=5, on_cut=tk.HOME)
        b, sb = tk.advance(f[k:], cuts[k:], sa, radius=5, on_cut=tk.HOME)
        assert np.concatenate([a, b]).tobytes() == whole.tobytes() and sb.tobytes() == sw.tobytes()
    for t in range(8):
        alone, s1 = tk.advance(f, cuts, tk.state(pts[t]), radius=5, on_cut=tk.HOME)
        assert alone[:, 0].tobytes() == whole[:, t].tobytes() and s1[0].tobytes() == sw[t].tobytes()


def test_hostile_states_are_sanitised():
    w, h = 20, 10
    bad = [np.nan, -5.0, 1e9, np.inf, -np.inf, -0.0, 1e-320, 19.0000001]
    want_x = [0.0, 0.0, 19.0, 19.0, 0.0, 0.0, 1e-320, 19.0]
    st = tk.state([(b, b) for b in bad], home=[(b, b) for b in bad[::-1]])
    rec, out = tk.advance(uniform(1, w, h, (0.0, 0.0)), NO_CUT, st, radius=32)
    assert list(rec["x"][0]) == want_x and list(rec["y"][0]) == [min(v, 9.0) for v in want_x]
    assert list(out["home_x"]) == want_x[::-1] and (rec["count"][0] == w * h).all()
    assert tk.clamp(np.nan, 5.0) == 0.0 and tk.clamp(5.5, 5.0) == 5.0 and tk.clamp(-1e-300, 5.0) == 0.0
    st2 = tk.state((1.0, 1.0))
    st2["lost_run"], st2["steps"] = 2 ** 31 - 1, 2 ** 63 - 1            # they wrap as two's complement
    f = np.full((1, h, w, 2), np.nan, np.float32)
    _, out2 = tk.advance(f, NO_CUT, st2, radius=1)
    assert out2["lost_run"][0] == -2 ** 31 and out2["steps"][0] == -2 ** 63


# ---- ROI maps ---------------------------------------------------------------------------------------------------------------
def test_roi_known_answers():
    w, h = 33, 21
    m = tk.roi_map(w, h, (16.0, 10.0), 8.0, 4.0, soft=True)
    assert m[10, 16] == 255 and m[10, 24] == 0 and m[14, 16] == 0 and m[10, 20] == int(0.75 * 255.0 + 0.5)   # e = 1/4
    assert m[12, 16] == int(0.75 * 255.0 + 0.5) and m[12, 20] == int(0.5 * 255.0 + 0.5)                      # ax != ay
    hard = tk.roi_map(w, h, (16.0, 10.0), 8.0, 4.0, soft=False)
    assert hard[10, 24] == 255 and hard[10, 8] == 255 and hard[14, 16] == 255 and hard[6, 16] == 255   # e == 1 exactly is inside
    assert hard[10, 25] == 0 and hard[14, 17] == 0 and hard[10, 16] == 255
    assert int(hard.sum()) // 255 == sum(1 for y in range(h) for x in range(w) if ((x - 16) / 8) ** 2 + ((y - 10) / 4) ** 2 <= 1.0)
    for c in ((np.nan, 10.0), (16.0, np.nan), (1e9, 10.0), (-np.inf, 3.0), (16.0, -1e300)):
        assert not tk.roi_map(w, h, c, 8.0, 4.0, True).any() and not tk.roi_map(w, h, c, 8.0, 4.0, False).any()
    sub = tk.roi_map(w, h, (16.5, 10.0), 0.5, 0.5, soft=False)         # the smallest ellipse, between two pixels: e == 1 at both
    assert int(sub.sum()) == 2 * 255 and sub[10, 16] == sub[10, 17] == 255


def test_roi_gate_and_in_place():
    w, h = 24, 16
    rng = np.random.default_rng(3)
    gate = rng.integers(0, 256, (3, h, w)).astype(np.uint8)
    cen = [(5.0, 5.0), (12.5, 8.0), (30.0, 8.0)]
    plain = tk.roi_maps(w, h, cen, 6.0, 5.0)
    gated = tk.roi_maps(w, h, cen, 6.0, 5.0, gate=gate)
    assert np.array_equal(gated, np.minimum(plain, gate))
    assert np.array_equal(tk.roi_maps(w, h, cen, 6.0, 5.0, gate=gate[0]), np.minimum(plain, gate[0][None]))
    buf = gate.copy()                                                   # gate = out: min-combined in place
    buf[:] = tk.roi_maps(w, h, cen, 6.0, 5.0, gate=buf)
    assert np.array_equal(buf, gated)


def test_window_centres_is_rule_g6():
    c = np.array([[1.0, 2.0], [3.0, 6.0], [5.0, 1.0], [7.0, 7.0]])
    got = tk.window_centres(c, 1)
    assert got[0].tolist() == [2.0, 4.0] and got[1].tolist() == [3.0, 3.0] and got[3].tolist() == [6.0, 4.0]
    assert tk.window_centres(c, 0).tobytes() == c.tobytes()             # radius 0: divisions by 1


# ---- the library's pure host checks ---------------------------------------------------------------------------------------------
def test_the_binding_names_the_new_calls():
    for name in ("ffl_track_default_params", "ffl_track_params_check", "ffl_track_advance", "ffl_roi_default_params",
                 "ffl_roi_params_check", "ffl_roi_weights", "ffl_radial_window_axes_weighted_centres"):
        assert name in _capi.SIGNATURES
    for name in ("track_advance", "roi_weights", "radial_window_axes_weighted_centres"):
        assert hasattr(_capi.Context, name)
    assert _capi.TRACK_STATE_DTYPE == tk.STATE_DTYPE and _capi.TRACK_DTYPE == tk.RECORD_DTYPE
    assert _capi.TRACK_STATE_DTYPE.itemsize == _capi.TRACK_DTYPE.itemsize == 48
    assert (_capi.FFL_MAX_TRACKS, _capi.FFL_MAX_TRACK_RADIUS) == (tk.MAX_TRACKS, tk.MAX_RADIUS) == (8, 32)
    assert (_capi.TRACK_OK, _capi.TRACK_CUT, _capi.TRACK_LOST, _capi.TRACK_CLAMPED) == (tk.OK, tk.CUT, tk.LOST, tk.CLAMPED)
    assert _capi.TRACK_ON_CUT == ("hold", "home") and _capi.CENTERS == ("variance", "track")


def test_track_params_defaults_and_check():
    assert _capi.TrackParams().as_dict() == {"radius": 12, "on_cut": "hold", "cut_threshold": 7.0}
    for kw in ({}, {"radius": 1}, {"radius": 32}, {"on_cut": "home"}, {"on_cut": 1}, {"cut_threshold": float("inf")},
               {"cut_threshold": -1.0}, {"radius": 7, "on_cut": "hold", "cut_threshold": 0.0}):
        assert isinstance(_capi.track_choice(kw), _capi.TrackParams)
    given = _capi.TrackParams(radius=3)
    assert _capi.track_choice(given) is given and _capi.track_choice(None).as_dict() == _capi.TrackParams().as_dict()
    bad = [({"radius": 0}, r"radius = 0 outside 1\.\.32"), ({"radius": 33}, r"radius = 33 outside 1\.\.32"),
           ({"radius": -4}, r"radius = -4 outside 1\.\.32"), ({"on_cut": 2}, r"on_cut = 2 is neither"),
           ({"on_cut": -1}, r"on_cut = -1 is neither"), ({"cut_threshold": float("nan")}, r"cut_threshold is NaN")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_track_params_check: " + match):
            _capi.track_choice(kw)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.track_params_check(None)
    with pytest.raises(ValueError, match="on_cut must be one of"):
        _capi.TrackParams(on_cut="stay")
    with pytest.raises(ValueError, match="unknown track parameter 'size'"):
        _capi.TrackParams(size=3)


def test_roi_params_defaults_and_check():
    assert _capi.RoiParams().as_dict() == {"ax": 48.0, "ay": 48.0, "soft": 1}
    for kw in ({}, {"ax": 0.5}, {"ay": 32768.0}, {"soft": 0}, {"ax": 10.0, "ay": 3.5, "soft": 0}):
        assert isinstance(_capi.roi_choice(kw), _capi.RoiParams)
    bad = [({"ax": 0.25}, r"half-axes \(0\.25, 48\) outside 0\.5\.\.32768"), ({"ay": 32769.0}, r"half-axes \(48, 32769\) outside"),
           ({"ax": float("nan")}, r"half-axes \(nan, 48\) outside"), ({"ay": float("inf")}, r"half-axes \(48, inf\) outside"),
           ({"ax": -3.0}, r"half-axes \(-3, 48\) outside"), ({"soft": 2}, r"soft = 2 is neither"), ({"soft": -1}, r"soft = -1 is neither")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_roi_params_check: " + match):
            _capi.roi_choice(kw)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.roi_params_check(None)
    with pytest.raises(ValueError, match="unknown ROI parameter 'radius'"):
        _capi.RoiParams(radius=3)


# ---- keywords ---------------------------------------------------------------------------------------------------------------------
def test_center_kwargs_and_the_new_refusals():
    ck = pipeline.center_kwargs
    assert ck({"hip_center": "variance"}) == {"center": "variance", "cells": 32}                 # unchanged
    trk = {"start": (10, 20), "radius": 12, "roi": (48, 48)}
    assert ck({"hip_center": "track", "hip_track": trk}) == {"center": "track", "track": trk}
    with pytest.raises(ValueError, match="hip_center = 'track' needs hip_track"):
        ck({"hip_center": "track"})
    with pytest.raises(ValueError, match="hip_track needs hip_center = 'track'"):
        ck({"hip_track": trk})
    with pytest.raises(ValueError, match="hip_track needs hip_center = 'track'"):
        ck({"hip_center": "variance", "hip_track": trk})
    with pytest.raises(ValueError, match="hip_track: unknown key 'size'"):
        ck({"hip_center": "track", "hip_track": {"start": (1, 2), "size": 3}})
    with pytest.raises(ValueError, match="hip_center together with hip_weights"):
        ck({"hip_center": "track", "hip_track": trk, "hip_weights": "texture"})
    with pytest.raises(ValueError, match="center must be None or one of"):
        ck({"hip_center": "tracker"})
    for fn, args in ((pipeline.process_chunk_sharded, (None, [], 0, 1, None)), (pipeline.process_chunk_sharded_halo, (None, [], 0, 1, None)),
                     (pipeline.process_chunk_local_ranks, ([], []))):
        with pytest.raises(ValueError, match="the sharded schedules take their centres from the .div. argmax; center= needs"):
            fn(*args, center="track")
    ct = pipeline._chunk_track
    assert ct(None, 4, None, None, None, None, None, None, 8, 7.0) is None and ct(None, 4, "variance", None, None, None, None, None, 8, 7.0) is None
    with pytest.raises(ValueError, match="track= and track_out= need center='track'"):
        ct(None, 4, "variance", {"start": (1, 2)}, None, None, None, None, 8, 7.0)
    for weights in ("texture", "residual", "consistency", np.ones((4, 4), np.uint8)):
        with pytest.raises(ValueError, match=r"center='track' together with weights= .* is not supported.*track=\{'roi': \(ax, ay\)\}"):
            ct(None, 4, "track", {"start": (1, 2)}, None, weights, None, None, 8, 7.0)
    for track, match in ((None, "needs track="), ({}, "needs track="), ({"start": (1, 2), "state": object()}, "one of the two"),
                         ({"start": (1, 2), "size": 3}, "unknown key 'size'"), ({"start": (1, 2), "radius": 33}, r"radius = 33 outside 1\.\.32"),
                         ({"start": (1, 2), "on_cut": "stay"}, "on_cut must be one of")):
        with pytest.raises(ValueError, match=match):
            ct(None, 4, "track", track, None, None, None, None, 8, 7.0)


def test_track_state_array_and_centre_spans():
    st = pipeline.track_state_array((3.5, 4.0))
    assert st.dtype == _capi.TRACK_STATE_DTYPE and st.tobytes() == tk.state((3.5, 4.0)).tobytes()
    st = pipeline.track_state_array([(1, 2), (3, 4)], home=[(5, 6), (7, 8)])
    assert st.tobytes() == tk.state([(1, 2), (3, 4)], home=[(5, 6), (7, 8)]).tobytes()
    for pts, hm in (([], None), ([(0, 0)] * 9, None), ([(1, 2)], [(1, 2), (3, 4)])):
        with pytest.raises(ValueError, match="track: "):
            pipeline.track_state_array(pts, hm)
    assert _capi._centre_entries((4096, 48 * 3), 5) == (4096, 144)      # an explicit (pointer, stride) span
    assert _capi._centre_entries((np.int64(8192), np.int64(16)), 1) == (8192, 16)
