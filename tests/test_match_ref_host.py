"""The template-matching rules N1-N10 on their numpy restatement tests/match_ref.py, the binding's
parameter check and the pipeline's keywords: what can be held without a device.  The GPU tests compare the kernels with this
restatement on bytes, so what is asserted here about it is asserted about them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import match_ref as mr   # noqa: E402
import track_ref as tk   # noqa: E402

from funscript_flow_amd import _capi, pipeline   # noqa: E402

D = mr.DEFAULTS


def textured(h, w, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (h, w), dtype=np.uint8)


def one(I, Tm, c, **kw):
    """the record of one (item, track) and the centre after a write-back"""
    rec, cen = mr.match([I], np.asarray(Tm)[None], np.array([[c]], np.float64), **{**D, **kw})
    return rec[0, 0], cen[0, 0]


def brute_surface(I, Tm, ix, iy, p, s, mode):
    """rules N2 and N3 once more, candidate by candidate with explicit clamped indices and Python integers"""
    h, w = I.shape
    N, out = (2 * p + 1) ** 2, np.zeros((2 * s + 1, 2 * s + 1), object)
    t = Tm.astype(np.int64)
    for dy in range(-s, s + 1):
        ys = np.clip(iy + dy + np.arange(2 * p + 1) - p, 0, h - 1)
        for dx in range(-s, s + 1):
            xs = np.clip(ix + dx + np.arange(2 * p + 1) - p, 0, w - 1)
            d = I[ys][:, xs].astype(np.int64) - t
            S1, S2 = int(d.sum()), int((d * d).sum())
            out[dy + s, dx + s] = N * S2 if mode == mr.SSD else N * S2 - S1 * S1
    return out


# ---- verdicts ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [mr.SSD, mr.ZSSD])
def test_a_pasted_square_is_found_exactly(mode):
    I = textured(96, 120, 1)
    Tm = mr.template(I, [(63, 41)], 8)[0]
    rec, cen = one(I, Tm, (60.2, 44.4), mode=mode)                 # anchor (60, 44): the square is at (+3, -3)
    assert (rec["dx"], rec["dy"], rec["cost"], rec["status"]) == (3, -3, 0, 0) and rec["second"] > 0
    assert (rec["x"], rec["y"]) == (63.0, 41.0) and tuple(cen) == (63.0, 41.0) and rec["pad"] == 0


def test_brightness_offset_zssd_exact_ssd_poor():
    I = textured(96, 120, 2, 0, 200)
    Tm = mr.template(I, [(63, 41)], 8)[0]
    J = (I + 20).astype(np.uint8)
    rec, _ = one(J, Tm, (60, 44), mode=mr.ZSSD, max_mse=100.0)
    assert (rec["dx"], rec["dy"], rec["cost"], rec["status"]) == (3, -3, 0, 0)
    rec, cen = one(J, Tm, (60, 44), mode=mr.SSD, max_mse=100.0)
    N = 17 * 17
    assert (rec["dx"], rec["dy"], rec["cost"]) == (3, -3, N * N * 400) and rec["status"] == mr.POOR
    assert tuple(cen) == (60.0, 44.0) and (rec["x"], rec["y"]) == (60.0, 44.0)   # rejected: the centre stays
    rec, _ = one(J, Tm, (60, 44), mode=mr.SSD, max_mse=400.0)                    # the bound is strict: mse == max_mse passes
    assert rec["status"] == 0


def test_a_flat_template_is_flat_and_an_all_equal_surface_gives_zero():
    I = textured(64, 64, 3)
    rec, cen = one(I, np.full((17, 17), 90, np.uint8), (30, 30))
    assert rec["status"] & mr.FLAT
    flat = np.full((64, 64), 77, np.uint8)
    rec, cen = one(flat, mr.template(I, [(30, 30)], 8)[0], (20.4, 25.6), mode=mr.SSD, max_mse=65025.0, ratio=1.0)
    assert (rec["dx"], rec["dy"]) == (0, 0) and rec["cost"] == rec["second"]    # N4: every cost ties, the smallest move wins
    assert rec["status"] == 0 and (rec["x"], rec["y"]) == (20.0, 26.0)           # an accepted match rounds the centre


def test_stripes_tie_order_and_ambiguity():
    q, s = 4, 8
    x = np.arange(160)
    stripes = np.tile(((x % q) * 60).astype(np.uint8), (120, 1))                 # vertical stripes of period 4 <= s
    Tm = mr.template(stripes, [(80, 60)], 8)[0]
    rec, _ = one(stripes, Tm, (78, 60), s=s)     # zero cost at dx = -6, -2, 2, 6 and every dy: (dist^2, dy, dx) picks (-2, 0)
    assert (rec["dx"], rec["dy"], rec["cost"], rec["second"]) == (-2, 0, 0, 0) and rec["status"] == 0   # 0 > ratio * 0 is false
    tile = np.random.default_rng(4).integers(0, 256, (q, q), dtype=np.uint8)
    both = np.tile(tile, (30, 40))                                               # period 4 in x and in y
    Tm = mr.template(both, [(80, 60)], 8)[0]
    rec, _ = one(both, Tm, (78, 58), s=s)        # zero cost at (+-2, +-2), dist^2 = 8 each: dy first, then dx
    assert (rec["dx"], rec["dy"], rec["cost"]) == (-2, -2, 0)
    noisy = np.clip(stripes.astype(np.int64) + np.random.default_rng(5).integers(-6, 7, stripes.shape), 0, 255).astype(np.uint8)
    rec, cen = one(noisy, Tm := mr.template(stripes, [(80, 60)], 8)[0], (80, 60), s=s, max_mse=65025.0)
    assert rec["cost"] > 0 and rec["second"] > 0 and rec["status"] == mr.AMBIGUOUS and tuple(cen) == (80.0, 60.0)
    assert float(rec["cost"]) > 0.8 * float(rec["second"])


def test_s_1_has_no_runner_up_at_the_centre():
    I = textured(64, 64, 6)
    Tm = mr.template(I, [(30, 30)], 4)[0]
    rec, _ = one(I, Tm, (30, 30), p=4, s=1)
    assert (rec["dx"], rec["dy"], rec["cost"], rec["second"], rec["status"]) == (0, 0, 0, -1, 0)
    rec, _ = one(I, Tm, (31, 30), p=4, s=1)      # the best at the edge: the far column exists
    assert (rec["dx"], rec["dy"], rec["cost"]) == (-1, 0, 0) and rec["second"] > 0


# ---- arithmetic and safety --------------------------------------------------------------------------------------------------------
def test_the_extremes_need_int64():
    p, N = 16, 33 * 33
    white, black = np.full((80, 80), 255, np.uint8), np.zeros((33, 33), np.uint8)
    rec, _ = one(white, black, (40, 40), p=p, s=16, mode=mr.SSD, max_mse=65025.0, ratio=1.0)
    assert rec["cost"] == N * N * 65025 == 77114513025 and rec["cost"] > 2 ** 32 and (rec["dx"], rec["dy"]) == (0, 0)
    assert rec["status"] == mr.FLAT                                   # cost == max_mse N^2 is not POOR; the template is flat
    rec, _ = one(white, black, (40, 40), p=p, s=16, mode=mr.SSD, max_mse=65024.0, ratio=1.0)
    assert rec["status"] == mr.FLAT | mr.POOR
    yy, xx = np.mgrid[0:80, 0:80]
    board = (((xx + yy) & 1) * 255).astype(np.uint8)
    Tm = mr.template(board, [(40, 41)], p)[0]                         # the inverse of the board about (40, 40)
    surf = mr.surface(board, Tm, 40, 40, p, 16, mr.ZSSD)
    assert int(surf[16, 16]) == N * N * 65025 - 255 ** 2 and int(surf[16, 17]) == 0   # S1 = +-255: 545 against 544 squares
    assert (surf == brute_surface(board, Tm, 40, 40, p, 16, mr.ZSSD)).all() and surf.min() >= 0
    rec, _ = one(board, Tm, (40, 40), p=p, s=16, mode=mr.ZSSD)
    assert (rec["dx"], rec["dy"], rec["cost"]) == (0, -1, 0)          # four neighbours tie at dist^2 = 1: dy = -1 first


@pytest.mark.parametrize("corner", [(0, 0), (15, 0), (0, 15), (15, 15)])
def test_corners_of_a_small_frame_use_clamped_samples(corner):
    I = textured(16, 16, 7)
    Tm = textured(33, 33, 8)
    for mode in (mr.SSD, mr.ZSSD):
        surf = mr.surface(I, Tm, corner[0], corner[1], 16, 16, mode)
        assert (surf == brute_surface(I, Tm, corner[0], corner[1], 16, 16, mode)).all()
    cap = mr.template(I, [corner], 16)[0]
    ys, xs = np.clip(corner[1] + np.arange(-16, 17), 0, 15), np.clip(corner[0] + np.arange(-16, 17), 0, 15)
    assert np.array_equal(cap, I[ys][:, xs])
    rec, _ = one(I, cap, corner, p=16, s=16)
    assert (rec["dx"], rec["dy"], rec["cost"]) == (0, 0, 0)


def test_hostile_centres_are_safe_and_write_back_stores_only_on_acceptance():
    I = textured(40, 50, 9)
    Tm = mr.template(I, [(25, 20)], 4)[0]
    nan, inf = float("nan"), float("inf")
    hostile = [(nan, nan), (-5.0, -5.0), (1e9, 1e9), (inf, -inf), (-inf, inf), (nan, 1e300)]
    tame = [(0, 0), (0, 0), (49, 39), (49, 0), (0, 39), (0, 39)]
    for bad, good in zip(hostile, tame):
        a, ca = one(I, Tm, bad, p=4, s=5)
        b, _ = one(I, Tm, good, p=4, s=5)
        assert a.tobytes() == b.tobytes() and (a["x"], a["y"]) == (float(good[0]), float(good[1]))
        assert a["status"] != 0                                       # rejected here, so N8 stores nothing:
        assert np.array(ca).tobytes() == np.array(bad, np.float64).tobytes()   # not even the sanitised value
    rec, cen = mr.match([I], Tm[None], np.array([[(nan, 20.0)]]), **{**D, "p": 4, "s": 5}, write_back=False)
    assert np.isnan(cen[0, 0, 0])
    near = (23.3, 21.9)
    rec, cen = mr.match([I], Tm[None], np.array([[near]]), **{**D, "p": 4, "s": 5}, write_back=False)
    assert rec[0, 0]["status"] == 0 and (rec[0, 0]["x"], rec[0, 0]["y"]) == (25.0, 20.0) and tuple(cen[0, 0]) == near
    rec, cen = mr.match([I], Tm[None], np.array([[near]]), **{**D, "p": 4, "s": 5}, write_back=True)
    assert tuple(cen[0, 0]) == (25.0, 20.0)


def test_independence_of_the_other_tracks_and_items():
    rng = np.random.default_rng(10)
    frames = [textured(48, 64, 11 + i) for i in range(3)]
    cen = rng.uniform(-4, 70, (3, 8, 2))
    Tm = np.stack([mr.template(frames[t % 3], [cen[t % 3, t]], 4)[0] for t in range(8)])
    rec8, cen8 = mr.match(frames, Tm, cen, **{**D, "p": 4, "s": 5})
    for t in (0, 3, 7):
        rec1, cen1 = mr.match(frames, Tm[t:t + 1], cen[:, t:t + 1], **{**D, "p": 4, "s": 5})
        assert rec1.tobytes() == rec8[:, t:t + 1].tobytes() and cen1.tobytes() == cen8[:, t:t + 1].tobytes()
    rec, _ = mr.match(frames[1:2], Tm, cen[1:2], **{**D, "p": 4, "s": 5})
    assert rec.tobytes() == rec8[1:2].tobytes()


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def test_params_check_and_defaults():
    assert _capi.MatchParams().as_dict() == {**D, "mode": "zssd"}
    assert _capi.MATCH_DTYPE == mr.RECORD_DTYPE and _capi.MATCH_DTYPE.itemsize == 48 == _capi.TRACK_DTYPE.itemsize
    assert (_capi.MATCH_FLAT, _capi.MATCH_POOR, _capi.MATCH_AMBIGUOUS) == (mr.FLAT, mr.POOR, mr.AMBIGUOUS)
    assert (_capi.FFL_MAX_MATCH_P, _capi.FFL_MAX_MATCH_S, _capi.MATCH_MODES.index("zssd")) == (mr.MAX_P, mr.MAX_S, mr.ZSSD)
    good = [{}, {"p": 1, "s": 1}, {"p": 16, "s": 16, "mode": "ssd"}, {"min_var": 0.0, "max_mse": 0.0, "ratio": 1.0},
            {"max_mse": 65025.0, "ratio": 1e-9, "min_var": 1e300}]
    for kw in good:
        prm = _capi.match_choice(kw)
        assert mr.params_ok(prm.p, prm.s, prm.mode, prm.min_var, prm.max_mse, prm.ratio)
    nan, inf = float("nan"), float("inf")
    bad = [({"p": 0}, r"p = 0 outside 1\.\.16"), ({"p": 17}, r"p = 17 outside 1\.\.16"), ({"s": 0}, r"s = 0 outside 1\.\.16"),
           ({"s": 17}, r"s = 17 outside 1\.\.16"), ({"mode": 2}, "mode = 2 is neither"), ({"mode": -1}, "mode = -1 is neither"),
           ({"min_var": -1.0}, "min_var = -1 outside"), ({"min_var": nan}, "min_var = nan outside"), ({"min_var": inf}, "min_var = inf outside"),
           ({"max_mse": -0.5}, "max_mse = -0.5 outside"), ({"max_mse": 65026.0}, "max_mse = 65026 outside"), ({"max_mse": nan}, "max_mse = nan"),
           ({"ratio": 0.0}, "ratio = 0 outside"), ({"ratio": 1.5}, "ratio = 1.5 outside"), ({"ratio": nan}, "ratio = nan outside"),
           ({"ratio": -inf}, "ratio = -inf outside")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_match_params_check: " + match):
            _capi.match_choice(kw)
        prm = _capi.MatchParams(**kw)
        assert not mr.params_ok(prm.p, prm.s, prm.mode, prm.min_var, prm.max_mse, prm.ratio)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.match_params_check(None)
    with pytest.raises(ValueError, match="unknown match parameter 'radius'"):
        _capi.MatchParams(radius=3)
    with pytest.raises(ValueError, match="mode must be one of"):
        _capi.MatchParams(mode="ncc")


# ---- keywords ---------------------------------------------------------------------------------------------------------------------
def test_the_pipelines_keywords_and_refusals():
    trk = {"start": (10, 20), "radius": 7, "match": {"p": 8, "s": 12, "mode": "zssd"}}
    assert pipeline.center_kwargs({"hip_center": "track", "hip_track": trk}) == {"center": "track", "track": trk}
    ct = pipeline._chunk_track
    with pytest.raises(ValueError, match="process_flows: track.'match'. needs the frames"):
        ct(None, 4, "track", trk, None, None, None, None, 8, 7.0, frames=False)
    with pytest.raises(ValueError, match="match_out= needs center='track'"):
        ct(None, 4, None, None, None, None, None, None, 8, 7.0, match_out=object())
    with pytest.raises(ValueError, match="match_out= needs track.'match'."):
        ct(None, 4, "track", {"start": (1, 2)}, None, None, None, None, 8, 7.0, match_out=object())
    for m, match in (({"radius": 3}, "unknown key 'radius'"), ("zssd", "unknown key 'match'"), ({"p": 17}, r"p = 17 outside 1\.\.16"),
                     ({"ratio": 2.0}, "ratio = 2 outside"), ({"mode": "ncc"}, "mode must be one of")):
        with pytest.raises(ValueError, match=match):
            ct(None, 4, "track", {"start": (1, 2), "match": m}, None, None, None, None, 8, 7.0)
    params = {"hip_center": "track", "hip_track": trk}
    for fn in (pipeline.flows_to_actions, pipeline.flows_to_scripts):
        with pytest.raises(ValueError, match=fn.__name__ + ": hip_track.'match'. needs the frames"):
            fn(None, [], 30.0, 1, params)
    for fn, args in ((pipeline.process_chunk_sharded, (None, [], 0, 1, None)), (pipeline.process_chunk_sharded_halo, (None, [], 0, 1, None)),
                     (pipeline.process_chunk_local_ranks, ([], []))):
        with pytest.raises(ValueError, match="the sharded schedules take their centres from the .div. argmax; center= needs"):
            fn(*args, center="track")   # they take no track= at all, so the key cannot reach them


# ---- the drift scene --------------------------------------------------------------------------------------------------------------
def test_the_drift_scene_on_the_restatement():
    d = mr.DRIFT
    frames, flows, true = mr.drift_scene()
    n, k = d["n"], d["split"]
    st0 = tk.state(true[0])
    rec, _ = tk.advance(flows, [False] * n, st0, d["radius"])
    off = np.hypot(rec["x"][-1, 0] - true[n - 1, 0], rec["y"][-1, 0] - true[n - 1, 1])
    assert off > 9.0, off                                             # pure advection: 0.3 px per frame
    prm = {**D, "p": d["p"], "s": d["s"]}
    Tm = mr.template(frames[0], true[:1], d["p"])
    ra, ma, sa, st = mr.corrected_batch(tk, frames[:k + 1], flows[:k], st0, Tm, d["radius"], prm)
    rb, mb, sb, st = mr.corrected_batch(tk, frames[k:], flows[k:], st, Tm, d["radius"], prm)
    rec, mrec = np.concatenate([ra, rb]), np.concatenate([ma, mb])
    assert (mrec["status"] == 0).all() and (mrec["cost"] == 0).all() and (sa["status"] == 0).all() and (sb["status"] == 0).all()
    assert np.array_equal(rec["x"][:, 0], true[:n, 0]) and np.array_equal(rec["y"][:, 0], true[:n, 1])   # every item, exactly
    assert (st["x"][0], st["y"][0]) == tuple(true[n])
    assert np.abs(mrec["dx"]).max() >= 4                              # the correction was needed: the advected heads were off
