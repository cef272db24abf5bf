"""The re-detection rules L1-L9 on the restatement tests/redetect_ref.py alone, the
binding's statement of ffl_redetect_params, the pipeline's key and refusals, and the lost-and-found scene on the
restatements.  Nothing here needs a GPU; the kernels are held to the same restatement on bytes in
tests/test_gpu_track_redetect.py."""
import numpy as np
import pytest

import match_ref as mr
import redetect_ref as rr
import track_ref as tk
from funscript_flow_amd import _capi, pipeline

D = rr.DEFAULTS
LOOSE = {"min_var": 0.0, "max_mse": 65025.0, "ratio": 1.0}


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def one(I, Tm, cx, cy, word=None, strict=False, **over):
    k = {**D, **over}
    return rr.redetect_one(I, Tm, cx, cy, k["p"], k["mode"], k["exclude"], k["reach"], k["min_var"], k["max_mse"], k["ratio"], word,
                           k["trigger_mask"], strict)


# ---- the rules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [rr.SSD, rr.ZSSD])
@pytest.mark.parametrize("at", [(8, 8), (150, 20), (191, 99), (70, 63), (0, 0)])
def test_a_pasted_square_is_found_anywhere(at, mode):
    w, h, p = 200, 108, 8
    I, sq = noise(w, h, 1), noise(17, 17, 2)
    x, y = at
    if at == (0, 0):                                                  # a corner: the template is what N10 would capture there
        Tm = mr.template(I, [(0, 0)], p)[0]
    else:
        I[y - p:y + p + 1, x - p:x + p + 1] = sq
        Tm = sq
    rec, ok = one(I, Tm, 100.3, 50.7, mode=mode)
    assert ok and rec[:2] == (float(x), float(y)) and rec[2:5] == (x - 100, y - 51, 0) and rec[5] > 0 and rec[6:] == (0, 0)


def test_brightness_offset_zssd_exact_ssd_poor():
    w, h, p = 120, 60, 4
    I, sq = noise(w, h, 3), np.random.default_rng(4).integers(0, 200, (9, 9), dtype=np.uint8)
    I[30:39, 70:79] = sq + 20
    N = 81
    rec, ok = one(I, sq, 5.0, 5.0, p=p, exclude=4, mode=rr.ZSSD)
    assert ok and rec[:2] == (74.0, 34.0) and rec[4] == 0
    rec, ok = one(I, sq, 5.0, 5.0, p=p, exclude=4, mode=rr.SSD, max_mse=100.0)
    assert not ok and rec[4] == N * N * 400 and rec[6] & rr.POOR and rec[2:4] == (69, 29) and rec[:2] == (5.0, 5.0)


def test_two_exact_copies_are_ambiguous_through_the_greater_or_equal():
    w, h, p = 160, 40, 4
    I, sq = noise(w, h, 5), noise(9, 9, 6)
    I[10:19, 20:29] = sq
    I[20:29, 120:129] = sq
    rec, ok = one(I, sq, 80.0, 20.0, p=p, exclude=4)
    assert not ok and rec[2:7] == (24 - 80, 14 - 20, 0, 0, rr.AMBIGUOUS)      # the first in row-major order is the best
    strict, ok = one(I, sq, 80.0, 20.0, p=p, exclude=4, strict=True)
    assert ok and strict[6] == 0 and strict[:2] == (24.0, 14.0)              # N6's > would have accepted it silently


def test_copies_at_exactly_exclude_and_one_beyond():
    w, h, p, e = 160, 60, 2, 7
    sq = noise(5, 5, 7)
    for gap, zero in ((e, False), (e + 1, True)):
        for dx, dy in ((gap, 0), (0, gap), (gap, gap), (-gap, gap)):
            I = noise(w, h, 8)
            I[18:23, 58:63] = sq                                      # about (60, 20)
            I[18 + dy:23 + dy, 58 + dx:63 + dx] = sq
            rec, _ = one(I, sq, 1.0, 1.0, p=p, exclude=e, **LOOSE)
            assert rec[4] == 0 and (rec[5] == 0) == zero and (zero or rec[5] > 0), (gap, dx, dy, rec)


def test_reach_1_with_exclude_2_has_no_runner_up():
    I = noise(40, 30, 9)
    Tm = mr.template(I, [(20, 15)], 3)[0]
    rec, ok = one(I, Tm, 20.0, 15.0, p=3, exclude=2, reach=1)
    assert ok and rec[4:7] == (0, -1, 0)                              # nine candidates, all inside the square: the test is skipped
    rec, ok = one(I, Tm, 0.0, 0.0, p=3, exclude=2, reach=1, **LOOSE)   # at a corner the window is 2 x 2
    assert rec[5] == -1 and ok
    assert rr.window(40, 30, 0, 0, 1) == (0, 1, 0, 1) and rr.window(40, 30, 39, 29, 5) == (34, 39, 24, 29)
    assert rr.window(40, 30, 7, 8, 0) == (0, 39, 0, 29)


def test_a_flat_template_is_flat_and_an_all_equal_surface_gives_the_first_candidate():
    I = noise(50, 40, 10)
    rec, ok = one(I, np.full((17, 17), 77, np.uint8), 25.0, 20.0)
    assert not ok and rec[6] & rr.FLAT
    flat = np.full((40, 50), 131, np.uint8)
    Tm = noise(9, 9, 11)
    rec, _ = one(flat, Tm, 25.0, 20.0, p=4, exclude=4, reach=6, **LOOSE)
    assert rec[2:4] == (-6, -6) and rec[4] == rec[5]                  # candidate (0, 0) of the reach window, row-major
    rec, _ = one(flat, Tm, 2.0, 3.0, p=4, exclude=4, reach=6, **LOOSE)
    assert rec[2:4] == (-2, -3)                                       # ... of the window clipped to the frame
    rec, _ = one(flat, Tm, 25.0, 20.0, p=4, exclude=4, reach=0, **LOOSE)
    assert rec[2:4] == (-25, -20)


def test_the_saturated_extremes_at_p_16_against_python_integers():
    w, h, p = 20, 18, 16
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((xx + yy) & 1) * 255).astype(np.uint8)
    white = np.full((h, w), 255, np.uint8)
    for I, Tm in ((white, np.zeros((33, 33), np.uint8)), (board, mr.template(board, [(9, 9)], p)[0]), (board, np.zeros((33, 33), np.uint8))):
        for mode in (rr.SSD, rr.ZSSD):
            got = rr.surface(I, Tm, p, mode)
            for cy in range(h):
                for cx in range(0, w, 3):
                    s1 = s2 = 0
                    for j in range(33):
                        row = I[min(max(cy + j - p, 0), h - 1)]
                        for i in range(33):
                            d = int(row[min(max(cx + i - p, 0), w - 1)]) - int(Tm[j, i])
                            s1 += d
                            s2 += d * d
                    assert int(got[cy, cx]) == (1089 * s2 if mode == rr.SSD else 1089 * s2 - s1 * s1)
    assert int(rr.surface(white, np.zeros((33, 33), np.uint8), p, rr.SSD).max()) == 1089 * 1089 * 65025 == 77114513025 < 2 ** 37


def test_hostile_centres_and_the_write_back():
    w, h, p = 90, 50, 4
    I = noise(w, h, 12)
    Tm = np.stack([mr.template(I, [(60, 30)], p)[0], np.full((9, 9), 3, np.uint8)])
    hostile = [(np.nan, 3.0), (-5.0, 57.0), (1e9, -1e9), (np.inf, -np.inf), (-np.inf, np.nan)]
    sane = [(0.0, 3.0), (0.0, 49.0), (89.0, 0.0), (89.0, 0.0), (0.0, 0.0)]
    cen = np.array([[c, c] for c in hostile])
    ref = np.array([[c, c] for c in sane])
    frames = [I] * len(hostile)
    for reach in (0, 7):
        got, after = rr.redetect(frames, Tm, cen, p=p, exclude=4, reach=reach)
        want, wafter = rr.redetect(frames, Tm, ref, p=p, exclude=4, reach=reach)
        assert got.tobytes() == want.tobytes()
        ok = got["status"] == 0
        assert after[ok].tobytes() == wafter[ok].tobytes() and after[~ok].tobytes() == cen[~ok].tobytes()   # rejected: the bits stand
        assert (~ok[:, 1]).all() and (ok[:, 0].all() if reach == 0 else not ok[:, 0].any())
        _, kept = rr.redetect(frames, Tm, cen, p=p, exclude=4, reach=reach, write_back=False)
        assert kept.tobytes() == cen.tobytes()
    trig = np.zeros((len(hostile), 2), np.int32)
    got, after = rr.redetect(frames, Tm, cen, p=p, exclude=4, trigger=trig)
    assert after.tobytes() == cen.tobytes() and (got["status"] == rr.SKIPPED).all() and (got["cost"] == -1).all()
    assert (got["second"] == -1).all() and not got["dx"].any() and not got["dy"].any() and not got["pad"].any()
    assert got["x"].tobytes() == ref[..., 0].tobytes() and got["y"].tobytes() == ref[..., 1].tobytes()   # L7: the sanitised centre


def test_trigger_words_against_masks():
    I = noise(60, 40, 13)
    Tm = mr.template(I, [(40, 20)], 4)[0]
    for mask in (2, 4):
        for word in (0, 2, 6, -1):
            rec, ok = one(I, Tm, 3.0, 3.0, word=word, p=4, exclude=4, trigger_mask=mask)
            if word & mask:
                assert ok and rec[:2] == (40.0, 20.0) and rec[6] == 0
            else:
                assert not ok and rec == (3.0, 3.0, 0, 0, -1, -1, rr.SKIPPED, 0)
    assert [bool(w_ & m) for m in (2, 4) for w_ in (0, 2, 6, -1)] == [False, True, True, True, False, False, True, True]


def test_independence_of_the_other_tracks_and_items():
    w, h, p, n = 70, 40, 4, 3
    frames = [noise(w, h, 20 + k) for k in range(n)]
    Tm = np.stack([mr.template(frames[k % n], [(10 + 6 * k, 8 + 3 * k)], p)[0] for k in range(8)])
    cen = np.random.default_rng(14).uniform(0, 40, (n, 8, 2))
    trig = np.random.default_rng(15).integers(0, 8, (n, 8)).astype(np.int32)
    all8, _ = rr.redetect(frames, Tm, cen, p=p, exclude=4, reach=20, trigger=trig, trigger_mask=3)
    for t in (0, 5, 7):
        alone, _ = rr.redetect(frames, Tm[t:t + 1], cen[:, t:t + 1], p=p, exclude=4, reach=20, trigger=trig[:, t:t + 1], trigger_mask=3)
        assert alone[:, 0].tobytes() == all8[:, t].tobytes()
    item, _ = rr.redetect(frames[1:2], Tm, cen[1:2], p=p, exclude=4, reach=20, trigger=trig[1:2], trigger_mask=3)
    assert item[0].tobytes() == all8[1].tobytes()
    assert (all8["status"] == rr.SKIPPED).any() and (all8["status"] != rr.SKIPPED).any()


# ---- the binding ------------------------------------------------------------------------------------------------------------------
def test_params_check_defaults_and_constants():
    assert _capi.RedetectParams().as_dict() == {**D, "mode": "zssd"}
    m = _capi.MatchParams()
    r = _capi.RedetectParams()
    assert (r.p, r.mode, r.min_var, r.max_mse, r.ratio, r.exclude, r.reach, r.trigger_mask) == (m.p, m.mode, m.min_var, m.max_mse, m.ratio,
                                                                                                m.p, 0, _capi.MATCH_POOR)
    assert (_capi.FFL_MAX_REDETECT_EXCLUDE, _capi.REDETECT_SKIPPED) == (rr.MAX_EXCLUDE, rr.SKIPPED) == (32, 8)
    assert _capi.MATCH_STATUS_OFFSET == _capi.MATCH_DTYPE.fields["status"][1] == 40
    assert rr.SKIPPED & (rr.FLAT | rr.POOR | rr.AMBIGUOUS) == 0
    good = [{}, {"p": 1, "exclude": 1}, {"p": 16, "exclude": 32, "reach": 32768, "mode": "ssd"}, {"reach": 1, "trigger_mask": -1},
            {"min_var": 0.0, "max_mse": 0.0, "ratio": 1.0}, {"max_mse": 65025.0, "ratio": 1e-9, "min_var": 1e300, "trigger_mask": 0}]
    for kw in good:
        q = _capi.redetect_choice(kw)
        assert rr.params_ok(q.p, q.mode, q.exclude, q.reach, q.min_var, q.max_mse, q.ratio)
    nan, inf = float("nan"), float("inf")
    bad = [({"p": 0}, r"p = 0 outside 1\.\.16"), ({"p": 17}, r"p = 17 outside 1\.\.16"), ({"mode": 2}, "mode = 2 is neither"),
           ({"exclude": 0}, r"exclude = 0 outside 1\.\.32 \(FFL_MAX_REDETECT_EXCLUDE; rule L5"), ({"exclude": 33}, r"exclude = 33 outside 1\.\.32"),
           ({"reach": -1}, r"reach = -1 outside 0 \(the whole frame\) or 1\.\.32768 \(rule L2\)"), ({"reach": 32769}, "reach = 32769 outside"),
           ({"min_var": -1.0}, "min_var = -1 outside"), ({"min_var": nan}, "min_var = nan outside"), ({"min_var": inf}, "min_var = inf outside"),
           ({"max_mse": -0.5}, "max_mse = -0.5 outside"), ({"max_mse": 65026.0}, "max_mse = 65026 outside"), ({"max_mse": nan}, "max_mse = nan"),
           ({"ratio": 0.0}, "ratio = 0 outside"), ({"ratio": 1.5}, "ratio = 1.5 outside"), ({"ratio": nan}, "ratio = nan outside")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_redetect_params_check: " + match):
            _capi.redetect_choice(kw)
        q = _capi.RedetectParams(**kw)
        assert not rr.params_ok(q.p, q.mode, q.exclude, q.reach, q.min_var, q.max_mse, q.ratio)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.redetect_params_check(None)
    with pytest.raises(ValueError, match="unknown redetect parameter 's'"):
        _capi.RedetectParams(s=3)
    with pytest.raises(ValueError, match="mode must be one of"):
        _capi.RedetectParams(mode="ncc")


def test_extra_bytes_needs_no_device():
    words = lambda w, h: ((w + 63) // 64) * ((h + 15) // 16) + 20   # noqa: E731  a key per 64 x 16 tile, the pick, 18 re-walked tiles
    for w, h, mb in ((16, 16, 1), (67, 35, 40), (1920, 1080, 32), (3840, 2160, 256)):
        assert _capi.redetect_extra_bytes(w, h, mb) == 8 * words(w, h) * mb * _capi.FFL_MAX_TRACKS
    for args, match in (((15, 16, 1), "unsupported frame size"), ((64, 64, 0), r"max_batch = 0 outside 1\.\.256"),
                        ((64, 64, 257), r"max_batch = 257 outside")):
        with pytest.raises(_capi.FFLError, match="ffl_redetect_extra_bytes.*" + match):
            _capi.redetect_extra_bytes(*args)


# ---- keywords ---------------------------------------------------------------------------------------------------------------------
def test_the_pipelines_key_and_refusals():
    match = {"p": 6, "s": 12, "mode": "ssd", "max_mse": 300.0}
    m = _capi.match_choice(match)
    r = pipeline._redetect_choice(m, True)
    assert r.as_dict() == {"p": 6, "mode": "ssd", "exclude": 6, "reach": 0, "trigger_mask": _capi.MATCH_POOR, "min_var": m.min_var,
                           "max_mse": 300.0, "ratio": m.ratio}
    r = pipeline._redetect_choice(m, {"reach": 70, "exclude": 9, "mask": 6})
    assert (r.reach, r.exclude, r.trigger_mask, r.p) == (70, 9, 6, 6)
    trk = {"start": (10, 20), "radius": 7, "match": {**match, "redetect": {"reach": 40}}}
    assert pipeline.center_kwargs({"hip_center": "track", "hip_track": trk}) == {"center": "track", "track": trk}
    ct = pipeline._chunk_track
    with pytest.raises(ValueError, match="process_flows: track.'match'. needs the frames"):
        ct(None, 4, "track", trk, None, None, None, None, 8, 7.0, frames=False)
    with pytest.raises(ValueError, match="redetect_out= needs center='track'"):
        ct(None, 4, None, None, None, None, None, None, 8, 7.0, redetect_out=object())
    with pytest.raises(ValueError, match="redetect_out= needs track.'match'..'redetect'."):
        ct(None, 4, "track", {"start": (1, 2), "match": {}}, None, None, None, None, 8, 7.0, redetect_out=object())
    with pytest.raises(ValueError, match="redetect_out= needs track.'match'..'redetect'."):
        ct(None, 4, "track", {"start": (1, 2)}, None, None, None, None, 8, 7.0, redetect_out=object())
    with pytest.raises(ValueError, match="'redetect' is a key of track.'match'."):                    # without track["match"]
        ct(None, 4, "track", {"start": (1, 2), "redetect": True}, None, None, None, None, 8, 7.0)
    with pytest.raises(ValueError, match="hip_track: unknown key 'redetect'"):
        pipeline.center_kwargs({"hip_center": "track", "hip_track": {"start": (1, 2), "redetect": True}})
    for rd, words in (({"s": 3}, "unknown key 's'"), ("whole", "unknown key 'redetect'"), ({"exclude": 33}, r"exclude = 33 outside 1\.\.32"),
                      ({"reach": -2}, "reach = -2 outside"), ({"exclude": 0}, "exclude = 0 outside")):
        with pytest.raises(ValueError, match=words):
            ct(None, 4, "track", {"start": (1, 2), "match": {"redetect": rd}}, None, None, None, None, 8, 7.0)
    params = {"hip_center": "track", "hip_track": trk}
    for fn in (pipeline.flows_to_actions, pipeline.flows_to_scripts):
        with pytest.raises(ValueError, match=fn.__name__ + ": hip_track.'match'. needs the frames"):
            fn(None, [], 30.0, 1, params)


# ---- the lost-and-found scene -----------------------------------------------------------------------------------------------------
def run_scene(rprm):
    d, B = mr.DRIFT, rr.JUMP["batch"]
    frames, flows, true = rr.lost_scene()
    prm = {**mr.DEFAULTS, "p": d["p"], "s": d["s"]}
    Tm = mr.template(frames[0], true[:1], d["p"])
    st, out = tk.state(true[0]), []
    for lo in range(0, d["n"], B):
        hi = min(lo + B, d["n"])
        rec, mrec, srec, rrec, st = rr.found_batch(tk, frames[lo:hi + 1], flows[lo:hi], st, Tm, d["radius"], prm, rprm)
        out.append((lo, hi, rec, mrec, srec, rrec, st))
    return true, out


def test_the_lost_and_found_scene_on_the_restatements():
    d, B, jump = mr.DRIFT, rr.JUMP["batch"], rr.JUMP["pair"]
    n = d["n"]
    assert B < jump < 2 * B - 1 and 2 * B < n                         # the jump lies inside the second batch; a third follows
    # without the key: the square is gone for the rest of the video
    true, out = run_scene(None)
    for lo, hi, rec, mrec, srec, rrec, st in out:
        if hi <= jump:
            assert (srec["status"] == 0).all() and (st["x"][0], st["y"][0]) == tuple(true[hi])
        else:
            assert (srec["status"] & rr.POOR).all() and rrec is None
            assert (mrec["status"][max(jump + 1 - lo, 0):] & rr.POOR).all()
    st = out[-1][-1]
    off = np.hypot(st["x"][0] - true[n, 0], st["y"][0] - true[n, 1])
    assert off > 60.0, off
    # with it: the state after the batch of the jump, and every later head, is the true integer centre
    true, out = run_scene({k: v for k, v in D.items() if k != "trigger_mask"} | {"trigger_mask": rr.POOR})
    for lo, hi, rec, mrec, srec, rrec, st in out:
        assert (st["x"][0], st["y"][0]) == tuple(true[hi]), (lo, hi)
        if lo <= jump < hi:                                           # the batch that loses it, and finds it again behind itself
            assert (srec["status"] == rr.POOR | rr.AMBIGUOUS).all()
            assert rrec["status"][0, 0] == 0 and rrec["cost"][0, 0] == 0 and rrec["second"][0, 0] > 10 ** 8
            assert (rrec["x"][0, 0], rrec["y"][0, 0]) == tuple(true[hi])
            heads = slice(0, jump + 1 - lo)                           # its items before the jump are still exact
        else:
            assert (srec["status"] == 0).all() and (rrec["status"] == rr.SKIPPED).all()
            heads = slice(0, hi - lo)
        assert np.array_equal(rec["x"][heads, 0], true[lo:hi][heads, 0]) and np.array_equal(rec["y"][heads, 0], true[lo:hi][heads, 1])
        assert (mrec["status"][heads] == 0).all()
