"""GPU side of the template-matching drift correction (ffl_track_template: k_track_template; ffl_track_match: k_track_match;
process_chunk with track["match"]), everything through the C ABI via _capi on frames placed with
upload_frames and fields placed with import_flows.  Records, written-back centres and templates are held on bytes against
the restatement tests/match_ref.py; the chunk schedule against a by-hand composition of the calls, batch by batch."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import chunk_by_hand as cbh
import match_ref as mr
import track_ref as tk
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
REC, STATE, ITEM = _capi.MATCH_DTYPE.itemsize, _capi.TRACK_STATE_DTYPE.itemsize, _capi.PASS2_AXES_DTYPE.itemsize
NEVER = float("inf")
SIZES = [(16, 16), (67, 35), (256, 256)]   # 16x16: every window of p + s > 8 clamps on all four sides; 67x35: odd, rows no multiple of 8
P_, S_, T_, N_ITEMS = (1, 4, 16), (1, 5, 16), (1, 3, 8), (1, 5, 33)
# an orthogonal array: every value of p, s, T, n meets every value of the other three once; and the defaults
L9 = [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 2, 2), (1, 0, 1, 2), (1, 1, 2, 0), (1, 2, 0, 1), (2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 1, 0)]
COMBOS = [(P_[a], S_[b], T_[c], N_ITEMS[d]) for a, b, c, d in L9] + [(8, 8, 2, 5)]
FSLOTS = 6
LOOSE = {"min_var": 0.0, "max_mse": 65025.0, "ratio": 1.0}     # accepts every match: the write-back always stores


def gid(v):
    return "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h, mb=40, fslots=FSLOTS, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=fslots, flow_slots=slots or mb)


@functools.lru_cache(maxsize=None)
def frames_of(w, h, p):
    """FSLOTS gray frames: noise; noise with frame 0's patch about the centre pasted at an offset; flat; vertical stripes of
    period 4; saturated blocks of 0 and 255; noise again"""
    rng = np.random.default_rng(1000 * w + h)
    f = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(FSLOTS)]
    side = min(2 * p + 1, w, h)
    y0, x0 = max(0, h // 2 - side // 2), max(0, w // 2 - side // 2)
    oy, ox = min(h - side, y0 + 2), max(0, x0 - 3)
    f[1][oy:oy + side, ox:ox + side] = f[0][y0:y0 + side, x0:x0 + side]
    f[2][:] = 131
    f[3][:] = ((np.arange(w) % 4) * 60).astype(np.uint8)[None, :]
    yy, xx = np.mgrid[0:h, 0:w]
    f[4][:] = ((((xx // 5) + (yy // 3)) & 1) * 255).astype(np.uint8)
    out = np.stack(f)
    out.setflags(write=False)
    return out


def templates_of(frames, T, p, w, h):
    """T templates of mixed content: frame 0 about the centre (what frame 1 holds at an offset), flat, the stripes, all 0,
    frame 5 about a corner, all 255, the saturated blocks, frame 0 about (0, 0)"""
    side = 2 * p + 1
    kinds = [mr.template(frames[0], [(w // 2, h // 2)], p)[0], np.full((side, side), 90, np.uint8),
             mr.template(frames[3], [(w // 2, h // 2)], p)[0], np.zeros((side, side), np.uint8),
             mr.template(frames[5], [(w - 1, h - 1)], p)[0], np.full((side, side), 255, np.uint8),
             mr.template(frames[4], [(w // 3, h // 3)], p)[0], mr.template(frames[0], [(0, 0)], p)[0]]
    return np.stack(kinds[:T])


def centres_of(n, T, w, h, seed):
    """(n, T, 2) centres: near the frame's centre, the corners, x.5 anchors, and hostile bit patterns"""
    rng = np.random.default_rng(seed)
    c = np.empty((n, T, 2))
    c[..., 0] = w // 2 + rng.integers(-3, 4, (n, T)) + rng.choice([0.0, 0.25, 0.5, -0.5], (n, T))
    c[..., 1] = h // 2 + rng.integers(-3, 4, (n, T)) + rng.choice([0.0, 0.25, 0.5, -0.5], (n, T))
    special = [(0.0, 0.0), (w - 1.0, h - 1.0), (np.nan, 3.0), (-5.0, h + 7.0), (1e9, -1e9), (np.inf, -np.inf), (w - 1.0, 0.0), (-0.0, 5e-324)]
    flat = c.reshape(-1, 2)
    for k in range(1, len(flat), 3):
        flat[k] = special[(k // 3 + seed) % len(special)]
    return c


def record_buffer(cen, fill=7.0):
    """(n, T) ffl_track_records whose heads are the centres: what a batch's track buffer holds; the other fields are sentinels"""
    n, T = cen.shape[:2]
    rec = np.zeros((n, T), _capi.TRACK_DTYPE)
    rec["x"], rec["y"], rec["du"], rec["dv"], rec["sw"], rec["count"], rec["status"] = cen[..., 0], cen[..., 1], fill, -fill, 3.0, 11, 4
    return rec


def run(ctx, fslots, tmpl, cbuf, stride, T, prm, write_back, stream=None):
    """track_match into a sentinel-filled record buffer: (records (n, T), the centre buffer's bytes afterwards)"""
    out = torch.full((len(fslots) * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ctx.track_match(fslots, tmpl, (cbuf, stride), out, prm, T, write_back, stream) is out
    return pipeline.match_records(out, T), cbuf.cpu().numpy().tobytes()


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in got.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


# ---- 1. k_track_match and k_track_template against the restatement ----------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=gid)
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_match_is_the_restatement(size, combo):
    (w, h), (p, s, T, n) = size, combo
    frames = frames_of(w, h, p)
    fslots = [(5 * i + 1) % FSLOTS for i in range(n)]               # repeated and out of order
    tm = templates_of(frames, T, p, w, h)
    cen = centres_of(n, T, w, h, seed=p + s + T + n)
    mode = ("ssd", "zssd")[(p + s + T + n + w) % 2]
    with context(w, h) as ctx:
        ctx.upload_frames(0, list(frames))
        dt = dev(tm)
        for prm in ({"p": p, "s": s, "mode": mode}, {"p": p, "s": s, "mode": mode, **LOOSE}):
            ref = {**mr.DEFAULTS, **prm, "mode": _capi.MATCH_MODES.index(mode)}
            want, wcen = mr.match([frames[k] for k in fslots], tm, cen, **ref, write_back=True)
            # track records, one every 48 * T bytes
            rec = record_buffer(cen)
            for wb in (0, 1):
                buf = dev(np.frombuffer(rec.tobytes(), np.uint8))
                got, after = run(ctx, fslots, dt, buf, 48 * T, T, prm, wb)
                same(got, want)
                exp = rec.copy()
                if wb:
                    exp["x"], exp["y"] = wcen[..., 0], wcen[..., 1]
                assert after == exp.tobytes()                           # write_back 0: not a byte of the centres changes
            if T == 1:                                                   # a plain (n, 2) array, stride 16
                for wb in (0, 1):
                    buf = dev(cen[:, 0, :])
                    out = torch.full((n * REC,), 0xA5, dtype=torch.uint8, device=DEV)
                    ctx.track_match(fslots, dt, buf, out, prm, 1, wb)
                    same(pipeline.match_records(out, 1), want)
                    assert buf.cpu().numpy().tobytes() == (wcen if wb else cen)[:, 0, :].tobytes()
            if n == 1:                                                   # a state, corrected in place
                st = tk.state(cen[0], home=cen[0][::-1])
                st["steps"], st["lost_run"], st["pad"] = 5, -2, 0x5A5A5A5A
                sd = dev(np.frombuffer(st.tobytes(), np.uint8))
                got, after = run(ctx, fslots, dt, sd, 48 * T, T, prm, 1)
                same(got, want)
                st["x"], st["y"] = wcen[0, :, 0], wcen[0, :, 1]
                assert after == st.tobytes()
        if s == 1:
            assert (want["second"][(want["dx"] == 0) & (want["dy"] == 0)] == -1).all()
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("mode", ["ssd", "zssd"])
def test_every_content_under_both_modes(mode):
    w, h, p, s = 67, 35, 4, 5
    frames = frames_of(w, h, p)
    m = _capi.MATCH_MODES.index(mode)
    with context(w, h, mb=8) as ctx:
        ctx.upload_frames(0, list(frames))
        # the pasted square: frame 0's patch about the centre sits in frame 1 at (-3, +2)
        sd = pipeline.track_state(ctx, [(w // 2, h // 2)])
        tmpl = pipeline.match_templates(ctx, 1, p)
        assert ctx.track_template(0, sd, tmpl, p) is tmpl
        assert tmpl.cpu().numpy().tobytes() == mr.template(frames[0], [(w // 2, h // 2)], p).tobytes()
        got, after = run(ctx, [1], tmpl, sd, 48, 1, {"p": p, "s": s, "mode": mode}, 1)
        assert (got["dx"][0, 0], got["dy"][0, 0], got["cost"][0, 0], got["status"][0, 0]) == (-3, 2, 0, 0)
        st = pipeline.track_state_records(sd)
        assert (st["x"][0], st["y"][0]) == (w // 2 - 3.0, h // 2 + 2.0) and (st["home_x"][0], st["home_y"][0]) == (w // 2, h // 2)
        # every frame against every template kind, T = 8, about the centre: the verdicts are the restatement's
        tm = templates_of(frames, 8, p, w, h)
        cen = np.tile(np.array([w // 2 - 1.0, h // 2 + 1.0]), (FSLOTS, 8, 1))
        prm = {"p": p, "s": s, "mode": mode}
        want, wcen = mr.match(list(frames), tm, cen, **{**mr.DEFAULTS, **prm, "mode": m})
        rec = record_buffer(cen)
        got, after = run(ctx, list(range(FSLOTS)), dev(tm), dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * 8, 8, prm, 1)
        same(got, want)
        rec["x"], rec["y"] = wcen[..., 0], wcen[..., 1]
        assert after == rec.tobytes()
        assert (got["status"][:, 1] & mr.FLAT).all() and (got["status"][:, 3] & mr.FLAT).all()       # flat templates
        assert got["status"][1, 0] == 0 and got["cost"][1, 0] == 0                                      # the pasted square
        assert (got["dx"][2] == 0).all() and (got["dy"][2] == 0).all()                                  # a flat frame: every cost ties
        assert got["cost"][3, 2] == 0 and got["second"][3, 2] == 0                                      # stripes on stripes
        assert (got["status"] == 0).any() and (got["status"] & mr.POOR).any()


def test_saturated_extremes_at_p_16():
    w, h, p, s = 67, 35, 16, 16
    white = np.full((h, w), 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((xx + yy) & 1) * 255).astype(np.uint8)
    tm = np.stack([np.zeros((33, 33), np.uint8), mr.template(board, [(30, 18)], p)[0]])
    cen = np.array([[(30.0, 17.0), (30.0, 17.0)], [(30.0, 17.0), (30.0, 17.0)]])
    with context(w, h, mb=4, fslots=2) as ctx:
        ctx.upload_frames(0, [white, board])
        for mode in ("ssd", "zssd"):
            prm = {"p": p, "s": s, "mode": mode, **LOOSE}
            want, _ = mr.match([white, board], tm, cen, **{**mr.DEFAULTS, **prm, "mode": _capi.MATCH_MODES.index(mode)})
            got, _ = run(ctx, [0, 1], dev(tm), dev(np.frombuffer(record_buffer(cen).tobytes(), np.uint8)), 96, 2, prm, 0)
            same(got, want)
        assert want["cost"].max() <= 1089 * 1089 * 65025
    with context(w, h, mb=4, fslots=2) as ctx:
        ctx.upload_frames(0, [white, board])
        got, _ = run(ctx, [0], dev(tm[:1]), dev(cen[0, :1]), 16, 1, {"p": p, "s": s, "mode": "ssd", **LOOSE}, 0)
        assert got["cost"][0, 0] == 1089 * 1089 * 65025 == 77114513025   # needs the int64 product


def test_1080p_corners_and_centre():
    w, h, n, T, p, s = 1920, 1080, 3, 8, 16, 16
    rng = np.random.default_rng(12)
    frames = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    pts = [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (w / 2.0, h / 2.0), (w - 1.5, h - 1.5), (31.5, 32.5),
           (w / 2.0 + 0.5, h / 2.0 - 0.5)]
    with context(w, h, mb=4, fslots=3) as ctx:
        ctx.upload_frames(0, list(frames))
        sd = pipeline.track_state(ctx, pts)
        tmpl = pipeline.match_templates(ctx, T, p)
        ctx.track_template(2, sd, tmpl, p)
        tm = mr.template(frames[2], pts, p)
        assert tmpl.cpu().numpy().tobytes() == tm.tobytes()
        cen = np.tile(np.array(pts), (n, 1, 1)) + np.array([3.0, -2.0])
        prm = {"p": p, "s": s, "mode": "zssd"}
        want, wcen = mr.match([frames[k] for k in (2, 0, 1)], tm, cen, **{**mr.DEFAULTS, **prm, "mode": mr.ZSSD})
        rec = record_buffer(cen)
        got, after = run(ctx, [2, 0, 1], tmpl, dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * T, T, prm, 1)
        same(got, want)
        rec["x"], rec["y"] = wcen[..., 0], wcen[..., 1]
        assert after == rec.tobytes()
        assert got["status"][0, 4] == 0 and (got["dx"][0, 4], got["dy"][0, 4], got["cost"][0, 4]) == (-3, 2, 0)   # its own frame
        assert (got["status"][1:] & mr.POOR).all()                       # other noise: nothing to find


def test_independence_and_a_map_read_straight_behind():
    w, h, p, s, n, T = 67, 35, 4, 5, 5, 3
    frames = frames_of(w, h, p)
    tm = templates_of(frames, 8, p, w, h)
    cen8 = centres_of(n, 8, w, h, seed=3)
    prm = {"p": p, "s": s, "mode": "zssd", **LOOSE}
    fslots = [1, 0, 1, 5, 3]
    with context(w, h, mb=8) as ctx:
        ctx.upload_frames(0, list(frames))
        all8, _ = run(ctx, fslots, dev(tm), dev(np.frombuffer(record_buffer(cen8).tobytes(), np.uint8)), 48 * 8, 8, prm, 1)
        for t in (0, 3, 7):                                              # N9: a track alone
            alone, _ = run(ctx, fslots, dev(tm[t:t + 1]), dev(cen8[:, t, :]), 16, 1, prm, 1)
            same(alone[:, 0], all8[:, t])
        one, _ = run(ctx, fslots[3:4], dev(tm), dev(np.frombuffer(record_buffer(cen8[3:4]).tobytes(), np.uint8)), 48 * 8, 8, prm, 1)
        same(one[0], all8[3])                                            # an item alone
        # track_match, roi_weights and the read on the caller's stream, queued back to back: the maps are about corrected centres
        cen = cen8[:, :T]
        want, wcen = mr.match([frames[k] for k in fslots], tm[:T], cen, **{**mr.DEFAULTS, **prm, "mode": mr.ZSSD})
        side = torch.cuda.Stream()
        buf = dev(np.frombuffer(record_buffer(cen).tobytes(), np.uint8))
        out = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        maps = torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV)
        dtm = dev(tm[:T])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ctx.track_match(fslots, dtm, (buf, 48 * T), out, prm, T, True, side)
            ctx.roi_weights(n, (buf, 48 * T), maps, {"ax": 9.0, "ay": 5.0}, stream=side)
            got_maps = maps.cpu().numpy()
        same(pipeline.match_records(out, T), want)
        assert np.array_equal(got_maps, tk.roi_maps(w, h, wcen[:, 0], 9.0, 5.0))
        assert not np.array_equal(got_maps, tk.roi_maps(w, h, np.nan_to_num(cen[:, 0], nan=0.0, posinf=1e9, neginf=-1e9), 9.0, 5.0))
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------------
class Span:
    """`nbytes` bytes at `ptr` as a __cuda_array_interface__ object, whatever memory that is"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": (int(nbytes),), "strides": None,
                                         "typestr": "|u1"}


def capture_refused(call):
    """[(code, "capturing" in the message)] of `call` made on a capturing stream; the graph still replays"""
    x = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    codes = []
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        try:
            call(torch.cuda.current_stream())
        except _capi.FFLError as err:
            codes.append((err.code, "capturing" in str(err)))
        x += 1
    g.replay()
    torch.cuda.synchronize()
    assert float(x.sum()) == 16.0
    return codes


def test_refusals():
    w, h, T, p = 67, 35, 2, 4
    side = 2 * p + 1
    INVALID, STATE_ = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    frames = frames_of(w, h, p)
    with _capi.Context(w, h, max_batch=4, frame_slots=4, flow_slots=4) as ctx:
        ctx.upload_frames(0, list(frames[:3]))                       # frame slot 3 is never uploaded
        tm = templates_of(frames, T, p, w, h)
        dt = dev(tm)
        cen = centres_of(4, T, w, h, seed=1)
        rec = record_buffer(cen)
        cb = dev(np.frombuffer(rec.tobytes(), np.uint8))
        out = torch.full((5 * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        keep_c, keep_t = cb.clone(), dt.clone()
        L, hd = ctx.L, ctx._h
        good = _capi.MatchParams(p=p, s=5)

        def raw(fslots, n_tracks=T, prm=None, tptr=None, cptr=None, stride=48 * T, wb=1, optr=None, null_list=False):
            ps, arr = _capi._iarr(fslots)
            q = good if prm is None else prm
            return lambda: (arr, ctx._chk(L.ffl_track_match(hd, len(fslots), None if null_list else ps, n_tracks, C.byref(q),
                                                            dt.data_ptr() if tptr is None else tptr,
                                                            cb.data_ptr() if cptr is None else cptr, stride, wb,
                                                            out.data_ptr() if optr is None else optr, _capi.stream_handle(None, 0))))

        def refused(match, code, call, fn="ffl_track_match"):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and fn in str(e.value)

        refused(r"n = 0 items outside 1\.\.4", INVALID, raw([]))
        refused(r"n = 5 items outside 1\.\.4", INVALID, raw([0, 1, 2, 0, 1]))
        refused(r"n_tracks = 0 outside 1\.\.8", INVALID, raw([0], 0))
        refused(r"n_tracks = 9 outside 1\.\.8", INVALID, raw([0], 9))
        refused(r"NULL fslots", INVALID, raw([0], null_list=True))
        refused(r"item 0: frame slot 4 out of range", INVALID, raw([4]))
        refused(r"item 1: frame slot -1 out of range", INVALID, raw([0, -1]))
        refused(r"item 1: frame slot 3 was never uploaded", STATE_, raw([0, 3]))
        nan = float("nan")
        for field, value, match in (("p", 0, r"p = 0 outside 1\.\.16"), ("p", 17, r"p = 17 outside 1\.\.16"), ("s", 0, r"s = 0 outside 1\.\.16"),
                                    ("s", 17, r"s = 17 outside 1\.\.16"), ("mode", 2, "mode = 2 is neither"), ("min_var", -1.0, "min_var = -1 outside"),
                                    ("min_var", nan, "min_var = nan outside"), ("max_mse", 65026.0, "max_mse = 65026 outside"),
                                    ("max_mse", nan, "max_mse = nan outside"), ("ratio", 0.0, "ratio = 0 outside"), ("ratio", 1.25, "ratio = 1.25 outside"),
                                    ("ratio", nan, "ratio = nan outside")):
            bad = _capi.MatchParams(p=p, s=5)
            setattr(bad, field, value)
            refused(match, INVALID, raw([0], prm=bad))
        refused(r"NULL templates_dev", INVALID, raw([0], tptr=0))
        refused(r"NULL centres_dev", INVALID, raw([0], cptr=0))
        refused(r"NULL out_dev", INVALID, raw([0], optr=0))
        refused(r"must be 8-byte aligned", INVALID, raw([0], cptr=cb.data_ptr() + 4))
        refused(r"must be 8-byte aligned", INVALID, raw([0], optr=out.data_ptr() + 4))
        refused(r"centre stride 100: a multiple of 8 bytes", INVALID, raw([0, 1], stride=100))
        refused(r"centre stride 56: a multiple of 8 bytes, at least 48 \* \(n_tracks - 1\) \+ 16 = 64", INVALID, raw([0, 1], stride=56))
        refused(r"centre stride 0:", INVALID, raw([0], stride=0))
        refused(r"centre stride -96:", INVALID, raw([0, 1], stride=-96))
        refused(r"write_back = 2 is neither 0 nor 1", INVALID, raw([0], wb=2))
        refused(r"write_back = -1 is neither 0 nor 1", INVALID, raw([0], wb=-1))
        refused(rf"overlap: centres_dev \({96 + 64} bytes\) and out_dev \({2 * T * REC} bytes\) share memory", INVALID,
                raw([0, 1], optr=cb.data_ptr() + 96))
        refused(r"overlap: centres_dev .* and out_dev", INVALID, raw([0, 1], cptr=out.data_ptr() + 48))
        refused(rf"overlap: templates_dev \({T * side * side} bytes\) and out_dev", INVALID, raw([0], optr=(dt.data_ptr() + 15) // 8 * 8))
        refused(r"overlap: templates_dev .* and centres_dev", INVALID, raw([0], cptr=(dt.data_ptr() + 15) // 8 * 8))
        pin = ctx.pinned_frames(1, channels=1)
        assert pin.size >= 2 * T * REC
        refused(r"out_dev is page-locked host memory.*device memory", INVALID, raw([0], optr=pin.ctypes.data))
        refused(r"centres_dev is page-locked host memory.*device memory", INVALID, raw([0], cptr=pin.ctypes.data))
        refused(r"templates_dev is page-locked host memory.*device memory", INVALID, raw([0], tptr=pin.ctypes.data))
        torch.cuda.empty_cache()
        big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)   # an allocation of its own
        end = big.data_ptr() + big.numel()
        refused(rf"out_dev spans {3 * T * REC} bytes, {T * REC} more than its allocation holds", INVALID, raw([0, 1, 2], optr=end - 2 * T * REC))
        refused(rf"centres_dev spans {96 + 64} bytes, 64 more than its allocation holds", INVALID, raw([0, 1], cptr=end - 96))
        refused(rf"templates_dev spans {T * side * side} bytes, {side * side} more than its allocation holds", INVALID,
                raw([0], tptr=end - side * side))
        assert capture_refused(lambda s: ctx.track_match([0], dt, (cb, 48 * T), out, good, T, True, s)) == [(STATE_, True)]
        with pytest.raises(ValueError, match="out holds"):
            ctx.track_match([0, 1], dt, (cb, 48 * T), Span(out.data_ptr(), T * REC), good, T)
        with pytest.raises(ValueError, match="not device memory"):
            ctx.track_match([0], torch.zeros(T * side * side, dtype=torch.uint8), (cb, 48 * T), out, good, T)

        # ffl_track_template
        def rawt(fslot=0, n_tracks=T, cptr=None, pp=p, tptr=None):
            return lambda: ctx._chk(L.ffl_track_template(hd, fslot, n_tracks, cb.data_ptr() if cptr is None else cptr, pp,
                                                         dt.data_ptr() if tptr is None else tptr, _capi.stream_handle(None, 0)))

        tfn = "ffl_track_template"
        refused(r"frame slot 4 out of range", INVALID, rawt(4), tfn)
        refused(r"frame slot -1 out of range", INVALID, rawt(-1), tfn)
        refused(r"frame slot 3 was never uploaded", STATE_, rawt(3), tfn)
        refused(r"n_tracks = 0 outside 1\.\.8", INVALID, rawt(n_tracks=0), tfn)
        refused(r"n_tracks = 9 outside 1\.\.8", INVALID, rawt(n_tracks=9), tfn)
        refused(r"p = 0 outside 1\.\.16", INVALID, rawt(pp=0), tfn)
        refused(r"p = 17 outside 1\.\.16", INVALID, rawt(pp=17), tfn)
        refused(r"NULL templates_dev", INVALID, rawt(tptr=0), tfn)
        refused(r"NULL centres_dev", INVALID, rawt(cptr=0), tfn)
        refused(r"must be 8-byte aligned", INVALID, rawt(cptr=cb.data_ptr() + 4), tfn)
        refused(r"overlap: templates_dev .* and centres_dev", INVALID, rawt(tptr=cb.data_ptr() + 8), tfn)
        refused(r"templates_dev is page-locked host memory", INVALID, rawt(tptr=pin.ctypes.data), tfn)
        refused(rf"templates_dev spans {T * side * side} bytes, {side * side} more than", INVALID, rawt(tptr=end - side * side), tfn)
        refused(r"centres_dev spans 64 bytes, 16 more than", INVALID, rawt(cptr=end - 48), tfn)
        assert capture_refused(lambda s: ctx.track_template(0, cb, dt, p, T, s)) == [(STATE_, True)]
        with pytest.raises(ValueError, match="templates holds"):
            ctx.track_template(0, cb, Span(dt.data_ptr(), side * side), p, T)
        # a refused call queues nothing: the sentinels, the centres and the templates stand, and the context still computes
        assert (out.cpu().numpy() == 0xA5).all() and torch.equal(cb, keep_c) and torch.equal(dt, keep_t)
        got, _ = run(ctx, [2, 0, 1, 0], dt, cb, 48 * T, T, good, 0)
        same(got, mr.match([frames[k] for k in (2, 0, 1, 0)], tm, cen, **{**mr.DEFAULTS, "p": p, "s": 5})[0])
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 3. the drift scene ---------------------------------------------------------------------------------------------------------------
def test_the_drift_scene_is_corrected_exactly():
    d = mr.DRIFT
    frames, flows, true = mr.drift_scene()
    n, k, r, size = d["n"], d["split"], d["radius"], d["size"]
    prm = {"p": d["p"], "s": d["s"]}
    ref = {**mr.DEFAULTS, **prm}
    tprm = {"radius": r, "cut_threshold": NEVER}
    with context(size, size, mb=n, fslots=n + 1, slots=n) as ctx:
        ctx.upload_frames(0, list(frames))
        ctx.import_flows(dev(flows), list(range(n)))
        # pure advection drifts
        sd = pipeline.track_state(ctx, [tuple(true[0])])
        buf = pipeline.track_buffer(ctx, n, 1)
        ctx.track_advance(list(range(k)), sd, buf[:k * 48], tprm)
        ctx.track_advance(list(range(k, n)), sd, buf[k * 48:], tprm)
        rec = pipeline.track_records(buf, 1)
        assert np.hypot(rec["x"][-1, 0] - true[n - 1, 0], rec["y"][-1, 0] - true[n - 1, 1]) > 9.0
        # the corrected run: two calls that hand on the state, each followed by its two match calls
        sd = pipeline.track_state(ctx, [tuple(true[0])])
        tmpl = pipeline.match_templates(ctx, 1, d["p"])
        ctx.track_template(0, sd, tmpl, d["p"])
        buf = pipeline.track_buffer(ctx, n, 1)
        mout = pipeline.match_buffer(ctx, n, 1)
        sout = pipeline.match_buffer(ctx, 2, 1)
        for b, (lo, hi) in enumerate(((0, k), (k, n))):
            part = buf[lo * 48:hi * 48]
            ctx.track_advance(list(range(lo, hi)), sd, part, tprm)
            ctx.track_match(list(range(lo, hi)), tmpl, (part, 48), mout[lo * 48:hi * 48], prm, 1, True)
            ctx.track_match([hi], tmpl, (sd, 48), sout[b * 48:(b + 1) * 48], prm, 1, True)
        rec, mrec, srec = pipeline.track_records(buf, 1), pipeline.match_records(mout, 1), pipeline.match_records(sout, 1)
        st = pipeline.track_state_records(sd)
    Tm = mr.template(frames[0], true[:1], d["p"])
    assert tmpl.cpu().numpy().tobytes() == Tm.tobytes()
    ra, ma, sa, s1 = mr.corrected_batch(tk, frames[:k + 1], flows[:k], tk.state(true[0]), Tm, r, ref)
    rb, mb, sb, s2 = mr.corrected_batch(tk, frames[k:], flows[k:], s1, Tm, r, ref)
    assert rec.tobytes() == np.concatenate([ra, rb]).tobytes() and mrec.tobytes() == np.concatenate([ma, mb]).tobytes()
    assert srec.tobytes() == np.concatenate([sa, sb]).tobytes() and st.tobytes() == s2.tobytes()
    assert (mrec["status"] == 0).all() and (srec["status"] == 0).all()
    assert np.array_equal(rec["x"][:, 0], true[:n, 0]) and np.array_equal(rec["y"][:, 0], true[:n, 1])   # every head, exactly
    assert (st["x"][0], st["y"][0]) == tuple(true[n])


# ---- 4. the chunk schedule ------------------------------------------------------------------------------------------------------------
W_, H_, NP_, B_ = 64, 64, 20, 2


@pytest.fixture(scope="module")
def clip():
    return list(sine_translate_frames(NP_ + 1, W_, H_, seed=3, zoom=0.02))


@pytest.fixture(scope="module")
def engine_ctx():
    slots = pipeline.min_flow_slots(B_)
    assert slots < NP_ and B_ < 2 * pipeline.SMOOTH_RADIUS + 1      # the chunk is longer than the ring, B below the window's span
    with _capi.Context(W_, H_, max_batch=B_, frame_slots=2 * B_ + 2, flow_slots=slots) as ctx:
        yield ctx
        assert ctx.graph_stats()["capture_failures"] == 0


def hand_chunk(ctx, frames, *, start, radius, match, roi, gate, thr, batch):
    """The chunk with center="track" by hand on a context that holds it whole: the flow call; the templates from frame 0 about
    the state; per batch of `batch` pairs track_advance, track_match on the f0 frames about the batch's records, track_match on
    the last f1 frame about the state, and with roi roi_weights; with roi pass1_weighted; ONE window call.  match None: today's
    calls alone.  Returns (post, track, state, match, templates, maps) as bytes or None."""
    n = len(frames) - 1
    slots = list(range(n))
    ctx.upload_frames(0, [np.ascontiguousarray(f) for f in frames])
    ctx.flow_pairs(slots, list(range(1, n + 1)), slots, False)
    sd = pipeline.track_state(ctx, start)
    T = sd.numel() // STATE
    buf = torch.full((n * T * 48,), 0xA5, dtype=torch.uint8, device=DEV)
    mout = tmpl = None
    if match is not None:
        prm = _capi.match_choice(match)
        mout = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        sout = pipeline.match_buffer(ctx, 1, T)
        tmpl = pipeline.match_templates(ctx, T, prm.p)
        ctx.track_template(0, sd, tmpl, prm.p)
    maps = torch.full((n, H_, W_), 0xA5, dtype=torch.uint8, device=DEV) if roi else None
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        part = buf[lo * T * 48:hi * T * 48]
        ctx.track_advance(slots[lo:hi], sd, part, {"radius": radius, "cut_threshold": thr})
        if match is not None:
            ctx.track_match(slots[lo:hi], tmpl, (part, 48 * T), mout[lo * T * REC:hi * T * REC], prm, T, True)
            ctx.track_match([hi], tmpl, (sd, 48 * T), sout, prm, T, True)
        if roi:
            ctx.roi_weights(hi - lo, (part, 48 * T), maps[lo:hi], {"ax": roi[0], "ay": roi[1]}, gate=gate)
    out = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    if roi:
        ctx.pass1_weighted(slots, maps, False)
        ctx.radial_window_axes_weighted_centres(slots, 0, n, maps, (buf, 48 * T), out, cbh.RADIUS, thr, False)
    else:
        ctx.radial_window_axes_centres(slots, 0, n, (buf, 48 * T), out, cbh.RADIUS, thr, False)
    b = lambda t: None if t is None else t.cpu().numpy().tobytes()   # noqa: E731
    return b(out), b(buf), b(sd), b(mout), b(tmpl), b(maps)


@pytest.mark.parametrize("loose", [True, False], ids=["loose", "defaults"])
@pytest.mark.parametrize("roi", [None, (20.0, 12.0)], ids=["centres", "roi"])
def test_process_chunk_with_match_is_the_by_hand_composition(clip, engine_ctx, roi, loose):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    start = [(40.0, 24.0), (5.0, 60.0), (33.0, 31.0)]
    match = {"p": 6, "s": 4, "mode": "zssd", **(LOOSE if loose else {})}
    gate = dev(cbh.random_map(W_, H_, 2)) if roi else None
    state = pipeline.track_state(ctx, start)
    tout, mout = pipeline.track_buffer(ctx, NP_, 3), pipeline.match_buffer(ctx, NP_, 3)
    tmpl = pipeline.match_templates(ctx, 3, 6)
    wout = torch.empty((NP_, H_, W_), dtype=torch.uint8, device=DEV) if roi else None
    kw = {"weights_out": wout, "weights_gate": gate} if roi else {}
    buf = eng.process_chunk(clip, False, 7.0, center="track", track_out=tout, match_out=mout,
                            track={"state": state, "radius": 9, "roi": roi, "match": {**match, "templates": tmpl, "capture": True}}, **kw)
    with cbh.hand_context(W_, H_, NP_) as one:
        post, trk, st, mrec, tm, maps = hand_chunk(one, clip, start=start, radius=9, match=match, roi=roi, gate=gate, thr=7.0, batch=B_)
    assert tmpl.cpu().numpy().tobytes() == tm and mout.cpu().numpy().tobytes() == mrec
    assert tout.cpu().numpy().tobytes() == trk and state.cpu().numpy().tobytes() == st
    assert buf.cpu().numpy().tobytes() == post
    if roi:
        assert wout.cpu().numpy().tobytes() == maps
    m = pipeline.match_records(mout, 3)
    if loose:                                                         # every match stored: the heads are whole numbers
        assert (m["status"] == 0).all()
        heads = pipeline.track_records(tout, 3)
        assert np.array_equal(heads["x"], np.floor(heads["x"])) and np.array_equal(heads["x"], m["x"]) and np.array_equal(heads["y"], m["y"])
    # the templates as the restatement captures them, and record 0 as the restatement finds it in frame 0
    want_tm = mr.template(clip[0], start, 6)
    assert tm == want_tm.tobytes()
    w0, _ = mr.match([clip[0]], want_tm, np.array([start]), **{**mr.DEFAULTS, **match, "mode": mr.ZSSD})
    assert m[0].tobytes() == w0[0].tobytes() and (m["cost"][0] == 0).all()


def test_without_the_key_the_chunk_queues_todays_calls(clip, engine_ctx, monkeypatch):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    start = [(40.0, 24.0), (5.0, 60.0)]

    def never(*a, **k):
        raise AssertionError("a match call was queued without track['match']")
    monkeypatch.setattr(ctx, "track_match", never)
    monkeypatch.setattr(ctx, "track_template", never)
    for roi in (None, (20.0, 12.0)):
        state = pipeline.track_state(ctx, start)
        tout = pipeline.track_buffer(ctx, NP_, 2)
        buf = eng.process_chunk(clip, False, 7.0, center="track", track={"state": state, "radius": 9, "roi": roi}, track_out=tout)
        with cbh.hand_context(W_, H_, NP_) as one:
            post, trk, st, _, _, _ = hand_chunk(one, clip, start=start, radius=9, match=None, roi=roi, gate=None, thr=7.0, batch=NP_)
        assert buf.cpu().numpy().tobytes() == post and tout.cpu().numpy().tobytes() == trk and state.cpu().numpy().tobytes() == st
    monkeypatch.undo()
    with pytest.raises(ValueError, match="match_out= needs track.'match'."):
        eng.process_chunk(clip, center="track", track={"start": start}, match_out=pipeline.match_buffer(ctx, NP_, 2))
    with pytest.raises(ValueError, match="match_out holds"):
        eng.process_chunk(clip, center="track", track={"start": start, "match": {}}, match_out=pipeline.match_buffer(ctx, NP_ - 1, 2))
    with pytest.raises(ValueError, match=r"track\['match'\]\['templates'\] holds"):
        eng.process_chunk(clip, center="track", track={"start": start, "match": {"templates": pipeline.match_templates(ctx, 1)}})
    with pytest.raises(ValueError, match="process_flows: track.'match'. needs the frames"):
        eng.process_flows(torch.zeros((2, H_, W_, 2), device=DEV), center="track", track={"start": start, "match": {}})


def test_the_params_path_carries_state_and_templates(clip, engine_ctx):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    match = {"p": 6, "s": 4, **LOOSE}
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 11, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 7.0, "hip_center": "track", "hip_track": {"start": (40.0, 24.0), "radius": 9, "match": match}}
    plan = pipeline.pair_plan(30.0, len(clip), params)
    assert len(plan) >= 2
    state, tmpl = pipeline.track_state(ctx, (40.0, 24.0)), pipeline.match_templates(ctx, 1, 6)
    want = []
    for k, chunk in enumerate(plan):                                  # the first chunk captures, the others reuse
        buf = eng.process_chunk([clip[i] for i in chunk], False, 7.0, center="track",
                                track={"state": state, "radius": 9, "match": {**match, "templates": tmpl, "capture": k == 0}})
        want.append(pipeline.post_records(buf, axes=True)[0])
    assert tmpl.cpu().numpy().tobytes() == mr.template(clip[plan[0][0]], [(40.0, 24.0)], 6).tobytes()
    got = pipeline._frame_chunks(eng, clip, 30.0, params, True)
    assert [c.tobytes() for _, c, _ in got] == [c.tobytes() for c in want]
    assert pipeline.frames_to_actions(eng, clip, 30.0, params)
