"""GPU side of the whole-frame template re-detection (ffl_track_redetect: k_redetect_sweep, k_redetect_pick, k_redetect_final;
process_chunk with track["match"]["redetect"]), everything through the C ABI via _capi on frames placed
with upload_frames.  Records and written-back centres are held on bytes against the restatement tests/redetect_ref.py, whose
whole-frame sums are formed once per (size, p, frame, template) and shared by every case that searches them."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import match_ref as mr
import redetect_ref as rr
import track_ref as tk
from funscript_flow_amd import _capi, pipeline

DEV = "cuda:0"
REC, STATE = _capi.MATCH_DTYPE.itemsize, _capi.TRACK_STATE_DTYPE.itemsize
CUT = 1e6   # no pair of the scene is a cut
# 16x16: at p = 16 the template is wider than the frame and every sample clamps; 67x35: one full and one 3-wide tile column, two
# full and one 3-high tile row; 130x50: three tile columns, four tile rows, the last ones 2 wide and 2 high; 256x256: 4 x 16 full tiles
SIZES = [(16, 16), (67, 35), (130, 50), (256, 256)]
P_, E_, T_, N_ITEMS, REACH = (1, 4, 16), (1, 5, 32), (1, 3, 8), (1, 5, 33), (0, 1, 9, 70)
# an orthogonal array: every value of p, exclude, T, n meets every value of the other three once (L9), crossed with every reach
L9 = [(0, 0, 0, 0), (0, 1, 1, 1), (0, 2, 2, 2), (1, 0, 1, 2), (1, 1, 2, 0), (1, 2, 0, 1), (2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 1, 0)]
COMBOS = [(P_[a], E_[b], T_[c], N_ITEMS[d], r) for a, b, c, d in L9 for r in REACH]
FSLOTS = 6
LOOSE = {"min_var": 0.0, "max_mse": 65025.0, "ratio": 1.0}     # accepts everything but an exact tie with the runner-up


def gid(v):
    return "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h, mb=40, fslots=FSLOTS):
    return _capi.Context(w, h, max_batch=mb, frame_slots=fslots, flow_slots=2)


@functools.lru_cache(maxsize=None)
def frames_of(w, h, p):
    """FSLOTS gray frames: noise; noise with frame 0's patch about the centre pasted at an offset; flat; vertical stripes of
    period 4; saturated blocks of 0 and 255; noise with that patch pasted twice"""
    rng = np.random.default_rng(1000 * w + h)
    f = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(FSLOTS)]
    side = min(2 * p + 1, w, h)
    y0, x0 = max(0, h // 2 - side // 2), max(0, w // 2 - side // 2)
    patch = f[0][y0:y0 + side, x0:x0 + side]
    oy, ox = min(h - side, y0 + 2), max(0, x0 - 3)
    f[1][oy:oy + side, ox:ox + side] = patch
    f[2][:] = 131
    f[3][:] = ((np.arange(w) % 4) * 60).astype(np.uint8)[None, :]
    yy, xx = np.mgrid[0:h, 0:w]
    f[4][:] = ((((xx // 5) + (yy // 3)) & 1) * 255).astype(np.uint8)
    f[5][0:side, 0:side] = patch
    f[5][h - side:h, w - side:w] = patch
    out = np.stack(f)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def templates_of(w, h, p):
    """8 templates of mixed content: frame 0 about the centre (what frames 1 and 5 hold elsewhere), flat, the stripes, all 0,
    frame 5 about a corner, all 255, the saturated blocks, frame 0 about (0, 0)"""
    frames, side = frames_of(w, h, p), 2 * p + 1
    kinds = [mr.template(frames[0], [(w // 2, h // 2)], p)[0], np.full((side, side), 90, np.uint8),
             mr.template(frames[3], [(w // 2, h // 2)], p)[0], np.zeros((side, side), np.uint8),
             mr.template(frames[5], [(w - 1, h - 1)], p)[0], np.full((side, side), 255, np.uint8),
             mr.template(frames[4], [(w // 3, h // 3)], p)[0], mr.template(frames[0], [(0, 0)], p)[0]]
    out = np.stack(kinds)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sums_of(w, h, p, slot, t):
    """the restatement's whole-frame S1, S2 of template t in frame `slot`: computed once, shared, never written"""
    S1, S2 = rr.sums(frames_of(w, h, p)[slot], templates_of(w, h, p)[t], p)
    S1.setflags(write=False)
    S2.setflags(write=False)
    return S1, S2


def centres_of(n, T, w, h, seed):
    """(n, T, 2) centres: anywhere in the frame, x.5 anchors, the corners, and hostile bit patterns"""
    rng = np.random.default_rng(seed)
    c = np.empty((n, T, 2))
    c[..., 0] = rng.integers(0, w, (n, T)) + rng.choice([0.0, 0.25, 0.5, -0.5], (n, T))
    c[..., 1] = rng.integers(0, h, (n, T)) + rng.choice([0.0, 0.25, 0.5, -0.5], (n, T))
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


def match_buffer_of(status):
    """(n, T) match records with the given status words; the other fields are sentinels"""
    rec = np.zeros(status.shape, _capi.MATCH_DTYPE)
    rec["x"], rec["y"], rec["dx"], rec["dy"], rec["cost"], rec["second"], rec["pad"] = 1.5, -2.5, 3, -4, 55, 66, 0x5A5A
    rec["status"] = status
    return rec


def run(ctx, fslots, tmpl, cbuf, stride, T, prm, write_back, trigger=None, stream=None):
    """track_redetect into a sentinel-filled record buffer: (records (n, T), the centre buffer's bytes afterwards)"""
    out = torch.full((len(fslots) * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    assert ctx.track_redetect(fslots, tmpl, (cbuf, stride), out, prm, T, trigger, write_back, stream) is out
    return pipeline.match_records(out, T), cbuf.cpu().numpy().tobytes()


def same(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in got.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


def ref_prm(prm):
    return {**rr.DEFAULTS, **prm, "mode": _capi.MATCH_MODES.index(prm.get("mode", "zssd"))}


# ---- 1. the kernels against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=gid)
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_redetect_is_the_restatement(size, combo):
    (w, h), (p, e, T, n, reach) = size, combo
    frames, tm = frames_of(w, h, p), templates_of(w, h, p)[:T]
    fslots = [(5 * i + 1) % FSLOTS for i in range(n)]               # repeated and out of order
    cen = centres_of(n, T, w, h, seed=p + e + T + n + reach)
    full = lambda i, t: sums_of(w, h, p, fslots[i], t)              # noqa: E731
    trig = match_buffer_of(np.random.default_rng(p + e + n).choice([0, 1, 2, 4, 6, 7], (n, T)).astype(np.int32))
    with context(w, h) as ctx:
        ctx.upload_frames(0, list(frames))
        dt, dg = dev(tm), dev(np.frombuffer(trig.tobytes(), np.uint8))
        for mode in ("ssd", "zssd"):
            for prm in ({"p": p, "exclude": e, "reach": reach, "mode": mode}, {"p": p, "exclude": e, "reach": reach, "mode": mode, **LOOSE}):
                want, wcen = rr.redetect([frames[k] for k in fslots], tm, cen, **ref_prm(prm), full=full)
                rec = record_buffer(cen)                                # track records, one every 48 * T bytes
                for wb in (0, 1):
                    got, after = run(ctx, fslots, dt, dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * T, T, prm, wb)
                    same(got, want)
                    exp = rec.copy()
                    if wb:
                        exp["x"], exp["y"] = wcen[..., 0], wcen[..., 1]
                    assert after == exp.tobytes()                       # write_back 0: not a byte of the centres changes
                # a match-record array with mixed statuses as the trigger: skipped and run searches share the launches
                want_t, wcen_t = rr.redetect([frames[k] for k in fslots], tm, cen, **ref_prm(prm), full=full, trigger=trig["status"])
                got, after = run(ctx, fslots, dt, dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * T, T, prm, 1, trigger=dg)
                same(got, want_t)
                exp = rec.copy()
                exp["x"], exp["y"] = wcen_t[..., 0], wcen_t[..., 1]
                assert after == exp.tobytes()
                skipped = (trig["status"] & rr.POOR) == 0
                assert (got["status"][skipped] == rr.SKIPPED).all() and (got["status"][~skipped] != rr.SKIPPED).all()
                assert dg.cpu().numpy().tobytes() == trig.tobytes()     # the trigger records are only read
                if T == 1:                                               # a plain (n, 2) array, stride 16
                    for wb in (0, 1):
                        buf = dev(cen[:, 0, :])
                        out = torch.full((n * REC,), 0xA5, dtype=torch.uint8, device=DEV)
                        ctx.track_redetect(fslots, dt, buf, out, prm, 1, None, wb)
                        same(pipeline.match_records(out, 1), want)
                        assert buf.cpu().numpy().tobytes() == (wcen if wb else cen)[:, 0, :].tobytes()
                if n == 1:                                               # a state, re-detected in place
                    st = tk.state(cen[0], home=cen[0][::-1])
                    st["steps"], st["lost_run"], st["pad"] = 5, -2, 0x5A5A5A5A
                    got, after = run(ctx, fslots, dt, dev(np.frombuffer(st.tobytes(), np.uint8)), 48 * T, T, prm, 1)
                    same(got, want)
                    st["x"], st["y"] = wcen[0, :, 0], wcen[0, :, 1]
                    assert after == st.tobytes()
        if reach == 1 and e >= 2:
            assert (want["second"] == -1).all()
        assert ctx.graph_stats()["capture_failures"] == 0


def paste(I, sq, x, y):
    """sq's centre onto (x, y)"""
    p = sq.shape[0] // 2
    I[y - p:y + p + 1, x - p:x + p + 1] = sq


@pytest.mark.parametrize("mode", ["ssd", "zssd"])
def test_pastes_across_tiles_corners_and_tile_edges(mode):
    """the best and its exclusion square against the 64 x 16 tiles: inside one tile, across a tile column's edge, on a tile corner;
    the best on a tile's last row and column; the best in each frame corner, where the re-walked tiles are clipped"""
    w, h, p = 256, 96, 3
    rng = np.random.default_rng(31)
    sq = rng.integers(0, 256, (7, 7), dtype=np.uint8)
    back = rng.integers(0, 256, (h, w), dtype=np.uint8)
    cases = [((32, 24), 1), ((32, 24), 5), ((63, 24), 3), ((64, 24), 3), ((64, 32), 4), ((63, 31), 4), ((127, 47), 32), ((127, 79), 32),
             ((100, 40), 32), ((63, 15), 1)]
    frames, where = [], []
    for (x, y), e in cases:                                          # a second copy further down: the runner-up is exact as well
        I = back.copy()
        paste(I, sq, x, y)
        paste(I, sq, 220, 90)
        frames.append(I)
        where.append((x, y))
    corners = back.copy()
    frames.append(corners)
    tm4 = mr.template(corners, [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)], p)
    with context(w, h, mb=16, fslots=len(frames)) as ctx:
        ctx.upload_frames(0, frames)
        for k, ((x, y), e) in enumerate(cases):
            for reach in (0, 40):
                prm = {"p": p, "exclude": e, "reach": reach, "mode": mode, **LOOSE}
                cen = np.array([[(x + 7.0, y - 5.0)]])
                want, wcen = rr.redetect([frames[k]], sq[None], cen, **ref_prm(prm))
                got, after = run(ctx, [k], dev(sq[None]), dev(cen[0]), 16, 1, prm, 1)
                same(got, want)
                assert after == wcen[0].tobytes()
                assert (got["dx"][0, 0], got["dy"][0, 0], got["cost"][0, 0]) == (-7, 5, 0)
                assert got["second"][0, 0] == (0 if reach == 0 else want["second"][0, 0]) and (reach == 0 or got["second"][0, 0] > 0)
                assert got["status"][0, 0] == (rr.AMBIGUOUS if reach == 0 else 0)
        for e in (1, 32):
            prm = {"p": p, "exclude": e, "mode": mode}
            cen = np.tile(np.array([w / 2.0, h / 2.0]), (1, 4, 1))
            want, wcen = rr.redetect([corners], tm4, cen, **ref_prm(prm))
            rec = record_buffer(cen)
            got, after = run(ctx, [len(frames) - 1], dev(tm4), dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * 4, 4, prm, 1)
            same(got, want)
            assert [(r["x"], r["y"], r["cost"], r["status"]) for r in got[0]] == [(0, 0, 0, 0), (w - 1, 0, 0, 0), (0, h - 1, 0, 0), (w - 1, h - 1, 0, 0)]


def test_every_content_and_a_call_with_everything_skipped():
    w, h, p = 130, 50, 4
    frames, tm = frames_of(w, h, p), templates_of(w, h, p)
    cen = np.tile(np.array([w // 2 - 1.0, h // 2 + 1.0]), (FSLOTS, 8, 1))
    full = lambda i, t: sums_of(w, h, p, i, t)                      # noqa: E731
    with context(w, h, mb=8) as ctx:
        ctx.upload_frames(0, list(frames))
        for mode in ("ssd", "zssd"):
            prm = {"p": p, "exclude": 4, "mode": mode}
            want, wcen = rr.redetect(list(frames), tm, cen, **ref_prm(prm), full=full)
            rec = record_buffer(cen)
            got, after = run(ctx, list(range(FSLOTS)), dev(tm), dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * 8, 8, prm, 1)
            same(got, want)
            rec["x"], rec["y"] = wcen[..., 0], wcen[..., 1]
            assert after == rec.tobytes()
            assert (got["status"][:, 1] & rr.FLAT).all() and (got["status"][:, 3] & rr.FLAT).all()      # flat templates
            assert got["status"][1, 0] == 0 and got["cost"][1, 0] == 0                                   # one paste: found
            assert got["status"][5, 0] == rr.AMBIGUOUS and got["cost"][5, 0] == 0 == got["second"][5, 0]  # two pastes: not accepted
            assert (got["dx"][2] == -(w // 2 - 1)).all() and (got["dy"][2] == -(h // 2 + 1)).all()        # a flat frame: (0, 0) wins
            assert got["cost"][3, 2] == 0 and got["second"][3, 2] == 0                                   # stripes on stripes
        # everything skipped: the records are L7's skipped form and not one byte of the centres differs, hostile bits included
        hostile = centres_of(FSLOTS, 8, w, h, seed=2)
        rec = record_buffer(hostile)
        for trig, mask in ((np.zeros((FSLOTS, 8), np.int32), rr.POOR), (np.full((FSLOTS, 8), 5, np.int32), rr.POOR)):
            dg = dev(np.frombuffer(match_buffer_of(trig).tobytes(), np.uint8))
            got, after = run(ctx, list(range(FSLOTS)), dev(tm), dev(np.frombuffer(rec.tobytes(), np.uint8)), 48 * 8, 8,
                             {"p": p, "exclude": 4, "trigger_mask": mask, **LOOSE}, 1, trigger=dg)
            assert after == rec.tobytes()
            want, _ = rr.redetect(list(frames), tm, hostile, **ref_prm({"p": p, "exclude": 4, **LOOSE}), trigger=trig)
            same(got, want)
            assert (got["status"] == rr.SKIPPED).all() and (got["cost"] == -1).all() and (got["second"] == -1).all()
        # a plain int32 array as an explicit span: words 0, 2, 6, -1 against masks 2 and 4
        words = np.array([[0], [2], [6], [-1]], np.int32)
        for mask in (2, 4):
            prm = {"p": p, "exclude": 4, "trigger_mask": mask}
            c4 = np.tile(np.array([3.0, 3.0]), (4, 1, 1))
            want, wcen = rr.redetect([frames[1]] * 4, tm[:1], c4, **ref_prm(prm), trigger=words, full=lambda i, t: sums_of(w, h, p, 1, 0))
            padded = np.zeros((4, 12), np.int32)
            padded[:, 0] = words[:, 0]
            got, after = run(ctx, [1] * 4, dev(tm[:1]), dev(c4[:, 0]), 16, 1, prm, 1, trigger=(dev(padded), 48))
            same(got, want)
            assert after == wcen[:, 0].tobytes() and [int(s) for s in got["status"][:, 0]] == [8 if not (int(x) & mask) else 0 for x in words[:, 0]]


def test_1080p_whole_frame_and_a_reach_at_a_corner():
    w, h = 1920, 1080
    rng = np.random.default_rng(12)
    I = rng.integers(0, 256, (h, w), dtype=np.uint8)
    with context(w, h, mb=1, fslots=2) as ctx:
        ctx.upload_frames(0, [I])
        # n = 1, T = 1, p = 8, the whole frame: 2 M candidates
        tm = mr.template(I, [(1501, 977)], 8)
        cen = np.array([[(100.5, 100.0)]])
        prm = {"p": 8, "exclude": 8}
        want, wcen = rr.redetect([I], tm, cen, **ref_prm(prm))
        got, after = run(ctx, [0], dev(tm), dev(cen[0]), 16, 1, prm, 1)
        same(got, want)
        assert after == wcen[0].tobytes() == np.array([1501.0, 977.0]).tobytes() and got["cost"][0, 0] == 0 and got["status"][0, 0] == 0
        # p = 16, reach 200 about the frame's last pixel: the window and the re-walked tiles are clipped on two sides
        tm = mr.template(I, [(1760, 1079)], 16)
        cen = np.array([[(1e9, np.inf)]])
        prm = {"p": 16, "exclude": 32, "reach": 200, "mode": "ssd"}
        want, wcen = rr.redetect([I], tm, cen, **ref_prm(prm))
        got, after = run(ctx, [0], dev(tm), dev(cen[0]), 16, 1, prm, 1)
        same(got, want)
        assert after == wcen[0].tobytes() == np.array([1760.0, 1079.0]).tobytes() and (got["dx"][0, 0], got["dy"][0, 0]) == (-159, 0)


def test_independence_and_a_map_read_straight_behind():
    w, h, p, n, T = 67, 35, 4, 5, 3
    frames, tm = frames_of(w, h, p), templates_of(w, h, p)
    cen8 = centres_of(n, 8, w, h, seed=3)
    prm = {"p": p, "exclude": 5, "reach": 30, "mode": "zssd", **LOOSE}
    fslots = [1, 0, 1, 5, 3]
    trig = match_buffer_of(np.random.default_rng(4).choice([0, 2, 3, 4], (n, 8)).astype(np.int32))
    with context(w, h, mb=8) as ctx:
        ctx.upload_frames(0, list(frames))
        dg = dev(np.frombuffer(trig.tobytes(), np.uint8))
        all8, _ = run(ctx, fslots, dev(tm), dev(np.frombuffer(record_buffer(cen8).tobytes(), np.uint8)), 48 * 8, 8, prm, 1, trigger=dg)
        assert (all8["status"] == rr.SKIPPED).any() and (all8["status"] != rr.SKIPPED).any()
        for t in (0, 3, 7):                                              # L9: a track alone, with its own trigger words
            alone, _ = run(ctx, fslots, dev(tm[t:t + 1]), dev(cen8[:, t, :]), 16, 1, prm, 1,
                           trigger=(dg.data_ptr() + 48 * t + _capi.MATCH_STATUS_OFFSET, 48 * 8))
            same(alone[:, 0], all8[:, t])
        one, _ = run(ctx, fslots[3:4], dev(tm), dev(np.frombuffer(record_buffer(cen8[3:4]).tobytes(), np.uint8)), 48 * 8, 8, prm, 1,
                     trigger=dg[3 * 8 * REC:4 * 8 * REC])
        same(one[0], all8[3])                                            # an item alone
        # track_redetect, roi_weights and the read on the caller's stream, queued back to back: the maps are about re-detected centres
        cen = cen8[:, :T]
        want, wcen = rr.redetect([frames[k] for k in fslots], tm[:T], cen, **ref_prm(prm))
        side = torch.cuda.Stream()
        buf = dev(np.frombuffer(record_buffer(cen).tobytes(), np.uint8))
        out = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        maps = torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV)
        dtm = dev(tm[:T])
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            ctx.track_redetect(fslots, dtm, (buf, 48 * T), out, prm, T, None, True, side)
            ctx.roi_weights(n, (buf, 48 * T), maps, {"ax": 9.0, "ay": 5.0}, stream=side)
            got_maps = maps.cpu().numpy()
        same(pipeline.match_records(out, T), want)
        assert np.array_equal(got_maps, tk.roi_maps(w, h, wcen[:, 0], 9.0, 5.0))
        assert not np.array_equal(got_maps, tk.roi_maps(w, h, np.nan_to_num(cen[:, 0], nan=0.0, posinf=1e9, neginf=-1e9), 9.0, 5.0))
        assert ctx.graph_stats()["capture_failures"] == 0


def test_extra_bytes_is_the_allocations_growth():
    w, h, mb = 1920, 1080, 64   # 8.4 MB: an allocation of its own, which the device's free memory shows
    frames = frames_of(67, 35, 4)
    with _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=2) as ctx:
        ctx.upload_frames(0, [np.zeros((h, w), np.uint8)])
        tm, cen, out = dev(frames[0][:9, :9]), dev(np.array([[5.0, 5.0]])), torch.zeros(REC, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info(0)[0]
        ctx.track_redetect([0], tm, cen, out, {"p": 4, "exclude": 4})
        torch.cuda.synchronize()
        grown = free0 - torch.cuda.mem_get_info(0)[0]
        need = _capi.redetect_extra_bytes(w, h, mb)
        assert need == 8 * (30 * 68 + 20) * mb * 8
        assert need <= grown <= need + (4 << 20), (need, grown)          # the allocator's granularity, nothing more
        ctx.track_redetect([0], tm, cen, out, {"p": 4, "exclude": 4})
        torch.cuda.synchronize()
        assert free0 - torch.cuda.mem_get_info(0)[0] == grown            # the first call allocated; the second allocates nothing


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
        tm = templates_of(w, h, p)[:T]
        dt = dev(tm)
        cen = centres_of(4, T, w, h, seed=1)
        rec = record_buffer(cen)
        cb = dev(np.frombuffer(rec.tobytes(), np.uint8))
        out = torch.full((5 * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        trig = match_buffer_of(np.full((4, T), 2, np.int32))
        dg = dev(np.frombuffer(trig.tobytes(), np.uint8))
        keep_c, keep_t, keep_g = cb.clone(), dt.clone(), dg.clone()
        L, hd = ctx.L, ctx._h
        good = _capi.RedetectParams(p=p, exclude=5)

        def raw(fslots, n_tracks=T, prm=None, tptr=None, cptr=None, stride=48 * T, gptr=None, gstride=48 * T, wb=1, optr=None,
                null_list=False):
            ps, arr = _capi._iarr(fslots)
            q = good if prm is None else prm
            return lambda: (arr, ctx._chk(L.ffl_track_redetect(hd, len(fslots), None if null_list else ps, n_tracks, C.byref(q),
                                                               dt.data_ptr() if tptr is None else tptr,
                                                               cb.data_ptr() if cptr is None else cptr, stride,
                                                               dg.data_ptr() + 40 if gptr is None else gptr, gstride, wb,
                                                               out.data_ptr() if optr is None else optr, _capi.stream_handle(None, 0))))

        def refused(match, code, call, fn="ffl_track_redetect"):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and fn in str(e.value)

        # everything ffl_track_match refuses
        refused(r"n = 0 items outside 1\.\.4", INVALID, raw([]))
        refused(r"n = 5 items outside 1\.\.4", INVALID, raw([0, 1, 2, 0, 1]))
        refused(r"n_tracks = 0 outside 1\.\.8", INVALID, raw([0], 0))
        refused(r"n_tracks = 9 outside 1\.\.8", INVALID, raw([0], 9))
        refused(r"NULL fslots", INVALID, raw([0], null_list=True))
        refused(r"item 0: frame slot 4 out of range", INVALID, raw([4]))
        refused(r"item 1: frame slot -1 out of range", INVALID, raw([0, -1]))
        refused(r"item 1: frame slot 3 was never uploaded", STATE_, raw([0, 3]))
        nan = float("nan")
        for field, value, match in (("p", 0, r"p = 0 outside 1\.\.16"), ("p", 17, r"p = 17 outside 1\.\.16"), ("mode", 2, "mode = 2 is neither"),
                                    ("exclude", 0, r"exclude = 0 outside 1\.\.32"), ("exclude", 33, r"exclude = 33 outside 1\.\.32.*rule L5"),
                                    ("reach", -1, r"reach = -1 outside.*rule L2"), ("reach", 32769, "reach = 32769 outside"),
                                    ("min_var", -1.0, "min_var = -1 outside"), ("min_var", nan, "min_var = nan outside"),
                                    ("max_mse", 65026.0, "max_mse = 65026 outside"), ("max_mse", nan, "max_mse = nan outside"),
                                    ("ratio", 0.0, "ratio = 0 outside"), ("ratio", 1.25, "ratio = 1.25 outside"), ("ratio", nan, "ratio = nan outside")):
            bad = _capi.RedetectParams(p=p, exclude=5)
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
        refused(r"write_back = 2 is neither 0 nor 1 \(rule L8\)", INVALID, raw([0], wb=2))
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
        # the trigger words
        refused(r"trigger_dev must be 4-byte aligned \(rule L1\)", INVALID, raw([0], gptr=dg.data_ptr() + 42))
        refused(r"trigger stride 98: a multiple of 4 bytes", INVALID, raw([0, 1], gstride=98))
        refused(r"trigger stride 48: a multiple of 4 bytes, at least 48 \* \(n_tracks - 1\) \+ 4 = 52 \(rule L1\)", INVALID, raw([0, 1], gstride=48))
        refused(r"trigger stride 0:", INVALID, raw([0], gstride=0))
        refused(r"trigger stride -96:", INVALID, raw([0, 1], gstride=-96))
        refused(rf"overlap: trigger_dev \({96 + 52} bytes\) and centres_dev \({96 + 64} bytes\) share memory", INVALID,
                raw([0, 1], gptr=cb.data_ptr() + 40))
        refused(r"overlap: trigger_dev \(52 bytes\) and out_dev", INVALID, raw([0], gptr=out.data_ptr() + 40))
        refused(r"overlap: trigger_dev .* and templates_dev", INVALID, raw([0], gptr=(dt.data_ptr() + 7) // 4 * 4))
        refused(r"trigger_dev is page-locked host memory.*device memory", INVALID, raw([0], gptr=pin.ctypes.data))
        refused(rf"trigger_dev spans {96 + 52} bytes, 44 more than its allocation holds", INVALID, raw([0, 1], gptr=end - 104))
        assert capture_refused(lambda s: ctx.track_redetect([0], dt, (cb, 48 * T), out, good, T, dg, True, s)) == [(STATE_, True)]
        with pytest.raises(ValueError, match="out holds"):
            ctx.track_redetect([0, 1], dt, (cb, 48 * T), Span(out.data_ptr(), T * REC), good, T)
        with pytest.raises(ValueError, match="trigger holds"):
            ctx.track_redetect([0, 1], dt, (cb, 48 * T), out, good, T, Span(dg.data_ptr(), T * REC))
        with pytest.raises(ValueError, match="not device memory"):
            ctx.track_redetect([0], torch.zeros(T * side * side, dtype=torch.uint8), (cb, 48 * T), out, good, T)
        # a refused call queues nothing: the sentinels, the centres, the templates and the trigger stand, and the context still computes
        assert (out.cpu().numpy() == 0xA5).all() and torch.equal(cb, keep_c) and torch.equal(dt, keep_t) and torch.equal(dg, keep_g)
        got, _ = run(ctx, [2, 0, 1, 0], dt, cb, 48 * T, T, good, 0, trigger=dg)
        same(got, rr.redetect([frames[k] for k in (2, 0, 1, 0)], tm, cen, **{**rr.DEFAULTS, "p": p, "exclude": 5}, trigger=trig["status"])[0])
        assert (got["status"] != rr.SKIPPED).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 3. the lost-and-found scene through the chunk ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_ctx():
    d, B = mr.DRIFT, rr.JUMP["batch"]
    with _capi.Context(d["size"], d["size"], max_batch=B, frame_slots=2 * B + 2, flow_slots=pipeline.min_flow_slots(B)) as ctx:
        yield ctx
        assert ctx.graph_stats()["capture_failures"] == 0


def test_the_lost_and_found_scene_through_process_chunk(scene_ctx):
    """The scene's frames through the real flow: the chunk's exported fields go through the restatements' schedule, batch by
    batch, and every buffer the chunk wrote equals it on bytes.  The square jumps 90 px inside the second batch of 11: the search
    about the state reads POOR there, the whole-frame search behind it finds the square on its true pixel, and the third batch
    starts from it."""
    d, B, jump = mr.DRIFT, rr.JUMP["batch"], rr.JUMP["pair"]
    n, size, T = d["n"], d["size"], 1
    frames, _, true = rr.lost_scene()
    ctx, eng = scene_ctx, pipeline.PairEngine(scene_ctx)
    match = {"p": d["p"], "s": d["s"]}
    state = pipeline.track_state(ctx, [tuple(true[0])])
    tout, mout = pipeline.track_buffer(ctx, n, T), pipeline.match_buffer(ctx, n, T)
    rout = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    flows = torch.empty((n, size, size, 2), dtype=torch.float32, device=DEV)
    eng.process_chunk(list(frames), False, CUT, center="track", track_out=tout, match_out=mout, redetect_out=rout, flows_out=flows,
                      track={"state": state, "radius": d["radius"], "match": {**match, "redetect": True}})
    fl = flows.cpu().numpy()
    got_r = pipeline.match_records(rout, T)
    Tm = mr.template(frames[0], true[:1], d["p"])
    prm, rprm = {**mr.DEFAULTS, **match}, dict(rr.DEFAULTS)
    st, recs, mrecs, last = tk.state(true[0]), [], [], []
    for lo in range(0, n, B):
        hi = min(lo + B, n)
        rec, mrec, srec, rrec, st = rr.found_batch(tk, frames[lo:hi + 1], fl[lo:hi], st, Tm, d["radius"], prm, rprm)
        recs.append(rec)
        mrecs.append(mrec)
        last.append(hi - 1)
        assert got_r[hi - 1].tobytes() == rrec[0].tobytes(), (lo, hi, got_r[hi - 1], rrec)
        assert (st["x"][0], st["y"][0]) == tuple(true[hi])            # found again behind the batch that lost it
        assert (rrec["status"][0, 0] == 0 and rrec["cost"][0, 0] == 0) if lo <= jump < hi else rrec["status"][0, 0] in (0, rr.SKIPPED)
    assert tout.cpu().numpy().tobytes() == np.concatenate(recs).tobytes() and mout.cpu().numpy().tobytes() == np.concatenate(mrecs).tobytes()
    assert state.cpu().numpy().tobytes() == st.tobytes()
    others = np.ones(n, bool)
    others[last] = False
    assert (rout.cpu().numpy().reshape(n, T * REC)[others] == 0xA5).all()   # the other entries are not written


def test_without_the_key_nothing_new_is_queued(scene_ctx, monkeypatch):
    d = mr.DRIFT
    frames, _, true = rr.lost_scene()
    ctx, eng = scene_ctx, pipeline.PairEngine(scene_ctx)

    def never(*a, **k):
        raise AssertionError("track_redetect was queued without track['match']['redetect']")
    monkeypatch.setattr(ctx, "track_redetect", never)
    clip = list(frames[:13])
    outs = []
    for match in ({"p": d["p"], "s": d["s"]}, {"p": d["p"], "s": d["s"], "redetect": False}, {"p": d["p"], "s": d["s"], "redetect": None}, None):
        state = pipeline.track_state(ctx, [tuple(true[0])])
        tout = pipeline.track_buffer(ctx, 12, 1)
        trk = {"state": state, "radius": d["radius"]}
        if match is not None:
            trk["match"] = match
        buf = eng.process_chunk(clip, False, CUT, center="track", track=trk, track_out=tout)
        outs.append((buf.cpu().numpy().tobytes(), tout.cpu().numpy().tobytes(), state.cpu().numpy().tobytes()))
    assert outs[0] == outs[1] == outs[2] and outs[0] != outs[3]
    with pytest.raises(AssertionError, match="track_redetect was queued"):
        eng.process_chunk(clip, False, CUT, center="track",
                          track={"start": tuple(true[0]), "radius": d["radius"], "match": {"p": d["p"], "s": d["s"], "redetect": True}})
    monkeypatch.undo()
    with pytest.raises(ValueError, match="redetect_out= needs track.'match'..'redetect'."):
        eng.process_chunk(clip, center="track", track={"start": (1, 2), "match": {}}, redetect_out=pipeline.match_buffer(ctx, 12, 1))
    with pytest.raises(ValueError, match="redetect_out holds"):
        eng.process_chunk(clip, center="track", track={"start": (1, 2), "match": {"redetect": True}}, redetect_out=pipeline.match_buffer(ctx, 11, 1))
    with pytest.raises(ValueError, match="process_flows: track.'match'. needs the frames"):
        eng.process_flows(torch.zeros((2, d["size"], d["size"], 2), device=DEV), center="track",
                          track={"start": (1, 2), "match": {"redetect": True}})
