"""GPU side of region tracking and ROI maps (ffl_track_advance: k_track; ffl_roi_weights: k_roi_weights;
ffl_radial_window_axes_weighted_centres; process_chunk / process_flows with center="track"), everything
through the C ABI via _capi on fields placed with import_flows / upload_flow.  Track records, states and ROI maps are held bit
for bit against the restatement tests/track_ref.py; the fifth window form against its two sibling forms on bytes and against
weights_ref's bound; the chunk schedules against a by-hand composition of the calls."""
import functools
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import chunk_by_hand as cbh
import grid_ref as gr
import track_ref as tk
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
REC, STATE, ITEM = _capi.TRACK_DTYPE.itemsize, _capi.TRACK_STATE_DTYPE.itemsize, _capi.PASS2_AXES_DTYPE.itemsize
BIG = 1e30
NEVER = float("inf")   # rule Q5: the only threshold that never cuts (a field with an inf has an infinite mean magnitude)
SIZES = [(16, 16), (67, 35), (256, 256)]   # 16x16: r = 12 and r = 32 clip on all four sides; 67x35: odd, rows not 8-byte multiples
# (radius, tracks, items): every value of r in {1, 7, 32}, T in {1, 3, 8}, n in {1, 5, 33} meets every value of the other two
COMBOS = [(1, 1, 1), (7, 3, 5), (32, 8, 33), (1, 3, 33), (7, 8, 1), (32, 1, 5), (1, 8, 5), (7, 1, 33), (32, 3, 1), (12, 2, 5)]


def gid(v):
    return "x".join(str(k) for k in v) if isinstance(v, tuple) else str(v)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h, mb=40, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=slots or mb)


def points(w, h, T, seed=0):
    """T start points: the four corners, the centre, an x.5 anchor and two random ones, in an order that depends on the seed"""
    rng = np.random.default_rng(100 + seed)
    p = [(0.0, 0.0), (w - 1.0, h - 1.0), (w / 2.0, h / 2.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w // 3 + 0.5, h // 3 + 0.5),
         tuple(rng.uniform(0, min(w, h) - 1, 2)), tuple(rng.uniform(0, min(w, h) - 1, 2))]
    return [p[(k + seed) % 8] for k in range(T)]


@functools.lru_cache(maxsize=None)
def content(kind, n, w, h):
    """(n, h, w, 2) float32 fields"""
    rng = np.random.default_rng(zlib.crc32(repr((kind, n, w, h)).encode()))
    if kind == "uniform":
        f = np.empty((n, h, w, 2), np.float32)
        f[..., 0], f[..., 1] = 1.25, -0.5
    elif kind == "rectangle":
        f = np.zeros((n, h, w, 2), np.float32)
        for i in range(n):
            x0, y0 = (w // 4 + 2 * i) % max(1, w - w // 3), max(0, h // 2 - i)
            f[i, y0:y0 + max(4, h // 3), x0:x0 + max(4, w // 3)] = (2.0, -1.0)
    elif kind == "noise":
        f = (rng.standard_normal((n, h, w, 2)) * 3.0).astype(np.float32)
    elif kind == "specks":
        f = (rng.standard_normal((n, h, w, 2)) * 2.0).astype(np.float32)
        bad = rng.random((n, h, w)) < 0.05
        f[bad, 0] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
        bad = rng.random((n, h, w)) < 0.05
        f[bad, 1] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(bad.sum()))
    elif kind == "all-nan":
        f = (rng.standard_normal((n, h, w, 2)) * 2.0).astype(np.float32)
        f[::2] = np.nan
    else:
        raise AssertionError(kind)
    f.setflags(write=False)
    return f


def run(ctx, slots, st, params=None, weights=None, stream=None):
    """track_advance into a sentinel-filled record buffer: (records (n, T), the state afterwards (T,)); st: host records"""
    T = len(st)
    sd = dev(np.frombuffer(st.tobytes(), np.uint8))
    out = torch.full((len(slots) * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.track_advance(slots, sd, out, params, weights, stream)
    return pipeline.track_records(out, T), pipeline.track_state_records(sd)


def cuts_of(ctx, slots, thr):
    return [r[4] for r in ctx.pass1_results(slots, thr)]


def same(got, want):
    """records or states, bit for bit (the restatement produces no NaN: Q1 and Q6 keep them out)"""
    assert got.dtype == want.dtype and got.shape == want.shape
    for k in got.dtype.names:
        assert got[k].tobytes() == want[k].tobytes(), (k, got[k], want[k])


# ---- 1. k_track against the restatement -------------------------------------------------------------------------------------
@pytest.mark.parametrize("combo", COMBOS, ids=gid)
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_track_matches_the_restatement(size, combo):
    (w, h), (r, T, n) = size, combo
    kinds = ["uniform", "rectangle", "noise", "specks", "all-nan"]
    kind = kinds[(r + T + n + w) % len(kinds)]
    f = content(kind, n, w, h)
    slots = [(3 * i + 1) % 40 for i in range(n)]
    with context(w, h) as ctx:
        ctx.import_flows(dev(f), slots)
        cuts = cuts_of(ctx, slots, 7.0)
        st = tk.state(points(w, h, T, seed=r), home=points(w, h, T, seed=r + 3))
        got, gst = run(ctx, slots, st, {"radius": r})
        want, wst = tk.advance(f, cuts, st, radius=r)
        same(got, want)
        same(gst, wst)
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("kind", ["uniform", "rectangle", "noise", "specks", "all-nan"])
def test_every_content_at_every_size(kind):
    for w, h in SIZES:
        n, T, r = 5, 3, 12 if kind != "rectangle" else 2
        f = content(kind, n, w, h)
        with context(w, h, mb=8) as ctx:
            ctx.import_flows(dev(f), list(range(n)))
            st = tk.state(points(w, h, T, seed=2)) if kind != "rectangle" else tk.state(
                [(w // 4 + max(4, w // 3) / 2.0, h // 2 + max(4, h // 3) / 2.0), (0.0, 0.0), (w - 1.0, h - 1.0)])
            got, gst = run(ctx, list(range(n)), st, {"radius": r, "cut_threshold": NEVER})
            want, wst = tk.advance(f, [False] * n, st, radius=r)
            same(got, want)
            same(gst, wst)
            if kind == "uniform":
                assert set(got["du"].ravel()) == {1.25} and set(got["dv"].ravel()) == {-0.5}
            if kind == "all-nan":
                assert (got["status"][::2] & tk.LOST).all() and not (got["status"][1::2] & tk.LOST).any()
                assert (got["count"][::2] == 0).all() and gst["lost_run"].tolist() == [1] * T


def test_1080p_corners_and_centre():
    w, h, n, T, r = 1920, 1080, 3, 8, 32
    rng = np.random.default_rng(11)
    f = np.zeros((n, h, w, 2), np.float32)
    for y0, x0 in ((0, 0), (0, w - 80), (h - 80, 0), (h - 80, w - 80), (h // 2 - 40, w // 2 - 40)):   # only what a window can see
        f[:, y0:y0 + 80, x0:x0 + 80] = (rng.standard_normal((n, 80, 80, 2)) * 4.0).astype(np.float32)
    pts = [(0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0), (w / 2.0, h / 2.0), (w - 1.5, h - 1.5), (31.5, 32.5),
           (w / 2.0 + 0.5, h / 2.0 - 0.5)]
    with context(w, h, mb=4) as ctx:
        ctx.import_flows(dev(f), [2, 0, 1])
        st = tk.state(pts)
        got, gst = run(ctx, [2, 0, 1], st, {"radius": r, "cut_threshold": NEVER})
        want, wst = tk.advance(f, [False] * n, st, radius=r)
        same(got, want)
        same(gst, wst)
        assert got["count"][0, 0] == 33 * 33 and got["count"][0, 4] == 65 * 65


def test_cut_items_under_both_on_cut_values_and_an_infinite_threshold():
    w, h, n = 67, 35, 6
    f = content("noise", n, w, h).copy()
    f[2] = 10.0     # mean magnitude 14.1 > 7: a cut
    f[3] = 10.0
    slots = list(range(n))
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(f), slots)
        cuts = cuts_of(ctx, slots, 7.0)
        assert cuts == [False, False, True, True, False, False]
        st = tk.state(points(w, h, 3, 1), home=[(5.0, 5.0), (60.0, 30.0), (33.0, 17.0)])
        for on_cut, code in (("hold", tk.HOLD), ("home", tk.HOME)):
            got, gst = run(ctx, slots, st, {"radius": 7, "on_cut": on_cut})
            want, wst = tk.advance(f, cuts, st, radius=7, on_cut=code)
            same(got, want)
            same(gst, wst)
            assert (got["status"][2:4] == tk.CUT).all() and (got["count"][2:4] == 0).all() and gst["steps"].tolist() == [n] * 3
        assert (got["x"][4] == [5.0, 60.0, 33.0]).all()           # HOME: the pair after the cut starts at home
        got, _ = run(ctx, slots, st, {"radius": 7, "cut_threshold": float("inf")})
        same(got, tk.advance(f, [False] * n, st, radius=7)[0])
        assert not (got["status"] & tk.CUT).any()
        got, _ = run(ctx, slots, st, {"radius": 7, "cut_threshold": -1.0})   # everything is a cut: nothing moves
        assert (got["status"] == tk.CUT).all() and (got["x"] == got["x"][0]).all()


def test_maps_static_per_item_padded_and_zero_over_the_window():
    w, h, n, T = 67, 35, 5, 3
    f = content("specks", n, w, h)
    slots = [4, 3, 2, 1, 0]
    maps = cbh.pair_maps(w, h, n, 7)
    maps[3, :, :] = 0                                               # the whole window (and frame) of item 3: LOST
    maps[1, 0:20, 0:20] = 0                                         # the window of the track at the corner only
    st = tk.state([(3.0, 3.0), (40.0, 20.0), (66.0, 34.0)])
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(f), slots)
        prm = {"radius": 7, "cut_threshold": NEVER}
        for given, ref in ((dev(maps[0]), maps[0]), (dev(maps), maps), (cbh.padded(maps, DEV), maps)):
            got, gst = run(ctx, slots, st, prm, given)
            want, wst = tk.advance(f, [False] * n, st, radius=7, maps=ref)
            same(got, want)
            same(gst, wst)
        assert (got["status"][3] & tk.LOST).all() and got["status"][1, 0] & tk.LOST and not got["status"][1, 1] & tk.LOST
        ones, _ = run(ctx, slots, st, prm, dev(np.ones((h, w), np.uint8)))
        none, _ = run(ctx, slots, st, prm)
        same(ones, none)                                            # a map of ones is no map


def test_q9_two_calls_and_hostile_states():
    w, h, n, T = 67, 35, 9, 8
    f = content("noise", n, w, h)
    slots = list(range(n))
    bits = np.array([np.nan, -5.0, 1e9, np.inf, -np.inf, -0.0, 5e-324, 33.5])
    st = tk.state(np.stack([bits, bits[::-1]], axis=1), home=np.stack([bits[::-1], bits], axis=1))
    st["steps"], st["lost_run"], st["pad"] = 2 ** 63 - 3, -7, 0x5A5A5A5A
    st["steps"][1], st["lost_run"][1] = -1, 2 ** 31 - 1
    raw = np.frombuffer(st.tobytes(), np.uint8).copy()
    raw[2 * STATE:2 * STATE + 8] = 0xFF                             # a NaN with every bit set
    st = np.frombuffer(raw.tobytes(), _capi.TRACK_STATE_DTYPE).copy()
    with context(w, h, mb=16) as ctx:
        ctx.import_flows(dev(f), slots)
        prm = {"radius": 5, "on_cut": "home", "cut_threshold": NEVER}
        whole, wst = run(ctx, slots, st, prm)
        want, rst = tk.advance(f, [False] * n, st, radius=5, on_cut=tk.HOME)
        same(whole, want)
        same(wst, rst)
        assert (whole["x"] >= 0).all() and (whole["x"] <= w - 1).all() and (whole["y"] >= 0).all() and (whole["y"] <= h - 1).all()
        for k in (1, n - 1, 4):
            sd = dev(np.frombuffer(st.tobytes(), np.uint8))
            out = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
            ctx.track_advance(slots[:k], sd, out[:k * T * REC], prm)
            ctx.track_advance(slots[k:], sd, out[k * T * REC:], prm)   # the state is handed on in device memory
            same(pipeline.track_records(out, T), whole)
            same(pipeline.track_state_records(sd), wst)
        for t in (0, 3, 7):                                          # a track alone
            alone, ast = run(ctx, slots, st[t:t + 1], prm)
            same(alone[:, 0], whole[:, t])
            same(ast[0:1], wst[t:t + 1])


def test_a_recycled_slot_orders_the_call_and_the_next_writer():
    w, h, n, T = 256, 256, 16, 4
    a, b = content("noise", n, w, h), content("specks", n, w, h)
    slots = list(range(n))
    st = tk.state(points(w, h, T, 4))
    with context(w, h, mb=16) as ctx:
        da, db = dev(a), dev(b)
        sa, sb = dev(np.frombuffer(st.tobytes(), np.uint8)), dev(np.frombuffer(st.tobytes(), np.uint8))
        oa = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        ob = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        torch.cuda.synchronize()
        prm = {"radius": 32, "cut_threshold": NEVER}
        ctx.import_flows(da, slots)                                 # the writer, the call, the next writer, the next call:
        ctx.track_advance(slots, sa, oa, prm)                       # queued back to back, nothing waits in between
        ctx.import_flows(db, slots)
        ctx.track_advance(slots, sb, ob, prm)
        same(pipeline.track_records(oa, T), tk.advance(a, [False] * n, st, radius=32)[0])
        same(pipeline.track_records(ob, T), tk.advance(b, [False] * n, st, radius=32)[0])
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 2. k_roi_weights ---------------------------------------------------------------------------------------------------------
def centre_sources(cen, T=3):
    """the same n centres as track 0 of a track buffer (stride 48 * T), as ffl_grid_centre records (32) and as (n, 2) (16)"""
    n = len(cen)
    trk = np.zeros((n, T), _capi.TRACK_DTYPE)
    trk["x"], trk["y"] = -123.0, 1e6
    trk["x"][:, 0], trk["y"][:, 0], trk["du"], trk["status"] = cen[:, 0], cen[:, 1], 7.0, 3
    grid = np.zeros(n, _capi.GRID_CENTRE_DTYPE)
    grid["cx"], grid["cy"], grid["total_var"], grid["cells"] = cen[:, 0], cen[:, 1], -7.0, 32
    return [((dev(np.frombuffer(trk.tobytes(), np.uint8)), REC * T), "track"), (dev(np.frombuffer(grid.tobytes(), np.uint8)), "grid"),
            (dev(cen), "plain")]


@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_roi_maps_match_the_restatement(size):
    w, h = size
    rng = np.random.default_rng(w)
    cen = np.array([(w // 2, h // 2), (0.0, 0.0), (w - 1.0, h - 0.5), (w / 3.0, h / 1.7), (-20.0, h / 2.0), (np.nan, 3.0), (1e9, 1e9)],
                   np.float64)
    n = len(cen)
    gate = rng.integers(0, 256, (n, h, w)).astype(np.uint8)
    with context(w, h, mb=8) as ctx:
        for ax, ay, soft in ((6.0, 6.0, 1), (w / 3.0, 2.5, 1), (4.0, h / 2.0, 0), (0.5, 0.5, 0), (32768.0, 32768.0, 1)):
            want = tk.roi_maps(w, h, cen, ax, ay, soft)
            for src, name in centre_sources(cen):
                out = torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV)
                assert ctx.roi_weights(n, src, out, {"ax": ax, "ay": ay, "soft": soft}) is out
                assert np.array_equal(out.cpu().numpy(), want), (name, ax, ay, soft)
            assert not want[5].any() and not want[6].any()          # a NaN centre, a far-away centre
            # a gate per item, one static gate, and the in-place form; a padded out whose gap bytes stay untouched
            prm = _capi.RoiParams(ax=ax, ay=ay, soft=soft)
            big = torch.full((n, h + 2, w + 13), 0x5A, dtype=torch.uint8, device=DEV)
            view = big[:, 1:h + 1, 5:5 + w]
            ctx.roi_weights(n, dev(cen), view, prm, gate=dev(gate))
            assert np.array_equal(view.cpu().numpy(), np.minimum(want, gate))
            host = big.cpu().numpy().copy()
            host[:, 1:h + 1, 5:5 + w] = 0x5A
            assert (host == 0x5A).all()
            ctx.roi_weights(n, dev(cen), view, prm, gate=cbh.padded(gate, DEV)[0])
            assert np.array_equal(view.cpu().numpy(), np.minimum(want, gate[0][None]))
            view.copy_(dev(gate))
            ctx.roi_weights(n, dev(cen), view, prm, gate=view)      # gate = out
            assert np.array_equal(view.cpu().numpy(), np.minimum(want, gate))
            host = big.cpu().numpy().copy()
            host[:, 1:h + 1, 5:5 + w] = 0x5A
            assert (host == 0x5A).all()
        one = torch.full((h, w), 0xA5, dtype=torch.uint8, device=DEV)   # one item, an (H, W) out
        ctx.roi_weights(1, dev(cen[:1]), one)
        assert np.array_equal(one.cpu().numpy(), tk.roi_map(w, h, cen[0], 48.0, 48.0, True))
        assert one.cpu().numpy()[h // 2, w // 2] == 255             # the centre is on a pixel
        assert ctx.graph_stats()["capture_failures"] == 0


def test_roi_reads_the_records_track_advance_wrote():
    w, h, n, T = 67, 35, 5, 3
    f = content("uniform", n, w, h)
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(f), list(range(n)))
        sd = pipeline.track_state(ctx, [(10.0, 20.0), (0.0, 0.0), (66.0, 34.0)])
        buf = pipeline.track_buffer(ctx, n, T)
        ctx.track_advance(list(range(n)), sd, buf, {"radius": 3, "cut_threshold": NEVER})
        out = torch.empty((n, h, w), dtype=torch.uint8, device=DEV)
        ctx.roi_weights(n, (buf, REC * T), out, {"ax": 9.0, "ay": 5.0})   # queued straight behind, nothing waits
        cen = np.array([(10.0 + 1.25 * i, 20.0 - 0.5 * i) for i in range(n)])
        assert np.array_equal(out.cpu().numpy(), tk.roi_maps(w, h, cen, 9.0, 5.0))


# ---- 3. the fifth window form -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def window_ctx():
    w, h, n = 130, 17, 20
    with _capi.Context(w, h, max_batch=32, frame_slots=2, flow_slots=32) as ctx:
        slots = list(range(5, 5 + n))
        fields = np.stack([gr.field(w, h, 100 + i) * np.float32(1 + 0.1 * (i % 5)) for i in range(n)])
        ctx.import_flows(dev(fields), slots)
        order = [int(s) for s in np.random.default_rng(1).permutation(slots)]
        mms = sorted(float(r[3]) for r in ctx.pass1_results(order, 0.0))
        yield ctx, order, (mms[9] + mms[10]) / 2, {s: fields[s - 5] for s in slots}
        assert ctx.graph_stats()["capture_failures"] == 0


def records(buf, n):
    return np.frombuffer(buf.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)


def fifth(ctx, order, first, n, maps, centres, radius, thr, pov=False):
    out = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.radial_window_axes_weighted_centres(order, first, n, maps, centres, out, radius, thr, pov)
    return records(out, n)


@pytest.mark.parametrize("radius", [0, 6, 32])
def test_fifth_form_against_the_restatement_and_its_siblings(window_ctx, radius):
    ctx, order, thr, fields = window_ctx
    w, h, nseq = 130, 17, len(order)
    cen = np.random.default_rng(5 + radius).uniform(-40.0, 200.0, (nseq, 2))
    maps = cbh.pair_maps(w, h, nseq, 3)
    for first, n in ((0, nseq), (3, 9), (nseq - 1, 1)):
        m = maps[first:first + n]
        got = fifth(ctx, order, first, n, dev(m), dev(cen), radius, thr)
        assert n != nseq or got["cut"].sum() == 10
        for i in range(n):
            tk.check_window(got[i], fields[order[first + i]], cen, first + i, m[i], False, radius)
        for src, name in centre_sources(cen):                         # every centre source, contiguous and padded maps: the same bytes
            assert fifth(ctx, order, first, n, cbh.padded(m, DEV), src, radius, thr).tobytes() == got.tobytes(), name
        # an all-ones map: the bits of radial_window_axes_centres
        ones = fifth(ctx, order, first, n, dev(np.ones((h, w), np.uint8)), dev(cen), radius, thr)
        out = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
        ctx.radial_window_axes_centres(order, first, n, dev(cen), out, radius, thr)
        assert ones.tobytes() == records(out, n).tobytes()
    pov = fifth(ctx, order, 0, nseq, dev(maps), dev(cen), radius, BIG, True)
    for i in range(nseq):
        tk.check_window(pov[i], fields[order[i]], cen, i, maps[i], True, radius)


def test_fifth_form_about_the_records_integer_centres_is_the_weighted_form(window_ctx):
    """radius 0 and centres equal to the records' integer (x, y) as doubles: both forms divide by 1, so the centre is the same
    double and the records the same bytes"""
    ctx, order, thr, _ = window_ctx
    w, h, nseq = 130, 17, len(order)
    maps = dev(cbh.pair_maps(w, h, nseq, 9))
    ctx.pass1_weighted(order, maps)                                  # x, y under the maps, as the weighted form reads them
    recs = ctx.pass1_results(order, thr)
    cen = np.array([(float(r[0]), float(r[1])) for r in recs])
    out = torch.full((nseq * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.radial_window_axes_weighted(order, 0, nseq, maps, out, 0, thr)
    want = records(out, nseq)
    assert fifth(ctx, order, 0, nseq, maps, dev(cen), 0, thr).tobytes() == want.tobytes()
    ctx.import_flows(dev(np.stack([gr.field(w, h, 100 + s - 5) * np.float32(1 + 0.1 * ((s - 5) % 5)) for s in order])), order)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
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


def test_track_refusals():
    w, h, T = 67, 35, 2
    INVALID, STATE_ = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    f = content("noise", 4, w, h)
    with _capi.Context(w, h, max_batch=4, frame_slots=2, flow_slots=8) as ctx:
        ctx.import_flows(dev(f), [0, 1, 2, 3])
        st = tk.state([(3.0, 3.0), (40.0, 20.0)])
        before = run(ctx, [0, 1, 2, 3], st, {"radius": 5})
        sd = dev(np.frombuffer(st.tobytes(), np.uint8))
        keep = sd.clone()
        out = torch.full((5 * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        L, hd = ctx.L, ctx._h

        def raw(slots, n_tracks=T, prm=None, wts=None, sptr=None, optr=None, n=None):
            import ctypes as C
            ps, arr = _capi._iarr(slots)
            p = _capi.TrackParams(radius=5) if prm is None else prm
            return lambda: (arr, ctx._chk(L.ffl_track_advance(hd, len(slots) if n is None else n, ps if slots is not None else None,
                                                              n_tracks, C.byref(p), None if wts is None else C.byref(wts),
                                                              sd.data_ptr() if sptr is None else sptr,
                                                              out.data_ptr() if optr is None else optr,
                                                              _capi.stream_handle(None, 0))))

        def refused(match, code, call):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and "ffl_track_advance" in str(e.value)

        refused(r"n = 0 items outside 1\.\.4", INVALID, raw([]))
        refused(r"n = 5 items outside 1\.\.4", INVALID, raw([0, 1, 2, 3, 4]))
        refused(r"n_tracks = 0 outside 1\.\.8", INVALID, raw([0], 0))
        refused(r"n_tracks = 9 outside 1\.\.8", INVALID, raw([0], 9))
        import ctypes as C
        refused(r"NULL flow_slots", INVALID, lambda: ctx._chk(L.ffl_track_advance(hd, 1, None, T, None, None, sd.data_ptr(), out.data_ptr(), 0)))
        refused(r"flow slot 8 out of range", INVALID, raw([8]))
        refused(r"flow slot -1 out of range", INVALID, raw([0, -1]))
        refused(r"flow slot 1 repeated in one call", INVALID, raw([0, 1, 1]))
        refused(r"flow slot 5 holds no flow", STATE_, raw([0, 5]))
        bad = _capi.TrackParams()
        for field, value, match in (("radius", 0, r"radius = 0 outside 1\.\.32"), ("radius", 33, r"radius = 33 outside 1\.\.32"),
                                    ("on_cut", 2, r"on_cut = 2 is neither"), ("cut_threshold", float("nan"), r"cut_threshold is NaN")):
            bad = _capi.TrackParams()
            setattr(bad, field, value)
            refused(match, INVALID, raw([0], prm=bad))
        maps = torch.ones((4, h, w), dtype=torch.uint8, device=DEV)
        refused(r"overlap: weight row pitch 66 below the width 67", INVALID, raw([0], wts=_capi.DevWeights(maps.data_ptr(), h * w, w - 1)))
        refused(r"NULL weight base", INVALID, raw([0], wts=_capi.DevWeights(None, h * w, w)))
        refused(r"NULL state_dev", INVALID, raw([0], sptr=0))
        refused(r"NULL out_dev", INVALID, raw([0], optr=0))
        refused(r"must be 8-byte aligned", INVALID, raw([0], sptr=sd.data_ptr() + 4))
        refused(r"must be 8-byte aligned", INVALID, raw([0], optr=out.data_ptr() + 4))
        refused(r"overlap: state_dev \(96 bytes\) and out_dev \(192 bytes\) share memory", INVALID, raw([0, 1], sptr=out.data_ptr() + 96))
        refused(r"overlap: state_dev", INVALID, raw([0, 1], optr=sd.data_ptr()))
        pin = ctx.pinned_frames(1, channels=1)
        assert pin.size >= T * REC
        refused(r"state_dev is page-locked host memory.*device memory", INVALID, raw([0], sptr=pin.ctypes.data))
        refused(r"out_dev is page-locked host memory.*device memory", INVALID, raw([0], optr=pin.ctypes.data))
        torch.cuda.empty_cache()
        big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)   # an allocation of its own
        refused(rf"out_dev spans {3 * T * REC} bytes, {T * REC} more than its allocation holds", INVALID,
                raw([0, 1, 2], optr=big.data_ptr() + big.numel() - 2 * T * REC))
        refused(rf"state_dev spans {T * STATE} bytes, {STATE} more than its allocation holds", INVALID,
                raw([0], sptr=big.data_ptr() + big.numel() - STATE))
        refused(rf"the weight maps spans {3 * h * w + (h - 1) * w + w} bytes, {h * w} more than its allocation holds", INVALID,
                raw([0, 1, 2, 3], wts=_capi.DevWeights(big.data_ptr() + big.numel() - 3 * h * w, h * w, w)))
        with pytest.raises(ValueError, match="out holds"):
            ctx.track_advance([0, 1], sd, Span(out.data_ptr(), T * REC))
        with pytest.raises(ValueError, match="no whole number"):
            ctx.track_advance([0], Span(sd.data_ptr(), STATE + 8), out)
        with pytest.raises(ValueError, match="not device memory"):
            ctx.track_advance([0], torch.zeros(STATE, dtype=torch.uint8), out)
        with pytest.raises(ValueError, match="2 weight maps for 1 items"):
            ctx.track_advance([0], sd, out, None, maps[:2])
        assert capture_refused(lambda s: ctx.track_advance([0], sd, out, None, None, s)) == [(STATE_, True)]
        # a refused call queues nothing: the sentinels and the state stand, and the context still computes
        assert (out.cpu().numpy() == 0xA5).all() and torch.equal(sd, keep)
        after = run(ctx, [0, 1, 2, 3], st, {"radius": 5})
        same(after[0], before[0])
        same(after[1], before[1])
        same(after[0], tk.advance(f, cuts_of(ctx, [0, 1, 2, 3], 7.0), st, radius=5)[0])
        assert ctx.graph_stats()["capture_failures"] == 0


def test_roi_and_fifth_form_refusals():
    w, h, n = 67, 35, 4
    INVALID, STATE_ = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    import ctypes as C
    with _capi.Context(w, h, max_batch=4, frame_slots=2, flow_slots=8) as ctx:
        f = content("noise", n, w, h)
        ctx.import_flows(dev(f), [0, 1, 2, 3])
        cen = dev(np.array([(10.0, 10.0), (20.0, 5.0), (66.0, 34.0), (33.5, 17.5)]))
        out = torch.full((5, h, w), 0xA5, dtype=torch.uint8, device=DEV)
        gate = torch.full((5, h, w), 200, dtype=torch.uint8, device=DEV)
        L, hd = ctx.L, ctx._h
        od = lambda t=out, item=h * w, pitch=w, off=0: _capi.DevWeights(t.data_ptr() + off, item, pitch)

        def raw(n_=n, ptr=None, stride=16, prm=None, g=None, o=None):
            p = _capi.RoiParams() if prm is None else prm
            o = od() if o is None else o
            return lambda: ctx._chk(L.ffl_roi_weights(hd, n_, cen.data_ptr() if ptr is None else ptr, stride, C.byref(p),
                                                      None if g is None else C.byref(g), C.byref(o), _capi.stream_handle(None, 0)))

        def refused(match, code, call, fn="ffl_roi_weights"):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and fn in str(e.value)

        refused(r"n = 0 items outside 1\.\.4", INVALID, raw(0))
        refused(r"n = 5 items outside 1\.\.4", INVALID, raw(5))
        for field, value, match in (("ax", 0.25, r"half-axes \(0\.25, 48\) outside 0\.5\.\.32768"), ("ay", float("inf"), r"half-axes \(48, inf\)"),
                                    ("ax", float("nan"), r"half-axes \(nan, 48\)"), ("soft", 2, r"soft = 2 is neither")):
            bad = _capi.RoiParams()
            setattr(bad, field, value)
            refused(match, INVALID, raw(prm=bad))
        refused(r"NULL out descriptor", INVALID, lambda: ctx._chk(L.ffl_roi_weights(hd, n, cen.data_ptr(), 16, None, None, None, 0)))
        refused(r"overlap: weight row pitch 66 below the width 67", INVALID, raw(o=od(pitch=w - 1)))
        refused(r"overlap: out item stride 0 with n = 4 maps to write", INVALID, raw(o=od(item=0)))
        refused(r"overlap: weight item stride", INVALID, raw(o=od(item=h * w - 1)))
        refused(r"overlap: weight row pitch", INVALID, raw(g=od(gate, pitch=3)))
        refused(r"overlap: out \(\d+ bytes\) and gate \(\d+ bytes\) share memory, and gate is not exactly out", INVALID,
                raw(g=od(out, off=w)))
        refused(r"gate is not exactly out", INVALID, raw(g=od(out, item=0)))   # the same base, another item stride
        refused(r"NULL centres_dev", INVALID, raw(ptr=0))
        refused(r"centres_dev must be 8-byte aligned", INVALID, raw(ptr=cen.data_ptr() + 4))
        refused(r"centre stride 8: a multiple of 8 bytes, at least 16", INVALID, raw(stride=8))
        refused(r"centre stride 20: a multiple of 8 bytes, at least 16", INVALID, raw(stride=20))
        refused(r"overlap: out \(\d+ bytes\) and the centres \(64 bytes\) share memory", INVALID, raw(ptr=out.data_ptr() + 8 * w))
        pin = ctx.pinned_frames(1, channels=1)
        refused(r"centres_dev is page-locked host memory.*device memory", INVALID, raw(2, ptr=pin.ctypes.data))
        torch.cuda.empty_cache()
        big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)
        refused(rf"centres_dev spans {3 * 48 + 16} bytes, 48 more than its allocation holds", INVALID,
                raw(ptr=big.data_ptr() + big.numel() - 3 * 48 + 32, stride=48))
        refused(r"out spans \d+ bytes, \d+ more than its allocation holds", INVALID,
                raw(o=_capi.DevWeights(big.data_ptr() + big.numel() - 3 * h * w, h * w, w)))
        refused(r"the gate maps spans \d+ bytes, \d+ more than its allocation holds", INVALID,
                raw(g=_capi.DevWeights(big.data_ptr() + big.numel() - 3 * h * w, h * w, w)))
        with pytest.raises(ValueError, match="not device memory"):
            ctx.roi_weights(n, cen, torch.zeros((n, h, w), dtype=torch.uint8))
        with pytest.raises(ValueError, match="3 weight maps for 4 items"):
            ctx.roi_weights(n, cen, out[:3])
        assert capture_refused(lambda s: ctx.roi_weights(n, cen, out[:n], stream=s)) == [(STATE_, True)]
        assert (out.cpu().numpy() == 0xA5).all()                     # nothing was queued
        ctx.roi_weights(n, cen, out[:n], {"ax": 9.0, "ay": 5.0}, gate=gate[0])
        assert np.array_equal(out[:n].cpu().numpy(), tk.roi_maps(w, h, cen.cpu().numpy(), 9.0, 5.0, gate=np.full((h, w), 200, np.uint8)))

        # the fifth form: out_dev is checked first, then the maps, then the centres
        order = [0, 1, 2, 3]
        rec = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
        maps = od(gate)
        ps, arr = _capi._iarr(order)

        def w5(optr=None, wts=maps, cptr=None, stride=16):
            return lambda: ctx._chk(L.ffl_radial_window_axes_weighted_centres(
                hd, n, ps, 0, n, 6, 7.0, 0, None if wts is None else C.byref(wts), cen.data_ptr() if cptr is None else cptr, stride,
                rec.data_ptr() if optr is None else optr, _capi.stream_handle(None, 0)))

        fn5 = "ffl_radial_window_axes_weighted_centres"
        refused(r"NULL out_dev", INVALID, w5(optr=0, wts=None, cptr=0), fn5)
        refused(r"out_dev must be 8-byte aligned", INVALID, w5(optr=rec.data_ptr() + 4, wts=None), fn5)
        refused(r"NULL weight descriptor", INVALID, w5(wts=None, cptr=0), fn5)
        refused(r"overlap: weight row pitch", INVALID, w5(wts=od(gate, pitch=3), cptr=0), fn5)
        refused(r"NULL centres_dev", INVALID, w5(cptr=0), fn5)
        refused(r"centres_dev must be 8-byte aligned", INVALID, w5(cptr=cen.data_ptr() + 4), fn5)
        refused(r"centre stride 12: a multiple of 8 bytes, at least 16", INVALID, w5(stride=12), fn5)
        refused(r"out_dev is page-locked host memory", INVALID, w5(optr=pin.ctypes.data, wts=od(gate, off=0), cptr=pin.ctypes.data), fn5)
        refused(r"the weight maps spans \d+ bytes", INVALID,
                w5(wts=_capi.DevWeights(big.data_ptr() + big.numel() - 3 * h * w, h * w, w), cptr=pin.ctypes.data), fn5)
        refused(r"centres_dev is page-locked host memory", INVALID, w5(cptr=pin.ctypes.data), fn5)
        refused(r"flow slot 5 holds no result", STATE_, lambda: ctx.radial_window_axes_weighted_centres([0, 5], 0, 1, gate[:1], cen[:2], rec), fn5)
        assert capture_refused(lambda s: ctx.radial_window_axes_weighted_centres(order, 0, n, gate[:n], cen, rec, stream=s)) == [(STATE_, True)]
        assert (rec.cpu().numpy() == 0xA5).all()
        got = fifth(ctx, order, 0, n, gate[:n], cen, 6, BIG)
        for i in range(n):
            tk.check_window(got[i], f[i], cen.cpu().numpy(), i, np.full((h, w), 200, np.uint8), False)
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 5. the schedules -----------------------------------------------------------------------------------------------------------
def hand_track(ctx, frames_or_fields, *, track, pov, thr, compensate=None):
    """The chunk with center="track" by hand, on a context that holds it whole (chunk_by_hand's form): the flow call;
    track_advance over all n slots in pair order -- on the raw fields --, then with roi roi_weights; compensate='s fit and
    subtraction; with roi pass1_weighted; ONE window call over the whole chunk.  Returns (post bytes, track bytes, state
    bytes, map bytes or None)."""
    given = not isinstance(frames_or_fields, (list, tuple))
    n = len(frames_or_fields) - (0 if given else 1)
    slots = list(range(n))
    if given:
        ctx.import_flows(frames_or_fields, slots, pov)
    else:
        ctx.upload_frames(0, [np.ascontiguousarray(f) for f in frames_or_fields])
        ctx.flow_pairs(list(range(n)), list(range(1, n + 1)), slots, pov)
    sd = pipeline.track_state(ctx, track["start"], track.get("home"))
    T = sd.numel() // STATE
    buf = torch.full((n * T * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.track_advance(slots, sd, buf, {"radius": track.get("radius", 12), "on_cut": track.get("on_cut", "hold"), "cut_threshold": thr})
    maps = None
    if track.get("roi") is not None:
        maps = torch.full((n, ctx.height, ctx.width), 0xA5, dtype=torch.uint8, device=DEV)
        ctx.roi_weights(n, (buf, REC * T), maps, {"ax": track["roi"][0], "ay": track["roi"][1], "soft": int(track.get("roi_soft", True))},
                        gate=track.get("gate"))
    if compensate is not None:
        mo = pipeline.motion_buffer(ctx, n)
        ctx.motion_fit(slots, _capi.motion_choice(compensate), out=mo)
        ctx.motion_subtract(slots, slots, mo, pov)
    out = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    if maps is not None:
        ctx.pass1_weighted(slots, maps, pov)
        ctx.radial_window_axes_weighted_centres(slots, 0, n, maps, (buf, REC * T), out, cbh.RADIUS, thr, pov)
    else:
        ctx.radial_window_axes_centres(slots, 0, n, (buf, REC * T), out, cbh.RADIUS, thr, pov)
    return (out.cpu().numpy().tobytes(), buf.cpu().numpy().tobytes(), sd.cpu().numpy().tobytes(),
            None if maps is None else maps.cpu().numpy().tobytes())


W_, H_, N_, B_ = 64, 64, 20, 2


@pytest.fixture(scope="module")
def clip():
    return list(sine_translate_frames(N_ + 1, W_, H_, seed=3, zoom=0.02))


@pytest.fixture(scope="module")
def engine_ctx():
    slots = pipeline.min_flow_slots(B_)
    assert slots < N_ and B_ < 2 * pipeline.SMOOTH_RADIUS + 1       # the chunk is longer than the ring, B below the window's span
    with _capi.Context(W_, H_, max_batch=B_, frame_slots=2 * B_ + 2, flow_slots=slots) as ctx:
        yield ctx
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("roi", [None, (20.0, 12.0)], ids=["centres", "roi"])
def test_process_chunk_about_the_track_is_the_by_hand_composition(clip, engine_ctx, roi):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    gate = dev(cbh.random_map(W_, H_, 2)) if roi else None
    track = {"start": [(40.0, 24.0), (5.0, 60.0), (63.0, 0.0)], "home": [(32.0, 32.0)] * 3, "radius": 9, "on_cut": "home", "roi": roi}
    for pov, thr in ((False, 7.0), (True, 0.5)):
        T = torch.empty((N_, H_, W_, 2), device=DEV)
        tout = pipeline.track_buffer(ctx, N_, 3)
        wout = torch.empty((N_, H_, W_), dtype=torch.uint8, device=DEV) if roi else None
        state = pipeline.track_state(ctx, track["start"], track["home"])
        kw = {"weights_out": wout, "weights_gate": gate} if roi else {}
        buf = eng.process_chunk(clip, pov, thr, center="track", track={**{k: v for k, v in track.items() if k not in ("start", "home")},
                                                                       "state": state}, track_out=tout, flows_out=T, **kw)
        assert buf.numel() == N_ * ITEM
        with cbh.hand_context(W_, H_, N_) as one:
            post, trk, st, maps = hand_track(one, clip, track={**track, "gate": gate}, pov=pov, thr=thr)
        assert tout.cpu().numpy().tobytes() == trk and state.cpu().numpy().tobytes() == st
        assert buf.cpu().numpy().tobytes() == post
        if roi:
            assert wout.cpu().numpy().tobytes() == maps
        rec = pipeline.track_records(tout, 3)
        if not pov:                                                   # the track is the restatement's on the exported fields
            cuts = [bool(c) for c in records(buf, N_)["cut"]] if not roi else None
            if cuts is not None:
                want, _ = tk.advance(T.cpu().numpy(), cuts, tk.state(track["start"], track["home"]), radius=9, on_cut=tk.HOME)
                same(rec, want)
        # the same records from the exported fields, with "start" and buffers of the engine's own
        tout2 = pipeline.track_buffer(ctx, N_, 3)
        buf2 = eng.process_flows(T, pov, thr, center="track", track=track, track_out=tout2,
                                 **({"weights_gate": gate} if roi else {}))
        assert tout2.cpu().numpy().tobytes() == trk and buf2.cpu().numpy().tobytes() == post


def test_state_carried_over_two_chunks_and_compensate_leaves_the_track_alone(clip, engine_ctx):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    opts = {"radius": 9, "roi": (20.0, 12.0)}
    start = [(40.0, 24.0), (10.0, 50.0)]
    whole = pipeline.track_buffer(ctx, N_, 2)
    s0 = pipeline.track_state(ctx, start)
    plain = eng.process_chunk(clip, center="track", track={**opts, "state": s0}, track_out=whole)
    # two chunks of 10 pairs that hand the state on
    s1 = pipeline.track_state(ctx, start)
    a, b = pipeline.track_buffer(ctx, 10, 2), pipeline.track_buffer(ctx, 10, 2)
    eng.process_chunk(clip[:11], center="track", track={**opts, "state": s1}, track_out=a)
    eng.process_chunk(clip[10:], center="track", track={**opts, "state": s1}, track_out=b)
    assert a.cpu().numpy().tobytes() + b.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    assert s1.cpu().numpy().tobytes() == s0.cpu().numpy().tobytes()
    assert pipeline.track_state_records(s1)["steps"].tolist() == [N_, N_]
    # compensate=: the track follows the raw field, pass 2 reads the compensated one
    comp = pipeline.track_buffer(ctx, N_, 2)
    got = eng.process_chunk(clip, center="track", track={**opts, "start": start}, track_out=comp, compensate="translation")
    assert comp.cpu().numpy().tobytes() == whole.cpu().numpy().tobytes()
    assert got.cpu().numpy().tobytes() != plain.cpu().numpy().tobytes()
    with cbh.hand_context(W_, H_, N_) as one:
        post, trk, _, _ = hand_track(one, clip, track={**opts, "start": start}, pov=False, thr=7.0, compensate="translation")
    assert got.cpu().numpy().tobytes() == post and comp.cpu().numpy().tobytes() == trk


def test_keywords_and_scripts_about_the_track(clip, engine_ctx):
    ctx, eng = engine_ctx, pipeline.PairEngine(engine_ctx)
    ones = torch.ones((H_, W_), dtype=torch.uint8, device=DEV)
    trk = {"start": (40.0, 24.0), "radius": 9}
    for weights in (ones, "texture", "residual", "consistency"):
        with pytest.raises(ValueError, match=r"center='track' together with weights= .*track=\{'roi'"):
            eng.process_chunk(clip, center="track", track=trk, weights=weights)
    with pytest.raises(ValueError, match=r"center='track' together with weights="):
        eng.process_flows(torch.zeros((2, H_, W_, 2), device=DEV), center="track", track=trk, weights=ones)
    with pytest.raises(ValueError, match="track= and track_out= need center='track'"):
        eng.process_chunk(clip, track=trk)
    with pytest.raises(ValueError, match="needs track="):
        eng.process_chunk(clip, center="track")
    with pytest.raises(ValueError, match="need track\\['roi'\\]"):
        eng.process_chunk(clip, center="track", track=trk, weights_gate=ones)
    with pytest.raises(ValueError, match="grid_out needs center='variance'"):
        eng.process_chunk(clip, center="track", track=trk, grid_out=pipeline.grid_buffer(ctx, N_, 8))
    with pytest.raises(ValueError, match="track_out holds"):
        eng.process_chunk(clip, center="track", track=trk, track_out=pipeline.track_buffer(ctx, N_ - 1, 1))
    with pytest.raises(ValueError, match="together with weights"):                 # the existing words stand
        eng.process_chunk(clip, center="variance", weights=ones)
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 11, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 7.0, "hip_axes": {"roll": "tangential"}, "hip_center": "track",
              "hip_track": {"start": (40.0, 24.0), "radius": 9, "roi": (20.0, 12.0)}}
    plan = pipeline.pair_plan(30.0, len(clip), params)
    assert len(plan) >= 2                                             # the state is carried from chunk to chunk
    state = pipeline.track_state(ctx, (40.0, 24.0))
    want = []
    for chunk in plan:
        buf = eng.process_chunk([clip[i] for i in chunk], False, 7.0, center="track",
                                track={"state": state, "radius": 9, "roi": (20.0, 12.0)})
        want.append(pipeline.post_records(buf, axes=True)[0])
    got = pipeline._frame_chunks(eng, clip, 30.0, params, True)
    assert [c.tobytes() for _, c, _ in got] == [c.tobytes() for c in want]
    scripts = pipeline.frames_to_scripts(eng, clip, 30.0, params)
    assert set(scripts) == {"", "roll"} and all(scripts[k] for k in scripts)
    assert pipeline.frames_to_actions(eng, clip, 30.0, params) == scripts[""]
    fields = []
    for chunk in plan:
        T = torch.empty((len(chunk) - 1, H_, W_, 2), device=DEV)
        eng.process_chunk([clip[i] for i in chunk], flows_out=T)
        fields.append(T)
    assert pipeline.flows_to_scripts(eng, fields, 30.0, len(clip), params) == scripts
