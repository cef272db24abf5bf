"""GPU side of the per-pixel weight maps (ffl_pass1_weighted, ffl_radial_window_axes_weighted),
everything through the C ABI via _capi and on fields placed with import_flows.

An all-ones map is held bit for bit against the unweighted calls; random maps against the restatement tests/weights_ref.py
(the argmax exactly, the mean magnitude in its accepted set, the components within the bound that file derives); integer
fields under integer weights with equality."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import axes_ref as ar
import post_ref as pr
import weights_ref as wr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
ITEM = 80
# 16x16: one wave, partly empty; 130x17: a 2-pixel second strip and a 1-row second row group; 257x40: 9 waves, the last
# workgroup with one wave; 16x16400: 1025 row groups of one strip = 257 workgroups, two trips of the final kernels' loops
SMALL = [(16, 16), (130, 17), (257, 40)]
TALL = (16, 16400)
W, H = 130, 17
PZERO = np.float64(0.0).tobytes()
BIG = 1e30   # a cut threshold nothing reaches
COMPS = ("dot", "tangential", "shift_x", "shift_y")


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def tall_size():
    """16x16400 where the context accepts it (nblk = 257), else 3840x2160 (nblk = 1013), as the axes tests use"""
    try:
        with _capi.Context(*TALL, max_batch=1, frame_slots=2, flow_slots=1):
            return TALL
    except _capi.FFLError:
        return (3840, 2160)


def sizes():
    return SMALL + ["tall"]


def resolve(size):
    return tall_size() if size == "tall" else size


def sid(s):
    return s if isinstance(s, str) else gid(s)


def context(w, h, mb=8, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=slots or 2 * mb)


@functools.lru_cache(maxsize=None)
def field(w, h, seed):
    """a smooth background with noise on top, both components of order 1"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 4).astype(np.float32)
    f = (rng.standard_normal((h, w, 2)) * 0.6).astype(np.float32)
    f[..., 0] += 2.0 * np.sin(x * np.float32(0.011) + ph[0]) * np.cos(y * np.float32(0.017) + ph[1])
    f[..., 1] += 1.5 * np.cos(x * np.float32(0.013) + ph[2]) * np.sin(y * np.float32(0.007) + ph[3])
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def random_map(w, h, seed):
    """random 1..255 with about a third zeros"""
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    m[rng.random((h, w)) < 1 / 3] = 0
    m.setflags(write=False)
    return m


def rec_bytes(recs):
    """pass1_results tuples as comparable bytes (a NaN equals itself)"""
    return [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in recs]


def axes_records(t, n):
    return np.frombuffer(t.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)


def window_w(ctx, seq, first, n, maps, radius=1, thr=BIG, pov=False):
    out = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
    out.fill_(0xA5)
    ctx.radial_window_axes_weighted(list(seq), first, n, maps, out, radius, thr, pov)
    return axes_records(out, n)


def window_plain(ctx, seq, first, n, radius=1, thr=BIG, pov=False):
    out = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
    out.fill_(0xA5)
    ctx.radial_window_axes(list(seq), first, n, out, radius, thr, pov)
    return axes_records(out, n)


def comps_of(rec, i):
    return [rec[k][i] for k in COMPS]


# ---- 1. an all-ones map: today's bits ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sizes(), ids=sid)
def test_all_ones_map_gives_the_unweighted_bits(size):
    w, h = resolve(size)
    n = 3
    fields = np.stack([field(w, h, 10 * w + i) for i in range(n)])
    shared, each = dev(np.ones((h, w), np.uint8)), dev(np.ones((n, h, w), np.uint8))
    seq = list(range(n))
    with context(w, h, mb=4) as ctx:
        for pov in (False, True):
            ctx.import_flows(dev(fields), seq, pov)
            before = rec_bytes(ctx.pass1_results(seq, 1.0))
            plain = window_plain(ctx, seq, 0, n, 1, 1.0, pov).tobytes()
            for maps in (shared, each, each.bool()):
                ctx.import_flows(dev(fields), seq, pov)
                ctx.pass1_weighted(seq, maps, pov)
                assert rec_bytes(ctx.pass1_results(seq, 1.0)) == before
                assert window_w(ctx, seq, 0, n, maps, 1, 1.0, pov).tobytes() == plain
            assert window_w(ctx, seq, 0, n, shared, 1, BIG, pov).tobytes() == window_plain(ctx, seq, 0, n, 1, BIG, pov).tobytes()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 2. random maps against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("size", sizes(), ids=sid)
def test_random_maps_match_the_restatement(size, capsys):
    w, h = resolve(size)
    n = 3
    fields = [field(w, h, 20 * w + i) for i in range(n)]
    maps = [random_map(w, h, 7 * w + i) for i in range(n)]
    seq = list(range(n))
    worst = 0.0
    with context(w, h, mb=4) as ctx:
        ctx.import_flows(dev(np.stack(fields)), seq)
        for pov in (False, True):
            ctx.pass1_weighted(seq, dev(np.stack(maps)), pov)
            got = ctx.pass1_results(seq, 1.0)
            for (x, y, d, mm, cut), f, m in zip(got, fields, maps):
                ex, ey, ed, mean, ecut = wr.pass1_record(f, m, pov, 1.0)
                assert (x, y) == (ex, ey) and np.float32(d).tobytes() == np.float32(ed).tobytes()
                wr.check_mean_mag(mm, f, m)
                assert cut == bool(np.float32(mm) > np.float32(1.0))
            rec = window_w(ctx, seq, 0, n, dev(np.stack(maps)), 1, BIG, pov)
            assert [(r["x"], r["y"]) for r in rec] == [(g[0], g[1]) for g in got]
            assert rec["mean_mag"].tobytes() == np.asarray([g[3] for g in got], np.float32).tobytes()
            for i, (f, m) in enumerate(zip(fields, maps)):
                worst = max(worst, wr.check_axes(comps_of(rec, i), f, (rec["cx"][i], rec["cy"][i]), m, pov))
            # one map for all items
            ctx.pass1_weighted(seq, dev(maps[0]), pov)
            for (x, y, d, mm, cut), f in zip(ctx.pass1_results(seq, 1.0), fields):
                ex, ey, ed, _, _ = wr.pass1_record(f, maps[0], pov, 1.0)
                assert (x, y) == (ex, ey) and np.float32(d).tobytes() == np.float32(ed).tobytes()
                wr.check_mean_mag(mm, f, maps[0])
            rec = window_w(ctx, seq, 0, n, dev(maps[0]), 0, BIG, pov)
            worst = max(worst, wr.check_axes(comps_of(rec, 2), fields[2], (rec["cx"][2], rec["cy"][2]), maps[0], pov))
    with capsys.disabled():
        print(f"\n  {w}x{h}: worst weighted component error {worst:.2f} u*S, bound {pr.radial_depth(w, h)}")


# ---- 3. known answers: equality ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SMALL, ids=gid)
def test_known_answers_are_exact(size):
    """POV mode, radius 0: the centre of a record is its own (w // 2, h - 1), an integer; integer fields, integer weights."""
    w, h = size
    centre = (w // 2, h - 1)
    known = ar.known_fields(w, h, centre)
    names = list(known)
    seq = list(range(len(names)))
    maps = np.stack([random_map(w, h, 40 + i) for i in seq])
    with context(w, h) as ctx:
        ctx.import_flows(dev(np.stack([known[k][0] for k in names])), seq, True)
        ones = window_w(ctx, seq, 0, len(seq), dev(np.ones((h, w), np.uint8)), 0, BIG, True)
        ctx.pass1_weighted(seq, dev(maps), True)
        rec = window_w(ctx, seq, 0, len(seq), dev(maps), 0, BIG, True)
        for i, name in enumerate(names):
            assert (rec["cx"][i], rec["cy"][i]) == centre and not rec["cut"][i]
            assert comps_of(ones, i) == known[name][1], (name, comps_of(ones, i), known[name][1])
            want = wr.known_weighted(known[name][0], centre, maps[i])
            assert comps_of(rec, i) == want, (name, comps_of(rec, i), want)


# ---- 4. non-finite values -----------------------------------------------------------------------------------------------------
def test_non_finite_values_outside_the_map_are_invisible():
    f = np.stack([field(W, H, 60 + i) for i in range(2)]).copy()
    maps = np.stack([random_map(W, H, 50 + i) for i in range(2)]).copy()
    maps[maps == 0] = 3                       # zeros only in the block below
    maps[:, 3:14, 40:61] = 0
    bad = f.copy()
    for (y, x, c), v in {(8, 50, 0): np.nan, (8, 51, 1): np.inf, (7, 50, 0): -np.inf, (10, 57, 1): np.nan, (6, 43, 0): np.inf}.items():
        assert (maps[:, y - 2:y + 3, x - 2:x + 3] == 0).all()            # at least two pixels from any W > 0
        bad[:, y, x, c] = v
    clean = np.where(np.isfinite(bad), bad, np.float32(0))
    seq = [0, 1]
    with context(W, H) as ctx:
        out = {}
        for name, fl in (("bad", bad), ("clean", clean)):
            for pov in (False, True):
                ctx.import_flows(dev(fl), seq, pov)
                ctx.pass1_weighted(seq, dev(maps), pov)
                out[name, pov] = (rec_bytes(ctx.pass1_results(seq, 1.0)), window_w(ctx, seq, 0, 2, dev(maps), 1, BIG, pov).tobytes())
        for pov in (False, True):
            assert out["bad", pov] == out["clean", pov]
            assert not np.isnan(np.frombuffer(out["bad", pov][1], _capi.PASS2_AXES_DTYPE)["dot"]).any()
        # a NaN under W > 0 follows the unweighted rule: the first NaN of |div| among the candidates, a NaN mean, never a cut
        g = f.copy()
        g[0, 9, 70, 0] = np.nan               # u: div is NaN at (70, 8) and (70, 10); the pixel's own magnitude is NaN
        ctx.import_flows(dev(g), seq)
        ctx.pass1_weighted(seq, dev(maps))
        (x, y, d, mm, cut), other = ctx.pass1_results(seq, 1.0)
        assert (x, y) == wr.argmax_weighted(g[0], maps[0])[:2] == (70, 8) and math.isnan(d) and math.isnan(mm) and not cut
        assert rec_bytes([other]) == [out["clean", False][0][1]]
        rec = window_w(ctx, seq, 0, 2, dev(maps), 0, 1.0)
        assert not rec["cut"][0] and np.isnan([rec[k][0] for k in ("dot", "tangential", "shift_x")]).all() and math.isfinite(rec["shift_y"][0])
        wr.check_axes(comps_of(rec, 0), g[0], (rec["cx"][0], rec["cy"][0]), maps[0], False)


# ---- 5. the empty map -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (130, 17)], ids=gid)
def test_empty_map(size):
    w, h = size
    fields = np.stack([field(w, h, 70 + i) for i in range(3)]).copy()
    fields[2, 1, 1] = np.nan                                              # invisible under an empty map
    maps = np.stack([np.zeros((h, w), np.uint8), random_map(w, h, 3), np.zeros((h, w), np.uint8)])
    seq = [0, 1, 2]
    with context(w, h) as ctx:
        for pov in (False, True):
            ctx.import_flows(dev(fields), seq, pov)
            ctx.pass1_weighted(seq, dev(maps), pov)
            got = ctx.pass1_results(seq, 0.0)
            for i in (0, 2):
                x, y, d, mm, cut = got[i]
                assert (x, y) == (w // 2, h // 2) and cut is False and np.float32(d).tobytes() == np.float32(mm).tobytes() == np.float32(0).tobytes()
            x, y, d, mm, cut = got[1]
            assert (x, y) == wr.pass1_record(fields[1], maps[1], pov)[:2]
            rec = window_w(ctx, seq, 0, 3, dev(maps), 0, BIG, pov)
            for i in (0, 2):
                assert np.frombuffer(rec[i:i + 1].tobytes(), np.uint8)[48:].tobytes() == PZERO * 4 and rec["dot"][i].tobytes() == PZERO
                assert (rec["x"][i], rec["y"][i], rec["cx"][i], rec["cy"][i]) == (w // 2, h // 2, w // 2, h // 2)
                assert rec["mean_mag"][i].tobytes() == np.float32(0).tobytes()
            wr.check_axes(comps_of(rec, 1), fields[1], (rec["cx"][1], rec["cy"][1]), maps[1], pov)
            # an empty shared map under ordinary records
            ctx.import_flows(dev(fields[:2]), [0, 1], pov)
            rec = window_w(ctx, [0, 1], 0, 2, dev(np.zeros((h, w), bool)), 0, BIG, pov)
            assert all(np.frombuffer(rec[i:i + 1].tobytes(), np.uint8)[48:].tobytes() == PZERO * 4 and
                       rec["dot"][i].tobytes() == PZERO for i in (0, 1))


def test_empty_map_cut_rule():
    """rule W5: cut = 0, through ffl_pass1_results and the window's own test alike, for any finite threshold >= 0"""
    with context(16, 16) as ctx:
        ctx.import_flows(dev(field(16, 16, 1)[None]), [0])
        ctx.pass1_weighted([0], dev(np.zeros((16, 16), np.uint8)))
        assert ctx.pass1_results([0], 0.0)[0][4] is False
        assert window_w(ctx, [0], 0, 1, dev(np.zeros((16, 16), np.uint8)), 0, 0.0)["cut"][0] == 0


# ---- 6. views --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(130, 17), (257, 40)], ids=gid)
def test_maps_as_views_into_a_larger_tensor(size):
    w, h = size
    n = 3
    fields = np.stack([field(w, h, 80 + i) for i in range(n)])
    maps = np.stack([random_map(w, h, 60 + i) for i in range(n)]).copy()
    maps[:, :, [0, -1]] = 0                                               # zeros where a read past a row would find 255
    maps[:, [0, -1], :] = 0
    pitch, off = w + 5, 3
    item = h * pitch + 7
    assert item % 4 and off % 2 and pitch > w
    buf = torch.full((off + n * item + 64,), 255, dtype=torch.uint8, device=DEV)
    view = torch.as_strided(buf, (n, h, w), (item, pitch, 1), off)
    view.copy_(dev(maps))
    assert int((buf == 255).sum()) >= buf.numel() - n * h * w
    seq = list(range(n))
    with context(w, h, mb=4) as ctx:
        for pov in (False, True):
            res = []
            for m in (dev(maps), view):
                ctx.import_flows(dev(fields), seq, pov)
                ctx.pass1_weighted(seq, m, pov)
                res.append((rec_bytes(ctx.pass1_results(seq, 1.0)), window_w(ctx, seq, 0, n, m, 1, BIG, pov).tobytes()))
            assert res[1] == res[0]
            # a static map as a view with a padded pitch and an odd base
            ctx.pass1_weighted(seq, view[1], pov)
            a = (rec_bytes(ctx.pass1_results(seq, 1.0)), window_w(ctx, seq, 0, n, view[1], 1, BIG, pov).tobytes())
            ctx.pass1_weighted(seq, dev(maps[1]), pov)
            assert a == (rec_bytes(ctx.pass1_results(seq, 1.0)), window_w(ctx, seq, 0, n, dev(maps[1]), 1, BIG, pov).tobytes())


# ---- 7. the window form -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def field_ctx():
    """13 fields in slots 3..15 of a 130x17 context, their records under 13 random maps"""
    with _capi.Context(W, H, max_batch=16, frame_slots=2, flow_slots=24) as ctx:
        slots = list(range(3, 16))
        ctx.import_flows(dev(np.stack([field(W, H, 50 + i) for i in range(13)])), slots)
        maps = dev(np.stack([random_map(W, H, 50 + i) for i in range(13)]))
        ctx.pass1_weighted(slots, maps)
        yield ctx, maps
        assert ctx.graph_stats()["capture_failures"] == 0


def test_window_form(field_ctx):
    ctx, maps = field_ctx
    order = [9, 4, 15, 3, 12, 7, 5, 14, 8, 6, 13, 10, 11]                  # seq position -> slot; slot s has map s - 3
    recs = ctx.pass1_results(order, 0.0)
    mms = sorted(float(r[3]) for r in recs)
    thr = (mms[5] + mms[6]) / 2                                           # cuts about half of the items
    assert mms[5] < thr < mms[6]
    recs = ctx.pass1_results(order, thr)
    assert sum(r[4] for r in recs) == 7
    per_pos = maps[[s - 3 for s in order]]                                # maps in seq order
    for radius in (0, 6, 32):
        cen = pipeline.smooth_centers([(r[0], r[1]) for r in recs], radius)
        for first, n in ((0, 13), (0, 1), (12, 1), (0, 5), (8, 5), (6, 1)):  # both clipped ends and the middle
            rec = window_w(ctx, order, first, n, per_pos[first:first + n], radius, thr)
            assert np.stack([rec["cx"], rec["cy"]], axis=1).tobytes() == np.ascontiguousarray(cen[first:first + n]).tobytes()
            for i in range(n):
                x, y, d, mm, cut = recs[first + i]
                assert (rec["x"][i], rec["y"][i], bool(rec["cut"][i]), rec["pad"][i]) == (x, y, cut, 0)
                assert rec["mean_mag"][i].tobytes() == np.float32(mm).tobytes() and rec["div_val"][i].tobytes() == np.float32(d).tobytes()
                assert rec["reserved"][i].tobytes() == PZERO
                if cut:
                    assert b"".join(np.float64(v).tobytes() for v in comps_of(rec, i)) == PZERO * 4
                # the same item in a call of its own
                solo = window_w(ctx, order, first + i, 1, per_pos[first + i:first + i + 1], radius, thr)
                assert solo.tobytes() == rec[i:i + 1].tobytes()
    # an uncut item against the restatement at the window's centre
    rec = window_w(ctx, order, 0, 13, per_pos, 6, BIG)
    m = per_pos.cpu().numpy()
    for i in (0, 6, 12):
        wr.check_axes(comps_of(rec, i), field(W, H, 50 + order[i] - 3), (rec["cx"][i], rec["cy"][i]), m[i], False)


# ---- 8. a later writer restores an ordinary record ------------------------------------------------------------------------------
def test_a_later_import_restores_the_record():
    f = dev(np.stack([field(W, H, 90), field(W, H, 91)]))
    with context(W, H) as ctx:
        for pov in (False, True):
            ctx.import_flows(f, [0, 1], pov)
            first = rec_bytes(ctx.pass1_results([0, 1], 1.0))
            ctx.pass1_weighted([0, 1], dev(random_map(W, H, 9)), pov)
            assert rec_bytes(ctx.pass1_results([0, 1], 1.0)) != first
            ctx.import_flows(f, [0, 1], pov)
            assert rec_bytes(ctx.pass1_results([0, 1], 1.0)) == first
            ctx.pass1_weighted([1], dev(random_map(W, H, 9)), pov)
            ctx.upload_flow(1, field(W, H, 91), pov)
            assert rec_bytes(ctx.pass1_results([0, 1], 1.0)) == first


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals(field_ctx):
    ctx, maps = field_ctx
    slots = list(range(3, 16))
    INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    before = rec_bytes(ctx.pass1_results(slots, 1.0))
    out = torch.empty(13 * ITEM, dtype=torch.uint8, device=DEV)
    one = maps[0]

    def refused(match, code, call, fn):
        with pytest.raises(_capi.FFLError, match=match) as e:
            call()
        assert e.value.code == code and fn in str(e.value)

    p1 = lambda s, m, stream=None: (lambda: ctx.pass1_weighted(s, m, stream=stream))
    win = lambda s, first, n, m, o=out, stream=None: (lambda: ctx.radial_window_axes_weighted(s, first, n, m, o, stream=stream))
    pin = ctx.pinned_frames(1, channels=1)
    assert pin.size >= W * H
    host = _capi.DevWeights(pin.ctypes.data, 0, W)
    torch.cuda.empty_cache()
    big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)           # an allocation of its own
    past = _capi.DevWeights(big.data_ptr() + big.numel() - 2 * W * H, W * H, W)   # room for two maps, three asked for
    for fn, mk in (("ffl_pass1_weighted", lambda d, n=3: p1(slots[:n], d)),
                   ("ffl_radial_window_axes_weighted", lambda d, n=3: win(slots, 0, n, d))):
        refused(r"the weight maps is page-locked host memory.*device memory", INVALID, mk(host), fn)
        refused(rf"the weight maps spans {3 * W * H} bytes, {W * H} more than its allocation holds", INVALID, mk(past), fn)
        refused(r"overlap: weight row pitch 129 below the width 130", INVALID, mk(_capi.DevWeights(one.data_ptr(), 0, W - 1)), fn)
        refused(r"NULL weight base", INVALID, mk(_capi.DevWeights(0, 0, W)), fn)
    refused(r"flow slot 2 holds no flow", STATE, p1([2, 3], one), "ffl_pass1_weighted")
    refused(r"flow slot 16 holds no flow", STATE, p1([16], one), "ffl_pass1_weighted")
    for _ in range(2):
        refused(r"flow slot 5 repeated in one call", INVALID, p1([4, 5, 5], one), "ffl_pass1_weighted")
    refused(r"flow slot 24 out of range", INVALID, p1([24], one), "ffl_pass1_weighted")
    refused(r"n = 0 slots outside 1\.\.16", INVALID, p1([], one), "ffl_pass1_weighted")
    refused(r"n = 17 slots outside 1\.\.16", INVALID, p1(list(range(17)), one), "ffl_pass1_weighted")
    refused(r"flow slot 2 holds no result", STATE, win([2, 3, 4], 1, 1, one), "ffl_radial_window_axes_weighted")
    refused(r"flow slot 5 repeated", INVALID, win([4, 5, 5], 0, 1, one), "ffl_radial_window_axes_weighted")
    with pytest.raises(ValueError, match="2 weight maps for 3 items"):
        ctx.pass1_weighted(slots[:3], maps[:2])
    with pytest.raises(ValueError, match="2 weight maps for 3 items"):
        ctx.radial_window_axes_weighted(slots, 0, 3, maps[:2], out)
    with pytest.raises(ValueError, match="not device memory"):
        ctx.pass1_weighted(slots[:1], torch.ones((H, W), dtype=torch.uint8))
    x = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    codes = []
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        for call in (p1(slots[:1], one, torch.cuda.current_stream()), win(slots, 0, 1, one, out, torch.cuda.current_stream())):
            try:
                call()
            except _capi.FFLError as err:
                codes.append((err.code, "capturing" in str(err)))
        x += 1
    g.replay()
    torch.cuda.synchronize()
    assert codes == [(STATE, True)] * 2 and float(x.sum()) == 16.0
    # nothing was queued: the records are what they were, and the context computes correct calls next
    assert rec_bytes(ctx.pass1_results(slots, 1.0)) == before
    a = window_w(ctx, slots, 0, 13, maps, 6, BIG)
    ctx.pass1_weighted(slots, maps)
    assert rec_bytes(ctx.pass1_results(slots, 1.0)) == before and window_w(ctx, slots, 0, 13, maps, 6, BIG).tobytes() == a.tobytes()


# ---- 10. the engine and the scripts ---------------------------------------------------------------------------------------------
def engine_ctx(w, h, B):
    return _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2))


def test_pipeline_static_and_per_pair_maps():
    w, h, B, n = 64, 48, 4, 11
    T = dev(np.stack([field(w, h, 200 + i) for i in range(n)]))
    m = random_map(w, h, 5)
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        for pov, thr in ((False, 7.0), (True, 1.5)):
            a = eng.process_flows(T, pov, thr, weights=dev(m))
            assert a.numel() == n * ITEM
            b = eng.process_flows(T, pov, thr, weights=dev(np.stack([m] * n)))
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
            comps, recs = pipeline.post_records(a, axes=True)
            # the schedule's records are pass1_weighted's and its windows smooth_centers'
            with context(w, h, mb=16) as one:
                one.import_flows(T, list(range(n)), pov)
                one.pass1_weighted(list(range(n)), dev(m), pov)
                want = one.pass1_results(list(range(n)), thr)
            assert rec_bytes(recs) == rec_bytes(want)
            rec = axes_records(a, n)
            cen = pipeline.smooth_centers([(r[0], r[1]) for r in want])
            assert np.stack([rec["cx"], rec["cy"]], axis=1).tobytes() == np.ascontiguousarray(cen).tobytes()
            for j in [i for i, r in enumerate(want) if not r[4]][:2]:
                wr.check_axes(comps[j], T[j].cpu().numpy(), cen[j], m, pov)
            for j in [i for i, r in enumerate(want) if r[4]]:
                assert comps[j].tobytes() == PZERO * 4
        # per-pair maps that differ: pair j under its own map
        maps = np.stack([random_map(w, h, 300 + i) for i in range(n)])
        c = eng.process_flows(T, False, BIG, weights=dev(maps))
        comps, recs = pipeline.post_records(c, axes=True)
        for j in (0, 5, 10):
            assert recs[j][:2] == wr.pass1_record(T[j].cpu().numpy(), maps[j])[:2]
        with pytest.raises(ValueError, match="3 maps for a chunk of 11 pairs"):
            eng.process_flows(T, weights=dev(maps[:3]))
        assert ctx.graph_stats()["capture_failures"] == 0


def test_scripts_under_an_all_ones_map_and_frames():
    w, h, B, n = 64, 48, 4, 11
    fr = list(sine_translate_frames(n + 1, w, h, seed=5))
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 7.0, "hip_axes": {"roll": "tangential"}}
    ones = np.ones((h, w), np.uint8)
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        T = torch.empty((n, h, w, 2), device=DEV)
        eng.process_chunk(fr, flows_out=T)
        want = pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, params)
        assert want[""] and want["roll"]
        assert pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**params, "hip_weights": ones}) == want
        assert pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**params, "hip_weights": torch.ones((h, w), dtype=torch.bool)}) == want
        assert pipeline.flows_to_actions(eng, [T], 30.0, n + 1, {**params, "hip_weights": ones}) == want[""]
        assert pipeline.frames_to_scripts(eng, fr, 30.0, {**params, "hip_weights": ones}) == want
        assert pipeline.frames_to_actions(eng, fr, 30.0, {**params, "hip_weights": dev(ones)}) == want[""]
        # frames and weights: the chunk's flow is untouched
        T2 = torch.empty((n, h, w, 2), device=DEV)
        m = random_map(w, h, 8)
        buf = eng.process_chunk(fr, flows_out=T2, weights=dev(m))
        assert torch.equal(T, T2)
        assert buf.cpu().numpy().tobytes() == eng.process_flows(T, weights=dev(m)).cpu().numpy().tobytes()
        with pytest.raises(ValueError, match=r"hip_weights: shape \(64, 48\) is not \(H, W\) = \(48, 64\)"):
            pipeline.flows_to_actions(eng, [T], 30.0, n + 1, {**params, "hip_weights": ones.T})
        with pytest.raises(ValueError, match="hip_weights: dtype torch.float32"):
            pipeline.flows_to_actions(eng, [T], 30.0, n + 1, {**params, "hip_weights": ones.astype(np.float32)})
        assert ctx.graph_stats()["capture_failures"] == 0


def test_half_masks_separate_expansion_from_contraction():
    """the left half expands about its own centre, the right half contracts about its own: under POV mode the radial
    component of an expansion about the centre of the masked region is positive about ANY centre (the cross term vanishes)"""
    w, h, B, n = 64, 48, 4, 5
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    f = np.empty((h, w, 2), np.float32)
    left = x < w // 2
    f[..., 0] = np.where(left, x - (w // 2 - 1) / 2, -(x - (w // 2 + (w // 2 - 1) / 2))) * np.float32(0.05)
    f[..., 1] = np.where(left, y - (h - 1) / 2, -(y - (h - 1) / 2)) * np.float32(0.05)
    T = dev(np.stack([f] * n))
    lm, rm = np.zeros((h, w), np.uint8), np.zeros((h, w), np.uint8)
    lm[:, :w // 2], rm[:, w // 2:] = 255, 1
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        cl, rl = pipeline.post_records(eng.process_flows(T, True, 7.0, weights=dev(lm)), axes=True)
        cr, rr = pipeline.post_records(eng.process_flows(T, True, 7.0, weights=dev(rm)), axes=True)
        assert not any(r[4] for r in rl + rr)
        assert (cl[:, 0] > 0).all() and (cr[:, 0] < 0).all()
