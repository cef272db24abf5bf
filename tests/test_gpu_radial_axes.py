"""GPU side of the four motion components (ffl_radial_axes, ffl_radial_window_axes), everything through
the C ABI via _capi and on fields placed with import_flows.

Component 0 and the 48-byte head of a record are held bit for bit against ffl_radial / ffl_radial_window on the same context
and slots; components 1..3 against the exact sums of tests/axes_ref.py within the bound that file derives, and against
closed forms with equality where every term is an integer."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import axes_ref as ar
import post_ref as pr
from funscript_flow_amd import _capi, pipeline, postchain
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
ITEM, ITEM1 = 80, 48
# 16x16: one wave, partly empty; 130x17: two strips (the second 2 pixels wide) x two row groups (the second 1 row); 257x40:
# 3 strips x 3 row groups = 9 waves, 3 workgroups, the last with one wave
SIZES = [(16, 16), (130, 17), (257, 40)]
W, H = 130, 17
PZERO = np.float64(0.0).tobytes()


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def context(w, h, mb=8, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=slots or 2 * mb)


def field(w, h, seed):
    """a smooth background with noise on top, both components of order 1"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 4).astype(np.float32)
    f = (rng.standard_normal((h, w, 2)) * 0.6).astype(np.float32)
    f[..., 0] += 2.0 * np.sin(x * np.float32(0.011) + ph[0]) * np.cos(y * np.float32(0.017) + ph[1])
    f[..., 1] += 1.5 * np.cos(x * np.float32(0.013) + ph[2]) * np.sin(y * np.float32(0.007) + ph[3])
    return f


def centres(w, h):
    """inside, on a pixel, on the borders, outside"""
    return [(0.37 * w + 0.25, 0.41 * h + 0.5), (float(w // 3), float(h // 4)), (0.0, 0.0), (w - 1.0, h - 1.0),
            (float(w // 2), h - 1.0), (-7.5, -3.25), (w + 4.5, h + 9.0)]


def axes_records(t, n):
    return np.frombuffer(t.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)


# ---- every component against its exact sum ------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_components_within_derived_bound(size, capsys):
    w, h = size
    fields = [field(w, h, 10 * w + i) for i in range(3)]
    cen = centres(w, h)
    worst = 0.0
    with context(w, h) as ctx:
        ctx.import_flows(dev(np.stack(fields)), [0, 1, 2])
        for pov in (False, True):
            for s, f in enumerate(fields):
                got = ctx.radial_axes([s] * len(cen), cen, [False] * len(cen), pov)
                assert got.shape == (len(cen), 4) and got.dtype == np.float64
                one = ctx.radial([s] * len(cen), cen, [False] * len(cen), pov)
                assert got[:, 0].tobytes() == np.asarray(one, np.float64).tobytes()      # the bits of ffl_radial
                for c, g in zip(cen, got):
                    worst = max(worst, ar.check_axes(g, f, c, pov))
            # the three fields in one call, each at its own centre: items do not see one another
            mixed = ctx.radial_axes([2, 0, 1], cen[:3], [False] * 3, pov)
            for s, c, g in zip((2, 0, 1), cen[:3], mixed):
                assert g.tobytes() == ctx.radial_axes([s], [c], [False], pov)[0].tobytes()
    with capsys.disabled():
        print(f"\n  {w}x{h}: worst error of components 1..3 {worst:.2f} u*S, bound {pr.radial_depth(w, h)}")


def test_components_at_3840x2160(capsys):
    """nblk = 1013 workgroups per item: the final kernel's loop makes 4 trips over each component's partials, and five items
    lie 4 * 1013 partials apart in the scratch.  Five fields in one call; the last one -- the deepest in the scratch -- is
    held against its exact sums (seconds of host time each), and every item against the same item alone and ffl_radial."""
    w, h = 3840, 2160
    assert -(-(-(-w // 128) * -(-h // 16)) // 4) == 1013
    base = field(w, h, 1)
    fields = [base[::-1], base[:, ::-1], base * np.float32(-0.5), base + np.float32(0.25), base]
    cen = [(1280.0, 540.0), (0.0, 0.0), (w + 4.5, -9.0), (w - 1.0, h - 1.0), (0.37 * w + 0.25, 0.41 * h + 0.5)]
    with context(w, h, mb=5) as ctx:
        for s, f in enumerate(fields):
            ctx.import_flows(dev(f[None]), [s])
        got = ctx.radial_axes(list(range(5)), cen, [False] * 5)
        one = ctx.radial(list(range(5)), cen, [False] * 5)
        assert got[:, 0].tobytes() == np.asarray(one, np.float64).tobytes()
        for s in (0, 3, 4):
            assert ctx.radial_axes([s], [cen[s]], [False])[0].tobytes() == got[s].tobytes()
        pov = ctx.radial_axes([4, 2], [cen[4], cen[2]], [False] * 2, True)
        assert pov[:, 0].tobytes() == np.asarray(ctx.radial([4, 2], [cen[4], cen[2]], [False] * 2, True), np.float64).tobytes()
    worst = ar.check_axes(got[4], base, cen[4], False)
    with capsys.disabled():
        print(f"\n  {w}x{h}: worst error of components 1..3 {worst:.2f} u*S, bound {pr.radial_depth(w, h)}")


# ---- the window form: ffl_radial_window's bytes, ffl_radial_axes' bits --------------------------------------------------------
@pytest.fixture(scope="module")
def field_ctx():
    """13 fields in slots 3..15 of a 130x17 context"""
    with _capi.Context(W, H, max_batch=16, frame_slots=2, flow_slots=24) as ctx:
        ctx.import_flows(dev(np.stack([field(W, H, 50 + i) for i in range(13)])), list(range(3, 16)))
        yield ctx
        assert ctx.graph_stats()["capture_failures"] == 0


def window_pair(ctx, seq, first, n, radius, thr=7.0, pov=False):
    """(axes records, plain records) of the same call"""
    a = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
    b = torch.empty(n * ITEM1, dtype=torch.uint8, device=DEV)
    a.fill_(0xA5)
    ctx.radial_window_axes(list(seq), first, n, a, radius, thr, pov)
    ctx.radial_window(list(seq), first, n, b, radius, thr, pov)
    return axes_records(a, n), np.frombuffer(b.cpu().numpy().tobytes(), _capi.PASS2_DTYPE, n)


def assert_window(ctx, seq, first, n, radius, thr=7.0, pov=False):
    rec, plain = window_pair(ctx, seq, first, n, radius, thr, pov)
    raw = np.frombuffer(rec.tobytes(), np.uint8).reshape(n, ITEM)
    assert raw[:, :ITEM1].tobytes() == plain.tobytes()                      # the first 48 bytes: ffl_radial_window's
    assert rec["reserved"].tobytes() == PZERO * n                           # +0.0
    items = [seq[first + i] for i in range(n)]
    want = ctx.radial_axes(items, np.stack([rec["cx"], rec["cy"]], axis=1), rec["cut"] != 0, pov)
    got = np.stack([rec["dot"], rec["tangential"], rec["shift_x"], rec["shift_y"]], axis=1)
    assert got.tobytes() == want.tobytes()                                  # the bits of ffl_radial_axes at (cx, cy)
    return rec


@pytest.mark.parametrize("radius", [0, 6, 32])
def test_window_records(field_ctx, radius):
    ctx = field_ctx
    order = [9, 4, 15, 3, 12, 7, 5, 14, 8, 6, 13, 10, 11]
    for first, n in ((0, 13), (0, 1), (12, 1), (0, 5), (8, 5), (6, 1)):      # both clipped ends of the sequence and the middle
        for pov in (False, True):
            rec = assert_window(ctx, order, first, n, radius, 7.0, pov)
            assert not rec["cut"].any()
    assert_window(ctx, order[:1], 0, 1, radius)
    assert_window(ctx, order[:3], 1, 2, radius)


@pytest.mark.parametrize("size", [(16, 16), (257, 40)], ids=gid)
def test_window_records_at_other_sizes(size):
    w, h = size
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(np.stack([field(w, h, 70 + i) for i in range(8)])), list(range(8)))
        for pov in (False, True):
            rec = assert_window(ctx, list(range(8)), 0, 8, 6, 7.0, pov)
            f5 = ctx.download_flow(5)
            ar.check_axes([rec[k][5] for k in ("dot", "tangential", "shift_x", "shift_y")], f5, (rec["cx"][5], rec["cy"][5]), pov)


# ---- exact known answers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_known_answers_are_exact(size):
    w, h = size
    with context(w, h) as ctx:
        for centre in ((w // 3, h // 4), (0, 0), (w - 1, h - 1)):
            known = ar.known_fields(w, h, centre)
            names = list(known)
            ctx.import_flows(dev(np.stack([known[k][0] for k in names])), list(range(len(names))))
            got = ctx.radial_axes(list(range(len(names))), [centre] * len(names), [False] * len(names), True)
            for name, g in zip(names, got):
                assert g.tolist() == known[name][1], (name, centre, g.tolist(), known[name][1])


def test_weighted_uniform_field_is_exact_at_16x16():
    with context(16, 16) as ctx:
        for centre in ((5, 9), (0, 0), (15, 15), (8, 8)):
            f, sx, sy = ar.weighted_uniform_16(centre)
            ctx.import_flows(dev(f[None]), [0])
            got = ctx.radial_axes([0], [centre], [False], False)[0]
            assert (got[2], got[3]) == (sx, sy), (centre, got, sx, sy)


# ---- cuts and non-finite fields ---------------------------------------------------------------------------------------------
def test_cuts_and_non_finite_fields():
    f = np.stack([field(W, H, 90 + i) for i in range(4)])
    f[1, H // 2, W // 2, 0] = np.nan                                        # one NaN, in u only
    f[3] = np.nan
    c = (40.5, 8.25)
    with context(W, H) as ctx:
        ctx.import_flows(dev(f), [0, 1, 2, 3])
        for pov in (False, True):
            alone = [ctx.radial_axes([s], [c], [False], pov)[0] for s in range(3)]
            got = ctx.radial_axes([0, 1, 2, 3, 1], [c] * 5, [False, False, True, True, False], pov)
            assert got[2].tobytes() == PZERO * 4                            # a cut item: four +0.0
            assert got[3].tobytes() == PZERO * 4                            # ... whatever its slot holds
            assert got[0].tobytes() == alone[0].tobytes()                   # its neighbours are not affected
            assert np.isnan(got[1][:3]).all() and math.isfinite(got[1][3])  # NaN in u: radial, tangential, shift_x
            assert np.isnan(got[4][:3]).all() and got[4][3].tobytes() == got[1][3].tobytes()
            ar.check_axes(got[1], f[1], c, pov, components=(3,))            # shift_y: finite and within its bound
            ar.check_axes(got[0], f[0], c, pov)
            assert not np.isnan(alone[2]).any()
            # the window form: slot 3's record has a NaN mean magnitude (never a cut), a low threshold cuts the others
            rec = assert_window_nan(ctx, [0, 1, 2, 3], pov)
            assert rec["cut"].tolist() == [1, 0, 1, 0]
            for j in (0, 2):
                assert np.frombuffer(rec[j:j + 1].tobytes(), np.uint8)[48:].tobytes() == PZERO * 4 and rec["dot"][j].tobytes() == PZERO
            assert np.isnan([rec[k][3] for k in ("dot", "tangential", "shift_x", "shift_y")]).all()
            assert np.isnan([rec[k][1] for k in ("dot", "tangential", "shift_x")]).all() and math.isfinite(rec["shift_y"][1])


def assert_window_nan(ctx, seq, pov):
    """assert_window for records with NaN: NaN where ffl_radial_axes has NaN, the same bits elsewhere"""
    n = len(seq)
    rec, plain = window_pair(ctx, seq, 0, n, 1, 0.5, pov)
    want = ctx.radial_axes(seq, np.stack([rec["cx"], rec["cy"]], axis=1), rec["cut"] != 0, pov)
    got = np.stack([rec["dot"], rec["tangential"], rec["shift_x"], rec["shift_y"]], axis=1)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all() and got[~nan].tobytes() == want[~nan].tobytes()
    assert rec["reserved"].tobytes() == PZERO * n
    for k in ("cx", "cy", "x", "y", "cut", "pad"):
        assert rec[k].tobytes() == plain[k].tobytes(), k
    return rec


# ---- two scratch sets on stream `post` ---------------------------------------------------------------------------------------
def test_shared_post_scratch_between_the_two_forms():
    """radial, radial_axes, radial_window and radial_window_axes alternate on stream `post`, the device-ordered ones with no
    host wait in between.  At 257x40 an item has 3 workgroups: the single-component partials of item b start at 3 * b, the
    four-component ones at 12 * b, so a shared or overlapping buffer, or a call overtaking another, would change a value.
    Every result equals what the same call gives on a context of its own."""
    w, h = 257, 40
    f = np.stack([field(w, h, 30 + i) for i in range(6)])
    cen = [(0.3 * w + i, 0.6 * h - i) for i in range(6)]
    seq = list(range(6))

    def alone(what):
        with context(w, h, mb=8) as ctx:
            ctx.import_flows(dev(f), seq)
            return what(ctx)

    def win(ctx, axes):
        out = torch.empty(6 * (ITEM if axes else ITEM1), dtype=torch.uint8, device=DEV)
        (ctx.radial_window_axes if axes else ctx.radial_window)(seq, 0, 6, out, 2)
        return out

    want = {"w1": alone(lambda c: win(c, False).cpu().numpy().tobytes()), "w4": alone(lambda c: win(c, True).cpu().numpy().tobytes()),
            "r1": alone(lambda c: np.asarray(c.radial(seq, cen, [False] * 6)).tobytes()),
            "r4": alone(lambda c: c.radial_axes(seq, cen, [False] * 6).tobytes())}
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(f), seq)
        a4 = win(ctx, True)
        a1 = win(ctx, False)
        b4 = win(ctx, True)
        r1 = np.asarray(ctx.radial(seq, cen, [False] * 6)).tobytes()
        c1 = win(ctx, False)
        c4 = win(ctx, True)
        r4 = ctx.radial_axes(seq, cen, [False] * 6).tobytes()
        d1 = win(ctx, False)
        r1b = np.asarray(ctx.radial(seq, cen, [False] * 6)).tobytes()
        r4b = ctx.radial_axes(seq[::-1], cen[::-1], [False] * 6)[::-1].tobytes()
        assert ctx.graph_stats()["capture_failures"] == 0
        for t in (a4, b4, c4):
            assert t.cpu().numpy().tobytes() == want["w4"]
        for t in (a1, c1, d1):
            assert t.cpu().numpy().tobytes() == want["w1"]
        assert r1 == want["r1"] and r1b == want["r1"] and r4 == want["r4"] and r4b == want["r4"]


def test_shared_post_scratch_between_all_eight_users():
    """The sibling of the test above for every user of stream `post`: radial, radial_axes, radial_window, radial_window_axes,
    radial_window_axes_weighted (a random uint8 map per item, a fifth of it zeros), cell_stats into a centre buffer (cells =
    8), radial_window_axes_centres out of that buffer, and pass1_weighted.  They alternate on one context, the device-ordered
    ones with no host wait in between; nothing is read back before the end.  257x40, three workgroups per item: the partials
    of item b start at 3 * b (one component), 12 * b (four) and 15 * b (four and SW).  Every result equals, byte for byte, what
    the same call gives on a context of its own.  pass1_weighted rewrites the slots' records, so it comes last, followed by
    one radial_window and one radial_window_axes_weighted whose expected bytes come from a fresh context that replays
    import_flows, pass1_weighted and that call.
    A context of its own runs the same code, so two exact relations tie the expected bytes to something outside it.  The
    maps are below 128: doubled maps double every term, every sum and SW exactly, so the quotients by SW keep their bits
    (a quotient by anything else does not).  And the centres read out of cell_stats' 32-byte records equal the same centres
    handed over as a float64 (6, 2) tensor, 16 bytes apart."""
    w, h, cells = 257, 40, 8
    f = np.stack([field(w, h, 30 + i) for i in range(6)])
    cen = [(0.3 * w + i, 0.6 * h - i) for i in range(6)]
    seq = list(range(6))
    rng = np.random.default_rng(8)
    maps = rng.integers(1, 128, (6, h, w)).astype(np.uint8)
    maps[rng.random((6, h, w)) < 0.2] = 0
    assert all((m == 0).any() and (m != 0).any() for m in maps)
    wts, wts2 = dev(maps), dev(maps * np.uint8(2))
    csize = _capi.GRID_CENTRE_DTYPE.itemsize

    def win(ctx, kind, centres=None):
        out = torch.empty(6 * (ITEM1 if kind == "w1" else ITEM), dtype=torch.uint8, device=DEV)
        if kind == "w1":
            ctx.radial_window(seq, 0, 6, out, 2)
        elif kind == "w4":
            ctx.radial_window_axes(seq, 0, 6, out, 2)
        elif kind in ("ww", "ww2"):
            ctx.radial_window_axes_weighted(seq, 0, 6, wts if kind == "ww" else wts2, out, 2)
        else:
            ctx.radial_window_axes_centres(seq, 0, 6, centres, out, 2)
        return out

    def grid(ctx):
        out = torch.empty(6 * csize, dtype=torch.uint8, device=DEV)
        ctx.cell_stats(seq, cells, None, out)
        return out

    def raw(t):
        return t.cpu().numpy().tobytes()

    def alone(what, reweight=False):
        with context(w, h, mb=8) as ctx:
            ctx.import_flows(dev(f), seq)
            if reweight:
                ctx.pass1_weighted(seq, wts)
            return what(ctx)

    def centred(ctx):
        g = grid(ctx)
        rec = np.frombuffer(raw(g), _capi.GRID_CENTRE_DTYPE, 6)
        plain = dev(np.stack([rec["cx"], rec["cy"]], axis=1))   # float64 (6, 2)
        return raw(g), raw(win(ctx, "wc", g)), raw(win(ctx, "wc", plain))

    want = {k: alone(lambda c, k=k: raw(win(c, k))) for k in ("w1", "w4", "ww", "ww2")}
    assert want["ww2"] == want["ww"]
    want["cs"], want["wc"], plain = alone(centred)
    assert plain == want["wc"]
    want["r1"] = alone(lambda c: np.asarray(c.radial(seq, cen, [False] * 6)).tobytes())
    want["r4"] = alone(lambda c: c.radial_axes(seq, cen, [False] * 6).tobytes())
    want["p1"] = alone(lambda c: [tuple(r) for r in c.pass1_results(seq)], reweight=True)
    want["z1"] = alone(lambda c: raw(win(c, "w1")), reweight=True)
    want["zw"] = alone(lambda c: raw(win(c, "ww")), reweight=True)
    assert want["cs"] != bytes(len(want["cs"])) and want["ww"] != want["w4"] and want["wc"] != want["w4"] and want["z1"] != want["w1"]
    got = []   # (key, device tensor or bytes)
    with context(w, h, mb=8) as ctx:
        ctx.import_flows(dev(f), seq)
        got.append(("w4", win(ctx, "w4")))
        got.append(("ww", win(ctx, "ww")))
        g1 = grid(ctx)
        got.append(("wc", win(ctx, "wc", g1)))
        got.append(("w1", win(ctx, "w1")))
        got.append(("ww", win(ctx, "ww")))
        got.append(("r1", np.asarray(ctx.radial(seq, cen, [False] * 6)).tobytes()))
        g2 = grid(ctx)
        got.append(("w4", win(ctx, "w4")))
        got.append(("wc", win(ctx, "wc", g2)))
        got.append(("ww", win(ctx, "ww")))
        got.append(("r4", ctx.radial_axes(seq, cen, [False] * 6).tobytes()))
        got.append(("w1", win(ctx, "w1")))
        got.append(("wc", win(ctx, "wc", g1)))
        g3 = grid(ctx)
        got.append(("w4", win(ctx, "w4")))
        got.append(("r1", np.asarray(ctx.radial(seq, cen, [False] * 6)).tobytes()))
        got.append(("r4", ctx.radial_axes(seq[::-1], cen[::-1], [False] * 6)[::-1].tobytes()))
        got += [("cs", g1), ("cs", g2), ("cs", g3)]
        ctx.pass1_weighted(seq, wts)
        got.append(("z1", win(ctx, "w1")))
        got.append(("zw", win(ctx, "ww")))
        assert ctx.graph_stats()["capture_failures"] == 0
        for i, (k, v) in enumerate(got):
            assert (v if isinstance(v, bytes) else raw(v)) == want[k], (i, k)
        assert [tuple(r) for r in ctx.pass1_results(seq)] == want["p1"]


# ---- refusals -------------------------------------------------------------------------------------------------------------
class Span:
    """`nbytes` bytes at `ptr` as a __cuda_array_interface__ object, whatever memory that is"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": (int(nbytes),), "strides": None,
                                         "typestr": "|u1"}


def test_refusals(field_ctx):
    ctx, seq = field_ctx, list(range(3, 16))
    out = torch.empty(300 * ITEM, dtype=torch.uint8, device=DEV)
    INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE

    def refused(match, code, seq_, first, n, out_=out, radius=6, stream=None):
        with pytest.raises(_capi.FFLError, match=match) as e:
            ctx.radial_window_axes(seq_, first, n, out_, radius, stream=stream)
        assert e.value.code == code and "ffl_radial_window_axes" in str(e.value)

    refused(r"n = 0 items outside 1\.\.256", INVALID, seq, 0, 0)
    refused(r"n = 257 items outside 1\.\.256", INVALID, seq, 0, 257)
    refused(r"n_seq = 0 slots outside 1\.\.320", INVALID, [], 0, 1)
    refused(r"n_seq = 321 slots outside 1\.\.320", INVALID, [3] * 321, 0, 1)
    refused(r"first = -1, n = 2: the items lie outside seq", INVALID, seq, -1, 2)
    refused(r"first = 10, n = 4: the items lie outside seq 0\.\.12", INVALID, seq, 10, 4)
    refused(r"first = 2147483647, n = 2: the items lie outside seq", INVALID, seq, 2 ** 31 - 1, 2)
    refused(r"radius -1 outside 0\.\.32", INVALID, seq, 0, 1, radius=-1)
    refused(r"radius 33 outside 0\.\.32", INVALID, seq, 0, 1, radius=33)
    refused(r"flow slot 24 out of range", INVALID, [3, 24], 0, 1)
    refused(r"flow slot -1 out of range", INVALID, [-1, 3], 1, 1)
    for _ in range(2):
        refused(r"flow slot 5 repeated", INVALID, [4, 5, 5], 0, 1)
    refused(r"flow slot 2 holds no result", STATE, [2, 3, 4], 1, 1)
    refused(r"flow slot 16 holds no result", STATE, [15, 16], 1, 1)
    refused(r"8-byte aligned", INVALID, seq, 0, 1, Span(out.data_ptr() + 4, 100 * ITEM))
    torch.cuda.empty_cache()
    big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)           # an allocation of its own
    refused(r"more than its allocation holds", INVALID, seq, 0, 3, Span(big.data_ptr() + big.numel() - 2 * ITEM, 3 * ITEM))
    # the extent is n * 80: room for three 48-byte records at the end of an allocation is not room for three of these
    refused(r"spans 240 bytes, 96 more than its allocation holds", INVALID, seq, 0, 3,
            Span(big.data_ptr() + big.numel() - 3 * ITEM1, 3 * ITEM))
    pin = ctx.pinned_frames(1, channels=1)
    refused(r"page-locked host memory.*ffl_radial", INVALID, seq, 0, 1, Span(pin.ctypes.data, pin.size))
    with pytest.raises(ValueError, match="not device memory"):
        ctx.radial_window_axes(seq, 0, 1, np.zeros(ITEM, np.uint8))
    with pytest.raises(ValueError, match="radial_window_axes: out holds 96 bytes, 2 records need 160"):
        ctx.radial_window_axes(seq, 0, 2, out[:2 * ITEM1])               # n * 48 bytes are not enough
    x = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    codes = []
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        try:
            ctx.radial_window_axes(seq, 0, 1, out, stream=torch.cuda.current_stream())
        except _capi.FFLError as err:
            codes.append((err.code, "capturing" in str(err)))
        x += 1
    g.replay()
    torch.cuda.synchronize()
    assert codes == [(STATE, True)] and float(x.sum()) == 16.0
    # ffl_radial_axes: ffl_radial's refusals
    for call, match in ((lambda: ctx.radial_axes([], np.zeros((0, 2)), []), "ffl_radial_axes: bad arguments"),
                        (lambda: ctx.radial_axes([24], [(0, 0)], [False]), "ffl_radial_axes: flow slot 24 out of range"),
                        (lambda: ctx.radial_axes([2], [(0, 0)], [False]), "ffl_radial_axes: flow slot 2 holds no flow")):
        with pytest.raises(_capi.FFLError, match=match):
            call()
    # and the context computes correct calls next
    assert_window(ctx, seq, 0, 13, 6)
    assert_window(ctx, [4, 5], 1, 1, 0)


# ---- the engine and the scripts --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clip(n, w, h, seed=3):
    return list(sine_translate_frames(n, w, h, seed=seed))


def engine_ctx(w, h, B):
    return _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2))


def test_engine_chunk_and_flows():
    w, h, B, n = 64, 48, 4, 11
    fr = clip(n + 1, w, h, seed=5)
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        T = torch.empty((n, h, w, 2), device=DEV)
        eng.process_chunk(fr, flows_out=T)
        for thr, pov in ((0.4, True), (7.0, False)):
            dots, recs = eng.process_chunk(fr, pov, thr)
            want = np.asarray(dots, np.float64).tobytes()
            comps, r1 = eng.process_chunk(fr, pov, thr, axes=True)
            assert comps.shape == (n, 4) and comps[:, 0].tobytes() == want and r1 == recs
            buf = pipeline.post_buffer(ctx, n, axes=True)
            assert buf.numel() == n * ITEM and eng.process_chunk(fr, pov, thr, post_out=buf, axes=True) is buf
            c2, r2 = pipeline.post_records(buf, axes=True)
            assert r2 == recs and c2.tobytes() == comps.tobytes()
            c3, r3 = eng.process_flows(T, pov, thr, axes=True)
            assert r3 == recs and c3.tobytes() == comps.tobytes()
            c4, r4 = pipeline.post_records(eng.process_flows(T, pov, thr, post_out=True, axes=True), n, axes=True)
            assert r4 == recs and c4.tobytes() == comps.tobytes()
            # the default is what it was
            d5, r5 = pipeline.post_records(eng.process_chunk(fr, pov, thr, post_out=True))
            assert r5 == recs and d5.tobytes() == want
        assert np.abs(comps[:, 1:]).max() > 0
        with pytest.raises(ValueError, match="records need 880"):
            eng.process_chunk(fr, post_out=pipeline.post_buffer(ctx, n), axes=True)
        assert eng.process_chunk(fr[:1], axes=True)[0].shape == (0, 4)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_frames_to_scripts(tmp_path):
    w, h, B, n = 64, 48, 4, 11
    fr = clip(n + 1, w, h, seed=5)
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 7.0}
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        main = pipeline.frames_to_actions(eng, fr, 30.0, params)
        plan = pipeline.pair_plan(30.0, n + 1, params)
        assert len(plan) == 1 and len(plan[0]) == n + 1
        comps, recs = eng.process_chunk(fr, False, 7.0, axes=True)
        roll = postchain.actions_from_scalars([float(v) for v in comps[:, 1]], [bool(r[4]) for r in recs], plan[0][:-1], 30.0, params)
        for extra in ({}, {"hip_pass2": "device"}):
            scripts = pipeline.frames_to_scripts(eng, fr, 30.0, {**params, **extra, "hip_axes": {"roll": "tangential"}})
            assert list(scripts) == ["", "roll"]
            assert scripts[""] == main and main and scripts["roll"] == roll and roll != main
        T = torch.empty((n, h, w, 2), device=DEV)
        eng.process_chunk(fr, flows_out=T)
        fs = pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**params, "hip_axes": {"roll": "tangential"}})
        assert fs == scripts
        paths = postchain.write_funscripts(tmp_path / "clip", scripts)
        assert sorted(p.name for p in tmp_path.iterdir()) == ["clip.funscript", "clip.roll.funscript"] and len(paths) == 2
        assert ctx.graph_stats()["capture_failures"] == 0
