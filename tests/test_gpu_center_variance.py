"""GPU side of the centre window over caller centres (ffl_radial_window_axes_centres: k_window_plan<80, true>) and of the
schedule about the variance centre (process_chunk / process_flows with center="variance", params["hip_center"]; DESIGN.md
section 17): records byte for byte against the composition download_flow -> grid_ref centres -> grid_ref.window ->
radial_axes, with pass1_results for the fields of a record that still come from the slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import grid_ref as gr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
ITEM = _capi.PASS2_AXES_DTYPE.itemsize
CELL, CEN = _capi.CELL_DTYPE.itemsize, _capi.GRID_CENTRE_DTYPE.itemsize
W, H, NSEQ = 130, 17, 20
BIG = 1e30


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def records(buf, n):
    return np.frombuffer(buf.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)


def composed(ctx, slots, centres, thr, pov=False):
    """the records radial_window_axes_centres owes for items `slots` about the (already windowed) `centres`: radial_axes for
    the components, pass1_results for the rest"""
    recs = ctx.pass1_results(slots, thr)
    comps = ctx.radial_axes(slots, centres, [r[4] for r in recs], pov)
    out = np.zeros(len(slots), _capi.PASS2_AXES_DTYPE)
    out["dot"], out["tangential"], out["shift_x"], out["shift_y"] = comps[:, 0], comps[:, 1], comps[:, 2], comps[:, 3]
    out["cx"], out["cy"] = np.asarray(centres, np.float64)[:, 0], np.asarray(centres, np.float64)[:, 1]
    out["x"], out["y"] = [r[0] for r in recs], [r[1] for r in recs]
    out["div_val"], out["mean_mag"], out["cut"] = [r[2] for r in recs], [r[3] for r in recs], [int(r[4]) for r in recs]
    return out


def same(a, b):
    """field by field; bytes where there is no NaN, NaN == NaN where there is"""
    for k in _capi.PASS2_AXES_DTYPE.names:
        x, y = a[k], b[k]
        if x.dtype.kind == "f" and (np.isnan(x).any() or np.isnan(y).any()):
            nan = np.isnan(x)
            assert np.array_equal(nan, np.isnan(y)) and x[~nan].tobytes() == y[~nan].tobytes(), k
        else:
            assert x.tobytes() == y.tobytes(), (k, x, y)


@pytest.fixture(scope="module")
def field_ctx():
    """20 fields in slots 5..24 of a 130x17 context, in a shuffled seq order, and a cut threshold that cuts about half"""
    with _capi.Context(W, H, max_batch=32, frame_slots=2, flow_slots=32) as ctx:
        slots = list(range(5, 5 + NSEQ))
        ctx.import_flows(dev(np.stack([gr.field(W, H, 100 + i) * np.float32(1 + 0.1 * (i % 5)) for i in range(NSEQ)])), slots)
        order = [int(s) for s in np.random.default_rng(1).permutation(slots)]
        mms = sorted(float(r[3]) for r in ctx.pass1_results(order, 0.0))
        thr = (mms[9] + mms[10]) / 2
        assert mms[9] < thr < mms[10]
        yield ctx, order, thr
        assert ctx.graph_stats()["capture_failures"] == 0


def centre_inputs(cen):
    """the same n_seq centres as a float64 (n, 2) tensor (stride 16) and as ffl_grid_centre records (stride 32)"""
    rec = np.zeros(len(cen), _capi.GRID_CENTRE_DTYPE)
    rec["cx"], rec["cy"], rec["total_var"], rec["cells"], rec["empty"] = cen[:, 0], cen[:, 1], -7.0, 32, 3
    return dev(cen), dev(np.frombuffer(rec.tobytes(), np.uint8))


@pytest.mark.parametrize("radius", [0, 6, 32])
def test_window_over_caller_centres(field_ctx, radius):
    ctx, order, thr = field_ctx
    rng = np.random.default_rng(5 + radius)
    cen = rng.uniform(-40.0, 200.0, (NSEQ, 2))           # inside and outside the image
    win = gr.window(cen, radius)
    for first, n in ((0, NSEQ), (3, 9), (NSEQ - 1, 1), (7, 1)):
        want = composed(ctx, order[first:first + n], win[first:first + n], thr)
        assert n != NSEQ or want["cut"].sum() == 10
        for src in centre_inputs(cen):
            out = torch.full((n * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
            ctx.radial_window_axes_centres(order, first, n, src, out, radius, thr)
            got = records(out, n)
            assert got.tobytes() == want.tobytes()
            cut = got["cut"] != 0
            for k in ("dot", "tangential", "shift_x", "shift_y", "reserved"):   # a cut item is all +0.0
                assert got[k][cut].tobytes() == np.zeros(int(cut.sum())).tobytes()
    # POV mode, no cuts
    want = composed(ctx, order, win, BIG, True)
    out = torch.full((NSEQ * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.radial_window_axes_centres(order, 0, NSEQ, dev(cen), out, radius, BIG, True)
    assert records(out, NSEQ).tobytes() == want.tobytes()


def test_a_nan_centre_follows_ieee(field_ctx):
    ctx, order, thr = field_ctx
    cen = np.random.default_rng(9).uniform(0.0, 130.0, (NSEQ, 2))
    cen[8, 0] = np.nan
    win = gr.window(cen, 2)
    assert np.isnan(win[6:11, 0]).all() and not np.isnan(win[:6]).any() and not np.isnan(win[11:]).any() and not np.isnan(win[:, 1]).any()
    want = composed(ctx, order, win, thr)
    out = torch.full((NSEQ * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    ctx.radial_window_axes_centres(order, 0, NSEQ, dev(cen), out, 2, thr)
    got = records(out, NSEQ)
    same(got, want)
    for j in range(6, 11):   # dot is NaN unless the item is cut
        assert got["cut"][j] or np.isnan(got["dot"][j])
        assert not got["cut"][j] or got["dot"][j].tobytes() == np.float64(0).tobytes()
    assert not np.isnan(got["dot"][:6]).any() and not np.isnan(got["dot"][11:]).any()


def test_centres_refusals_and_stream_contract(field_ctx):
    ctx, order, thr = field_ctx
    INVALID = _capi.FFL_ERR_INVALID
    cen = np.random.default_rng(3).uniform(0.0, 130.0, (NSEQ, 2))
    out = torch.full((NSEQ * ITEM,), 0xA5, dtype=torch.uint8, device=DEV)
    L, h = ctx.L, ctx._h

    def raw(ptr, stride, n_seq=NSEQ):
        ps, keep = _capi._iarr(order[:n_seq])
        return lambda: ctx._chk(L.ffl_radial_window_axes_centres(h, n_seq, ps, 0, 1, 6, 7.0, 0, ptr, stride, out.data_ptr(),
                                                                 _capi.stream_handle(None, 0)))

    def refused(match, call):
        with pytest.raises(_capi.FFLError, match=match) as e:
            call()
        assert e.value.code == INVALID and "ffl_radial_window_axes_centres" in str(e.value)

    d = dev(cen)
    refused(r"centre stride 8: a multiple of 8 bytes, at least 16", raw(d.data_ptr(), 8))
    refused(r"centre stride 20: a multiple of 8 bytes, at least 16", raw(d.data_ptr(), 20))
    refused(r"NULL centres_dev", raw(None, 16))
    refused(r"centres_dev must be 8-byte aligned", raw(d.data_ptr() + 4, 16))
    pin = ctx.pinned_frames(1, channels=1)
    refused(r"centres_dev is page-locked host memory.*device memory", raw(pin.ctypes.data, 16, 2))
    torch.cuda.empty_cache()
    big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)
    refused(rf"centres_dev spans {(NSEQ - 1) * 32 + 16} bytes, 32 more than its allocation holds",
            raw(big.data_ptr() + big.numel() - (NSEQ - 1) * 32 + 16, 32))
    with pytest.raises(ValueError, match=r"float64 shape \(19, 2\)"):
        ctx.radial_window_axes_centres(order, 0, 1, dev(cen[:19]), out)
    with pytest.raises(ValueError, match="centre records need"):
        ctx.radial_window_axes_centres(order, 0, 1, torch.empty(NSEQ * 32 - 8, dtype=torch.uint8, device=DEV), out)
    assert (out.cpu().numpy() == 0xA5).all()      # nothing was queued
    # the centres are freed and their memory overwritten right after the call, the records overwritten behind a reader
    want = composed(ctx, order, gr.window(cen, 6), thr)
    for side in (None, torch.cuda.Stream()):
        torch.cuda.synchronize()
        with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
            src = dev(cen)
            ctx.radial_window_axes_centres(order, 0, NSEQ, src, out, 6, thr, stream=side)
            del src
            junk = torch.full((NSEQ, 2), float("nan"), dtype=torch.float64, device=DEV)
            copy = out.clone()
            out.zero_()
        (side or torch.cuda.current_stream()).synchronize()
        assert records(copy, NSEQ).tobytes() == want.tobytes() and not out.cpu().numpy().any()
        del junk


# ---- the schedule ------------------------------------------------------------------------------------------------------------
def chunk_composition(T, cells, pov, thr):
    """(80-byte records, cell records) of a chunk whose pair fields are T, composed on a context of its own"""
    n, h, w = T.shape[0], T.shape[1], T.shape[2]
    fields = T.cpu().numpy()
    grids = np.stack([gr.cell_records(f, cells) for f in fields])
    cen = np.array([gr.centre_of(g[..., 3], w, h)[:2] for g in grids], np.float64)
    with _capi.Context(w, h, max_batch=32, frame_slots=2, flow_slots=32) as one:
        one.import_flows(T, list(range(n)), pov)
        return composed(one, list(range(n)), gr.window(cen, pipeline.SMOOTH_RADIUS), thr, pov), grids


@pytest.mark.parametrize("B,cells", [(8, 32), (2, 8)], ids=["B8-three-batches", "B2-slots-recycled"])
def test_process_chunk_about_the_variance_centre(B, cells):
    w, h, n = 64, 64, 20
    fr = list(sine_translate_frames(n + 1, w, h, seed=3, zoom=0.02))
    slots = pipeline.min_flow_slots(B)
    assert (slots < n) == (B == 2)                # B = 2: 17 slots for 20 pairs, neighbours' slots are recycled
    with _capi.Context(w, h, max_batch=B, frame_slots=2 * B + 2, flow_slots=slots) as ctx:
        eng = pipeline.PairEngine(ctx)
        plain = eng.process_chunk(fr, post_out=True, axes=True).cpu().numpy().tobytes()   # before any grid call
        for pov, thr in ((False, 7.0), (True, 0.5)):
            T = torch.empty((n, h, w, 2), device=DEV)
            grid = pipeline.grid_buffer(ctx, n, cells)
            buf = eng.process_chunk(fr, pov, thr, center="variance", cells=cells, grid_out=grid, flows_out=T)
            assert buf.numel() == n * ITEM
            want, grids = chunk_composition(T, cells, pov, thr)
            same(records(buf, n), want)
            assert records(buf, n).tobytes() == want.tobytes()
            got = pipeline.grid_records(grid, cells)
            assert got.shape == (n, cells, cells) and got.tobytes() == np.ascontiguousarray(grids).tobytes()
            # the same through flows the caller computed, and with a buffer of the caller's
            mine = pipeline.post_buffer(ctx, n, axes=True)
            assert eng.process_flows(T, pov, thr, center="variance", cells=cells, post_out=mine) is mine
            assert mine.cpu().numpy().tobytes() == buf.cpu().numpy().tobytes()
        assert eng.process_chunk(fr, post_out=True, axes=True).cpu().numpy().tobytes() == plain
        with pytest.raises(ValueError, match="together with weights"):
            eng.process_chunk(fr, center="variance", weights=torch.ones((h, w), dtype=torch.uint8, device=DEV))
        with pytest.raises(ValueError, match="center must be None or one of"):
            eng.process_chunk(fr, center="argmax")
        with pytest.raises(ValueError, match="grid_out needs center"):
            eng.process_chunk(fr, grid_out=grid)
        with pytest.raises(_capi.FFLError, match="rule G1"):
            eng.process_chunk(fr, center="variance", cells=65)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_scripts_about_the_variance_centre():
    w, h, B, n = 64, 64, 8, 20
    fr = list(sine_translate_frames(n + 1, w, h, seed=3, zoom=0.02))
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 7.0, "hip_axes": {"roll": "tangential", "sway": "shift_x"}}
    var = {**params, "hip_center": "variance", "hip_center_cells": 16}
    with _capi.Context(w, h, max_batch=B, frame_slots=2 * B + 2, flow_slots=pipeline.min_flow_slots(B)) as ctx:
        eng = pipeline.PairEngine(ctx)
        T = torch.empty((n, h, w, 2), device=DEV)
        eng.process_chunk(fr, flows_out=T)
        want, _ = chunk_composition(T, 16, False, 7.0)
        comps, recs = pipeline._chunk_scalars(eng, fr, var, True)
        assert comps[:, 0].tobytes() == want["dot"].tobytes() and comps[:, 1].tobytes() == want["tangential"].tobytes()
        assert [r[:2] for r in recs] == list(zip(want["x"].tolist(), want["y"].tolist()))
        scripts = pipeline.frames_to_scripts(eng, fr, 30.0, var)
        assert set(scripts) == {"", "roll", "sway"} and all(scripts[k] for k in scripts)
        assert pipeline.frames_to_actions(eng, fr, 30.0, var) == scripts[""]
        assert pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, var) == scripts
        assert pipeline.flows_to_actions(eng, [T], 30.0, n + 1, var) == scripts[""]
        assert scripts != pipeline.frames_to_scripts(eng, fr, 30.0, params)       # another centre, other scripts
        with pytest.raises(ValueError, match="hip_center together with hip_weights"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**var, "hip_weights": np.ones((h, w), np.uint8)})
        assert ctx.graph_stats()["capture_failures"] == 0
