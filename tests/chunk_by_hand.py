"""The composed chunk, stated once, without an engine (fixtures).

PairEngine.process_chunk / process_flows string the library's calls together per batch, on a ring of flow slots that later
batches recycle.  by_hand runs the same chunk on a context that holds every pair at once -- at least n flow slots and
max_batch >= n -- so nothing recycles and every step is ONE documented _capi.Context call over slots 0 .. n-1, in the order
process_chunk's docstring promises:

    1. the flow call (flow_pairs / flow_pairs_dis / flow_pairs_farneback(..., window=)), or import_flows of given fields;
    2. compensate=: motion_fit (under the maps when there are maps), then motion_subtract in place;
    3. weights=: pass1_weighted            -- or --   center=: cell_stats;
    4. one window call over the whole chunk (seq = range(n), first = 0, count = n, radius 6): radial_window[_axes],
       radial_window_axes_weighted or radial_window_axes_centres.

One whole-chunk window call has the bits of the engine's chunked calls (pipeline.window_calls: every computed item's clipped
window lies inside its call's seq); the per-feature tests rely on that and so does this.

The helper is anchored to the CPU at two points (check_anchors), so that by-hand and engine cannot agree on a wrong answer
upstream: every raw field of the tuned Farneback path is oracle.farneback of its pair, and every compensated field is
motion_ref.subtract(raw, model), both on bytes.  No pytest marks: test_gpu_chunk_compose.py compares the engine with it on
bytes, and test_chunk_schedule_host.py holds the engine's schedules to the same order without a device."""
import numpy as np

from funscript_flow_amd import _capi, pipeline

RADIUS = pipeline.SMOOTH_RADIUS


def random_map(w, h, seed):
    """random 1..255 with about a third zeros (the generator of test_gpu_motion.random_map)"""
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    m[rng.random((h, w)) < 1 / 3] = 0
    return m


def pair_maps(w, h, n, seed):
    """(n, h, w): one map per pair, a different seed each"""
    return np.stack([random_map(w, h, seed + j) for j in range(n)])


def padded(maps, device):
    """(n, h, w) maps as a device view with a padded row pitch and item stride"""
    import torch
    n, h, w = maps.shape
    big = torch.full((n, h + 2, w + 13), 0x5A, dtype=torch.uint8, device=device)
    view = big[:, 1:h + 1, 5:5 + w]
    view.copy_(torch.from_numpy(np.array(maps, order="C")).to(device))
    return view


def hand_context(w, h, n, device=0):
    """a context on which a chunk of n pairs never recycles anything"""
    return _capi.Context(w, h, device=device, max_batch=max(n, 1), frame_slots=n + 1, flow_slots=max(n, 1))


def _fields(ctx, slots):
    return ctx.export_flows(slots).cpu().numpy()


def by_hand(ctx, frames_or_fields, *, pov, thr, axes=True, weights=None, center=None, cells=8, compensate=None, algo=None,
            window="box"):
    """The chunk of `frames_or_fields` -- n + 1 gray frames (a list or an (n + 1, H, W) uint8 array), or the n pair fields as a
    device array (n, H, W, 2) -- on `ctx`, which holds it whole.  weights: None, or an (H, W) / (n, H, W) uint8 device tensor;
    center: None or "variance" over cells x cells; compensate: as process_chunk takes it; algo: None (Farneback) or ("dis",
    DisParams or None); window: "box" or "gaussian".  Returns dict(post = the n records as bytes, motion = the n 64-byte
    records as bytes or None, grid = the cell records as bytes or None, flows = (n, H, W, 2) float32 as left in the slots,
    pass1 = pass1_results' tuples of the slots as left, raw = (n, H, W, 2) float32 as the flow call left them)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    given = not isinstance(frames_or_fields, (list, tuple)) and getattr(frames_or_fields, "ndim", 0) == 4
    n = len(frames_or_fields) - (0 if given else 1)
    assert 1 <= n <= min(ctx.flow_slots, ctx.max_batch), "by_hand needs a context that holds the whole chunk"
    assert weights is None or center is None
    assert axes or (weights is None and center is None)
    slots = list(range(n))
    # 1. the flow call
    if given:
        ctx.import_flows(frames_or_fields, slots, pov)
    else:
        assert ctx.frame_slots >= n + 1
        ctx.upload_frames(0, [np.ascontiguousarray(f) for f in frames_or_fields])
        f0, f1 = list(range(n)), list(range(1, n + 1))
        if algo is not None and algo[0] == "dis":
            ctx.flow_pairs_dis(f0, f1, slots, pov, algo[1])
        elif window != "box":
            ctx.flow_pairs_farneback(f0, f1, slots, pov, None, window=window)
        else:
            ctx.flow_pairs(f0, f1, slots, pov)
    raw = _fields(ctx, slots)
    # 2. the fit, then the subtraction in place
    motion = None
    if compensate is not None:
        mo = pipeline.motion_buffer(ctx, n)
        ctx.motion_fit(slots, _capi.motion_choice(compensate), weights=weights, out=mo)
        ctx.motion_subtract(slots, slots, mo, pov)
        motion = mo.cpu().numpy().tobytes()
    # 3. the records under the maps, or the cell grid and its centres
    item = (_capi.PASS2_AXES_DTYPE if axes else _capi.PASS2_DTYPE).itemsize
    out = torch.full((n * item,), 0xA5, dtype=torch.uint8, device=dev)
    grid = None
    if weights is not None:
        ctx.pass1_weighted(slots, weights, pov)
        ctx.radial_window_axes_weighted(slots, 0, n, weights, out, RADIUS, thr, pov)
    elif center is not None:
        assert center == "variance"
        cell_out = pipeline.grid_buffer(ctx, n, cells)
        centres = torch.full((n * _capi.GRID_CENTRE_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.cell_stats(slots, cells, cell_out, centres)
        ctx.radial_window_axes_centres(slots, 0, n, centres, out, RADIUS, thr, pov)
        grid = cell_out.cpu().numpy().tobytes()
    # 4. (the plain forms of) the one window call
    elif axes:
        ctx.radial_window_axes(slots, 0, n, out, RADIUS, thr, pov)
    else:
        ctx.radial_window(slots, 0, n, out, RADIUS, thr, pov)
    return dict(post=out.cpu().numpy().tobytes(), motion=motion, grid=grid, flows=_fields(ctx, slots),
                pass1=ctx.pass1_results(slots, thr), raw=raw)


def records(post, axes=True):
    """the post bytes of by_hand (or of an engine) as a numpy record array"""
    return np.frombuffer(post, _capi.PASS2_AXES_DTYPE if axes else _capi.PASS2_DTYPE)


def rec_bytes(recs):
    """pass1_results' tuples with their floats as bytes: NaN-safe equality"""
    return [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in recs]


def oracle_fields(frames):
    """(n, H, W, 2): oracle.farneback of every pair of `frames`, on the CPU"""
    import oracle as orc
    return np.stack([orc.farneback(frames[j], frames[j + 1]) for j in range(len(frames) - 1)])


def check_anchors(res, oracle=None):
    """The two CPU anchors of a by_hand result: with `oracle` (oracle_fields of the chunk's frames; the tuned Farneback path
    only) every raw field is the oracle's; with a fit, every field left in the slots is motion_ref.subtract(raw, the pair's
    model) -- for ALL n pairs, on bytes -- and without one it is the raw field."""
    import motion_ref as mr
    n = len(res["raw"])
    if oracle is not None:
        for j in range(n):
            assert res["raw"][j].tobytes() == oracle[j].tobytes(), f"raw field {j} is not the oracle's"
    if res["motion"] is None:
        assert res["flows"].tobytes() == res["raw"].tobytes()
        return
    models = np.frombuffer(res["motion"], _capi.MOTION_DTYPE, n)
    for j in range(n):
        assert res["flows"][j].tobytes() == mr.subtract(res["raw"][j], mr.six(models[j])).tobytes(), f"compensated field {j}"
