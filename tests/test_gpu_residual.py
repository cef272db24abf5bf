"""GPU side of the photometric-residual maps (ffl_residual_weights, k_residual), everything
through the C ABI via _capi, on frames placed with upload_frames and fields placed with upload_flow.

Every output byte is held against the numpy restatement tests/residual_ref.py with equality; the inputs are that file's
synthetic triples, whose conditions tests/test_residual_ref_host.py asserts.  Sizes: 16x16 (one partly empty wave, every row
4-byte aligned), 130x17 (a width that is 2 mod 4: every other row of a frame is unaligned, an odd height), 257x40 (several
workgroups, a 1-pixel tail, rows at every alignment).  k_residual has no loop, so there is no two-trip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import chunk_by_hand as bh
import residual_ref as rr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
FILL = 0xA5
N = 5
FS0, FS1 = [6, 0, 3, 5, 2], [1, 7, 4, 8, 9]   # not in order, and interleaved in the slot space
FLOW = [5, 0, 3, 7, 1]                        # flow slots 2, 4 and 6 hold nothing
PARAMS = [None, {"soft": 0}, {"alpha": 0.0, "beta": 6.0}, {"alpha": 0.0, "beta": 9.0, "soft": 0}, {"alpha": 16.0, "beta": 1.0},
          {"alpha": 3.0, "beta": 255.0, "soft": 0}]
INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h):
    return _capi.Context(w, h, max_batch=6, frame_slots=11, flow_slots=8)   # frame slot 10 is never uploaded


def place(ctx, trips, fs0=FS0, fs1=FS1, flow=FLOW):
    """item i's I0 into frame slot fs0[i], its I1 into fs1[i], its field into flow slot flow[i]"""
    for (I0, I1, F), a, b, s in zip(trips, fs0, fs1, flow):
        ctx.upload_frames(a, [np.ascontiguousarray(I0)])
        ctx.upload_frames(b, [np.ascontiguousarray(I1)])
        ctx.upload_flow(s, F)


def gate_map(w, h, seed):
    rng = np.random.default_rng(400 + seed)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    g[rng.random((h, w)) < 0.25] = 0
    return g


def prm(kw):
    return {k: np.float32(v) if k != "soft" else v for k, v in (kw or {}).items()}


def run(ctx, w, h, n=N, params=None, gate=None, pitch=None, offset=0, fs0=FS0, fs1=FS1, flow=FLOW, stream=None):
    """one call into a buffer pre-filled with FILL: (the n maps, every byte outside them) as numpy arrays"""
    pitch = pitch or w
    item = h * pitch + 5
    raw = torch.full((offset + n * item + 7,), FILL, dtype=torch.uint8, device=DEV)
    ctx.residual_weights(fs0[:n], fs1[:n], flow[:n], _capi.DevWeights(raw.data_ptr() + offset, item, pitch), params, gate, stream)
    host = raw.cpu().numpy()
    body = host[offset:offset + n * item].reshape(n, item)
    rows = body[:, :h * pitch].reshape(n, h, pitch)
    rest = np.concatenate([host[:offset], host[offset + n * item:], body[:, h * pitch:].ravel(), rows[:, :, w:].ravel()])
    return rows[:, :, :w].copy(), rest


def want(trips, params=None, gates=None):
    return np.stack([rr.residual(*t, gate=None if gates is None else gates[i], **prm(params)) for i, t in enumerate(trips)])


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_bytes_equal_the_restatement(size):
    w, h = size
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    shared, each = gate_map(w, h, 0), np.stack([gate_map(w, h, 1 + i) for i in range(N)])
    with context(w, h) as ctx:
        place(ctx, trips)
        for kw in PARAMS:
            got, rest = run(ctx, w, h, params=kw)
            assert (got == want(trips, kw)).all(), kw
            assert (rest == FILL).all()
        for kw in (None, {"soft": 0}):
            got, rest = run(ctx, w, h, params=kw, gate=dev(shared))                       # item_stride 0: one gate for all
            assert (got == want(trips, kw, [shared] * N)).all() and (rest == FILL).all()
            got, rest = run(ctx, w, h, params=kw, gate=dev(each))
            assert (got == want(trips, kw, each)).all() and (rest == FILL).all()
        ref = want(trips)
        assert (ref == 0).any() and (ref == 255).any()
        for offset in (0, 1, 2, 3):
            for pitch in (w, w + 1, w + 6):
                got, rest = run(ctx, w, h, pitch=pitch, offset=offset)
                assert (got == ref).all(), (offset, pitch)
                assert (rest == FILL).all(), (offset, pitch)
        # a gate whose rows are padded and whose base is odd
        pad = torch.zeros((N, h, w + 3), dtype=torch.uint8, device=DEV)
        pad[:, :, 1:w + 1] = dev(each)
        got, _ = run(ctx, w, h, gate=pad[:, :, 1:w + 1])
        assert (got == want(trips, None, each)).all()
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_frame_slots_shared_between_items(size):
    """a run of frames as a chunk holds it: frame j + 1 of item j is frame j of item j + 1; and one pair with the roles swapped"""
    w, h = size
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    chain = [trips[0][0], trips[0][1], trips[1][1], trips[2][1]]
    with context(w, h) as ctx:
        ctx.upload_frames(2, [np.ascontiguousarray(f) for f in chain])     # frame slots 2 .. 5, one transfer
        for i in range(3):
            ctx.upload_flow(FLOW[i], trips[i][2])
        got, rest = run(ctx, w, h, n=3, fs0=[2, 3, 4], fs1=[3, 4, 5], pitch=w + 3, offset=1)
        ref = np.stack([rr.residual(chain[i], chain[i + 1], trips[i][2]) for i in range(3)])
        assert (got == ref).all() and (rest == FILL).all()
        got, rest = run(ctx, w, h, n=2, fs0=[3, 2], fs1=[2, 2], flow=[FLOW[2], FLOW[0]])   # slot 2 three times, once as both operands
        ref = np.stack([rr.residual(chain[1], chain[0], trips[2][2]), rr.residual(chain[0], chain[0], trips[0][2])])
        assert (got == ref).all() and (rest == FILL).all()


def test_tensor_outputs_and_bool_gate():
    w, h = 130, 17
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    with context(w, h) as ctx:
        place(ctx, trips)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        assert ctx.residual_weights(FS0, FS1, FLOW, out, _capi.ResidualParams(soft=0)) is out
        assert (out.cpu().numpy() == want(trips, {"soft": 0})).all()
        g = gate_map(w, h, 9) > 100
        ctx.residual_weights(FS0, FS1, FLOW, out, gate=dev(g))
        assert (out.cpu().numpy() == want(trips, None, [g.astype(np.uint8)] * N)).all()
        one = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        ctx.residual_weights(FS0[:1], FS1[:1], FLOW[:1], one)
        assert (one.cpu().numpy() == want(trips[:1])[0]).all()
        with pytest.raises(ValueError, match="5 and 4 frame slots for 5 flow slots"):
            ctx.residual_weights(FS0, FS1[:4], FLOW, out)
        with pytest.raises(ValueError, match="2 weight maps for 5 items"):
            ctx.residual_weights(FS0, FS1, FLOW, out[:2])


# ---- 2. hostile content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_hostile_content(size):
    w, h = size
    trips = [rr.hostile(w, h, s) for s in rr.SEEDS]
    with context(w, h) as ctx:
        place(ctx, trips)
        for kw in (None, {"soft": 0}, {"alpha": 0.0, "beta": 2.0}, {"alpha": 16.0, "beta": 255.0}):
            got, rest = run(ctx, w, h, params=kw, pitch=w + 1, offset=1)
            ref = want(trips, kw)
            assert (got == ref).all(), kw
            assert (rest == FILL).all()
            assert ref[0, 1, 1] == 0 and ref[0, 2, 2] == 0 and ref[0, 3, 2] == 0


# ---- 3. side effects -----------------------------------------------------------------------------------------------------------
def test_frames_flows_and_records_are_only_read():
    w, h = 130, 17
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]

    def state(ctx):
        return (bh.rec_bytes(ctx.pass1_results(FLOW, 1.0)), [ctx.download_flow(s).tobytes() for s in FLOW],
                [ctx.download_frame(s).tobytes() for s in FS0 + FS1])

    with context(w, h) as ctx:
        place(ctx, trips)
        before = state(ctx)
        assert before[1][0] == trips[0][2].tobytes() and before[2][0] == trips[0][0].tobytes() and before[2][N] == trips[0][1].tobytes()
        run(ctx, w, h)
        run(ctx, w, h, params={"soft": 0}, gate=dev(gate_map(w, h, 0)))
        assert state(ctx) == before
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    w, h = 130, 17
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    with context(w, h) as ctx:
        place(ctx, trips)
        buf = torch.full((N * h * w + 16,), FILL, dtype=torch.uint8, device=DEV)
        out = _capi.DevWeights(buf.data_ptr(), h * w, w)
        gate = dev(gate_map(w, h, 0))
        L, byref, iarr = ctx.L, _capi.C.byref, lambda v: _capi._iarr(v)[0]

        def refused(match, code, call):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and "ffl_residual_weights" in str(e.value)
            assert (buf.cpu().numpy() == FILL).all()

        rw = lambda a=FS0, b=FS1, f=FLOW, o=out, p=None, g=None, s=None: (lambda: ctx.residual_weights(a, b, f, o, p, g, s))
        refused(r"n = 0 items outside 1\.\.6", INVALID, rw([], [], []))
        refused(r"n = 7 items outside 1\.\.6", INVALID, rw([0] * 7, [1] * 7, [0, 1, 2, 3, 4, 5, 6]))
        for args, name in (((None, iarr(FS1), iarr(FLOW)), "fslot0"), ((iarr(FS0), None, iarr(FLOW)), "fslot1"),
                           ((iarr(FS0), iarr(FS1), None), "flow_slots")):
            assert L.ffl_residual_weights(ctx._h, N, *args, None, None, byref(out), 0) == INVALID
            assert f"ffl_residual_weights: NULL {name}" in L.ffl_last_error(ctx._h).decode()
        refused(r"flow slot 8 out of range", INVALID, rw(f=[5, 0, 8, 7, 1]))
        refused(r"flow slot -1 out of range", INVALID, rw(f=[5, -1, 3, 7, 1]))
        for _ in range(2):   # the scratch marks are cleared again
            refused(r"flow slot 5 repeated among the flow slots of one call", INVALID, rw(f=[5, 0, 3, 5, 1]))
        refused(r"flow slot 4 holds no flow", STATE, rw(f=[5, 4, 3, 7, 1]))
        refused(r"item 2: frame slot 11 out of range", INVALID, rw(a=[6, 0, 11, 5, 2]))
        refused(r"item 0: frame slot -1 out of range", INVALID, rw(b=[-1, 7, 4, 8, 9]))
        refused(r"item 4: frame slot 10 was never uploaded", STATE, rw(b=[1, 7, 4, 8, 10]))
        refused(r"alpha = 17 outside 0\.\.16", INVALID, rw(p={"alpha": 17.0}))
        refused(r"alpha = -1 outside 0\.\.16", INVALID, rw(p={"alpha": -1.0}))
        refused(r"beta = 0 outside 0 < beta <= 255", INVALID, rw(p={"beta": 0.0}))
        refused(r"beta = 256 outside 0 < beta <= 255", INVALID, rw(p={"beta": 256.0}))
        refused(r"beta = nan outside", INVALID, rw(p={"beta": float("nan")}))
        refused(r"alpha = inf outside", INVALID, rw(p={"alpha": float("inf")}))
        refused(r"soft = 3 is neither", INVALID, rw(p={"soft": 3}))
        assert L.ffl_residual_weights(ctx._h, N, iarr(FS0), iarr(FS1), iarr(FLOW), None, None, None, 0) == INVALID
        assert "NULL out descriptor" in L.ffl_last_error(ctx._h).decode()
        refused(r"NULL weight base", INVALID, rw(o=_capi.DevWeights(0, h * w, w)))
        refused(r"overlap: weight row pitch 129 below the width 130", INVALID, rw(o=_capi.DevWeights(buf.data_ptr(), h * w, w - 1)))
        refused(r"overlap: weight item stride 2209 below one map's extent 2210", INVALID, rw(o=_capi.DevWeights(buf.data_ptr(), h * w - 1, w)))
        refused(r"negative weight stride", INVALID, rw(o=_capi.DevWeights(buf.data_ptr(), -h * w, w)))
        refused(r"overlap: out item stride 0 with n = 5 maps to write", INVALID, rw(o=_capi.DevWeights(buf.data_ptr(), 0, w)))
        refused(r"overlap: weight row pitch 100 below the width 130", INVALID, rw(g=_capi.DevWeights(gate.data_ptr(), 0, 100)))
        refused(r"NULL weight base", INVALID, rw(g=_capi.DevWeights(0, 0, w)))
        # memory that is not the device's, or not all inside one allocation
        pin = ctx.pinned_frames(N, channels=1)
        refused(r"out is page-locked host memory.*device memory", INVALID, rw(o=_capi.DevWeights(pin.ctypes.data, h * w, w)))
        refused(r"the gate maps is page-locked host memory.*device memory", INVALID, rw(g=_capi.DevWeights(pin.ctypes.data, 0, w)))
        torch.cuda.empty_cache()
        big = torch.full((18 << 20,), FILL, dtype=torch.uint8, device=DEV)   # an allocation of its own
        past = big.data_ptr() + big.numel() - 4 * w * h                     # room for four maps, five asked for
        refused(rf"out spans {5 * w * h} bytes, {w * h} more than its allocation holds", INVALID, rw(o=_capi.DevWeights(past, h * w, w)))
        refused(rf"the gate maps spans {5 * w * h} bytes, {w * h} more than its allocation holds", INVALID,
                rw(g=_capi.DevWeights(past, h * w, w)))
        assert (big.cpu().numpy() == FILL).all()
        # out overlapping gate
        refused(r"overlap: out \(11050 bytes\) and gate \(2210 bytes\) share memory", INVALID,
                rw(g=_capi.DevWeights(buf.data_ptr() + 4 * h * w, 0, w)))
        refused(r"overlap: out .* and gate .* share memory", INVALID, rw(g=_capi.DevWeights(buf.data_ptr(), h * w, w)))
        with pytest.raises(ValueError, match="not device memory"):
            ctx.residual_weights(FS0, FS1, FLOW, torch.empty((N, h, w), dtype=torch.uint8))
        # a capturing stream
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                rw(s=torch.cuda.current_stream())()
            except _capi.FFLError as err:
                codes.append((err.code, "capturing" in str(err), "ffl_residual_weights" in str(err)))
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [(STATE, True, True)] and float(x.sum()) == 16.0
        assert (buf.cpu().numpy() == FILL).all()
        # nothing was queued, and the context computes a correct call next
        got, rest = run(ctx, w, h)
        assert (got == want(trips)).all() and (rest == FILL).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 5. the stream contract ----------------------------------------------------------------------------------------------------
def test_side_stream_may_overwrite_the_gate_and_read_the_maps_at_once():
    w, h = 257, 40
    trips = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    gates = np.stack([gate_map(w, h, 20 + i) for i in range(N)])
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        place(ctx, trips)
        gate = dev(gates)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                gate.copy_(dev(gates), non_blocking=True)
                ctx.residual_weights(FS0, FS1, FLOW, out, gate=gate, stream=side)
                gate.zero_()                      # runs behind the call's read of the gate
                got = out.cpu().numpy()           # runs behind the call's write of the maps
                assert (got == want(trips, None, gates)).all()
                out.fill_(FILL)
        torch.cuda.current_stream().wait_stream(side)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_an_upload_into_a_frame_slot_runs_behind_the_call_that_reads_it():
    """The call is held back behind work queued on the caller's stream (a chain of matrix products, some tens of milliseconds); the
    frame slots it reads are overwritten at once.  The uploads must wait for the call: the maps are those of the frames the
    slots held when the call was made, and a second call sees the new frames."""
    w, h = 257, 40
    old = [rr.synthetic(w, h, s) for s in rr.SEEDS]
    new = [rr.synthetic(w, h, s) for s in rr.SEEDS[1:] + rr.SEEDS[:1]]
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        place(ctx, old)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        a = torch.randn(4096, 4096, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(30):
                a = (a @ a).clamp_(-1, 1)
            ctx.residual_weights(FS0, FS1, FLOW, out, stream=side)
        for (I0, I1, _), s0, s1 in zip(new, FS0, FS1):   # on the host these run at once; on the device behind the call
            ctx.upload_frames(s0, [np.ascontiguousarray(I0)])
            ctx.upload_frames(s1, [np.ascontiguousarray(I1)])
        side.synchronize()
        assert (out.cpu().numpy() == want(old)).all()
        ctx.residual_weights(FS0, FS1, FLOW, out)
        assert (out.cpu().numpy() == np.stack([rr.residual(n_[0], n_[1], o_[2]) for n_, o_ in zip(new, old)])).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 6. the schedule -----------------------------------------------------------------------------------------------------------
SW, SH = 64, 48
SPARAMS = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
           "cut_threshold": 7.0, "hip_axes": {"roll": "tangential"}}


def engine_ctx(B, smallest=False):
    """the rings of an engine of depth 2, or the smallest legal ones (depth 1)"""
    d = 1 if smallest else 2
    return _capi.Context(SW, SH, max_batch=B, frame_slots=pipeline.min_frame_slots(B, d), flow_slots=pipeline.min_flow_slots(B, d))


def by_hand(fr, kw=None, gate=None, compensate=None):
    """The chunk in chunk_by_hand.by_hand's form, on a context that holds it whole, every step ONE call over slots 0 .. n-1: the
    flow call, residual_weights on the raw fields, (compensate=: motion_fit under the maps, motion_subtract in place,)
    pass1_weighted, one radial_window_axes_weighted over the whole chunk.  dict(post, motion, maps, raw, flows)."""
    n = len(fr) - 1
    slots = list(range(n))
    with bh.hand_context(SW, SH, n) as ctx:
        ctx.upload_frames(0, [np.ascontiguousarray(f) for f in fr])
        f0, f1 = slots, [j + 1 for j in slots]
        ctx.flow_pairs(f0, f1, slots)
        raw = ctx.export_flows(slots).cpu().numpy()
        maps = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        ctx.residual_weights(f0, f1, slots, maps, kw, gate)
        motion = None
        if compensate is not None:
            mo = pipeline.motion_buffer(ctx, n)
            ctx.motion_fit(slots, _capi.motion_choice(compensate), weights=maps, out=mo)
            ctx.motion_subtract(slots, slots, mo, False)
            motion = mo.cpu().numpy().tobytes()
        ctx.pass1_weighted(slots, maps)
        out = pipeline.post_buffer(ctx, n, axes=True)
        ctx.radial_window_axes_weighted(slots, 0, n, maps, out, pipeline.SMOOTH_RADIUS, 7.0, False)
        frames = np.stack([ctx.download_frame(j) for j in range(n + 1)])
        assert ctx.graph_stats()["capture_failures"] == 0
        return dict(post=out.cpu().numpy().tobytes(), motion=motion, maps=maps.cpu().numpy(), raw=raw,
                    flows=ctx.export_flows(slots).cpu().numpy(), frames=frames)


def restated(res, kw=None, gate=None):
    """the restatement applied to the downloaded frames and the exported raw fields of a by-hand result"""
    n = len(res["raw"])
    return np.stack([rr.residual(res["frames"][j], res["frames"][j + 1], res["raw"][j], gate=gate, **prm(kw)) for j in range(n)])


@pytest.mark.parametrize("frames,B,smallest", [(12, 4, False), (12, 5, True), (27, 4, True)], ids=["12f-B4", "12f-B5-min", "27f-B4-min"])
def test_process_chunk_equals_the_calls_by_hand(frames, B, smallest):
    """12 frames with max_batch 4 on the rings of depth 2 (15 frame slots, 25 flow slots); 12 frames with max_batch 5 on the
    smallest rings the engine accepts (12 frame slots, which those 12 frames fill exactly once, and 23 flow slots); 27 frames
    with max_batch 4 on the smallest rings: the 10 frame slots wrap nearly three times, so that from batch 2 on every upload
    recycles slots a residual call queued two batches earlier read, with nothing on the host waiting in between, and the 21
    flow slots wrap once under the 26 pairs."""
    fr = list(sine_translate_frames(frames, SW, SH, seed=5))
    n = frames - 1
    res = by_hand(fr)
    assert (res["frames"] == np.stack(fr)).all()
    assert (res["maps"] == restated(res)).all()
    assert len(np.unique(res["maps"])) > 32 and (res["maps"] == 255).any() and (res["maps"] == 0).any()
    with engine_ctx(B, smallest) as ctx:
        eng = pipeline.PairEngine(ctx)
        assert (ctx.frame_slots < frames) == (frames == 27) and (ctx.flow_slots < n) == (frames == 27)
        T, T0 = (torch.empty((n, SH, SW, 2), device=DEV) for _ in range(2))
        M = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        buf = eng.process_chunk(fr, flows_out=T, weights="residual", weights_out=M, post_out=True)
        assert buf.cpu().numpy().tobytes() == res["post"]
        assert (M.cpu().numpy() == res["maps"]).all()
        assert (T.cpu().numpy() == res["raw"]).all()
        eng.process_chunk(fr, flows_out=T0)
        assert torch.equal(T, T0)
        # the same records when the maps the mode made are handed back as caller maps
        assert eng.process_chunk(fr, weights=M).cpu().numpy().tobytes() == res["post"]
        assert ctx.graph_stats()["capture_failures"] == 0


def test_process_chunk_with_compensation():
    """the order behind a batch: the maps from the raw fields, the fit under the maps, the subtraction, the weighted calls"""
    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    n, B = 11, 4
    res = by_hand(fr, compensate="translation")
    assert (res["maps"] == restated(res)).all() and res["flows"].tobytes() != res["raw"].tobytes()
    plain = by_hand(fr)
    assert (plain["maps"] == res["maps"]).all() and plain["post"] != res["post"]
    with engine_ctx(B) as ctx:
        eng = pipeline.PairEngine(ctx)
        M = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        T = torch.empty((n, SH, SW, 2), device=DEV)
        mo = pipeline.motion_buffer(ctx, n)
        buf = eng.process_chunk(fr, weights="residual", weights_out=M, compensate="translation", motion_out=mo, flows_out=T)
        assert buf.cpu().numpy().tobytes() == res["post"]
        assert mo.cpu().numpy().tobytes() == res["motion"]
        assert (M.cpu().numpy() == res["maps"]).all()
        assert (T.cpu().numpy() == res["flows"]).all()
        with pytest.raises(ValueError, match="compensate= together with weights='consistency' is not supported"):
            eng.process_chunk(fr, weights="consistency", compensate="translation")
        assert ctx.graph_stats()["capture_failures"] == 0


def test_process_chunk_parameters_gate_and_refusals():
    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    n, B = 11, 4
    kw = {"alpha": 0.25, "beta": 2.0, "soft": 0}
    g = gate_map(SW, SH, 3)
    res = by_hand(fr, kw, dev(g))
    assert (res["maps"] == restated(res, kw, g)).all()
    with engine_ctx(B) as ctx:
        eng = pipeline.PairEngine(ctx)
        M = torch.empty((n, SH, SW), dtype=torch.uint8, device=DEV)
        buf = eng.process_chunk(fr, weights="residual", residual=kw, weights_out=M, weights_gate=dev(g))
        assert buf.cpu().numpy().tobytes() == res["post"] and (M.cpu().numpy() == res["maps"]).all()
        # without weights_out the maps live in a tensor of the chunk's own; a ResidualParams is taken as it is
        got = eng.process_chunk(fr, weights="residual", residual=_capi.ResidualParams(**kw), weights_gate=dev(g))
        assert got.cpu().numpy().tobytes() == res["post"]
        with pytest.raises(ValueError, match=r"weights_out must be a uint8 device tensor of shape \(11, 48, 64\)"):
            eng.process_chunk(fr, weights="residual", weights_out=M[:5])
        with pytest.raises(ValueError, match="residual= needs weights='residual'"):
            eng.process_chunk(fr, residual=kw)
        with pytest.raises(ValueError, match="residual= needs weights='residual'"):
            eng.process_chunk(fr, weights="consistency", residual=kw)
        with pytest.raises(ValueError, match="consistency= needs weights='consistency', not weights='residual'"):
            eng.process_chunk(fr, weights="residual", consistency={"soft": 0})
        with pytest.raises(ValueError, match="got 'census'; or 'residual', the mode that needs no backward flow"):
            eng.process_chunk(fr, weights="census")
        with pytest.raises(ValueError, match="alpha = 20 outside"):
            eng.process_chunk(fr, weights="residual", residual={"alpha": 20})
        with pytest.raises(ValueError, match="weights_gate: one static"):
            eng.process_chunk(fr, weights="residual", weights_gate=dev(np.stack([g] * n)))
        with pytest.raises(ValueError, match="center='variance' together with weights= is not supported"):
            eng.process_chunk(fr, weights="residual", center="variance")
        T = torch.zeros((n, SH, SW, 2), device=DEV)
        with pytest.raises(ValueError, match="process_flows: weights='residual' needs the frames.*Context.residual_weights"):
            eng.process_flows(T, weights="residual")
        with pytest.raises(ValueError, match="flows_to_scripts: hip_weights = 'residual' needs the frames.*Context.residual_weights"):
            pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**SPARAMS, "hip_weights": "residual"})
        with pytest.raises(ValueError, match="hip_center together with hip_weights"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_weights": "residual", "hip_center": "variance"})
        for fn, args in ((pipeline.process_chunk_sharded, (eng, fr, 0, 1, None)), (pipeline.process_chunk_sharded_halo, (eng, fr, 0, 1, None)),
                         (pipeline.process_chunk_local_ranks, ([eng], fr))):
            with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
                fn(*args, weights="residual")
        assert ctx.graph_stats()["capture_failures"] == 0
    with _capi.Context(SW, SH, max_batch=1, frame_slots=4, flow_slots=pipeline.min_flow_slots(1)) as ctx:   # no batch is halved
        assert pipeline.PairEngine(ctx).process_chunk(fr, weights="residual", residual=kw, weights_gate=dev(g)).cpu().numpy().tobytes() == res["post"]


def test_an_engine_without_the_hook_keeps_serving_the_plain_chunk():
    class Old(pipeline.PairEngine):
        def pass1_pairs(self, frames, pairs, slot_of, pov_mode=False, cut_threshold=7.0, on_batch=None, algo=None,
                        farneback=pipeline.OWN, window=pipeline.OWN, queued=None, batch=None, reverse_slot_of=None, behind=None):
            return super().pass1_pairs(frames, pairs, slot_of, pov_mode, cut_threshold, on_batch, algo, farneback, window, queued,
                                       batch, reverse_slot_of, behind)

    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    with engine_ctx(4) as ctx:
        want_dots, want_recs = pipeline.PairEngine(ctx).process_chunk(fr)
        dots, recs = Old(ctx).process_chunk(fr)
        assert dots.tobytes() == want_dots.tobytes() and bh.rec_bytes(recs) == bh.rec_bytes(want_recs)
        a = Old(ctx).process_chunk(fr, post_out=True).cpu().numpy().tobytes()
        assert a == pipeline.PairEngine(ctx).process_chunk(fr, post_out=True).cpu().numpy().tobytes()


def test_frames_to_scripts_under_residual_maps():
    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    plan = pipeline.pair_plan(30.0, len(fr), SPARAMS)
    assert len(plan) == 1
    chunk = plan[0]
    kw = {"beta": 2.0}
    g = gate_map(SW, SH, 4)
    with engine_ctx(4) as ctx:
        eng = pipeline.PairEngine(ctx)
        for extra, ckw in (({}, {}), ({"hip_residual": kw, "hip_weights_gate": g}, {"residual": kw, "weights_gate": dev(g)})):
            buf = eng.process_chunk([fr[i] for i in chunk], weights="residual", **ckw)
            comps, recs = pipeline.post_records(buf, axes=True)
            want_scripts = pipeline._scripts_from_chunks([(chunk[:-1], comps, recs)], pipeline.script_axes(SPARAMS), 30.0, SPARAMS)
            assert want_scripts[""] and want_scripts["roll"]
            params = {**SPARAMS, "hip_weights": "residual", **extra}
            assert pipeline.frames_to_scripts(eng, fr, 30.0, params) == want_scripts
            assert pipeline.frames_to_actions(eng, fr, 30.0, params) == want_scripts[""]
        with pytest.raises(ValueError, match="hip_residual needs hip_weights = 'residual'"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_residual": kw})
        with pytest.raises(ValueError, match="hip_consistency needs hip_weights = 'consistency', got 'residual'"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_weights": "residual", "hip_consistency": {"soft": 0}})
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 7. the rule on real flow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (130, 72)], ids=gid)
def test_translating_texture_has_a_small_residual_away_from_the_border(size):
    """Frame 1 is frame 0's texture displaced by the integers (3, -2) (two windows of one larger texture, seed 5), the flow is
    the tuned Farneback's: under the defaults every pixel at least 16 px from the border whose landing is inside has W >= 128.
    The CPU oracle's flow for the same frames gives, through the restatement, a minimum of 193 at both sizes (its largest flow
    error there is 0.71 px).  The inputs matter: on the texture of seed 3 at 130x72 the oracle's own flow is off by up to 2.5 px
    inside that region and the restatement gives 71 there -- the map doing its work, not a case for this bound."""
    w, h = size
    dx, dy, m = 3, -2, 8
    big = sine_translate_frames(1, w + 2 * m, h + 2 * m, seed=5, amp=(0.0, 0.0))[0]
    f0 = np.ascontiguousarray(big[m:m + h, m:m + w])
    f1 = np.ascontiguousarray(big[m - dy:m - dy + h, m - dx:m - dx + w])
    assert (f1[8:h - 8, 8:w - 8] == f0[8 - dy:h - 8 - dy, 8 - dx:w - 8 - dx]).all()
    with _capi.Context(w, h, max_batch=2, frame_slots=2, flow_slots=2) as ctx:
        ctx.upload_frames(0, [f0, f1])
        ctx.flow_pairs([0], [1], [0])
        out = torch.empty((1, h, w), dtype=torch.uint8, device=DEV)
        ctx.residual_weights([0], [1], [0], out)
        got = out.cpu().numpy()[0]
        F = ctx.download_flow(0)
    ref, outside = rr.residual(f0, f1, F, with_outside=True)
    assert (got == ref).all()
    inner, lands = got[16:h - 16, 16:w - 16], ~outside[16:h - 16, 16:w - 16]
    err = np.abs(F - np.array([dx, dy], np.float32))[16:h - 16, 16:w - 16].max()
    print(f"{w}x{h}: min W of the inner pixels that land inside = {int(inner[lands].min())}, mean {inner.mean():.1f}, "
          f"largest flow error there {err:.3f} px, {int((~lands).sum())} land outside")
    assert lands.any() and (inner[lands] >= 128).all()
    zero = rr.residual(f0, f1, np.zeros_like(F))
    assert zero.mean() < got.mean()
