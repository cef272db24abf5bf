"""GPU side of the forward-backward consistency maps (ffl_consistency_weights, k_consistency; DESIGN.md section 18, appendix
K), everything through the C ABI via _capi and on fields placed with import_flows.

Every output byte is held against the numpy restatement tests/consistency_ref.py with equality; the inputs are that file's
synthetic pairs, whose conditions tests/test_consistency_ref_host.py asserts.  Sizes: 16x16 (one partly empty wave), 130x17
(a width that is no multiple of 4, an odd height), 257x40 (several workgroups and a 1-pixel tail).  k_consistency has no loop,
so there is no two-trip size."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import consistency_ref as cr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
FILL = 0xA5
N = 3
FWD, BWD = [5, 0, 3], [2, 6, 1]   # not in order, and interleaved in the slot space
ALL = FWD + BWD
PARAMS = [None, {"soft": 0}, {"alpha": 0.05, "beta": 0.25}, {"alpha": 0.0, "beta": 2.0, "soft": 0}, {"alpha": 1.0, "beta": 1e-3}]
INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h):
    return _capi.Context(w, h, max_batch=4, frame_slots=2, flow_slots=8)


def place(ctx, pairs):
    """the pairs' forward fields into FWD, their backward fields into BWD"""
    ctx.import_flows(dev(np.stack([p[0] for p in pairs])), FWD)
    ctx.import_flows(dev(np.stack([p[1] for p in pairs])), BWD)


def gate_map(w, h, seed):
    rng = np.random.default_rng(400 + seed)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    g[rng.random((h, w)) < 0.25] = 0
    return g


def prm(kw):
    return {k: np.float32(v) if k != "soft" else v for k, v in (kw or {}).items()}


def run(ctx, w, h, n=N, params=None, gate=None, pitch=None, offset=0, fwd=FWD, bwd=BWD, stream=None):
    """one call into a buffer pre-filled with FILL: (the n maps, every byte outside them) as numpy arrays"""
    pitch = pitch or w
    item = h * pitch + 5
    raw = torch.full((offset + n * item + 7,), FILL, dtype=torch.uint8, device=DEV)
    ctx.consistency_weights(fwd[:n], bwd[:n], _capi.DevWeights(raw.data_ptr() + offset, item, pitch), params, gate, stream)
    host = raw.cpu().numpy()
    body = host[offset:offset + n * item].reshape(n, item)
    rows = body[:, :h * pitch].reshape(n, h, pitch)
    rest = np.concatenate([host[:offset], host[offset + n * item:], body[:, h * pitch:].ravel(), rows[:, :, w:].ravel()])
    return rows[:, :, :w].copy(), rest


def want(pairs, params=None, gates=None):
    return np.stack([cr.consistency(F, B, gate=None if gates is None else gates[i], **prm(params)) for i, (F, B) in enumerate(pairs)])


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cr.SIZES, ids=gid)
def test_bytes_equal_the_restatement(size):
    w, h = size
    pairs = [cr.synthetic_pair(w, h, s) for s in range(N)]
    shared, each = gate_map(w, h, 0), np.stack([gate_map(w, h, 1 + i) for i in range(N)])
    with context(w, h) as ctx:
        place(ctx, pairs)
        for kw in PARAMS:
            got, rest = run(ctx, w, h, params=kw)
            assert (got == want(pairs, kw)).all(), kw
            assert (rest == FILL).all()
        for kw in (None, {"soft": 0}):
            got, rest = run(ctx, w, h, params=kw, gate=dev(shared))                       # item_stride 0: one gate for all
            assert (got == want(pairs, kw, [shared] * N)).all() and (rest == FILL).all()
            got, rest = run(ctx, w, h, params=kw, gate=dev(each))
            assert (got == want(pairs, kw, each)).all() and (rest == FILL).all()
        ref = want(pairs)
        assert (ref == 0).any() and (ref == 255).any()
        for offset in (0, 1, 2, 3):
            for pitch in (w, w + 1, w + 6):
                got, rest = run(ctx, w, h, pitch=pitch, offset=offset)
                assert (got == ref).all(), (offset, pitch)
                assert (rest == FILL).all(), (offset, pitch)
        got, rest = run(ctx, w, h, n=1, fwd=[6], bwd=[5], pitch=w + 3, offset=1)            # the roles swapped, one item
        assert (got[0] == cr.consistency(pairs[1][1], pairs[0][0])).all() and (rest == FILL).all()
        # a gate whose rows are padded and whose base is odd
        pad = torch.zeros((N, h, w + 3), dtype=torch.uint8, device=DEV)
        pad[:, :, 1:w + 1] = dev(each)
        got, _ = run(ctx, w, h, gate=pad[:, :, 1:w + 1])
        assert (got == want(pairs, None, each)).all()
        assert ctx.graph_stats()["capture_failures"] == 0


def test_tensor_outputs_and_bool_gate():
    w, h = 130, 17
    pairs = [cr.synthetic_pair(w, h, s) for s in range(N)]
    with context(w, h) as ctx:
        place(ctx, pairs)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        assert ctx.consistency_weights(FWD, BWD, out, _capi.ConsistencyParams(soft=0)) is out
        assert (out.cpu().numpy() == want(pairs, {"soft": 0})).all()
        g = gate_map(w, h, 9) > 100
        ctx.consistency_weights(FWD, BWD, out, gate=dev(g))
        assert (out.cpu().numpy() == want(pairs, None, [g.astype(np.uint8)] * N)).all()
        one = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        ctx.consistency_weights(FWD[:1], BWD[:1], one)
        assert (one.cpu().numpy() == want(pairs[:1])[0]).all()
        with pytest.raises(ValueError, match="3 forward slots for 2 backward slots"):
            ctx.consistency_weights(FWD, BWD[:2], out)
        with pytest.raises(ValueError, match="2 weight maps for 3 items"):
            ctx.consistency_weights(FWD, BWD, out[:2])


# ---- 2. hostile content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", cr.SIZES, ids=gid)
def test_hostile_content(size):
    w, h = size
    pairs = [cr.hostile_pair(w, h, s) for s in range(N)]
    with context(w, h) as ctx:
        place(ctx, pairs)
        for kw in (None, {"soft": 0}, {"alpha": 0.0, "beta": 2.0}):
            got, rest = run(ctx, w, h, params=kw, pitch=w + 1, offset=1)
            ref = want(pairs, kw)
            assert (got == ref).all(), kw
            assert (rest == FILL).all()
            assert ref[0, 1, 1] == 0 and ref[0, 2, 2] == 0 and ref[0, h // 2 - 3, w // 2 - 1] == 255


# ---- 3. side effects -----------------------------------------------------------------------------------------------------------
def test_flows_and_records_are_only_read():
    w, h = 130, 17
    pairs = [cr.synthetic_pair(w, h, s) for s in range(N)]

    def state(ctx):
        recs = [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in
                ctx.pass1_results(FWD, 1.0) + ctx.pass1_results(BWD, 1.0)]
        return recs, [ctx.download_flow(s).tobytes() for s in ALL]

    with context(w, h) as ctx:
        place(ctx, pairs)
        before = state(ctx)
        assert before[1][0] == pairs[0][0].tobytes() and before[1][N] == pairs[0][1].tobytes()
        run(ctx, w, h)
        run(ctx, w, h, params={"soft": 0}, gate=dev(gate_map(w, h, 0)))
        assert state(ctx) == before
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    w, h = 130, 17
    pairs = [cr.synthetic_pair(w, h, s) for s in range(N)]
    with context(w, h) as ctx:
        place(ctx, pairs)   # slots 4 and 7 hold nothing
        buf = torch.full((N * h * w + 16,), FILL, dtype=torch.uint8, device=DEV)
        out = _capi.DevWeights(buf.data_ptr(), h * w, w)
        gate = dev(gate_map(w, h, 0))
        L = ctx.L

        def refused(match, code, call):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and "ffl_consistency_weights" in str(e.value)
            assert (buf.cpu().numpy() == FILL).all()

        cw = lambda f=FWD, b=BWD, o=out, p=None, g=None, s=None: (lambda: ctx.consistency_weights(f, b, o, p, g, s))
        refused(r"n = 0 items outside 1\.\.4", INVALID, cw([], []))
        refused(r"n = 5 items outside 1\.\.4", INVALID, cw([0, 1, 2, 3, 5], [6, 6, 6, 6, 6]))
        for args, name in (((None, _capi._iarr(BWD)[0]), "fwd_slots"), ((_capi._iarr(FWD)[0], None), "bwd_slots")):
            assert L.ffl_consistency_weights(ctx._h, N, args[0], args[1], None, None, _capi.C.byref(out), 0) == INVALID
            assert f"ffl_consistency_weights: NULL {name}" in L.ffl_last_error(ctx._h).decode()
        refused(r"flow slot 8 out of range", INVALID, cw([5, 0, 8]))
        refused(r"flow slot -1 out of range", INVALID, cw(b=[2, -1, 1]))
        for _ in range(2):   # the scratch marks are cleared again
            refused(r"flow slot 5 repeated among the forward and backward slots", INVALID, cw(b=[2, 5, 1]))
        refused(r"flow slot 0 repeated among", INVALID, cw([0, 0, 3]))
        refused(r"flow slot 4 holds no flow", STATE, cw([5, 4, 3]))
        refused(r"flow slot 7 holds no flow", STATE, cw(b=[2, 6, 7]))
        refused(r"alpha = 2 outside 0\.\.1", INVALID, cw(p={"alpha": 2.0}))
        refused(r"beta = 0 outside 0 < beta <= 1e6", INVALID, cw(p={"beta": 0.0}))
        refused(r"beta = nan outside", INVALID, cw(p={"beta": float("nan")}))
        refused(r"soft = 3 is neither", INVALID, cw(p={"soft": 3}))
        assert L.ffl_consistency_weights(ctx._h, N, _capi._iarr(FWD)[0], _capi._iarr(BWD)[0], None, None, None, 0) == INVALID
        assert "NULL out descriptor" in L.ffl_last_error(ctx._h).decode()
        refused(r"NULL weight base", INVALID, cw(o=_capi.DevWeights(0, h * w, w)))
        refused(r"overlap: weight row pitch 129 below the width 130", INVALID, cw(o=_capi.DevWeights(buf.data_ptr(), h * w, w - 1)))
        refused(r"overlap: weight item stride 2209 below one map's extent 2210", INVALID, cw(o=_capi.DevWeights(buf.data_ptr(), h * w - 1, w)))
        refused(r"negative weight stride", INVALID, cw(o=_capi.DevWeights(buf.data_ptr(), -h * w, w)))
        refused(r"overlap: out item stride 0 with n = 3 maps to write", INVALID, cw(o=_capi.DevWeights(buf.data_ptr(), 0, w)))
        refused(r"overlap: weight row pitch 100 below the width 130", INVALID, cw(g=_capi.DevWeights(gate.data_ptr(), 0, 100)))
        refused(r"NULL weight base", INVALID, cw(g=_capi.DevWeights(0, 0, w)))
        # memory that is not the device's, or not all inside one allocation
        pin = ctx.pinned_frames(N, channels=1)
        refused(r"out is page-locked host memory.*device memory", INVALID, cw(o=_capi.DevWeights(pin.ctypes.data, h * w, w)))
        refused(r"the gate maps is page-locked host memory.*device memory", INVALID, cw(g=_capi.DevWeights(pin.ctypes.data, 0, w)))
        torch.cuda.empty_cache()
        big = torch.full((18 << 20,), FILL, dtype=torch.uint8, device=DEV)   # an allocation of its own
        past = big.data_ptr() + big.numel() - 2 * w * h                     # room for two maps, three asked for
        refused(rf"out spans {3 * w * h} bytes, {w * h} more than its allocation holds", INVALID, cw(o=_capi.DevWeights(past, h * w, w)))
        refused(rf"the gate maps spans {3 * w * h} bytes, {w * h} more than its allocation holds", INVALID,
                cw(g=_capi.DevWeights(past, h * w, w)))
        assert (big.cpu().numpy() == FILL).all()
        # out overlapping gate
        refused(r"overlap: out \(6630 bytes\) and gate \(2210 bytes\) share memory", INVALID,
                cw(g=_capi.DevWeights(buf.data_ptr() + 2 * h * w, 0, w)))
        refused(r"overlap: out .* and gate .* share memory", INVALID, cw(g=_capi.DevWeights(buf.data_ptr(), h * w, w)))
        with pytest.raises(ValueError, match="not device memory"):
            ctx.consistency_weights(FWD, BWD, torch.empty((N, h, w), dtype=torch.uint8))
        # a capturing stream
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                cw(s=torch.cuda.current_stream())()
            except _capi.FFLError as err:
                codes.append((err.code, "capturing" in str(err), "ffl_consistency_weights" in str(err)))
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [(STATE, True, True)] and float(x.sum()) == 16.0
        assert (buf.cpu().numpy() == FILL).all()
        # nothing was queued, and the context computes a correct call next
        got, rest = run(ctx, w, h)
        assert (got == want(pairs)).all() and (rest == FILL).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 5. the stream contract ----------------------------------------------------------------------------------------------------
def test_side_stream_may_overwrite_the_gate_and_read_the_maps_at_once():
    w, h = 257, 40
    pairs = [cr.synthetic_pair(w, h, s) for s in range(N)]
    gates = np.stack([gate_map(w, h, 20 + i) for i in range(N)])
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        place(ctx, pairs)
        gate = dev(gates)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                gate.copy_(dev(gates), non_blocking=True)
                ctx.consistency_weights(FWD, BWD, out, gate=gate, stream=side)
                gate.zero_()                      # runs behind the call's read of the gate
                got = out.cpu().numpy()           # runs behind the call's write of the maps
                assert (got == want(pairs, None, gates)).all()
                out.fill_(FILL)
        torch.cuda.current_stream().wait_stream(side)
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 6. the schedule -----------------------------------------------------------------------------------------------------------
SW, SH = 64, 48
SPARAMS = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
           "cut_threshold": 7.0, "hip_axes": {"roll": "tangential"}}


def engine_ctx(B, slots=None):
    return _capi.Context(SW, SH, max_batch=B, frame_slots=2 * B + 2, flow_slots=slots or pipeline.min_flow_slots(B))


def by_hand(fr, B, kw=None, gate=None):
    """the chunk's pairs with Context.flow_pairs both ways, consistency_weights, pass1_weighted and radial_window_axes_weighted:
    (records bytes, maps, forward fields, backward fields)"""
    n, Bh = len(fr) - 1, B // 2
    with _capi.Context(SW, SH, max_batch=B, frame_slots=n + 1, flow_slots=2 * n) as ctx:
        ctx.upload_frames(0, list(fr))
        maps = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        for j0 in range(0, n, Bh):
            js = list(range(j0, min(j0 + Bh, n)))
            f0, f1 = js, [j + 1 for j in js]
            ctx.flow_pairs(f0 + f1, f1 + f0, js + [n + j for j in js])
        for j0 in range(0, n, B):
            js = list(range(j0, min(j0 + B, n)))
            ctx.consistency_weights(js, [n + j for j in js], maps[js[0]:js[-1] + 1], kw, gate)
            ctx.pass1_weighted(js, maps[js[0]:js[-1] + 1])
        out = pipeline.post_buffer(ctx, n, axes=True)
        ctx.radial_window_axes_weighted(list(range(n)), 0, n, maps, out, pipeline.SMOOTH_RADIUS, 7.0, False)
        fwd = np.stack([ctx.download_flow(j) for j in range(n)])
        bwd = np.stack([ctx.download_flow(n + j) for j in range(n)])
        return out.cpu().numpy().tobytes(), maps.cpu().numpy(), fwd, bwd


@pytest.mark.parametrize("frames,B,slots", [(12, 4, None), (12, 5, "min"), (27, 4, None)], ids=["12f-B4", "12f-B5-min", "27f-B4"])
def test_process_chunk_equals_the_calls_by_hand(frames, B, slots):
    """12 frames with max_batch 4 (default flow slots) and with max_batch 5 on the smallest flow-slot count the engine accepts:
    the backward region (4 slots) wraps twice; the forward ring of those contexts (17 and 19 slots) is longer than the 11
    pairs, so a third case of 27 frames lets it wrap too (26 pairs over 17 slots)."""
    fr = list(sine_translate_frames(frames, SW, SH, seed=5))
    n = frames - 1
    rec, maps, fwd, bwd = by_hand(fr, B)
    assert (maps == np.stack([cr.consistency(fwd[j], bwd[j]) for j in range(n)])).all()
    with engine_ctx(B, pipeline.min_flow_slots(B) if slots == "min" else None) as ctx:
        eng = pipeline.PairEngine(ctx)
        ring = ctx.flow_slots - (eng.depth + 1) * (B // 2)
        assert (ring < n) == (frames == 27) and (eng.depth + 1) * (B // 2) < n
        T, T0 = (torch.empty((n, SH, SW, 2), device=DEV) for _ in range(2))
        M = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        buf = eng.process_chunk(fr, flows_out=T, weights="consistency", weights_out=M)
        assert buf.cpu().numpy().tobytes() == rec
        assert (M.cpu().numpy() == maps).all()
        assert (T.cpu().numpy() == fwd).all()
        eng.process_chunk(fr, flows_out=T0)
        assert torch.equal(T, T0)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_process_chunk_parameters_gate_and_refusals():
    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    n, B = 11, 4
    kw = {"alpha": 0.02, "beta": 0.125, "soft": 0}
    g = gate_map(SW, SH, 3)
    rec, maps, fwd, bwd = by_hand(fr, B, kw, dev(g))
    assert (maps == np.stack([cr.consistency(fwd[j], bwd[j], gate=g, **prm(kw)) for j in range(n)])).all()
    with engine_ctx(B) as ctx:
        eng = pipeline.PairEngine(ctx)
        M = torch.empty((n, SH, SW), dtype=torch.uint8, device=DEV)
        buf = eng.process_chunk(fr, weights="consistency", consistency=kw, weights_out=M, weights_gate=dev(g))
        assert buf.cpu().numpy().tobytes() == rec and (M.cpu().numpy() == maps).all()
        # without weights_out the maps live in a tensor of the chunk's own
        assert eng.process_chunk(fr, weights="consistency", consistency=kw, weights_gate=dev(g)).cpu().numpy().tobytes() == rec
        with pytest.raises(ValueError, match=r"weights_out must be a uint8 device tensor of shape \(11, 48, 64\)"):
            eng.process_chunk(fr, weights="consistency", weights_out=M[:5])
        with pytest.raises(ValueError, match="need weights='consistency'"):
            eng.process_chunk(fr, weights_out=M)
        with pytest.raises(ValueError, match="one of \\('consistency',\\), got 'census'"):
            eng.process_chunk(fr, weights="census")
        with pytest.raises(ValueError, match="alpha = 3 outside"):
            eng.process_chunk(fr, weights="consistency", consistency={"alpha": 3})
        with pytest.raises(ValueError, match="center='variance' together with weights= is not supported"):
            eng.process_chunk(fr, weights="consistency", center="variance")
        T = torch.zeros((n, SH, SW, 2), device=DEV)
        with pytest.raises(ValueError, match="process_flows: weights='consistency' needs the backward fields"):
            eng.process_flows(T, weights="consistency")
        with pytest.raises(ValueError, match="flows_to_scripts: hip_weights = 'consistency' needs the backward fields"):
            pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**SPARAMS, "hip_weights": "consistency"})
        with pytest.raises(ValueError, match="hip_center together with hip_weights"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_weights": "consistency", "hip_center": "variance"})
        for fn, args in ((pipeline.process_chunk_sharded, (eng, fr, 0, 1, None)), (pipeline.process_chunk_sharded_halo, (eng, fr, 0, 1, None)),
                         (pipeline.process_chunk_local_ranks, ([eng], fr))):
            with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
                fn(*args, weights="consistency")
        assert ctx.graph_stats()["capture_failures"] == 0
    with _capi.Context(SW, SH, max_batch=1, frame_slots=4, flow_slots=pipeline.min_flow_slots(1)) as ctx:
        with pytest.raises(ValueError, match="weights='consistency' needs max_batch >= 2"):
            pipeline.PairEngine(ctx).process_chunk(fr, weights="consistency")


def test_frames_to_scripts_under_consistency_maps():
    fr = list(sine_translate_frames(12, SW, SH, seed=5))
    plan = pipeline.pair_plan(30.0, len(fr), SPARAMS)
    assert len(plan) == 1
    chunk = plan[0]
    kw = {"beta": 0.25}
    g = gate_map(SW, SH, 4)
    with engine_ctx(4) as ctx:
        eng = pipeline.PairEngine(ctx)
        for extra, ckw in (({}, {}), ({"hip_consistency": kw, "hip_weights_gate": g}, {"consistency": kw, "weights_gate": dev(g)})):
            buf = eng.process_chunk([fr[i] for i in chunk], weights="consistency", **ckw)
            comps, recs = pipeline.post_records(buf, axes=True)
            want_scripts = pipeline._scripts_from_chunks([(chunk[:-1], comps, recs)], pipeline.script_axes(SPARAMS), 30.0, SPARAMS)
            assert want_scripts[""] and want_scripts["roll"]
            params = {**SPARAMS, "hip_weights": "consistency", **extra}
            assert pipeline.frames_to_scripts(eng, fr, 30.0, params) == want_scripts
            assert pipeline.frames_to_actions(eng, fr, 30.0, params) == want_scripts[""]
        with pytest.raises(ValueError, match="hip_consistency needs hip_weights = 'consistency'"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_consistency": kw})
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 7. the rule on real flow --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(64, 64), (130, 72)], ids=gid)
def test_translating_texture_is_consistent_away_from_the_border(size):
    """frames 0 and 1 of a translating texture: in hard mode at least 99 % of the pixels more than 8 from the border are 255
    (the CPU oracle's forward and backward fields give 100 % at both sizes)"""
    w, h = size
    fr = sine_translate_frames(3, w, h, seed=3)
    with _capi.Context(w, h, max_batch=2, frame_slots=2, flow_slots=2) as ctx:
        ctx.upload_frames(0, [fr[0], fr[1]])
        ctx.flow_pairs([0, 1], [1, 0], [0, 1])
        out = torch.empty((1, h, w), dtype=torch.uint8, device=DEV)
        ctx.consistency_weights([0], [1], out, {"soft": 0})
        got = out.cpu().numpy()[0]
        F, B = ctx.download_flow(0), ctx.download_flow(1)
    assert (got == cr.consistency(F, B, soft=0)).all()
    inner = got[9:h - 9, 9:w - 9]
    share = float((inner == 255).mean())
    print(f"{w}x{h}: {100 * share:.2f} % of the inner pixels are 255, mean |F| = {float(np.abs(F).mean()):.3f}")
    assert set(np.unique(got)) <= {0, 255}
    assert share >= 0.99
