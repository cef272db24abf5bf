"""GPU side of the texture (structure-tensor) maps (ffl_texture_weights, k_texture), everything
through the C ABI via _capi, on frames placed with upload_frames.

Every output byte is held against the numpy restatement tests/texture_ref.py with equality; the inputs are that file's
frames, whose conditions tests/test_texture_ref_host.py asserts.  k_texture's tile is 64 x 16 output pixels.  Sizes: 16x16
(smaller than a tile, and smaller than the window of radius 8: every window position clamps), 130x17 (three tile columns, the
last 2 wide; two tile rows, the last 1 high; a width that is 2 mod 4), 257x40 (five tile columns with a 1-pixel tail, two whole
tile rows and a ragged third), 96x70 (a half tile column, four whole tile rows and a ragged fifth)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import chunk_by_hand as bh
import motion_ref as mr
import residual_ref as rr
import texture_ref as tr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
FILL = 0xA5
N = 5
SLOTS = [6, 0, 3, 2]          # where the four frames go: not in order
FS = [6, 0, 3, 6, 2]          # item i reads frame slot FS[i]: slot 6 twice
ITEM = [0, 1, 2, 0, 3]        # ... which holds frame ITEM[i]
INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
_REF = {}


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h):
    return _capi.Context(w, h, max_batch=6, frame_slots=8, flow_slots=8)   # frame slot 7 is never uploaded


def frames_of(w, h):
    return [tr.thirds(w, h, s) for s in tr.SEEDS] + [rr.to_u8(rr.texture(w, h, 4))]


def place(ctx, frames, slots=SLOTS):
    for f, s in zip(frames, slots):
        ctx.upload_frames(s, [np.ascontiguousarray(f)])


def gate_map(w, h, seed):
    rng = np.random.default_rng(400 + seed)
    g = rng.integers(0, 256, (h, w)).astype(np.uint8)
    g[rng.random((h, w)) < 0.25] = 0
    return g


def ref(I, params=None, gate=None):
    """the restatement, computed once per (frame, parameters) and left unchanged"""
    p = {"radius": tr.RADIUS, "tau": tr.TAU, "soft": tr.SOFT, **(params or {})}
    key = (I.shape, I.tobytes(), p["radius"], float(np.float32(p["tau"])), p["soft"])
    if key not in _REF:
        _REF[key] = tr.texture_map(I, p["radius"], p["tau"], p["soft"])
        _REF[key].setflags(write=False)
    return _REF[key] if gate is None else np.minimum(_REF[key], gate)


def want(frames, params=None, gates=None, item=ITEM):
    return np.stack([ref(frames[j], params, None if gates is None else gates[i]) for i, j in enumerate(item)])


def run(ctx, w, h, n=N, params=None, gate=None, pitch=None, offset=0, fs=FS, stream=None):
    """one call into a buffer pre-filled with FILL: (the n maps, every byte outside them) as numpy arrays"""
    pitch = pitch or w
    item = h * pitch + 5
    raw = torch.full((offset + n * item + 7,), FILL, dtype=torch.uint8, device=DEV)
    ctx.texture_weights(fs[:n], _capi.DevWeights(raw.data_ptr() + offset, item, pitch), params, gate, stream)
    host = raw.cpu().numpy()
    body = host[offset:offset + n * item].reshape(n, item)
    rows = body[:, :h * pitch].reshape(n, h, pitch)
    rest = np.concatenate([host[:offset], host[offset + n * item:], body[:, h * pitch:].ravel(), rows[:, :, w:].ravel()])
    return rows[:, :, :w].copy(), rest


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_bytes_equal_the_restatement(size):
    w, h = size
    frames = frames_of(w, h)
    shared, each = gate_map(w, h, 0), np.stack([gate_map(w, h, 1 + i) for i in range(N)])
    with context(w, h) as ctx:
        place(ctx, frames)
        d_shared, d_each = dev(shared), dev(each)
        for r in tr.RADII:
            for soft in (1, 0):
                kw = {"radius": r, "soft": soft}
                got, rest = run(ctx, w, h, params=kw)
                assert (got == want(frames, kw)).all(), kw
                assert (rest == FILL).all()
                got, rest = run(ctx, w, h, params=kw, gate=d_shared)                          # item_stride 0: one gate for all
                assert (got == want(frames, kw, [shared] * N)).all() and (rest == FILL).all(), kw
                got, rest = run(ctx, w, h, params=kw, gate=d_each)
                assert (got == want(frames, kw, each)).all() and (rest == FILL).all(), kw
        for kw in ({"tau": 1.0}, {"radius": 2, "tau": 300.0}, {"radius": 5, "tau": 65025.0, "soft": 0}, {"radius": 4, "tau": 0.01},
                   {"radius": 6, "tau": 40.0, "soft": 0}):
            got, rest = run(ctx, w, h, params=kw)
            assert (got == want(frames, kw)).all() and (rest == FILL).all(), kw
        base = want(frames)
        if (w, h) != (16, 16):
            assert (base == 0).any() and (base == 255).any() and ((base > 0) & (base < 255)).any()
        for offset in (0, 1, 2, 3):
            for pitch in (w, w + 1, w + 6):
                got, rest = run(ctx, w, h, pitch=pitch, offset=offset)
                assert (got == base).all(), (offset, pitch)
                assert (rest == FILL).all(), (offset, pitch)
        # a gate whose rows are padded and whose base is odd
        pad = torch.zeros((N, h, w + 3), dtype=torch.uint8, device=DEV)
        pad[:, :, 1:w + 1] = d_each
        got, _ = run(ctx, w, h, gate=pad[:, :, 1:w + 1], pitch=w + 2, offset=3)
        assert (got == want(frames, None, each)).all()
        assert ctx.graph_stats()["capture_failures"] == 0


def test_tensor_outputs_and_bool_gate():
    w, h = 130, 17
    frames = frames_of(w, h)
    with context(w, h) as ctx:
        place(ctx, frames)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        assert ctx.texture_weights(FS, out, _capi.TextureParams(radius=3, soft=0)) is out
        assert (out.cpu().numpy() == want(frames, {"radius": 3, "soft": 0})).all()
        g = gate_map(w, h, 9) > 100
        ctx.texture_weights(FS, out, {"radius": 3}, gate=dev(g))
        assert (out.cpu().numpy() == want(frames, {"radius": 3}, [g.astype(np.uint8)] * N)).all()
        one = torch.empty((h, w), dtype=torch.uint8, device=DEV)
        ctx.texture_weights(FS[:1], one)
        assert (one.cpu().numpy() == ref(frames[0])).all()
        with pytest.raises(ValueError, match="2 weight maps for 5 items"):
            ctx.texture_weights(FS, out[:2])
        with pytest.raises(ValueError, match="unknown texture parameter 'alpha'"):
            ctx.texture_weights(FS, out, {"alpha": 1.0})


# ---- 2. hostile content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_hostile_content(size):
    """the 2 x 2 checkerboard (at radius 8 Sxx * Syy = 3.5e14: a 32-bit product gives other bytes), a constant frame (tr = 0: no
    division), a single 255 pixel on 0, and 0 / 255 steps on all four edges and corners"""
    w, h = size
    frames = [f(w, h) for f in tr.HOSTILE.values()]
    with context(w, h) as ctx:
        place(ctx, frames)
        for kw in ({"radius": 8}, {"radius": 8, "soft": 0}, {"radius": 8, "tau": 65025.0}, {"radius": 8, "tau": 16256.25, "soft": 0},
                   {"radius": 1}, {"radius": 1, "soft": 0}, None):
            got, rest = run(ctx, w, h, params=kw, pitch=w + 1, offset=1)
            expect = want(frames, kw)
            assert (got == expect).all(), kw
            assert (rest == FILL).all()
            assert (expect[1] == 0).all()
        Sxx, Sxy, Syy = tr.window_sums(frames[0], 8)
        assert int((Sxx * Syy).max()) > 2 ** 32


# ---- 3. in place ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_gate_equal_to_out_min_combines_in_place(size):
    w, h = size
    frames = frames_of(w, h)
    rng = np.random.default_rng(77)
    with context(w, h) as ctx:
        place(ctx, frames)
        changed = 0   # radius 1 has zeros at every size (test_texture_ref_host.py); wider windows leave 16x16 all 255
        for pitch, offset, kw in ((w, 0, {"radius": 1}), (w + 3, 1, {"radius": 7, "soft": 0}), (w + 6, 2, None)):
            item = h * pitch + 5
            pattern = rng.integers(0, 256, offset + N * item + 7).astype(np.uint8)
            raw = dev(pattern)
            desc = _capi.DevWeights(raw.data_ptr() + offset, item, pitch)
            ctx.texture_weights(FS, desc, kw, desc)
            host = raw.cpu().numpy()
            expect = pattern.copy()
            for i in range(N):
                rows = expect[offset + i * item:offset + i * item + h * pitch].reshape(h, pitch)
                rows[:, :w] = np.minimum(rows[:, :w], ref(frames[ITEM[i]], kw))
            assert (host == expect).all(), (pitch, offset)       # the maps are the minimum, every other byte is untouched
            changed += int((host != pattern).sum())
        assert changed > 0
        # tensors: gate=out reaches the same form, and so does an equal view
        pat = rng.integers(0, 256, (N, h, w)).astype(np.uint8)
        out = dev(pat)
        assert ctx.texture_weights(FS, out, {"radius": 3}, gate=out) is out
        assert (out.cpu().numpy() == np.minimum(pat, want(frames, {"radius": 3}))).all()
        out = dev(pat)
        ctx.texture_weights(FS[1:3], out[1:3], {"radius": 3}, gate=out[1:3])
        expect = pat.copy()
        expect[1:3] = np.minimum(pat[1:3], want(frames, {"radius": 3})[1:3])
        assert (out.cpu().numpy() == expect).all()
        # any other overlap stays refused, before any device work
        buf = dev(pat.ravel())
        o = _capi.DevWeights(buf.data_ptr(), h * w, w)
        for g in (_capi.DevWeights(buf.data_ptr() + h * w, h * w, w),     # shifted by one item
                  _capi.DevWeights(buf.data_ptr(), 0, w),                 # the same base, one static map
                  _capi.DevWeights(buf.data_ptr() + 1, h * w, w)):        # shifted by one byte
            with pytest.raises(_capi.FFLError, match=r"overlap: out \(\d+ bytes\) and gate \(\d+ bytes\) share memory.*not exactly out"):
                ctx.texture_weights(FS[:4], o, None, g)
        if w > 16:
            with pytest.raises(_capi.FFLError, match="overlap: out .* and gate .* share memory"):   # the same base, another pitch
                ctx.texture_weights(FS[:2], _capi.DevWeights(buf.data_ptr(), 2 * h * w, w), None, _capi.DevWeights(buf.data_ptr(), 2 * h * w, w + 1))
        assert (buf.cpu().numpy() == pat.ravel()).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 4. side effects -----------------------------------------------------------------------------------------------------------
def test_frames_are_only_read():
    w, h = 130, 17
    frames = frames_of(w, h)
    with context(w, h) as ctx:
        place(ctx, frames)
        ctx.upload_flow(2, np.ones((h, w, 2), np.float32))
        before = ([ctx.download_frame(s).tobytes() for s in SLOTS], ctx.download_flow(2).tobytes(), bh.rec_bytes(ctx.pass1_results([2], 1.0)))
        assert before[0] == [f.tobytes() for f in frames]
        run(ctx, w, h)
        run(ctx, w, h, params={"radius": 8, "soft": 0}, gate=dev(gate_map(w, h, 0)))
        after = ([ctx.download_frame(s).tobytes() for s in SLOTS], ctx.download_flow(2).tobytes(), bh.rec_bytes(ctx.pass1_results([2], 1.0)))
        assert after == before
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals():
    w, h = 130, 17
    frames = frames_of(w, h)
    with context(w, h) as ctx:
        place(ctx, frames)
        buf = torch.full((N * h * w + 16,), FILL, dtype=torch.uint8, device=DEV)
        out = _capi.DevWeights(buf.data_ptr(), h * w, w)
        gate = dev(gate_map(w, h, 0))
        L, byref, iarr = ctx.L, _capi.C.byref, lambda v: _capi._iarr(v)[0]

        def refused(match, code, call):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and "ffl_texture_weights" in str(e.value)
            assert (buf.cpu().numpy() == FILL).all()

        tw = lambda f=FS, o=out, p=None, g=None, s=None: (lambda: ctx.texture_weights(f, o, p, g, s))
        refused(r"n = 0 items outside 1\.\.6", INVALID, tw([]))
        refused(r"n = 7 items outside 1\.\.6", INVALID, tw([0] * 7))
        assert L.ffl_texture_weights(ctx._h, N, None, None, None, byref(out), 0) == INVALID
        assert "ffl_texture_weights: NULL fslots" in L.ffl_last_error(ctx._h).decode()
        refused(r"item 2: frame slot 8 out of range", INVALID, tw([6, 0, 8, 6, 2]))
        refused(r"item 0: frame slot -1 out of range", INVALID, tw([-1, 0, 3, 6, 2]))
        refused(r"item 4: frame slot 7 was never uploaded", STATE, tw([6, 0, 3, 6, 7]))
        refused(r"radius = 0 outside 1\.\.8", INVALID, tw(p={"radius": 0}))
        refused(r"radius = 9 outside 1\.\.8", INVALID, tw(p={"radius": 9}))
        refused(r"tau = 0 outside 0 < tau <= 65025", INVALID, tw(p={"tau": 0.0}))
        refused(r"tau = 65026 outside 0 < tau <= 65025", INVALID, tw(p={"tau": 65026.0}))
        refused(r"tau = nan outside", INVALID, tw(p={"tau": float("nan")}))
        refused(r"tau = inf outside", INVALID, tw(p={"tau": float("inf")}))
        refused(r"soft = 3 is neither", INVALID, tw(p={"soft": 3}))
        assert L.ffl_texture_weights(ctx._h, N, iarr(FS), None, None, None, 0) == INVALID
        assert "NULL out descriptor" in L.ffl_last_error(ctx._h).decode()
        refused(r"NULL weight base", INVALID, tw(o=_capi.DevWeights(0, h * w, w)))
        refused(r"overlap: weight row pitch 129 below the width 130", INVALID, tw(o=_capi.DevWeights(buf.data_ptr(), h * w, w - 1)))
        refused(r"overlap: weight item stride 2209 below one map's extent 2210", INVALID, tw(o=_capi.DevWeights(buf.data_ptr(), h * w - 1, w)))
        refused(r"negative weight stride", INVALID, tw(o=_capi.DevWeights(buf.data_ptr(), -h * w, w)))
        refused(r"overlap: out item stride 0 with n = 5 maps to write", INVALID, tw(o=_capi.DevWeights(buf.data_ptr(), 0, w)))
        refused(r"overlap: out item stride 0 with n = 5 maps to write", INVALID,
                tw(o=_capi.DevWeights(buf.data_ptr(), 0, w), g=_capi.DevWeights(buf.data_ptr(), 0, w)))   # in place changes nothing here
        refused(r"overlap: weight row pitch 100 below the width 130", INVALID, tw(g=_capi.DevWeights(gate.data_ptr(), 0, 100)))
        refused(r"NULL weight base", INVALID, tw(g=_capi.DevWeights(0, 0, w)))
        # memory that is not the device's, or not all inside one allocation
        pin = ctx.pinned_frames(N, channels=1)
        refused(r"out is page-locked host memory.*device memory", INVALID, tw(o=_capi.DevWeights(pin.ctypes.data, h * w, w)))
        refused(r"the gate maps is page-locked host memory.*device memory", INVALID, tw(g=_capi.DevWeights(pin.ctypes.data, 0, w)))
        in_place = _capi.DevWeights(pin.ctypes.data, h * w, w)
        refused(r"out is page-locked host memory.*device memory", INVALID, tw(o=in_place, g=in_place))
        torch.cuda.empty_cache()
        big = torch.full((18 << 20,), FILL, dtype=torch.uint8, device=DEV)   # an allocation of its own
        past = big.data_ptr() + big.numel() - 4 * w * h                     # room for four maps, five asked for
        refused(rf"out spans {5 * w * h} bytes, {w * h} more than its allocation holds", INVALID, tw(o=_capi.DevWeights(past, h * w, w)))
        refused(rf"the gate maps spans {5 * w * h} bytes, {w * h} more than its allocation holds", INVALID,
                tw(g=_capi.DevWeights(past, h * w, w)))
        refused(rf"out spans {5 * w * h} bytes, {w * h} more than its allocation holds", INVALID,
                tw(o=_capi.DevWeights(past, h * w, w), g=_capi.DevWeights(past, h * w, w)))
        assert (big.cpu().numpy() == FILL).all()
        # out overlapping gate other than exactly
        refused(r"overlap: out \(11050 bytes\) and gate \(2210 bytes\) share memory", INVALID,
                tw(g=_capi.DevWeights(buf.data_ptr() + 4 * h * w, 0, w)))
        refused(r"overlap: out .* and gate .* share memory.*not exactly out", INVALID, tw(g=_capi.DevWeights(buf.data_ptr() + 2, h * w, w)))
        with pytest.raises(ValueError, match="not device memory"):
            ctx.texture_weights(FS, torch.empty((N, h, w), dtype=torch.uint8))
        # a capturing stream
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                tw(s=torch.cuda.current_stream())()
            except _capi.FFLError as err:
                codes.append((err.code, "capturing" in str(err), "ffl_texture_weights" in str(err)))
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [(STATE, True, True)] and float(x.sum()) == 16.0
        assert (buf.cpu().numpy() == FILL).all()
        # nothing was queued, and the context computes a correct call next
        got, rest = run(ctx, w, h)
        assert (got == want(frames)).all() and (rest == FILL).all()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 6. the stream contract ----------------------------------------------------------------------------------------------------
def test_side_stream_may_overwrite_the_gate_and_read_the_maps_at_once():
    w, h = 257, 40
    frames = frames_of(w, h)
    gates = np.stack([gate_map(w, h, 20 + i) for i in range(N)])
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        place(ctx, frames)
        gate = dev(gates)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                gate.copy_(dev(gates), non_blocking=True)
                ctx.texture_weights(FS, out, gate=gate, stream=side)
                gate.zero_()                      # runs behind the call's read of the gate
                got = out.cpu().numpy()           # runs behind the call's write of the maps
                assert (got == want(frames, None, gates)).all()
                out.fill_(FILL)
        torch.cuda.current_stream().wait_stream(side)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_an_upload_into_a_frame_slot_runs_behind_the_call_that_reads_it():
    """The call is held back behind work queued on the caller's stream (a chain of matrix products, some tens of milliseconds); the
    frame slots it reads are overwritten at once.  The uploads must wait for the call: the maps are those of the frames the
    slots held when the call was made, and a second call sees the new frames."""
    w, h = 257, 40
    old = frames_of(w, h)
    new = old[1:] + old[:1]
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        place(ctx, old)
        out = torch.full((N, h, w), FILL, dtype=torch.uint8, device=DEV)
        a = torch.randn(4096, 4096, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            for _ in range(30):
                a = (a @ a).clamp_(-1, 1)
            ctx.texture_weights(FS, out, stream=side)
        place(ctx, new)   # on the host these run at once; on the device behind the call
        side.synchronize()
        assert (out.cpu().numpy() == want(old)).all()
        ctx.texture_weights(FS, out)
        assert (out.cpu().numpy() == want(new)).all()
        assert (want(old) != want(new)).any()
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 7. the schedule -----------------------------------------------------------------------------------------------------------
SW, SH = 64, 64
SPARAMS = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 3000, "keyframe_reduction": False, "pov_mode": False,
           "cut_threshold": 7.0, "hip_axes": {"roll": "tangential"}}


def engine_ctx(B, smallest=False):
    """the rings of an engine of depth 2, or the smallest legal ones (depth 1)"""
    d = 1 if smallest else 2
    return _capi.Context(SW, SH, max_batch=B, frame_slots=pipeline.min_frame_slots(B, d), flow_slots=pipeline.min_flow_slots(B, d))


def chunk_frames(frames):
    """a translating texture with a constant band (16 columns) and a band of sensor noise (10 columns) on the left, so that the
    maps hold zeros, ramps and 255s"""
    fr = [f.copy() for f in sine_translate_frames(frames, SW, SH, seed=5)]
    rng = np.random.default_rng(31)
    for f in fr:
        f[:, :16] = 128
        f[:, 16:26] = np.clip(np.rint(128 + rng.standard_normal((SH, 10))), 0, 255).astype(np.uint8)
    return fr


def by_hand(fr, mode, texture=None, residual=None, gate=None, compensate=None):
    """The chunk on a context that holds it whole, every step ONE call over slots 0 .. n-1: the flow call, then the maps --
    mode "texture": texture_weights on the pairs' frame 0; mode "residual": residual_weights on the raw fields, then
    texture_weights with gate = out = those maps, in place -- (compensate=: motion_fit under the maps, motion_subtract in place,)
    pass1_weighted, one radial_window_axes_weighted over the whole chunk."""
    n = len(fr) - 1
    slots = list(range(n))
    with bh.hand_context(SW, SH, n) as ctx:
        ctx.upload_frames(0, [np.ascontiguousarray(f) for f in fr])
        f0, f1 = slots, [j + 1 for j in slots]
        ctx.flow_pairs(f0, f1, slots)
        raw = ctx.export_flows(slots).cpu().numpy()
        maps = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        if mode == "texture":
            ctx.texture_weights(f0, maps, texture, gate)
        else:
            ctx.residual_weights(f0, f1, slots, maps, residual, gate)
            ctx.texture_weights(f0, maps, texture, maps)
        motion = None
        if compensate is not None:
            mo = pipeline.motion_buffer(ctx, n)
            ctx.motion_fit(slots, _capi.motion_choice(compensate), weights=maps, out=mo)
            ctx.motion_subtract(slots, slots, mo, False)
            motion = mo.cpu().numpy().tobytes()
        ctx.pass1_weighted(slots, maps)
        out = pipeline.post_buffer(ctx, n, axes=True)
        ctx.radial_window_axes_weighted(slots, 0, n, maps, out, pipeline.SMOOTH_RADIUS, 7.0, False)
        assert ctx.graph_stats()["capture_failures"] == 0
        return dict(post=out.cpu().numpy().tobytes(), motion=motion, maps=maps.cpu().numpy(), raw=raw,
                    flows=ctx.export_flows(slots).cpu().numpy())


def restated(fr, res, mode, texture=None, residual=None, gate=None):
    n = len(fr) - 1
    t = np.stack([ref(fr[j], texture if isinstance(texture, dict) else None, gate if mode == "texture" else None) for j in range(n)])
    if mode == "texture":
        return t
    rp = {k: np.float32(v) if k != "soft" else v for k, v in (residual or {}).items()}
    return np.minimum(t, np.stack([rr.residual(fr[j], fr[j + 1], res["raw"][j], gate=gate, **rp) for j in range(n)]))


@pytest.mark.parametrize("mode", ["texture", "residual"])
@pytest.mark.parametrize("frames,B,smallest", [(12, 4, False), (12, 5, True)], ids=["12f-B4", "12f-B5-min"])
def test_process_chunk_equals_the_calls_by_hand(frames, B, smallest, mode):
    """12 frames with max_batch 4 on the rings of depth 2; 12 frames with max_batch 5 on the smallest rings the engine accepts"""
    fr = chunk_frames(frames)
    n = frames - 1
    res = by_hand(fr, mode)
    assert (res["maps"] == restated(fr, res, mode)).all()
    assert len(np.unique(res["maps"])) > 32 and (res["maps"] == 255).any() and (res["maps"] == 0).any()
    with engine_ctx(B, smallest) as ctx:
        eng = pipeline.PairEngine(ctx)
        T, T0 = (torch.empty((n, SH, SW, 2), device=DEV) for _ in range(2))
        M = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        kw = {"weights": "texture"} if mode == "texture" else {"weights": "residual", "texture": True}
        buf = eng.process_chunk(fr, flows_out=T, weights_out=M, post_out=True, **kw)
        assert buf.cpu().numpy().tobytes() == res["post"]
        assert (M.cpu().numpy() == res["maps"]).all()
        assert (T.cpu().numpy() == res["raw"]).all()
        eng.process_chunk(fr, flows_out=T0)
        assert torch.equal(T, T0)
        # the same records when the maps the mode made are handed back as caller maps
        assert eng.process_chunk(fr, weights=M).cpu().numpy().tobytes() == res["post"]
        if mode == "residual":   # the combination is not the residual mode alone
            assert (eng.process_chunk(fr, weights="residual", weights_out=M) is not None) and (M.cpu().numpy() != res["maps"]).any()
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("mode", ["texture", "residual"])
def test_process_chunk_with_compensation_parameters_and_gate(mode):
    """the order behind a batch: the maps from the raw fields and the frames, the fit under the maps, the subtraction, the
    weighted calls; with parameters of both maps and a static gate"""
    fr = chunk_frames(12)
    n, B = 11, 4
    tk, rk = {"radius": 3, "tau": 30.0}, {"beta": 2.0}
    g = gate_map(SW, SH, 3)
    hand = dict(texture=tk, gate=dev(g), **({} if mode == "texture" else {"residual": rk}))
    res = by_hand(fr, mode, compensate="translation", **hand)
    assert (res["maps"] == restated(fr, res, mode, tk, rk, g)).all() and res["flows"].tobytes() != res["raw"].tobytes()
    plain = by_hand(fr, mode, **hand)
    assert (plain["maps"] == res["maps"]).all() and plain["post"] != res["post"]
    with engine_ctx(B) as ctx:
        eng = pipeline.PairEngine(ctx)
        M = torch.full((n, SH, SW), FILL, dtype=torch.uint8, device=DEV)
        T = torch.empty((n, SH, SW, 2), device=DEV)
        mo = pipeline.motion_buffer(ctx, n)
        kw = dict(weights=mode, texture=tk, weights_gate=dev(g), **({} if mode == "texture" else {"residual": rk}))
        buf = eng.process_chunk(fr, weights_out=M, compensate="translation", motion_out=mo, flows_out=T, **kw)
        assert buf.cpu().numpy().tobytes() == res["post"]
        assert mo.cpu().numpy().tobytes() == res["motion"]
        assert (M.cpu().numpy() == res["maps"]).all()
        assert (T.cpu().numpy() == res["flows"]).all()
        # without weights_out the maps live in a tensor of the chunk's own; a TextureParams is taken as it is
        got = eng.process_chunk(fr, **{**kw, "texture": _capi.TextureParams(**tk)})
        assert got.cpu().numpy().tobytes() == plain["post"]
        assert ctx.graph_stats()["capture_failures"] == 0


def test_process_chunk_keyword_refusals():
    fr = chunk_frames(12)
    n = 11
    g = gate_map(SW, SH, 3)
    with engine_ctx(4) as ctx:
        eng = pipeline.PairEngine(ctx)
        M = torch.empty((n, SH, SW), dtype=torch.uint8, device=DEV)
        with pytest.raises(ValueError, match=r"weights_out must be a uint8 device tensor of shape \(11, 64, 64\)"):
            eng.process_chunk(fr, weights="texture", weights_out=M[:5])
        with pytest.raises(ValueError, match="texture= needs weights='texture', or weights='residual'"):
            eng.process_chunk(fr, texture={"radius": 3})
        with pytest.raises(ValueError, match="texture= needs weights='texture', or weights='residual'"):
            eng.process_chunk(fr, weights=torch.ones((SH, SW), dtype=torch.uint8, device=DEV), texture=True)
        with pytest.raises(ValueError, match="texture= needs weights='texture'.*weights='consistency' has no frames hook"):
            eng.process_chunk(fr, weights="consistency", texture=True)
        with pytest.raises(ValueError, match="residual= needs weights='residual'"):
            eng.process_chunk(fr, weights="texture", residual={"soft": 0})
        with pytest.raises(ValueError, match="consistency= needs weights='consistency', not weights='texture'"):
            eng.process_chunk(fr, weights="texture", consistency={"soft": 0})
        with pytest.raises(ValueError, match="radius = 20 outside"):
            eng.process_chunk(fr, weights="texture", texture={"radius": 20})
        with pytest.raises(ValueError, match="tau = -1 outside"):
            eng.process_chunk(fr, weights="residual", texture={"tau": -1.0})
        with pytest.raises(ValueError, match="weights_gate: one static"):
            eng.process_chunk(fr, weights="texture", weights_gate=dev(np.stack([g] * n)))
        with pytest.raises(ValueError, match="center='variance' together with weights= is not supported"):
            eng.process_chunk(fr, weights="texture", center="variance")
        T = torch.zeros((n, SH, SW, 2), device=DEV)
        with pytest.raises(ValueError, match="process_flows: weights='texture' needs the frames.*Context.texture_weights"):
            eng.process_flows(T, weights="texture")
        with pytest.raises(ValueError, match="flows_to_scripts: hip_weights = 'texture' needs the frames.*Context.texture_weights"):
            pipeline.flows_to_scripts(eng, [T], 30.0, n + 1, {**SPARAMS, "hip_weights": "texture"})
        for fn, args in ((pipeline.process_chunk_sharded, (eng, fr, 0, 1, None)), (pipeline.process_chunk_sharded_halo, (eng, fr, 0, 1, None)),
                         (pipeline.process_chunk_local_ranks, ([eng], fr))):
            with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
                fn(*args, weights="texture")
        assert ctx.graph_stats()["capture_failures"] == 0


def test_an_engine_without_the_hook_keeps_serving_the_plain_chunk():
    class Old(pipeline.PairEngine):
        def pass1_pairs(self, frames, pairs, slot_of, pov_mode=False, cut_threshold=7.0, on_batch=None, algo=None,
                        farneback=pipeline.OWN, window=pipeline.OWN, queued=None, batch=None, reverse_slot_of=None, behind=None):
            return super().pass1_pairs(frames, pairs, slot_of, pov_mode, cut_threshold, on_batch, algo, farneback, window, queued,
                                       batch, reverse_slot_of, behind)

    fr = chunk_frames(12)
    with engine_ctx(4) as ctx:
        want_dots, want_recs = pipeline.PairEngine(ctx).process_chunk(fr)
        dots, recs = Old(ctx).process_chunk(fr)
        assert dots.tobytes() == want_dots.tobytes() and bh.rec_bytes(recs) == bh.rec_bytes(want_recs)
        a = Old(ctx).process_chunk(fr, post_out=True).cpu().numpy().tobytes()
        assert a == pipeline.PairEngine(ctx).process_chunk(fr, post_out=True).cpu().numpy().tobytes()
        with pytest.raises(TypeError, match="with_frames"):   # the mode needs the hook, and says so rather than run without maps
            Old(ctx).process_chunk(fr, weights="texture")


def test_frames_to_scripts_under_texture_maps():
    fr = chunk_frames(12)
    plan = pipeline.pair_plan(30.0, len(fr), SPARAMS)
    assert len(plan) == 1
    chunk = plan[0]
    tk = {"radius": 3}
    g = gate_map(SW, SH, 4)
    with engine_ctx(4) as ctx:
        eng = pipeline.PairEngine(ctx)
        cases = (({"hip_weights": "texture"}, {"weights": "texture"}),
                 ({"hip_weights": "texture", "hip_texture": tk, "hip_weights_gate": g}, {"weights": "texture", "texture": tk, "weights_gate": dev(g)}),
                 ({"hip_weights": "residual", "hip_texture": True}, {"weights": "residual", "texture": True}),
                 ({"hip_weights": "residual", "hip_residual": {"beta": 2.0}, "hip_texture": tk},
                  {"weights": "residual", "residual": {"beta": 2.0}, "texture": tk}))
        seen = set()
        for extra, ckw in cases:
            buf = eng.process_chunk([fr[i] for i in chunk], **ckw)
            seen.add(buf.cpu().numpy().tobytes())
            comps, recs = pipeline.post_records(buf, axes=True)
            want_scripts = pipeline._scripts_from_chunks([(chunk[:-1], comps, recs)], pipeline.script_axes(SPARAMS), 30.0, SPARAMS)
            assert want_scripts[""] and want_scripts["roll"]
            params = {**SPARAMS, **extra}
            assert pipeline.frames_to_scripts(eng, fr, 30.0, params) == want_scripts
            assert pipeline.frames_to_actions(eng, fr, 30.0, params) == want_scripts[""]
        assert len(seen) == len(cases)   # every case weights differently
        with pytest.raises(ValueError, match="hip_texture needs hip_weights = 'texture'"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_texture": tk})
        with pytest.raises(ValueError, match="hip_texture needs hip_weights = 'texture', got 'consistency'"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_weights": "consistency", "hip_texture": tk})
        with pytest.raises(ValueError, match="hip_center together with hip_weights"):
            pipeline.frames_to_scripts(eng, fr, 30.0, {**SPARAMS, "hip_weights": "texture", "hip_center": "variance"})
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 8. what the map is for ----------------------------------------------------------------------------------------------------
REC = _capi.MOTION_DTYPE.itemsize


@pytest.mark.parametrize("radius", [3, 7])
@pytest.mark.parametrize("size", [(64, 64), (130, 72), (257, 40)], ids=gid)
def test_the_map_frees_the_camera_fit_from_a_flat_wall_on_the_device(size, radius):
    """test_texture_ref_host's scene through the device: the frames uploaded, the fields imported, texture_weights and then three
    chained motion_fit passes with and without the maps.  Every pass is held against motion_ref as the motion tests hold it
    (the sums within the derived bound of the restated terms, the record the host solve of those sums), and the two
    inequalities hold on the device's records."""
    w, h = size
    n = len(tr.SEEDS)
    scenes = [tr.wall_scene(w, h, s) for s in tr.SEEDS]
    slots = list(range(n))
    with _capi.Context(w, h, max_batch=n, frame_slots=n, flow_slots=n) as ctx:
        ctx.upload_frames(0, [np.ascontiguousarray(I) for I, _ in scenes])
        ctx.import_flows(dev(np.stack([F for _, F in scenes])), slots)
        maps = torch.full((n, h, w), FILL, dtype=torch.uint8, device=DEV)
        ctx.texture_weights(slots, maps, {"radius": radius})
        W = maps.cpu().numpy()
        assert (W == np.stack([ref(I, {"radius": radius}) for I, _ in scenes])).all()
        final = {}
        for name, wts in (("plain", None), ("weighted", maps)):
            buf = torch.full((n * REC,), FILL, dtype=torch.uint8, device=DEV)
            sums = torch.full((n, 12), float("nan"), dtype=torch.float64, device=DEV)
            prior = [None] * n
            for it in range(3):
                ctx.motion_fit(slots, "translation", 1, 1.0, weights=wts, prior=None if it == 0 else buf, out=buf, sums_out=sums)
                rec, s = np.frombuffer(buf.cpu().numpy().tobytes(), _capi.MOTION_DTYPE, n), sums.cpu().numpy()
                for i, (_, F) in enumerate(scenes):
                    mr.check_sums(s[i], F, None if wts is None else W[i], prior[i], 1.0)
                    assert rec[i].tobytes() == _capi.motion_solve(s[i], "translation").tobytes()
                prior = [mr.six(rec[i]) for i in range(n)]
            one = torch.full((n * REC,), FILL, dtype=torch.uint8, device=DEV)
            ctx.motion_fit(slots, "translation", 3, 1.0, weights=wts, out=one)     # the call a chunk makes: three passes at once
            assert one.cpu().numpy().tobytes() == buf.cpu().numpy().tobytes()
            final[name] = rec
        for i in range(n):
            p, q = final["plain"][i], final["weighted"][i]
            print(f"{w}x{h} seed {tr.SEEDS[i]} r {radius}: unweighted ({p['a0']:.3f}, {p['b0']:.3f}), weighted ({q['a0']:.3f}, {q['b0']:.3f})")
            assert abs(float(p["a0"])) < 1.0
            assert abs(float(q["a0"]) - tr.MOVE[0]) <= 0.15 and abs(float(q["b0"]) - tr.MOVE[1]) <= 0.15
        assert ctx.graph_stats()["capture_failures"] == 0
