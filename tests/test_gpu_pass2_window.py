"""GPU side of the device pass 2 (ffl_radial_window), everything through the C ABI via _capi.

The comparisons are bit for bit against the host path on the same context and slots: pass1_results -> smooth_centers ->
radial.  One run per size is also held against numpy (tests/post_ref.py) within the bounds that file derives."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import post_ref as pr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
ITEM = 48
# 130x17: two 128-pixel strips, the second 2 pixels wide, and a 1-row second row group; 257x40: three strips and a partial
# third row group
SIZES = [(16, 16), (130, 17), (257, 40)]
W, H = 130, 17


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def records(t, n):
    return np.frombuffer(t.cpu().numpy().tobytes(), _capi.PASS2_DTYPE, n)


def host_path(ctx, seq, first, n, radius=6, thr=7.0, pov=False):
    """the parent's host path for items first .. first+n-1 of seq: (records, centres, dots)"""
    recs = ctx.pass1_results(list(seq), thr)
    cen = pipeline.smooth_centers([(r[0], r[1]) for r in recs], radius)[first:first + n]
    items = range(first, first + n)
    dots = ctx.radial([seq[j] for j in items], cen, [recs[j][4] for j in items], pov)
    return recs[first:first + n], cen, dots


def device_path(ctx, seq, first, n, radius=6, thr=7.0, pov=False, stream=None):
    out = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
    ctx.radial_window(list(seq), first, n, out, radius, thr, pov, stream)
    return records(out, n)


def same_bits(got, want, dtype, nan_aware, what):
    got, want = np.ascontiguousarray(got, dtype), np.ascontiguousarray(want, dtype)
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan = np.isnan(want) if nan_aware else np.zeros(len(want), bool)
    assert np.array_equal(got.view(u)[~nan], want.view(u)[~nan]), (what, got, want)
    assert np.isnan(got[nan]).all(), (what, got, want)       # not the bits: the default NaN's sign is the producer's


def assert_same(rec, host, nan_aware=False):
    recs, cen, dots = host
    assert len(rec) == len(recs)
    same_bits(rec["dot"], dots, np.float64, nan_aware, "dot")
    same_bits(rec["cx"], cen[:, 0], np.float64, False, "cx")
    same_bits(rec["cy"], cen[:, 1], np.float64, False, "cy")
    assert rec["x"].tolist() == [r[0] for r in recs] and rec["y"].tolist() == [r[1] for r in recs]
    same_bits(rec["div_val"], [r[2] for r in recs], np.float32, nan_aware, "div_val")
    same_bits(rec["mean_mag"], [r[3] for r in recs], np.float32, nan_aware, "mean_mag")
    assert rec["cut"].tolist() == [int(r[4]) for r in recs]
    assert not rec["pad"].any()


def compare(ctx, seq, first, n, radius=6, thr=7.0, pov=False, nan_aware=False):
    rec = device_path(ctx, seq, first, n, radius, thr, pov)       # queued behind the producers, nothing waited for
    assert_same(rec, host_path(ctx, seq, first, n, radius, thr, pov), nan_aware)
    return rec


@functools.lru_cache(maxsize=None)
def clip(n, w, h, seed=3):
    return list(sine_translate_frames(n, w, h, seed=seed))


def random_fields(n, w, h, seed, scale=2.5):
    return (np.random.default_rng(seed).standard_normal((n, h, w, 2)) * scale).astype(np.float32)


# ---- sizes: 40 Farneback pairs in a ring of slots that wraps ------------------------------------------------------------
@pytest.mark.parametrize("pov", [False, True], ids=["weighted", "pov"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_sizes(size, pov):
    w, h = size
    n, B = 40, 16
    fs = pipeline.min_flow_slots(B)                               # 45
    slots = [(30 + j) % fs for j in range(n)]                     # the seq of every call crosses the ring's end
    fr = clip(n + 1, w, h)
    with _capi.Context(w, h, max_batch=B, frame_slots=n + 1, flow_slots=fs) as ctx:
        ctx.upload_frames(0, fr)
        for j0 in range(0, n, B):
            js = list(range(j0, min(j0 + B, n)))
            ctx.flow_pairs(js, [j + 1 for j in js], [slots[j] for j in js], pov)
        calls = pipeline.window_calls(n, B)
        assert len(calls) == 3
        out = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
        for lo, hi, first, count, _ in calls:                     # all queued before anything is read
            ctx.radial_window(slots[lo:hi], first, count, out[(lo + first) * ITEM:], 6, 7.0, pov)
        rec = records(out, n)
        for lo, hi, first, count, _ in calls:
            assert_same(rec[lo + first:lo + first + count], host_path(ctx, slots[lo:hi], first, count, 6, 7.0, pov))
        assert ctx.graph_stats()["capture_failures"] == 0
        # the independent check: numpy on the downloaded fields, within post_ref's bounds
        flows = [ctx.download_flow(s) for s in slots]
        pos = []
        for j, f in enumerate(flows):
            if pov:
                want_xy = (w // 2, h - 1)
                assert float(rec["div_val"][j]) == 0.0
            else:
                x, y, v = pr.argmax_ref(f)
                want_xy = (x, y)
                assert np.float32(rec["div_val"][j]).tobytes() == np.float32(v).tobytes()
            assert (int(rec["x"][j]), int(rec["y"][j])) == want_xy
            pos.append(want_xy)
            pr.check_mean_mag(rec["mean_mag"][j], f)
            assert int(rec["cut"][j]) == int(rec["mean_mag"][j] > np.float32(7.0))
        cen = pipeline.smooth_centers(pos)
        assert cen.tobytes() == np.stack([rec["cx"], rec["cy"]], axis=1).tobytes()
        for j, f in enumerate(flows):
            if rec["cut"][j]:
                assert rec["dot"][j].tobytes() == np.float64(0.0).tobytes()
            else:
                pr.check_radial(float(rec["dot"][j]), f, tuple(cen[j]), pov)


# ---- window shapes, cuts, non-finite fields: imported / uploaded fields at 130x17 --------------------------------------
@pytest.fixture(scope="module")
def field_ctx():
    """13 random fields in slots 3..15 of a 130x17 context (slot 0..2 and 16.. stay empty)"""
    with _capi.Context(W, H, max_batch=16, frame_slots=2, flow_slots=24) as ctx:
        ctx.import_flows(dev(random_fields(13, W, H, 1)), list(range(3, 16)))
        yield ctx
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("radius", [0, 1, 6, 32])
def test_window_shapes(field_ctx, radius):
    ctx = field_ctx
    order = [9, 4, 15, 3, 12, 7, 5, 14, 8, 6, 13, 10, 11]         # time order is the caller's, not the slots'
    for n_seq in (1, 3, 13):
        seq = order[:n_seq]
        ranges = {(0, n_seq), (0, 1), (n_seq - 1, 1), (n_seq // 2, 1), (0, max(1, n_seq // 2)),
                  (n_seq // 3, max(1, n_seq // 3)), (n_seq - max(1, n_seq // 2), max(1, n_seq // 2))}
        for first, n in sorted(ranges):
            for pov in (False, True):
                compare(ctx, seq, first, n, radius, 7.0, pov)


def test_cuts():
    n, thr = 10, 3.0
    scales = [0.5, 4.0, 1.0, 3.5, 2.0, 2.8, 5.0, 0.1, 2.2, 6.0]   # mean |N(0, s)| pairs = 1.2533 s: 0.6 .. 7.5 around 3.0
    fields = [random_fields(1, W, H, 40 + i, s)[0] for i, s in enumerate(scales)]
    with _capi.Context(W, H, max_batch=16, frame_slots=2, flow_slots=16) as ctx:
        for i, f in enumerate(fields):
            ctx.upload_flow(i, f)
        for pov in (False, True):
            rec = compare(ctx, list(range(n)), 0, n, 6, thr, pov)
            cut = rec["cut"] != 0
            assert cut.sum() >= 3 and (~cut).sum() >= 3
            assert (rec["dot"][cut].view(np.uint64) == 0).all()   # +0.0, not -0.0
            assert (rec["dot"][~cut] != 0.0).all()
        # the threshold is the call's: the same records under another one
        assert compare(ctx, list(range(n)), 2, 5, 1, 0.0)["cut"].all()
        assert not compare(ctx, list(range(n)), 2, 5, 1, 100.0)["cut"].any()


def test_non_finite_fields():
    f = random_fields(5, W, H, 77)
    f[1, H // 2, W // 2, 0] = np.nan
    f[3, H // 2, W // 2, 1] = np.inf
    with _capi.Context(W, H, max_batch=16, frame_slots=2, flow_slots=16) as ctx:
        ctx.import_flows(dev(f), [4, 5, 6, 7, 8])
        for pov in (False, True):
            rec = compare(ctx, [4, 5, 6, 7, 8], 0, 5, 6, 7.0, pov, nan_aware=True)
            assert math.isnan(rec["dot"][1]) and math.isnan(rec["mean_mag"][1]) and rec["cut"][1] == 0
            assert rec["mean_mag"][3] == np.inf and rec["cut"][3] == 1 and rec["dot"][3].tobytes() == np.float64(0.0).tobytes()
            assert np.isfinite(rec["dot"][[0, 2, 4]]).all()
            compare(ctx, [4, 5, 6, 7, 8], 1, 3, 1, 7.0, pov, nan_aware=True)


# ---- one scratch set on stream `post` -----------------------------------------------------------------------------------
def test_shared_post_scratch_between_users():
    """ffl_upload_flow, ffl_import_flows, ffl_radial and ffl_radial_window share one pass-1 table, one key buffer, one sum
    buffer and one item table on stream `post`.  At 253x33 pass 1 walks 3 strips x 3 row groups (3 workgroups per item)
    and the radial pass 2 strips x 3 row groups (2 workgroups per item), so the two index the shared sums differently.
    The calls follow one another with no host wait between the device-ordered ones; a second context runs the same calls,
    each followed by sync(), and every record, dot and exported field must be the same bytes."""
    w, h = 253, 33
    f = random_fields(7, w, h, 91)
    pos = [pr.argmax_ref(f[j])[:2] for j in range(4)]
    cen = pipeline.smooth_centers(pos, 1)                         # the window's centres, without a look at the device

    def run(ctx, wait):
        done = ctx.sync if wait else (lambda: None)
        a, b = dev(f[1:4]), dev(f[4:7])
        out = torch.empty(4 * ITEM, dtype=torch.uint8, device=DEV)
        ctx.upload_flow(0, f[0]); done()
        ctx.import_flows(a, [1, 2, 3]); done()
        ctx.radial_window([0, 1, 2, 3], 0, 4, out, 1); done()
        ctx.import_flows(b, [4, 5, 6]); done()
        dots = ctx.radial([0, 1, 2, 3], cen, [False] * 4); done()
        exported = ctx.export_flows([4, 5, 6]); done()
        recs = ctx.pass1_results(list(range(7)))
        assert ctx.graph_stats()["capture_failures"] == 0
        return {"window": out.cpu().numpy().tobytes(), "dots": np.asarray(dots, np.float64).tobytes(),
                "exported": exported.cpu().numpy().tobytes(), "pass1": np.asarray(recs, np.float64).tobytes()}

    got = []
    for wait in (False, True):
        with _capi.Context(w, h, max_batch=3, frame_slots=2, flow_slots=8) as ctx:
            got.append(run(ctx, wait))
    for key in got[0]:
        assert got[0][key] == got[1][key], key
    rec = np.frombuffer(got[0]["window"], _capi.PASS2_DTYPE, 4)
    dots = np.frombuffer(got[0]["dots"], np.float64)
    assert not rec["cut"].any() and rec["dot"].tobytes() == dots.tobytes()     # the two forms, same slots and centres
    assert np.stack([rec["cx"], rec["cy"]], axis=1).tobytes() == cen.tobytes()
    assert got[0]["exported"] == f[4:7].tobytes()
    for j in range(4):
        pr.check_radial(float(dots[j]), f[j], tuple(cen[j]), False)
        pr.check_radial(float(rec["dot"][j]), f[j], tuple(cen[j]), False)


# ---- stream contract --------------------------------------------------------------------------------------------------
def test_stream_sentinel_and_reader(field_ctx):
    """`out` is filled by work queued on the stream before the call and read by work queued after it; no host
    synchronisation in between.  Once on torch's current stream, once on a second stream passed explicitly."""
    ctx, seq = field_ctx, list(range(3, 16))
    want = host_path(ctx, seq, 2, 9)
    for side in (None, torch.cuda.Stream()):
        torch.cuda.synchronize()
        with torch.cuda.stream(side if side is not None else torch.cuda.current_stream()):
            out = torch.empty(9 * ITEM, dtype=torch.uint8, device=DEV)
            big = torch.ones(1 << 22, device=DEV)
            for _ in range(10):                                   # keep the stream busy ahead of the sentinel
                big = big * 1.0001
            out.fill_(0xA5)
            ctx.radial_window(seq, 2, 9, out, stream=side)
            copy = out.clone()
            out.zero_()                                           # overwritten behind the reader
        (side or torch.cuda.current_stream()).synchronize()
        assert_same(records(copy, 9), want)
        assert not out.cpu().numpy().any()


def test_recycling_batch_queued_behind_the_call():
    n = 16
    fr = clip(n + 2, W, H, seed=8)
    with _capi.Context(W, H, max_batch=n, frame_slots=n + 2, flow_slots=n) as ctx:
        slots = list(range(n))
        ctx.upload_frames(0, fr)
        ctx.flow_pairs(slots, list(range(1, n + 1)), slots)
        want = host_path(ctx, slots, 0, n)
        out = torch.empty(n * ITEM, dtype=torch.uint8, device=DEV)
        ctx.radial_window(slots, 0, n, out)
        ctx.flow_pairs(list(range(n + 1, 1, -1)), list(range(n, 0, -1)), slots)   # other pairs into the same slots, at once
        assert_same(records(out, n), want)
        new = host_path(ctx, slots, 0, n)
        assert not np.array_equal(np.asarray(new[2]), np.asarray(want[2]))          # the slots did change afterwards
        assert_same(device_path(ctx, slots, 0, n), new)
        assert ctx.graph_stats()["capture_failures"] == 0


class Span:
    """`nbytes` bytes at `ptr` as a __cuda_array_interface__ object, whatever memory that is"""

    def __init__(self, ptr, nbytes):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": (int(nbytes),), "strides": None,
                                         "typestr": "|u1"}


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refusals(field_ctx):
    ctx, seq = field_ctx, list(range(3, 16))
    out = torch.empty(300 * ITEM, dtype=torch.uint8, device=DEV)
    INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE

    def refused(match, code, seq_, first, n, out_=out, radius=6, stream=None):
        with pytest.raises(_capi.FFLError, match=match) as e:
            ctx.radial_window(seq_, first, n, out_, radius, stream=stream)
        assert e.value.code == code

    refused(r"n = 0 items outside 1\.\.256", INVALID, seq, 0, 0)
    refused(r"n = 257 items outside 1\.\.256", INVALID, seq, 0, 257)
    refused(r"n_seq = 0 slots outside 1\.\.320", INVALID, [], 0, 1)
    refused(r"n_seq = 321 slots outside 1\.\.320", INVALID, [3] * 321, 0, 1)
    refused(r"first = -1, n = 2: the items lie outside seq", INVALID, seq, -1, 2)
    refused(r"first = 10, n = 4: the items lie outside seq 0\.\.12", INVALID, seq, 10, 4)
    refused(r"first = 2147483647, n = 2: the items lie outside seq", INVALID, seq, 2 ** 31 - 1, 2)   # first + n wraps
    refused(r"radius -1 outside 0\.\.32", INVALID, seq, 0, 1, radius=-1)
    refused(r"radius 33 outside 0\.\.32", INVALID, seq, 0, 1, radius=33)
    refused(r"flow slot 24 out of range", INVALID, [3, 24], 0, 1)
    refused(r"flow slot -1 out of range", INVALID, [-1, 3], 1, 1)
    for _ in range(2):                                            # refused twice: the refusal leaves no mark behind
        refused(r"flow slot 5 repeated", INVALID, [4, 5, 5], 0, 1)
    refused(r"flow slot 2 holds no result", STATE, [2, 3, 4], 1, 1)      # an empty neighbour
    refused(r"flow slot 16 holds no result", STATE, [15, 16], 1, 1)      # an empty computed slot
    refused(r"8-byte aligned", INVALID, seq, 0, 1, Span(out.data_ptr() + 4, 100 * ITEM))
    torch.cuda.empty_cache()
    big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)           # an allocation of its own (>= 10 MiB, a 2 MiB multiple)
    refused(r"more than its allocation holds", INVALID, seq, 0, 3, Span(big.data_ptr() + big.numel() - 2 * ITEM, 3 * ITEM))
    pin = ctx.pinned_frames(1, channels=1)                               # ffl_host_alloc memory
    refused(r"page-locked host memory.*ffl_radial", INVALID, seq, 0, 1, Span(pin.ctypes.data, pin.size))
    with pytest.raises(ValueError, match="not device memory"):
        ctx.radial_window(seq, 0, 1, np.zeros(ITEM, np.uint8))
    with pytest.raises(ValueError, match="2 records need 96"):
        ctx.radial_window(seq, 0, 2, out[:ITEM])
    # a capture open on the stream: refused with FFL_ERR_STATE before anything touches the stream
    x = torch.zeros(16, device=DEV)
    g = torch.cuda.CUDAGraph()
    codes = []
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        try:
            ctx.radial_window(seq, 0, 1, out, stream=torch.cuda.current_stream())
        except _capi.FFLError as err:
            codes.append((err.code, "capturing" in str(err)))
        x += 1
    g.replay()
    torch.cuda.synchronize()
    assert codes == [(STATE, True)] and float(x.sum()) == 16.0
    # and the context computes a correct call next
    compare(ctx, seq, 0, 13)
    compare(ctx, [4, 5], 1, 1, 0)


# ---- the engine and the whole-video paths --------------------------------------------------------------------------------
def engine_ctx(w, h, B):
    return _capi.Context(w, h, max_batch=B, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2))


def test_engine_chunk_and_flows():
    n, B = 39, 16
    fr = clip(n + 1, W, H, seed=5)
    with engine_ctx(W, H, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        T = torch.empty((n, H, W, 2), device=DEV)
        dots, recs = eng.process_chunk(fr, flows_out=T)
        for thr, pov in ((7.0, False), (2.0, True)):
            dots, recs = eng.process_chunk(fr, pov, thr)
            buf = pipeline.post_buffer(ctx, n)
            assert eng.process_chunk(fr, pov, thr, post_out=buf) is buf
            d2, r2 = pipeline.post_records(buf)
            assert r2 == recs and d2.tobytes() == np.asarray(dots, np.float64).tobytes()
            df, rf = eng.process_flows(T, pov, thr)
            d3, r3 = pipeline.post_records(eng.process_flows(T, pov, thr, post_out=True), n)
            assert r3 == rf and d3.tobytes() == np.asarray(df, np.float64).tobytes()
        with pytest.raises(ValueError, match="records need"):
            eng.process_chunk(fr, post_out=pipeline.post_buffer(ctx, n - 1))
        assert ctx.graph_stats()["capture_failures"] == 0


def test_actions_device_pass2():
    w, h, B, total = 64, 48, 8, 50
    fr = clip(total, w, h, seed=6)
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 2.5}
    on = {**params, "hip_pass2": "device"}
    plan = pipeline.pair_plan(30.0, total, params)
    assert len(plan) >= 2
    with engine_ctx(w, h, B) as ctx:
        eng = pipeline.PairEngine(ctx)
        acts = pipeline.frames_to_actions(eng, fr, 30.0, params)
        assert acts and pipeline.frames_to_actions(eng, fr, 30.0, on) == acts
        assert pipeline.frames_to_actions(eng, fr, 30.0, {**params, "hip_pass2": "host"}) == acts
        chunk_flows = []
        for chunk in plan:
            T = torch.empty((len(chunk) - 1, h, w, 2), device=DEV)
            eng.process_chunk([fr[i] for i in chunk], flows_out=T)
            chunk_flows.append(T)
        assert pipeline.flows_to_actions(eng, chunk_flows, 30.0, total, params) == acts
        assert pipeline.flows_to_actions(eng, chunk_flows, 30.0, total, on) == acts
        assert ctx.graph_stats()["capture_failures"] == 0


def test_video_to_actions_device_pass2_through_a_small_ring():
    """prefetch.video_to_actions under "hip_pass2": "device": the page-locked ring holds 3B + 1 frames, fewer than a chunk,
    so its slots are recycled inside every chunk while the transfers read them in place; batches of 4 pairs are shorter
    than the window's radius, so the first batch of a chunk has no window call behind it.  The actions are the default
    schedule's."""
    from funscript_flow_amd import prefetch
    from funscript_flow_amd.synth import gray_to_bgr
    sw, sh, n, fps, B = 160, 120, 101, 60.0, 4
    src = gray_to_bgr(sine_translate_frames(n, sw, sh, seed=9, amp=(3.0, 2.0), period=24, zoom=0.03), gains=(0.9, 1.0, 0.8))

    class Cap:
        def __init__(self):
            self.pos = 0

        def get(self, prop):
            return {prefetch.CAP_PROP_FRAME_COUNT: n, prefetch.CAP_PROP_FPS: fps, prefetch.CAP_PROP_FRAME_WIDTH: sw,
                    prefetch.CAP_PROP_FRAME_HEIGHT: sh}[prop]

        def grab(self):
            self.pos += 1
            return self.pos <= n

        def read(self, image=None):
            if self.pos >= n:
                return False, None
            np.copyto(image, src[self.pos])
            self.pos += 1
            return True, image

    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False,
              "cut_threshold": 2.5}
    with engine_ctx(64, 48, B) as ctx:
        want = prefetch.video_to_actions(ctx, Cap(), params, ring_frames=3 * B + 1)
        got = prefetch.video_to_actions(ctx, Cap(), {**params, "hip_pass2": "device"}, ring_frames=3 * B + 1)
        assert want and got == want and len(got) == 48      # 51 sampled frames -> 19 + 19 + 10 pairs
        assert ctx.graph_stats()["capture_failures"] == 0
