"""GPU side of device-memory I/O: frames ingested from torch tensors on cuda:0 give the host paths'
operands byte for byte; whole chunks give the same records and dots; the stream contract orders producers and consumers
without host synchronisation; exported flow fields equal download_flow bit for bit; device-side refusals."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle as orc
import yuv_ref
from funscript_flow_amd import _capi, frontend, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"


def rnd(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bgr_clip(n, w, h, seed):
    g = sine_translate_frames(n, w, h, seed=seed)
    return [np.ascontiguousarray(np.stack([f, np.roll(f, 3, 1), 255 - f], -1)) for f in g]


def host_operand(case, f):
    """what the host path puts into a 256x256 (or VR) context for frame f of a case, through a fresh context"""
    kind, resize, crop = case["kind"], case["resize"], case["crop"]
    with _capi.Context(256, 256, max_batch=1, frame_slots=2) as h:
        if kind == "gray":
            h.upload_frames(0, [f])
        elif kind in ("i420", "nv12"):
            h.upload_frames_yuv(0, [f], kind, resize, crop)
        else:
            h.upload_frames_raw(0, [f], resize, crop, rgb_order=kind == "rgb")
        return h.download_frame(0)


def operand_cases():
    c = []
    g = rnd((256, 256), 1)
    c.append(("gray", dict(kind="gray", resize=None, crop=(0, 0)), g, dev(g)))
    gw = rnd((256, 300), 2)
    c.append(("gray_strided", dict(kind="gray", resize=None, crop=(0, 0)), gw[:, 20:276], dev(gw)[:, 20:276]))
    b = rnd((1080, 1920, 3), 3)
    c.append(("bgr_1080p", dict(kind="bgr", resize=(256, 256), crop=(0, 0)), b, dev(b)))
    c.append(("rgb_1080p", dict(kind="rgb", resize=(256, 256), crop=(0, 0)), b, dev(b)))
    c.append(("bgr_vr", dict(kind="bgr", resize=(512, 512), crop=(0, 256)), b, dev(b)))
    a = rnd((720, 1280, 4), 4)
    c.append(("bgra", dict(kind="bgr", resize=(256, 256), crop=(0, 0)), a[..., :3], dev(a)))
    p = rnd((360, 640, 3), 5)
    c.append(("planar_rgb", dict(kind="rgb", resize=(256, 256), crop=(0, 0)), p, dev(p.transpose(2, 0, 1))))
    u = rnd((90, 160, 3), 6)
    c.append(("upscale_160x90", dict(kind="bgr", resize=(256, 256), crop=(0, 0)), u, dev(u)))
    nv = yuv_ref.random_frame(640, 360, "nv12", 7, pitch=704)
    c.append(("nv12_pitch", dict(kind="nv12", resize=(256, 256), crop=(0, 0)), nv, dev(nv.base)[:, :640]))
    i4 = yuv_ref.random_frame(640, 360, "i420", 8)
    c.append(("i420", dict(kind="i420", resize=(256, 256), crop=(0, 0)), i4, dev(i4)))
    big = yuv_ref.random_frame(5760, 2880, "nv12", 9)
    c.append(("nv12_5760_vr", dict(kind="nv12", resize=(512, 512), crop=(0, 256)), big, dev(big)))
    return c


NAMES = ["gray", "gray_strided", "bgr_1080p", "rgb_1080p", "bgr_vr", "bgra", "planar_rgb", "upscale_160x90", "nv12_pitch",
         "i420", "nv12_5760_vr"]   # operand_cases(), built on the device at run time


@pytest.mark.parametrize("which", NAMES)
def test_device_operands_equal_host_paths(which):
    name, case, host, t = {c[0]: c for c in operand_cases()}[which]
    fmt = {"gray": "gray", "bgr": "bgr", "rgb": "rgb", "i420": "i420", "nv12": "nv12"}[case["kind"]]
    with _capi.Context(256, 256, max_batch=1, frame_slots=4) as ctx:
        ctx.upload_frames_device(1, [t, t], fmt, case["resize"], case["crop"])
        want = host_operand(case, host)
        assert np.array_equal(ctx.download_frame(1), want)
        assert np.array_equal(ctx.download_frame(2), want)
        if case["kind"] == "bgr" and host.shape[2] == 3 and name != "bgra":
            vr = case["crop"] != (0, 0)
            assert np.array_equal(want, orc.frontend(np.ascontiguousarray(host), vr_mode=vr))


def engines(B, n_frames):
    fs, fl = pipeline.min_frame_slots(B, 2), pipeline.min_flow_slots(B, 2)
    return (_capi.Context(256, 256, max_batch=B, frame_slots=fs, flow_slots=fl),
            _capi.Context(256, 256, max_batch=B, frame_slots=fs, flow_slots=fl))


@pytest.mark.parametrize("kw", [{}, {"flow": "dis"}, {"farneback": "iter2"}], ids=["farneback", "dis", "fb_params"])
def test_chain_equals_host_chain(kw):
    kw = dict(kw)
    if kw.get("farneback") == "iter2":
        kw["farneback"] = _capi.FarnebackParams(iterations=2)
    clip = bgr_clip(65, 256, 256, 11)
    tens = dev(np.stack(clip))
    a, b = engines(64, 65)
    with a, b:
        d_dots, d_recs = pipeline.PairEngine(a, frontend.DeviceUploader(a, "bgr"), **kw).process_chunk(tens)
        h_dots, h_recs = pipeline.PairEngine(b, frontend.DecodedUploader(b), **kw).process_chunk(clip)
        assert d_recs == h_recs
        assert np.array_equal(d_dots, h_dots)
        assert a.graph_stats()["capture_failures"] == 0
        if not kw:
            assert a.graph_stats()["replayed"] > 0


def test_chain_1080p_bgr_and_frames_to_actions():
    clip = bgr_clip(33, 1920, 1080, 12)
    tens = [dev(f) for f in clip]
    a, b = engines(16, 33)
    with a, b:
        ea, eb = pipeline.PairEngine(a, frontend.DeviceUploader(a, "bgr")), pipeline.PairEngine(b, frontend.DecodedUploader(b))
        d_dots, d_recs = ea.process_chunk(tens)
        h_dots, h_recs = eb.process_chunk(clip)
        assert d_recs == h_recs and np.array_equal(d_dots, h_dots)
        params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False}
        acts = pipeline.frames_to_actions(ea, tens, 30.0, params)
        assert acts and acts == pipeline.frames_to_actions(eb, clip, 30.0, params)
        assert a.graph_stats()["capture_failures"] == 0


def test_producer_and_consumer_ordering():
    """The frames are produced on a side stream by a long chain of torch ops and consumed with no synchronisation; right
    after the call the sources are zeroed on the same stream.  The slots hold the original operands."""
    n = 64
    base = [rnd((1080, 1920, 3), 20 + k) for k in range(4)]
    host = [((base[i % 4].astype(np.int32) + i) % 256).astype(np.uint8) for i in range(n)]
    s = torch.cuda.Stream(device=DEV)
    src = dev(np.stack(base))
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        t = src.repeat(n // 4, 1, 1, 1).to(torch.int32)
        off = torch.arange(n, device=DEV, dtype=torch.int32).view(n, 1, 1, 1)   # repeat() tiles: row i holds base[i % 4]
        for k in range(24):
            t = t + k
        t = (t - sum(range(24)) + off) % 256
        frames = t.to(torch.uint8)
    with _capi.Context(256, 256, max_batch=1, frame_slots=2 * n) as ctx:
        ctx.upload_frames_device(0, frames, "bgr", (256, 256), (0, 0), stream=s)
        with torch.cuda.stream(s):
            frames.fill_(0)
        ctx.upload_frames_raw(n, host, (256, 256))
        for i in range(n):
            assert np.array_equal(ctx.download_frame(i), ctx.download_frame(n + i)), i
        s.synchronize()
        assert int(frames.sum()) == 0


def flows_ctx(n_pairs=6):
    ctx = _capi.Context(256, 256, max_batch=n_pairs, frame_slots=n_pairs + 1, flow_slots=n_pairs + 2)
    fr = sine_translate_frames(n_pairs + 1, 256, 256, seed=3)
    ctx.upload_frames(0, list(fr))
    ctx.flow_pairs(list(range(n_pairs)), list(range(1, n_pairs + 1)), list(range(n_pairs)))
    return ctx


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def test_export_layouts_slices_and_stream_order():
    with flows_ctx() as ctx:
        slots = [4, 0, 5, 2]
        want = [ctx.download_flow(k) for k in slots]
        out = ctx.export_flows(slots)
        assert out.shape == (4, 256, 256, 2) and out.dtype == torch.float32
        assert all(np.array_equal(bits(out[i].cpu().numpy()), bits(w)) for i, w in enumerate(want))
        out = ctx.export_flows(slots, layout="nchw")
        assert all(np.array_equal(bits(out[i].cpu().numpy()), bits(w.transpose(2, 0, 1))) for i, w in enumerate(want))
        big = torch.full((8, 256, 256, 2), float("nan"), device=DEV)
        ctx.export_flows(slots, big[::2])
        got = big.cpu().numpy()
        assert all(np.array_equal(bits(got[2 * i]), bits(w)) for i, w in enumerate(want))
        assert np.isnan(got[1::2]).all()
        planes = torch.zeros((4, 3, 256, 256), device=DEV)
        ctx.export_flows(slots, planes[:, 1:], layout="nchw")
        got = planes.cpu().numpy()
        assert all(np.array_equal(bits(got[i, 1:]), bits(w.transpose(2, 0, 1))) for i, w in enumerate(want))
        assert not got[:, 0].any()
        odd = torch.zeros((4 * 256 * 256 * 2 + 1,), device=DEV)[1:].view(4, 256, 256, 2)   # 4-byte aligned only
        ctx.export_flows(slots, odd)
        assert all(np.array_equal(bits(odd[i].cpu().numpy()), bits(w)) for i, w in enumerate(want))
        # a reduction queued right after the export on its stream, no synchronisation in between
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            o = ctx.export_flows(slots, stream=s)
            total = o.double().sum()
        s.synchronize()
        ref = float(sum(w.astype(np.float64).sum() for w in want))
        assert abs(float(total) - ref) <= 1e-9 * max(1.0, abs(ref))


def test_process_chunk_flows_out_crosses_batches():
    n = 300
    fr = list(sine_translate_frames(n + 1, 256, 256, seed=8))
    B = 64
    fs, fl = pipeline.min_frame_slots(B, 2), pipeline.min_flow_slots(B, 2)
    with _capi.Context(256, 256, max_batch=B, frame_slots=fs, flow_slots=fl) as a, \
            _capi.Context(256, 256, max_batch=B, frame_slots=fs, flow_slots=fl) as b:
        out = torch.full((n, 256, 256, 2), float("nan"), device=DEV)
        dots, recs = pipeline.PairEngine(a).process_chunk(fr, flows_out=out)
        want = [None] * n

        def grab(js, got):
            for j in js:
                want[j] = b.download_flow(j % b.flow_slots)
        eb = pipeline.PairEngine(b)
        h_recs = eb.pass1(fr, 0, n, on_batch=grab)
        h_dots, h_recs2 = pipeline.PairEngine(b).process_chunk(fr)
        assert recs == h_recs == h_recs2 and np.array_equal(dots, h_dots)
        got = out.cpu().numpy()
        for j in range(n):
            assert np.array_equal(bits(got[j]), bits(want[j])), j
        planar = torch.zeros((n, 2, 256, 256), device=DEV)
        pipeline.PairEngine(a).process_chunk(fr, flows_out=planar)
        assert np.array_equal(bits(planar.cpu().numpy()), bits(got.transpose(0, 3, 1, 2)))


class Cai:
    def __init__(self, ptr, shape, strides=None, typestr="|u1"):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": shape, "strides": strides,
                                         "typestr": typestr}


def test_device_refusals():
    with flows_ctx(2) as ctx:
        pin = ctx.pinned_frames(1, channels=3)
        with pytest.raises(_capi.FFLError, match="page-locked host memory"):
            ctx.upload_frames_device(0, [Cai(pin.ctypes.data, (256, 256, 3))], "bgr")
        with pytest.raises(ValueError, match="uint8"):
            ctx.upload_frames_device(0, [torch.zeros((256, 256, 3), device=DEV)], "bgr")
        t = torch.zeros((256, 256, 3), dtype=torch.uint8, device=DEV)
        with pytest.raises(_capi.FFLError, match="bad frame slot range") as e:
            ctx.upload_frames_device(ctx.frame_slots, [t], "bgr")
        assert e.value.code == _capi.FFL_ERR_INVALID
        with pytest.raises(_capi.FFLError, match="more than its allocation holds"):
            ctx.upload_frames_device(0, [Cai(t.data_ptr(), (32768, 32768, 3))], "bgr", (256, 256))
        with pytest.raises(_capi.FFLError, match="out of range"):
            ctx.export_flows([0, ctx.flow_slots])
        with pytest.raises(_capi.FFLError, match="holds no flow") as e:
            ctx.export_flows([ctx.flow_slots - 1])
        assert e.value.code == _capi.FFL_ERR_STATE
        with pytest.raises(ValueError, match="float32"):
            ctx.export_flows([0], torch.zeros((1, 256, 256, 2), dtype=torch.float64, device=DEV))
        with pytest.raises(_capi.FFLError, match="allocation holds"):
            small = torch.zeros((1, 256, 256, 2), device=DEV)
            ctx.export_flows([0, 1], Cai(small.data_ptr(), (2, 256, 256, 2), (1 << 32, 2048, 8, 4), "<f4"))
        # a capture open on the stream: refused with FFL_ERR_STATE before anything touches the stream
        out = torch.zeros((1, 256, 256, 2), device=DEV)
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            cur = torch.cuda.current_stream()
            for call in (lambda: ctx.upload_frames_device(0, [t], "bgr", (256, 256), stream=cur),
                         lambda: ctx.export_flows([0], out, stream=cur)):
                try:
                    call()
                except _capi.FFLError as err:
                    codes.append(err.code)
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [_capi.FFL_ERR_STATE, _capi.FFL_ERR_STATE]
        assert float(x.sum()) == 16.0
        assert ctx.graph_stats()["capture_failures"] == 0
        # and the context still works afterwards
        ctx.upload_frames_device(0, [t], "bgr", (256, 256))
        assert not ctx.download_frame(0).any()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs a second visible GPU")
def test_tensor_on_another_device_is_refused():
    with _capi.Context(256, 256, device=0, max_batch=1, frame_slots=2) as ctx:
        t = torch.zeros((256, 256, 3), dtype=torch.uint8, device="cuda:1")
        with pytest.raises(_capi.FFLError, match="device 1"):
            ctx.upload_frames_device(0, [t], "bgr", (256, 256))
