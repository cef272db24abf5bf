"""GPU side of the flow import: fields imported from torch tensors on cuda:0 give upload_flow's
records and the reference goldens; flows exported by process_chunk and imported again by process_flows give the same
dots and records; float16 / bfloat16 equal their float32 widening; strided sources; stream ordering without host
synchronisation; device-side refusals; flows_to_actions against frames_to_actions."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle as orc
import post_ref as pr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
GOLDENS = ["noise_36x64", "smooth_90x160", "noise_256x256", "ties_40x72", "negfirst_24x40", "farneback_180x320", "edge_32x48"]


@pytest.fixture(scope="module")
def post(golden_dir):
    return np.load(os.path.join(golden_dir, "post_goldens.npz"))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def uploaded_records(ctx, fields, slot0, pov=False):
    """upload_flow's records of host (H, W, 2) float32 fields, through slots slot0, slot0 + 1, ..."""
    for i, f in enumerate(fields):
        ctx.upload_flow(slot0 + i, np.ascontiguousarray(f, np.float32), pov)
    return ctx.pass1_results(list(range(slot0, slot0 + len(fields))))


@pytest.mark.parametrize("layout", ["nhwc", "nchw"])
@pytest.mark.parametrize("name", GOLDENS)
def test_goldens(post, name, layout):
    flow = post[f"{name}.flow"]
    h, w, _ = flow.shape
    t = dev(flow)[None] if layout == "nhwc" else dev(flow.transpose(2, 0, 1))[None]
    with _capi.Context(w, h, max_batch=2, flow_slots=8) as ctx:
        want = uploaded_records(ctx, [flow], 0)[0]
        ctx.import_flows(t, [1])
        got = ctx.pass1_result(1)
        assert got == want
        x, y, v, mm, _ = got
        assert (x, y) == tuple(post[f"{name}.maxdiv"])
        assert np.float32(v).tobytes() == np.float32(post[f"{name}.maxdiv_val"]).tobytes()
        ref_mm = float(orc.mean_mag_np(flow))
        assert abs(float(mm) - ref_mm) <= 1e-4 * max(ref_mm, 1e-30)
        pr.check_mean_mag(mm, flow)
        assert np.array_equal(bits(ctx.download_flow(1)), bits(flow))
        scale = float(np.mean(np.abs(flow))) * max(h, w)
        for c, (gw, gp, gc) in zip(post[f"{name}.centers"], post[f"{name}.radial"]):
            assert abs(ctx.radial([1], [c], [False], False)[0] - gw) <= 1e-4 * max(abs(gw), 1e-6 * scale)
            assert abs(ctx.radial([1], [c], [False], True)[0] - gp) <= 1e-4 * max(abs(gp), 1e-6 * scale)
            for pov in (False, True):
                pr.check_radial(ctx.radial([1], [c], [False], pov)[0], flow, c, pov)
            assert ctx.radial([1], [c], [True], False)[0] == gc == 0.0
        # pov_mode as in upload_flow
        ctx.import_flows(t, [2], pov_mode=True)
        assert ctx.pass1_result(2) == uploaded_records(ctx, [flow], 3, pov=True)[0]


def engines(B, w=256, h=256):
    fs, fl = pipeline.min_frame_slots(B, 2), pipeline.min_flow_slots(B, 2)
    return (_capi.Context(w, h, max_batch=B, frame_slots=fs, flow_slots=fl),
            _capi.Context(w, h, max_batch=B, frame_slots=fs, flow_slots=fl))


ROUND_TRIPS = [("farneback", 256, 256, 64, 200), ("dis", 256, 256, 64, 200), ("farneback_w21", 256, 256, 64, 200),
               ("farneback", 1920, 1080, 32, 40)]


@pytest.mark.parametrize("algo,w,h,B,n", ROUND_TRIPS)
def test_round_trip(algo, w, h, B, n):
    fr = list(sine_translate_frames(n + 1, w, h, seed=21))
    kw = {"dis": dict(flow="dis"), "farneback_w21": dict(farneback=_capi.FarnebackParams(winsize=21))}.get(algo, {})
    a, b = engines(B, w, h)
    with a, b:
        T = torch.empty((n, h, w, 2), device=DEV)
        dots, recs = pipeline.PairEngine(a, **kw).process_chunk(fr, flows_out=T)
        d2, r2 = pipeline.PairEngine(b).process_flows(T)
        assert r2 == recs and np.array_equal(d2, dots)
        d3, r3 = pipeline.PairEngine(b).process_flows(T.permute(0, 3, 1, 2).contiguous())
        assert r3 == recs and np.array_equal(d3, dots)
        if algo == "farneback" and w == 256:
            # half precision: the import of a float16 / bfloat16 field equals that of its float32 widening
            for dt in (torch.float16, torch.bfloat16):
                lo = T.to(dt)
                dl, rl = pipeline.PairEngine(b).process_flows(lo)
                dw, rw = pipeline.PairEngine(b).process_flows(lo.float())
                assert rl == rw and np.array_equal(dl, dw)
                dl, rl = pipeline.PairEngine(b).process_flows(lo.permute(0, 3, 1, 2).contiguous())
                assert rl == rw and np.array_equal(dl, dw)
            # a sequence of arrays (single fields and a block) in pair order
            parts = [T[0], T[1:70], T[70], T[71:]]
            d4, r4 = pipeline.PairEngine(b).process_flows(parts)
            assert r4 == recs and np.array_equal(d4, dots)
        assert a.graph_stats()["capture_failures"] == 0 and b.graph_stats()["capture_failures"] == 0


def test_strided_sources():
    w, h, n = 200, 72, 5
    g = torch.Generator(device=DEV).manual_seed(5)
    with _capi.Context(w, h, max_batch=n, flow_slots=8 * n) as ctx:
        cases = []
        big = torch.randn((n, h + 5, w + 9, 2), device=DEV, generator=g) * 4
        cases.append(big[:, 2:2 + h, 3:3 + w, :])                                   # padded row pitch, float32 NHWC
        cl = (torch.randn((n, 2, h, w), device=DEV, generator=g) * 4).contiguous(memory_format=torch.channels_last)
        cases.append(cl)                                                            # channels-last (n, 2, H, W)
        hb = (torch.randn((n, h + 2, w + 3, 2), device=DEV, generator=g) * 4).half()
        cases.append(hb[:, 1:1 + h, 1:1 + w, :])                                    # float16 at an odd offset
        bb = (torch.randn((n, 2, h, w + 7), device=DEV, generator=g) * 4).bfloat16()
        cases.append(bb[..., 7:])                                                   # bfloat16 planes, padded pitch
        for k, t in enumerate(cases):
            host = (t if t.shape[-1] == 2 else t.permute(0, 2, 3, 1)).float().cpu().numpy()
            slots = list(range(2 * k * n, 2 * k * n + n))
            want = uploaded_records(ctx, list(host), slots[-1] + 1)
            ctx.import_flows(t, slots)
            assert ctx.pass1_results(slots) == want, k
            for i, s in enumerate(slots):
                assert np.array_equal(bits(ctx.download_flow(s)), bits(host[i])), (k, i)


def test_stream_order_producer_and_overwrite():
    w, h, n = 256, 256, 16
    with _capi.Context(w, h, max_batch=n, flow_slots=2 * n) as ctx:
        src = torch.randn((n, h, w, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) * 3
        want = uploaded_records(ctx, list(src.cpu().numpy() * np.float32(1.5)), n)
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            t = src * 1.5                         # produced on the side stream, no host synchronisation
            for _ in range(20):                   # keep the producer busy for a while
                t = (t * 2.0) * 0.5
            ctx.import_flows(t, list(range(n)), stream=s)
            t.fill_(float("nan"))                 # overwritten on the same stream straight after the call
        assert ctx.pass1_results(list(range(n))) == want
        torch.cuda.synchronize()
        assert torch.isnan(t).all()


def test_import_into_slots_of_a_queued_batch():
    w, h, B = 256, 256, 8
    fr = list(sine_translate_frames(B + 1, w, h, seed=4))
    with _capi.Context(w, h, max_batch=B, frame_slots=B + 1, flow_slots=2 * B) as ctx:
        fields = torch.randn((B, h, w, 2), device=DEV, generator=torch.Generator(device=DEV).manual_seed(2))
        host = fields.cpu().numpy()
        want = uploaded_records(ctx, list(host), B)
        ctx.upload_frames(0, fr)
        ctx.flow_pairs(list(range(B)), list(range(1, B + 1)), list(range(B)))   # still queued when the import comes
        ctx.import_flows(fields, list(range(B)))
        assert ctx.pass1_results(list(range(B))) == want
        for j in range(B):
            assert np.array_equal(bits(ctx.download_flow(j)), bits(host[j]))


class Cai:
    def __init__(self, ptr, shape, strides=None, typestr="<f4"):
        self.__cuda_array_interface__ = {"version": 2, "data": (int(ptr), False), "shape": shape, "strides": strides,
                                         "typestr": typestr}


def test_device_refusals():
    w, h = 256, 256
    with _capi.Context(w, h, max_batch=2, frame_slots=4, flow_slots=4) as ctx:
        t = torch.zeros((2, h, w, 2), device=DEV)
        with pytest.raises(ValueError, match="not device memory"):
            ctx.import_flows(np.zeros((h, w, 2), np.float32), [0])
        with pytest.raises(ValueError, match="not device memory"):
            ctx.import_flows(torch.zeros((h, w, 2)), [0])
        pin = ctx.pinned_frames(2, channels=4)          # ffl_host_alloc memory: 2 * H * W * 4 bytes = one field
        with pytest.raises(_capi.FFLError, match="page-locked host memory.*upload_flow") as e:
            ctx.import_flows(Cai(pin.ctypes.data, (1, h, w, 2)), [0])
        assert e.value.code == _capi.FFL_ERR_INVALID
        with pytest.raises(_capi.FFLError, match="more than its allocation holds"):
            ctx.import_flows(Cai(t.data_ptr(), (2, h, w, 2), (1 << 32, w * 8, 8, 4)), [0, 1])
        with pytest.raises(_capi.FFLError, match="outside 1..2"):
            ctx.import_flows(torch.zeros((3, h, w, 2), device=DEV), [0, 1, 2])
        for _ in range(2):                              # refused twice in a row, and the refusal leaves no mark behind:
            with pytest.raises(_capi.FFLError, match="repeated"):
                ctx.import_flows(t, [1, 1])
        ctx.import_flows(t, [1, 2])                     # a legal import naming the same slot goes through
        assert ctx.pass1_results([1, 2]) == uploaded_records(ctx, list(t.cpu().numpy()), 1)
        with pytest.raises(_capi.FFLError, match="out of range"):
            ctx.import_flows(t, [0, 4])
        with pytest.raises(ValueError, match="not supported"):
            ctx.import_flows(t.double(), [0, 1])
        with pytest.raises(ValueError, match="size"):
            ctx.import_flows(torch.zeros((2, h, w - 2, 2), device=DEV), [0, 1])
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            try:
                ctx.import_flows(t, [0, 1], stream=torch.cuda.current_stream())
            except _capi.FFLError as err:
                codes.append(err.code)
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [_capi.FFL_ERR_STATE]
        assert float(x.sum()) == 16.0
        assert ctx.graph_stats()["capture_failures"] == 0
        ctx.import_flows(t, [0, 1])                     # the context still works afterwards
        assert ctx.pass1_results([0, 1]) == uploaded_records(ctx, list(t.cpu().numpy()), 2)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_flows_to_actions_equals_frames_to_actions():
    n_frames, B = 65, 8
    fr = list(sine_translate_frames(n_frames, 256, 256, seed=30))
    params = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False}
    plan = pipeline.pair_plan(30.0, n_frames, params)
    assert len(plan) > 2
    a, b = engines(B)
    with a, b:
        ea = pipeline.PairEngine(a)
        chunk_flows = []
        for chunk in plan:
            out = torch.empty((len(chunk) - 1, 256, 256, 2), device=DEV)
            ea.process_chunk([fr[i] for i in chunk], flows_out=out)
            chunk_flows.append(out)
        want = pipeline.frames_to_actions(pipeline.PairEngine(b), fr, 30.0, params)
        got = pipeline.flows_to_actions(pipeline.PairEngine(b), chunk_flows, 30.0, n_frames, params)
        assert want and got == want
