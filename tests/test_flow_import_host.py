"""Host side of the flow import: descriptors built from __cuda_array_interface__ objects, every refusal
of ffl_dev_flow_check and of the Python layer by its rule, and pair_plan / flows_to_actions against frames_to_actions with
stand-in engines.  No device is needed: the pointers are never read."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from funscript_flow_amd import _capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7F0000000000
W, H = 40, 24


class Cai:
    """a fake device array: only __cuda_array_interface__"""

    def __init__(self, shape, strides=None, typestr="<f4", ptr=BASE, version=3):
        self.__cuda_array_interface__ = {"version": version, "data": (ptr, False), "shape": tuple(shape),
                                         "strides": None if strides is None else tuple(strides), "typestr": typestr}


def fields(d):
    return d.base, d.item_stride, d.row_pitch, d.pixel_stride, d.channel_stride


def test_nhwc_float32():
    d, dt, n = _capi.device_flows(Cai((5, H, W, 2)), W, H)
    assert (fields(d), dt, n) == ((BASE, H * W * 8, W * 8, 8, 4), 0, 5)
    _capi.dev_flow_check(dt, n, W, H, d)


def test_nchw_float32():
    d, dt, n = _capi.device_flows(Cai((3, 2, H, W)), W, H)
    assert (fields(d), dt, n) == ((BASE, 2 * H * W * 4, W * 4, 4, H * W * 4), 0, 3)
    _capi.dev_flow_check(dt, n, W, H, d)


def test_float16_nhwc_and_nchw():
    d, dt, n = _capi.device_flows(Cai((2, H, W, 2), typestr="<f2"), W, H)
    assert (fields(d), dt, n) == ((BASE, H * W * 4, W * 4, 4, 2), 1, 2)
    _capi.dev_flow_check(dt, n, W, H, d)
    d, dt, n = _capi.device_flows(Cai((2, 2, H, W), typestr="<f2"), W, H)
    assert (fields(d), dt, n) == ((BASE, 2 * H * W * 2, W * 2, 2, H * W * 2), 1, 2)
    _capi.dev_flow_check(dt, n, W, H, d)


def test_slice_with_padded_row_pitch():
    # x[:, 3:3 + H, 5:5 + W, :] of a (4, 32, 48, 2) float32 array
    st = (32 * 48 * 8, 48 * 8, 8, 4)
    ptr = BASE + 3 * st[1] + 5 * st[2]
    d, dt, n = _capi.device_flows(Cai((4, H, W, 2), strides=st, ptr=ptr), W, H)
    assert (fields(d), dt, n) == ((ptr,) + st, 0, 4)
    _capi.dev_flow_check(dt, n, W, H, d)


def test_single_field_and_row_planar():
    d, dt, n = _capi.device_flows(Cai((H, W, 2)), W, H)
    assert (fields(d), dt, n) == ((BASE, 0, W * 8, 8, 4), 0, 1)
    _capi.dev_flow_check(dt, n, W, H, d)
    # u row then v row inside one row pitch: (n, H, 2, W) viewed as (n, H, W, 2)
    d = _capi.DevFlow(BASE, H * 2 * W * 4, 2 * W * 4, 4, W * 4)
    _capi.dev_flow_check(0, 2, W, H, d)


def rule(dtype, n, desc, w=W, h=H):
    L = _capi.load()
    assert L.ffl_dev_flow_check(dtype, n, w, h, None if desc is None else C.byref(desc)) == _capi.FFL_ERR_INVALID
    return L.ffl_last_error(None).decode()


def test_library_refusals_name_their_rule():
    ok = _capi.DevFlow(BASE, H * W * 8, W * 8, 8, 4)
    assert "NULL descriptor" in rule(0, 1, None)
    assert "unknown dtype 3" in rule(3, 1, ok)
    assert "n = 0 fields" in rule(0, 0, ok)
    assert "size 1x24" in rule(0, 1, ok, w=1)
    assert "NULL base" in rule(0, 1, _capi.DevFlow(None, 0, W * 8, 8, 4))
    assert "negative stride" in rule(0, 1, _capi.DevFlow(BASE, -8, W * 8, 8, 4))
    assert "negative stride" in rule(0, 1, _capi.DevFlow(BASE, 0, -W * 8, 8, 4))
    assert "beyond 2^40" in rule(0, 1, _capi.DevFlow(BASE, 1 << 41, W * 8, 8, 4))
    assert "misaligned" in rule(0, 1, _capi.DevFlow(BASE + 2, 0, W * 8, 8, 4))
    assert "misaligned" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 8 + 2, 8, 4))
    assert "misaligned" in rule(1, 1, _capi.DevFlow(BASE + 1, 0, W * 4, 4, 2))
    assert "pixel stride 0 below" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 8, 0, 4))
    assert "row pitch 312 too small" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 8 - 8, 8, 4))
    assert "u and v overlap" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 8, 8, 0))          # the same element
    assert "u and v overlap" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 8, 8, 8))          # v on the next pixel's u
    assert "u and v overlap" in rule(0, 1, _capi.DevFlow(BASE, 0, W * 4, 4, W * 4 * (H - 1)))   # planes overlap
    assert "overlap" in rule(0, 1, _capi.DevFlow(BASE, 0, 4, H * 4, W * H * 4))        # a transposed view


def test_python_refusals_name_their_rule():
    with pytest.raises(ValueError, match="not device memory"):
        _capi.device_flows(np.zeros((H, W, 2), np.float32), W, H)
    with pytest.raises(ValueError, match="dtype '<f8' is not supported"):
        _capi.device_flows(Cai((1, H, W, 2), typestr="<f8"), W, H)
    with pytest.raises(ValueError, match="dtype '|u1' is not supported"):
        _capi.device_flows(Cai((1, H, W, 2), typestr="|u1"), W, H)
    with pytest.raises(ValueError, match="size"):
        _capi.device_flows(Cai((1, H, W + 8, 2)), W, H)
    with pytest.raises(ValueError, match="size"):
        _capi.device_flows(Cai((H + 2, W, 2)), W, H)
    with pytest.raises(ValueError, match="size"):
        _capi.device_flows(Cai((1, 2, H, W - 1)), W, H)
    with pytest.raises(ValueError, match="shape"):
        _capi.device_flows(Cai((1, H, W, 3)), W, H)
    with pytest.raises(ValueError, match="shape"):
        _capi.device_flows(Cai((H * W * 2,)), W, H)
    with pytest.raises(ValueError, match="version"):
        _capi.device_flows(Cai((1, H, W, 2), version=1), W, H)


def test_import_leaves_torch_out():
    code = "import sys, funscript_flow_amd, funscript_flow_amd._capi, funscript_flow_amd.pipeline; " \
           "print('torch' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False"


def _scalars(pairs):
    """stand-in pass-1 / pass-2 results of pairs (a, b) of frame indices: deterministic and varied"""
    recs = [(int(a * 7 % 40), int(b * 3 % 24), np.float32(0.5), np.float32(1.0), a % 37 == 5) for a, b in pairs]
    dots = np.array([np.sin(0.37 * a) + 0.1 * b for a, b in pairs], np.float64)
    return dots, recs


class FrameEngine:
    """stand-in for frames_to_actions: frames are arrays filled with their own frame index"""

    def __init__(self):
        self.chunks = []

    def process_chunk(self, frames, pov_mode=False, cut_threshold=7.0, **kw):
        idx = [int(f[0, 0]) for f in frames]
        self.chunks.append(idx)
        return _scalars(list(zip(idx[:-1], idx[1:])))


class FlowEngine:
    """stand-in for flows_to_actions: a chunk's "flows" are the list of its pairs"""

    def process_flows(self, flows, pov_mode=False, cut_threshold=7.0):
        return _scalars(flows)


PARAMS = {"detrend_window": 1.5, "norm_window": 4.0, "keyframe_reduction": True}


@pytest.mark.parametrize("fps,total,bracket", [(30.0, 65, 16), (60.0, 200, 3000.0), (59.94, 301, 37), (24.0, 20, 5),
                                               (30.0, 46, 15)])
def test_pair_plan_and_flows_to_actions_match_frames_to_actions(fps, total, bracket):
    params = dict(PARAMS, batch_size=bracket)
    frames = [np.full((4, 4), i, np.int64) for i in range(total)]
    eng = FrameEngine()
    want = pipeline.frames_to_actions(eng, frames, fps, params)
    plan = pipeline.pair_plan(fps, total, params)
    assert plan == eng.chunks
    chunk_flows = [list(zip(c[:-1], c[1:])) for c in plan]
    assert pipeline.flows_to_actions(FlowEngine(), chunk_flows, fps, total, params) == want
    if plan:
        with pytest.raises(ValueError, match="chunks"):
            pipeline.flows_to_actions(FlowEngine(), chunk_flows[:-1], fps, total, params)
        with pytest.raises(ValueError, match="needs"):
            pipeline.flows_to_actions(FlowEngine(), [f[:-1] for f in chunk_flows], fps, total, params)
