"""Host side of device-memory I/O: descriptors built from __cuda_array_interface__ objects, and every
refusal of ffl_dev_frame_check and of the Python layer, by its rule.  No device is needed: the pointers are never read."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from funscript_flow_amd import _capi, frontend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = 0x7F0000000000


class Cai:
    """a fake device array: only __cuda_array_interface__"""

    def __init__(self, shape, strides=None, typestr="|u1", ptr=BASE, version=3):
        self.__cuda_array_interface__ = {"version": version, "data": (ptr, False), "shape": tuple(shape),
                                         "strides": None if strides is None else tuple(strides), "typestr": typestr}


def fields(f):
    return list(f.plane), list(f.pitch), f.pixel_stride, f.channel_stride, (f.width, f.height)


def test_packed_bgr():
    f = _capi.device_frame(Cai((1080, 1920, 3)), "bgr")
    assert fields(f) == ([BASE, None, None], [5760, 0, 0], 3, 1, (1920, 1080))
    _capi.dev_frame_check("bgr", f, (256, 256), (0, 0), (256, 256))


def test_bgra_ignores_channel_3():
    f = _capi.device_frame(Cai((720, 1280, 4), version=2), "bgr")
    assert fields(f) == ([BASE, None, None], [5120, 0, 0], 4, 1, (1280, 720))
    _capi.dev_frame_check("bgr", f, (256, 256), (0, 0), (256, 256))


def test_chw_planar():
    f = _capi.device_frame(Cai((3, 90, 160)), "rgb")
    assert fields(f) == ([BASE, None, None], [160, 0, 0], 1, 160 * 90, (160, 90))
    _capi.dev_frame_check("rgb", f, (256, 256), (0, 0), (256, 256))


def test_sliced_view_with_padded_pitch():
    # x[:, 8:8 + 640, :] of a (360, 704, 3) array: the row pitch of the parent, the data pointer moved by 8 pixels
    f = _capi.device_frame(Cai((360, 640, 3), strides=(704 * 3, 3, 1), ptr=BASE + 24), "bgr")
    assert fields(f) == ([BASE + 24, None, None], [2112, 0, 0], 3, 1, (640, 360))
    g = _capi.device_frame(Cai((256, 256), strides=(512, 1)), "gray")
    assert fields(g) == ([BASE, None, None], [512, 0, 0], 1, 0, (256, 256))
    _capi.dev_frame_check("gray", g, (256, 256), (0, 0), (256, 256))


def test_nv12_and_i420_single_arrays():
    nv = _capi.device_frame(Cai((540, 640), strides=(704, 1)), "nv12")   # 360 rows of Y, 180 of UV, pitch 704
    assert fields(nv) == ([BASE, BASE + 360 * 704, None], [704, 704, 0], 1, 0, (640, 360))
    i4 = _capi.device_frame(Cai((540, 640)), "i420")
    u = BASE + 360 * 640
    assert fields(i4) == ([BASE, u, u + 180 * 320], [640, 320, 320], 1, 0, (640, 360))
    for fmt, f in (("nv12", nv), ("i420", i4)):
        _capi.dev_frame_check(fmt, f, (256, 256), (0, 0), (256, 256))


def test_batched_array_rows():
    rows, size = _capi.Context._device_rows(Cai((5, 90, 160, 3)), _capi.DEV_FORMATS["bgr"])
    assert size == (160, 90)
    assert [int(r[0]) for r in rows] == [BASE + i * 90 * 160 * 3 for i in range(5)]
    assert all(list(map(int, r[3:])) == [480, 0, 0, 3, 1] for r in rows)


def refused(fmt, frame, resize=(256, 256), crop=(0, 0), out=(256, 256)):
    with pytest.raises(ValueError) as e:
        _capi.dev_frame_check(fmt, frame, resize, crop, out)
    return str(e.value)


def test_python_refusals_name_their_rule():
    with pytest.raises(ValueError, match="uint8"):
        _capi.device_frame(Cai((256, 256, 3), typestr="<f4"), "bgr")
    with pytest.raises(ValueError, match="not device memory"):
        _capi.device_frame(np.zeros((256, 256, 3), np.uint8), "bgr")
    with pytest.raises(ValueError, match="unknown device frame format"):
        _capi.device_frame(Cai((256, 256, 3)), "yuyv")
    with pytest.raises(ValueError, match="unknown flow layout"):
        _capi.flow_layout("nhcw")
    with pytest.raises(ValueError, match="3h/2"):
        _capi.device_frame(Cai((361, 640)), "nv12")
    with pytest.raises(ValueError, match="contiguous"):
        _capi.device_frame(Cai((540, 640), strides=(1280, 2)), "nv12")
    with pytest.raises(ValueError, match="I420 needs contiguous rows"):
        _capi.device_frame(Cai((540, 640), strides=(704, 1)), "i420")
    with pytest.raises(ValueError, match="version"):
        _capi.device_frame(Cai((256, 256), version=1), "gray")
    with pytest.raises(ValueError):
        frontend.DeviceUploader(object(), fmt="p010")


def test_library_refusals_name_their_rule():
    bgr = lambda shape, strides: _capi.device_frame(Cai(shape, strides), "bgr")
    assert "negative stride" in refused("bgr", bgr((256, 256, 3), (-768, 3, 1)))
    assert "pixel stride 0 too small" in refused("bgr", bgr((256, 256, 3), (768, 0, 1)))
    assert "pitch 700 too small" in refused("bgr", bgr((256, 256, 3), (700, 3, 1)))
    assert "channel stride 0 too small" in refused("bgr", bgr((256, 256, 3), (768, 3, 0)))
    assert "neither packed" in refused("rgb", _capi.device_frame(Cai((3, 256, 256), (1000, 256, 1)), "rgb"))
    gray = _capi.device_frame(Cai((256, 256)), "gray")
    assert "a resize (256x256 -> 512x512) is refused" in refused("gray", gray, resize=(512, 512), crop=(0, 256))
    assert "must be the context size" in refused("gray", _capi.device_frame(Cai((128, 256)), "gray"), resize=(256, 128))
    odd = _capi.device_frame(Cai((543, 641)), "nv12")
    assert "even width and height" in refused("nv12", odd)
    assert "does not fit" in refused("bgr", bgr((1080, 1920, 3), None), resize=(256, 256), crop=(1, 0))
    assert "does not fit" in refused("bgr", bgr((1080, 1920, 3), None), resize=(512, 512), crop=(0, 257))
    nv = _capi.device_frame(Cai((540, 640), (600, 1)), "nv12")
    assert "Y pitch 600 too small" in refused("nv12", nv)
    f = _capi.device_frame(Cai((256, 256, 3)), "bgr")
    L = _capi.load()
    assert L.ffl_dev_frame_check(7, 256, 256, C.byref(f), 256, 256, 0, 0, 256, 256) == _capi.FFL_ERR_INVALID
    assert "unknown format 7" in L.ffl_last_error(None).decode()
    assert L.ffl_dev_frame_check(1, 256, 256, None, 256, 256, 0, 0, 256, 256) == _capi.FFL_ERR_INVALID
    assert "NULL descriptor" in L.ffl_last_error(None).decode()


def test_import_leaves_torch_out():
    code = "import sys, funscript_flow_amd, funscript_flow_amd._capi, funscript_flow_amd.frontend, funscript_flow_amd.pipeline; " \
           "print('torch' in sys.modules)"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    assert out.strip() == "False"
