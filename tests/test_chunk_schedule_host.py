"""Slot liveness of every chunk schedule of funscript_flow_amd/pipeline.py, on the CPU (no GPU, no gpu mark).

PairEngine.process_chunk / process_flows queue work behind each batch on flow slots that a later batch recycles:
_ChunkMotion.behind, _DevicePost.after_batch, _ChunkConsistency's split ring, the calls of window_calls, the host schedule
_ChunkPost.  Here they run against LedgerCtx, a recording stand-in for _capi.Context that keeps a ledger per flow slot -- which
chunk pair it holds, forward or reversed, whether its field is raw or compensated, whether its record is plain or weighted --
and per address of the chunk-long buffers (centre records, cell grids, motion records, consistency maps, post records,
flows_out).  The stand-in executes every call the moment it is issued, which is the order the library guarantees on the
device (a call is ordered behind the batches that wrote its slots, a recycling batch behind the calls that still read them).
Every READER asserts against the ledger at that moment: a slot recycled too early, a fit on an already compensated field, a
map or a centre of another pair, a record read before it was rewritten all show as the wrong pair or the wrong state.

The order held is the one tests/chunk_by_hand.py states for the device: flow -> motion_fit -> motion_subtract ->
pass1_weighted | cell_stats -> window, with flows_out exported behind the subtraction.

The cross product n x B x depth x spare slots x schedule x entry point x keyword set x flows_out layout x engine flavour is
some 10^6 chunks; every AXIS is swept whole, the product is trimmed: every (n, B, depth, spare) context runs a rotating
choice of four keyword sets, each on a rotating schedule, entry point, layout and flavour, and the test asserts that every
keyword set met every n, every B, every (depth, spare), both schedules, every entry point and every layout."""
import itertools
import os
import re
import sys
import types

import numpy as np
import pytest

from funscript_flow_amd import _capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, CELLS = 64, 48, 8
RADIUS = pipeline.SMOOTH_RADIUS
NS, BS, DEPTHS, SPARE = range(0, 46), range(1, 10), (1, 2), (0, 1, 5)


# ---- stand-ins for device memory ----------------------------------------------------------------------------------------------
class Arena:
    """hands out address ranges that never touch; find() names the allocation an address lies in"""

    def __init__(self):
        self.next, self.allocs = 1 << 20, []

    def take(self, nbytes):
        base = self.next
        self.next += (max(int(nbytes), 1) + 8191) // 4096 * 4096
        self.allocs.append((base, max(int(nbytes), 1)))
        return base

    def find(self, ptr):
        for i, (base, nbytes) in enumerate(self.allocs):
            if base <= ptr < base + nbytes:
                return i, ptr - base
        raise AssertionError(f"address {ptr:#x} lies in no allocation")


class DType:
    def __init__(self, name, size, typestr):
        self.name, self.size, self.typestr = name, size, typestr

    def __repr__(self):
        return f"torch.{self.name}"


DTYPES = {d.name: d for d in (DType("uint8", 1, "|u1"), DType("bool", 1, "|b1"), DType("uint16", 2, "<u2"), DType("float16", 2, "<f2"),
                              DType("bfloat16", 2, "bfloat16"), DType("float32", 4, "<f4"), DType("float64", 8, "<f8"))}


class FakeTensor:
    """what pipeline.py and _capi's descriptor functions ask of a torch device tensor, over an Arena address"""
    is_cuda = True

    def __init__(self, ptr, shape, dtype, strides=None):
        self.ptr, self.shape, self.dtype = int(ptr), tuple(int(d) for d in shape), dtype
        if strides is None:
            strides, acc = [], 1
            for d in reversed(self.shape):
                strides.insert(0, acc)
                acc *= d
        self._strides = tuple(strides)

    ndim = property(lambda self: len(self.shape))

    def data_ptr(self):
        return self.ptr

    def stride(self):
        return self._strides

    def element_size(self):
        return self.dtype.size

    def numel(self):
        return int(np.prod(self.shape, dtype=np.int64))

    def __len__(self):
        return self.shape[0]

    def __getitem__(self, key):
        step = self._strides[0] * self.dtype.size
        if isinstance(key, slice):
            lo, hi, st = key.indices(self.shape[0])
            assert st == 1
            return FakeTensor(self.ptr + lo * step, (max(hi - lo, 0),) + self.shape[1:], self.dtype, self._strides)
        assert 0 <= key < self.shape[0]
        return FakeTensor(self.ptr + key * step, self.shape[1:], self.dtype, self._strides[1:])

    @property
    def __cuda_array_interface__(self):
        return {"version": 2, "data": (self.ptr, False), "shape": self.shape, "typestr": self.dtype.typestr,
                "strides": tuple(s * self.dtype.size for s in self._strides)}


def fake_torch(arena):
    """the few names of torch that pipeline.py and _capi touch on the way to a Context call"""
    t = types.ModuleType("torch")
    t.Tensor = FakeTensor
    for name, d in DTYPES.items():
        setattr(t, name, d)
    t.device = lambda kind, index=0: (kind, index)

    def empty(*size, dtype=None, device=None):
        shape = tuple(size[0]) if isinstance(size[0], (tuple, list)) else tuple(size)
        return FakeTensor(arena.take(int(np.prod(shape, dtype=np.int64)) * dtype.size), shape, dtype)

    t.empty = empty
    return t


def span(obj):
    return _capi._device_span(obj)[0]


# ---- the ledger ---------------------------------------------------------------------------------------------------------------
def position(p):
    return (p * 37) % 61, (p * 11) % 47


def record(p):
    x, y = position(p)
    return x, y, np.float32(0.25 * p), np.float32(0.5 * p), p % 3 == 0


class Slot:
    def __init__(self, pair, reverse):
        self.pair, self.reverse, self.fits, self.subtractions, self.weighted = pair, reverse, 0, 0, 0


class LedgerCtx:
    """Stands in for _capi.Context under every schedule.  `want` is what the chunk was asked for: n, device (schedule), comp,
    maps (None | ("static", base) | ("pair", base, stride)), variance, grid (tensor or None), cons (None | dict(maps, gate)),
    flows_out ((tensor, layout) or None), motion (tensor or None), item, axes, pov, thr, src (the source arrays of process_flows)."""

    def __init__(self, arena, max_batch, frame_slots, flow_slots):
        self.arena, self.width, self.height, self.device = arena, W, H, 0
        self.max_batch, self.frame_slots, self.flow_slots = max_batch, frame_slots, flow_slots

    def begin(self, want):
        self.want, n = want, want["n"]
        self.frames, self.slots = {}, [None] * self.flow_slots
        self.post, self.motion, self.exported, self.collected = [0] * n, [0] * n, [0] * n, [0] * n
        self.centres, self.maps = [0] * n, [0] * n
        self.buffers = {}                       # role -> allocation: one buffer per role and chunk
        self.fwd_slots, self.bwd_slots, self.flow_calls = set(), set(), set()

    # -- helpers
    def _stream(self, stream):
        assert stream == ("side" if self.want["device"] else None), f"stream {stream!r}"

    def _where(self, role, ptr, item, known=None):
        """the index of the `item`-byte entry at ptr in the chunk's `role` buffer"""
        alloc, off = self.arena.find(ptr)
        if known is not None:
            assert alloc == self.arena.find(known.data_ptr())[0], f"{role}: not the caller's buffer"
        assert self.buffers.setdefault(role, alloc) == alloc, f"{role}: a second buffer"
        assert off % item == 0, f"{role}: offset {off} is no multiple of {item}"
        return off // item

    def _write_slots(self, slots, pairs):
        assert len(slots) <= self.max_batch and len(set(slots)) == len(slots), slots
        for s, (p, reverse) in zip(slots, pairs):
            assert 0 <= s < self.flow_slots, f"flow slot {s} out of range"
            assert 0 <= p < self.want["n"]
            self.slots[s] = Slot(p, reverse)
            (self.bwd_slots if reverse else self.fwd_slots).add(s)

    def _held(self, slots, first=None, reverse=False, who=""):
        """the consecutive pairs the slots hold (starting at `first` when given), as the readers mean them"""
        assert len(set(slots)) == len(slots) and 1 <= len(slots), (who, slots)
        got = []
        for s in slots:
            assert 0 <= s < self.flow_slots, f"{who}: flow slot {s} out of range"
            assert self.slots[s] is not None, f"{who}: flow slot {s} holds no flow"
            assert self.slots[s].reverse == reverse, f"{who}: flow slot {s} holds pair {self.slots[s].pair} in the wrong direction"
            got.append(self.slots[s].pair)
        first = got[0] if first is None else first
        assert got == list(range(first, first + len(slots))), f"{who}: slots {slots} hold pairs {got}, meant {first}..{first + len(slots) - 1}"
        return first

    def _compensated(self, slots, who):
        """every field and record a reader sees is compensated exactly once under compensate=, never without"""
        for s in slots:
            assert self.slots[s].subtractions == (1 if self.want["comp"] else 0), \
                f"{who}: pair {self.slots[s].pair} in slot {s} read after {self.slots[s].subtractions} subtractions"

    def _maps(self, desc, first, who):
        """the map address handed over is the map of the pair held"""
        kind = self.want["maps"]
        if kind is None:
            assert desc is None, f"{who}: maps without weights="
            return
        assert isinstance(desc, _capi.DevWeights), who
        if kind[0] == "static":
            assert (desc.base, desc.item_stride) == (kind[1], 0), f"{who}: not the static map"
        else:
            assert desc.item_stride == kind[2], who
            assert desc.base == kind[1] + first * kind[2], f"{who}: the maps of pair {(desc.base - kind[1]) / kind[2]} for pair {first}"

    # -- frames and flow calls
    def upload_frames(self, first, frames):
        for k, f in enumerate(frames):
            assert 0 <= first + k < self.frame_slots
            self.frames[first + k] = f

    def _flow(self, name, f0, f1, slots, pov):
        assert pov == self.want["pov"] and len(f0) == len(f1) == len(slots)
        self.flow_calls.add(name)
        pairs = []
        for a, b in zip(f0, f1):
            a, b = self.frames[a], self.frames[b]
            assert abs(a - b) == 1, f"frames {a}, {b} are no pair"
            pairs.append((min(a, b), a > b))
        if self.want["cons"] is None:
            assert not any(r for _, r in pairs), "a reversed pair without weights='consistency'"
        else:   # one call: the batch forward, then the same pairs reversed
            h = len(pairs) // 2
            assert [p for p, r in pairs[:h]] == [p for p, r in pairs[h:]] and not any(r for _, r in pairs[:h]) and all(r for _, r in pairs[h:])
        self._write_slots(slots, pairs)

    def flow_pairs(self, f0, f1, slots, pov=False):
        self._flow("tuned", f0, f1, slots, pov)

    def flow_pairs_dis(self, f0, f1, slots, pov=False, params=None):
        self._flow("dis", f0, f1, slots, pov)

    def flow_pairs_farneback(self, f0, f1, slots, pov=False, params=None, window="box", initial_flow=False):
        self._flow("gaussian" if window != "box" else "params", f0, f1, slots, pov)

    def import_flows_desc(self, desc, dtype, slots, pov=False, stream=None):
        assert pov == self.want["pov"] and stream is None
        for first, t in self.want["src"]:
            alloc, off = self.arena.find(desc.base)
            if alloc == self.arena.find(t.data_ptr())[0]:
                d, _, k = _capi.device_flows(t, W, H)
                assert (desc.item_stride, desc.row_pitch, desc.pixel_stride, desc.channel_stride) == \
                    (d.item_stride, d.row_pitch, d.pixel_stride, d.channel_stride)
                i = 0 if d.item_stride == 0 else (desc.base - d.base) // d.item_stride
                assert desc.base == d.base + i * d.item_stride and i + len(slots) <= k, "fields outside their source array"
                self._write_slots(slots, [(first + i + m, False) for m in range(len(slots))])
                return
        raise AssertionError("import_flows_desc: not a source array of the chunk")

    # -- what is queued behind a batch
    def motion_fit(self, slots, model="translation", iterations=3, tau=1.0, weights=None, prior=None, out=None, sums_out=None, stream=None):
        self._stream(stream)
        assert self.want["comp"] and isinstance(model, _capi.MotionParams) and prior is None
        first = self._held(slots, who="motion_fit")
        for s in slots:
            assert (self.slots[s].fits, self.slots[s].subtractions, self.slots[s].weighted) == (0, 0, 0), f"motion_fit: pair {self.slots[s].pair} is not raw"
            self.slots[s].fits += 1
        self._maps(weights, first, "motion_fit")
        assert self._where("motion", span(out), 64, self.want["motion"]) == first, "motion_out record j is written by the fit of pair j"
        for p in range(first, first + len(slots)):
            self.motion[p] += 1

    def motion_subtract(self, src, dst, models, pov=False, stream=None):
        self._stream(stream)
        assert self.want["comp"] and list(src) == list(dst) and pov == self.want["pov"]
        first = self._held(src, who="motion_subtract")
        assert self._where("motion", span(models), 64, self.want["motion"]) == first
        for s in src:
            assert (self.slots[s].fits, self.slots[s].subtractions) == (1, 0), f"motion_subtract: pair {self.slots[s].pair}: a second subtraction, or none fitted"
            self.slots[s].subtractions += 1
            self.slots[s].weighted = 0            # the records are those of the compensated field

    def pass1_weighted(self, slots, weights, pov=False, stream=None):
        self._stream(stream)
        assert self.want["maps"] is not None and pov == self.want["pov"]
        first = self._held(slots, who="pass1_weighted")
        self._compensated(slots, "pass1_weighted")
        self._maps(weights, first, "pass1_weighted")
        if self.want["cons"] is not None:
            assert all(self.maps[p] == 1 for p in range(first, first + len(slots))), "pass1_weighted before the batch's consistency maps"
        for s in slots:
            assert self.slots[s].weighted == 0
            self.slots[s].weighted += 1

    def cell_stats(self, slots, cells=32, cells_out=None, centres_out=None, stream=None):
        self._stream(stream)
        assert self.want["variance"] and cells == CELLS and centres_out is not None
        first = self._held(slots, who="cell_stats")
        self._compensated(slots, "cell_stats")
        assert self._where("centres", span(centres_out), _capi.GRID_CENTRE_DTYPE.itemsize) == first
        if self.want["grid"] is None:
            assert cells_out is None
        else:
            assert self._where("grid", span(cells_out), CELLS * CELLS * _capi.CELL_DTYPE.itemsize, self.want["grid"]) == first
        for p in range(first, first + len(slots)):
            self.centres[p] += 1

    def consistency_weights(self, fwd, bwd, out, params=None, gate=None, stream=None):
        self._stream(stream)
        cons = self.want["cons"]
        assert cons is not None and isinstance(params, _capi.ConsistencyParams)
        first = self._held(fwd, who="consistency_weights (forward)")
        assert self._held(bwd, first, reverse=True, who="consistency_weights (backward)") == first
        assert all(self.slots[s].subtractions == 0 for s in list(fwd) + list(bwd))
        self._maps(out, first, "consistency_weights")
        if cons["gate"] is None:
            assert gate is None
        else:
            assert (gate.base, gate.item_stride) == (cons["gate"].data_ptr(), 0)
        for p in range(first, first + len(fwd)):
            self.maps[p] += 1

    # -- the window calls
    def _window(self, form, seq, first, count, out, radius, thr, pov, stream, weights=None, centres=None):
        self._stream(stream)
        w, n = self.want, self.want["n"]
        want_form = ("centres" if w["variance"] else "weighted" if w["maps"] is not None else "axes" if w["axes"] else "plain")
        assert form == want_form, f"radial_window form {form}, meant {want_form}"
        assert (radius, thr, pov) == (RADIUS, w["thr"], w["pov"]) and 1 <= count and 0 <= first and first + count <= len(seq)
        j0 = self._where("post", span(out), w["item"], w["post"])
        lo = self._held(seq, j0 - first, who=f"radial_window of pairs {j0}..{j0 + count - 1}")
        self._compensated(seq, "radial_window")
        for s in seq:
            assert self.slots[s].weighted == (1 if w["maps"] is not None else 0), f"radial_window: the record of pair {self.slots[s].pair} is not the one meant"
        for j in range(j0, j0 + count):
            assert lo <= max(0, j - RADIUS) and min(n, j + RADIUS + 1) <= lo + len(seq), f"the window of pair {j} is clipped by its call"
            self.post[j] += 1
        if form == "weighted":
            self._maps(weights, j0, "radial_window_axes_weighted")
        if form == "centres":
            assert self._where("centres", span(centres), _capi.GRID_CENTRE_DTYPE.itemsize) == lo
            assert all(self.centres[p] == 1 for p in range(lo, lo + len(seq))), "a centre read before cell_stats of its pair wrote it"
        return out

    def radial_window(self, seq, first, n, out, radius=6, thr=7.0, pov=False, stream=None):
        return self._window("plain", seq, first, n, out, radius, thr, pov, stream)

    def radial_window_axes(self, seq, first, n, out, radius=6, thr=7.0, pov=False, stream=None):
        return self._window("axes", seq, first, n, out, radius, thr, pov, stream)

    def radial_window_axes_weighted(self, seq, first, n, weights, out, radius=6, thr=7.0, pov=False, stream=None):
        return self._window("weighted", seq, first, n, out, radius, thr, pov, stream, weights=weights)

    def radial_window_axes_centres(self, seq, first, n, centres, out, radius=6, thr=7.0, pov=False, stream=None):
        return self._window("centres", seq, first, n, out, radius, thr, pov, stream, centres=centres)

    # -- flows_out and the host schedule
    def export_flows(self, slots, out=None, layout="nhwc", stream=None):
        assert stream is None and self.want["flows_out"] is not None
        t, want_layout = self.want["flows_out"]
        assert layout == want_layout and out.shape[0] == len(slots) and out.shape[1:] == t.shape[1:]
        first = self._where("flows_out", out.data_ptr(), H * W * 2 * 4, t)
        self._held(slots, first, who="export_flows")
        self._compensated(slots, "export_flows")
        for p in range(first, first + len(slots)):
            self.exported[p] += 1
        return out

    def pass1_results(self, slots, thr=7.0):
        assert not self.want["device"], "the device schedule never collects records"
        assert thr == self.want["thr"]
        first = self._held(slots, who="pass1_results")
        self._compensated(slots, "pass1_results")
        for p in range(first, first + len(slots)):
            self.collected[p] += 1
        return [record(p) for p in range(first, first + len(slots))]

    def _radial(self, slots, cs, cuts, pov):
        assert not self.want["device"] and pov == self.want["pov"]
        first = self._held(slots, who="radial")
        self._compensated(slots, "radial")
        pairs = range(first, first + len(slots))
        cen = pipeline.smooth_centers([position(p) for p in range(self.want["n"])])
        assert np.asarray(cs, np.float64).tobytes() == np.ascontiguousarray(cen[first:first + len(slots)]).tobytes(), "radial: not the window's centres"
        assert [bool(c) for c in cuts] == [record(p)[4] for p in pairs]
        for p in pairs:
            self.post[p] += 1
        return pairs

    def radial(self, slots, cs, cuts, pov=False):
        assert not self.want["axes"]
        return [float(p) for p in self._radial(slots, cs, cuts, pov)]

    def radial_axes(self, slots, cs, cuts, pov=False):
        assert self.want["axes"]
        return np.array([[p, p + 0.25, p + 0.5, p + 0.75] for p in self._radial(slots, cs, cuts, pov)], np.float64).reshape(-1, 4)

    def sync(self):
        raise AssertionError("nothing waits for the device without a prefetch ring")

    # -- the end of a chunk
    def end(self, result):
        w, n = self.want, self.want["n"]
        ones = [1] * n
        assert self.post == ones, f"records written {self.post}"
        assert self.motion == (ones if w["comp"] else [0] * n)
        assert self.exported == (ones if w["flows_out"] is not None else [0] * n)
        assert self.centres == (ones if w["variance"] else [0] * n)
        assert self.maps == (ones if w["cons"] is not None else [0] * n)
        assert not (self.fwd_slots & self.bwd_slots), "a flow slot held forward and reversed pairs"
        if w["device"]:
            assert self.collected == [0] * n and isinstance(result, FakeTensor)
            if w["post"] is not None:
                assert result is w["post"]
            elif n:
                assert self.arena.find(result.data_ptr())[0] == self.buffers["post"]
            assert result.numel() >= n * w["item"]
        else:
            assert self.collected == ones
            dots, recs = result
            want = np.arange(n, dtype=np.float64)
            if w["axes"]:
                want = want[:, None] + np.array([0.0, 0.25, 0.5, 0.75])
            assert np.asarray(dots).shape == want.shape and np.asarray(dots).tobytes() == want.tobytes()
            assert list(recs) == [record(p) for p in range(n)]


# ---- keyword sets -------------------------------------------------------------------------------------------------------------
def tensor(arena, shape, dtype="uint8", pad=0):
    """a device tensor; pad > 0: a view with a padded row pitch and item stride, as a caller's crop would be"""
    d = DTYPES[dtype]
    if not pad:
        return FakeTensor(arena.take(int(np.prod(shape, dtype=np.int64)) * d.size), shape, d)
    n, h, w = shape
    big = FakeTensor(arena.take(n * (h + 2) * (w + pad) * d.size), (n, h + 2, w + pad), d)
    return FakeTensor(big.ptr + ((w + pad) + 5) * d.size, shape, d, big.stride())


def static_map(arena, n):
    t = tensor(arena, (H, W))
    return {"weights": t}, {"maps": ("static", t.data_ptr())}


def pair_maps(arena, n):
    t = tensor(arena, (n, H, W), pad=13)
    return {"weights": t}, {"maps": ("pair", t.data_ptr(), t.stride()[0])}


def variance(arena, n, grid=False):
    kw, want = {"center": "variance", "cells": CELLS}, {"variance": True}
    if grid:
        kw["grid_out"] = want["grid"] = tensor(arena, (max(n, 1) * CELLS * CELLS * _capi.CELL_DTYPE.itemsize,))
    return kw, want


def consistency(arena, n, gate=False, own=False):
    kw, want = {"weights": "consistency"}, {"cons": {"gate": None}}
    if gate:
        kw["weights_gate"] = want["cons"]["gate"] = tensor(arena, (H, W))
        kw["consistency"] = {"alpha": 0.02, "beta": 0.75}
    if own:
        kw["weights_out"] = tensor(arena, (n, H, W))
    return kw, want


def compensate(arena, n, model="translation", out=True):
    kw, want = {"compensate": model}, {"comp": True}
    if out:
        kw["motion_out"] = want["motion"] = tensor(arena, (max(n, 1) * 64,))
    return kw, want


def both(a, b):
    def make(arena, n):
        (k1, w1), (k2, w2) = a(arena, n), b(arena, n)
        return {**k1, **k2}, {**w1, **w2}
    return make


KEYWORDS = {
    "plain": lambda arena, n: ({}, {}),
    "axes": lambda arena, n: ({"axes": True}, {"axes": True}),
    "static-map": static_map,
    "pair-maps": pair_maps,
    "variance": variance,
    "variance-grid": lambda arena, n: variance(arena, n, grid=True),
    "consistency": consistency,
    "consistency-gate": lambda arena, n: consistency(arena, n, gate=True, own=True),
    "compensate": compensate,
    "compensate-axes": both(lambda arena, n: ({"axes": True}, {"axes": True}),
                            lambda arena, n: compensate(arena, n, {"model": "affine", "iterations": 2, "tau": 0.5}, out=False)),
    "compensate-static-map": both(lambda arena, n: compensate(arena, n, "rigid"), static_map),
    "compensate-pair-maps": both(lambda arena, n: compensate(arena, n, "similarity", out=False), pair_maps),
    "compensate-variance": both(lambda arena, n: compensate(arena, n, "affine"), lambda arena, n: variance(arena, n, grid=True)),
}
ENTRIES = ("chunk", "flows", "segments")
LAYOUTS = (None, "nhwc", "nchw")
FLAVOURS = {"tuned": {}, "dis": {"flow": "dis"}, "gaussian": {"window": "gaussian"},
            "params": {"farneback": _capi.FarnebackParams(winsize=13)}}


def segments(n, turn):
    """lengths of source arrays that straddle batch borders; a length of one is a single (H, W, 2) field"""
    if n >= 7:
        return (5, 1, n - 6) if turn % 2 == 0 else (1, n - 3, 2)
    return (1,) * n if turn % 2 == 0 else ((n - 1, 1) if n >= 2 else (n,))


def run_chunk(n, B, depth, spare, device, entry, name, layout, flavour, turn=0):
    """one simulated chunk; raises AssertionError where a reader meets the wrong pair or the wrong state"""
    arena = Arena()
    saved = sys.modules.get("torch")
    sys.modules["torch"] = fake_torch(arena)
    try:
        ctx = LedgerCtx(arena, B, pipeline.min_frame_slots(B, depth) + spare, pipeline.min_flow_slots(B, depth) + spare)
        eng = pipeline.PairEngine(ctx, depth=depth, **(FLAVOURS[flavour] if entry == "chunk" else {}))
        kw, want = KEYWORDS[name](arena, n)
        pov, thr = bool((n + B) & 1), 0.5 + depth
        forced = any(k in want for k in ("maps", "variance", "cons"))      # these run the device schedule whatever post_out says
        want = {"n": n, "comp": False, "maps": None, "variance": False, "grid": None, "cons": None, "flows_out": None, "motion": None,
                "axes": False, "post": None, "src": (), "pov": pov, "thr": thr, **want}
        want["device"] = device or forced
        want["axes"] = want["axes"] or forced
        want["item"] = (_capi.PASS2_AXES_DTYPE if want["axes"] else _capi.PASS2_DTYPE).itemsize
        if device:
            kw["post_out"] = True
            if turn % 2:
                kw["post_out"] = want["post"] = tensor(arena, (max(n, 1) * want["item"] + 16,))
        if entry == "chunk":
            if layout is not None:
                t = tensor(arena, (n, H, W, 2) if layout == "nhwc" else (n, 2, H, W), "float32")
                kw["flows_out"], want["flows_out"] = t, (t, layout)
            if want["cons"] is not None:            # the chunk's maps: the caller's tensor, or one the schedule makes
                own = kw.get("weights_out")
                want["maps"] = ("pair", own.data_ptr(), H * W) if own is not None else ("pair-unknown",)
            ctx.begin(want)
            if want["maps"] == ("pair-unknown",):
                real = sys.modules["torch"].empty

                def empty(*size, dtype=None, device=None):
                    t = real(*size, dtype=dtype, device=device)
                    if t.shape == (max(n, 0), H, W):
                        want["maps"] = ("pair", t.data_ptr(), H * W)
                    return t
                sys.modules["torch"].empty = empty
            result = eng.process_chunk(list(range(n + 1)), pov, thr, **kw)
            if n:
                assert ctx.flow_calls == {flavour}
        else:
            dt = "float32" if turn % 3 else "float16"
            if entry == "flows":
                src = tensor(arena, (n, H, W, 2) if turn % 2 else (n, 2, H, W), dt)
                want["src"], flows = [(0, src)], src
            else:
                flows, first, want["src"] = [], 0, []
                for k in segments(n, turn):
                    t = tensor(arena, (k, H, W, 2), dt)
                    flows.append(t[0] if k == 1 else t)
                    want["src"].append((first, flows[-1]))
                    first += k
                if not flows:
                    flows = [tensor(arena, (0, H, W, 2), dt)]
            ctx.begin(want)
            result = eng.process_flows(flows, pov, thr, **kw)
        ctx.end(result)
        return ctx
    finally:
        if saved is None:
            del sys.modules["torch"]
        else:
            sys.modules["torch"] = saved


@pytest.fixture(autouse=True)
def no_device(monkeypatch):
    monkeypatch.setattr(pipeline, "_side_stream", lambda ctx: "side")
    monkeypatch.setattr(pipeline, "_stream_event", lambda ctx, stream=None: (_ for _ in ()).throw(AssertionError("no ring, no events")))
    monkeypatch.setattr(pipeline._DevicePost, "finish", lambda self: None)      # joins two torch streams: no device here


def applicable(name, entry, n, B):
    if name.startswith("consistency"):
        return entry == "chunk" and B >= 2          # process_flows has no backward fields; a batch is max_batch // 2 pairs
    if "pair-maps" in name:
        return n >= 1                               # (0, H, W) is no tensor of maps
    return True


def test_every_schedule_keeps_every_slot_live_for_its_readers():
    names = list(KEYWORDS)
    seen = {k: set() for k in ("n", "B", "ctx", "device", "entry", "layout", "flavour")}
    chunks = 0
    for c, (n, B, depth, spare) in enumerate(itertools.product(NS, BS, DEPTHS, SPARE)):
        for i in range(4):
            t = c * 4 + i
            name = names[(c + 3 * i + n) % len(names)]
            entry = ENTRIES[(t // 2 + n) % 3]
            if not applicable(name, entry, n, B):
                entry = "chunk"
                if not applicable(name, entry, n, B):
                    continue
            device = bool((t + n // 3) % 2)
            layout = LAYOUTS[(t // 3 + B) % 3] if entry == "chunk" else None
            flavour = list(FLAVOURS)[(t // 5) % 4] if entry == "chunk" else "tuned"
            try:
                ctx = run_chunk(n, B, depth, spare, device, entry, name, layout, flavour, turn=t)
            except AssertionError as e:
                raise AssertionError(f"n={n} B={B} depth={depth} spare={spare} device={device} {entry} {name} {layout} {flavour}: {e}") from e
            chunks += 1
            for key, v in (("n", n), ("B", B), ("ctx", (depth, spare)), ("device", ctx.want["device"]), ("entry", entry)):
                seen[key].add((name, v))
            if entry == "chunk":
                seen["layout"].add((name, layout))
                seen["flavour"].add((name, flavour))
    # the product was trimmed, the axes were not
    for name in names:
        cons, maps = name.startswith("consistency"), "pair-maps" in name
        forced = name not in ("plain", "axes", "compensate", "compensate-axes")
        assert {v for k, v in seen["n"] if k == name} == set(NS) - ({0} if maps else set()), name
        assert {v for k, v in seen["B"] if k == name} == set(BS) - ({1} if cons else set()), name
        assert {v for k, v in seen["ctx"] if k == name} == set(itertools.product(DEPTHS, SPARE)), name
        assert {v for k, v in seen["device"] if k == name} == ({True} if forced else {True, False}), name
        assert {v for k, v in seen["entry"] if k == name} == ({"chunk"} if cons else set(ENTRIES)), name
        assert {v for k, v in seen["layout"] if k == name} == set(LAYOUTS), name
        assert {v for k, v in seen["flavour"] if k == name} == set(FLAVOURS), name
    assert chunks > 9000


# ---- window_calls, a pure function ------------------------------------------------------------------------------------------------
def test_window_calls_never_name_a_recycled_slot():
    """Derived from the schedules, not from min_flow_slots.  Pair p lives in flow slot p % ring (PairEngine.pass1,
    process_flows), so the next pair written over it is p + ring, queued with batch (p + ring) // B.  The host schedule
    collects batch k -- and only then issues the calls window_calls lists after batch k -- once batch k + depth has been
    queued (pass1_pairs keeps depth + 1 batches pending before it collects the oldest); the device schedule issues them
    earlier, straight after batch k.  So when a call is issued, batches 0 .. after + depth have written their slots and a pair
    p of its seq is intact iff (p + ring) // B > after + depth or pair p + ring does not exist.

    How long must the ring be?  The calls after batch k start at pair done, where done >= k * B - radius is where the calls after
    batch k - 1 stopped, so their seq starts at lo >= k * B - 2 * radius; the last pair queued by then is (k + depth + 1) * B - 1.
    Every pair between the two is live at once: (depth + 1) * B + 2 * radius pairs.  The + 2 * radius are the pairs still
    waiting for their window to fill and the window of the oldest of them; min_flow_slots adds one to that, so this
    inequality holds with one slot to spare and first fails two slots below the bound.

    Neither schedule of today uses the whole of it: the device schedule issues its calls straight after batch k (B + 2 *
    radius live pairs), and the host schedule, depth batches later, re-reads only the slots of the pairs it computes, their
    centres coming from records it already holds ((depth + 1) * B + radius).  The bound is the one a caller needs who runs the
    device's window calls depth batches behind its flow calls, which is what include/ffl.h documents."""
    for n, B, depth in itertools.product(NS, BS, DEPTHS):
        ring = pipeline.min_flow_slots(B, depth)
        calls = pipeline.window_calls(n, B)
        issued = [0] * n
        for lo, hi, first, count, after in calls:
            assert 0 <= lo <= lo + first and lo + first + count <= hi <= n and count >= 1
            for j in range(lo + first, lo + first + count):
                issued[j] += 1
                assert lo <= max(0, j - RADIUS) and min(n, j + RADIUS + 1) <= hi
            last_queued = min((after + 1) * B, n) - 1
            assert hi - 1 <= last_queued, "a seq names a pair later than its after_batch"
            for p in range(lo, hi):
                assert p + ring >= n or (p + ring) // B > after + depth, (n, B, depth, lo, hi, after, p)
            assert min((after + depth + 1) * B, n) - lo <= (depth + 1) * B + 2 * RADIUS
        assert issued == [1] * n, (n, B)
        assert [c[4] for c in calls] == sorted(c[4] for c in calls)


def test_min_flow_slots_is_the_bound_the_header_documents():
    """include/ffl.h tells callers of ffl_create what a streaming two-pass schedule needs; the Python bound at depth 1 is that
    sentence, and every further batch in flight adds max_batch"""
    text = open(os.path.join(ROOT, "include", "ffl.h")).read()
    m = re.search(r"needs\s*>=\s*(\d+)\s*\*\s*max_batch\s*\+\s*(\d+)", text)
    assert m, "ffl.h no longer states the flow-slot bound"
    per_batch, const = int(m.group(1)), int(m.group(2))
    for B in BS:
        assert pipeline.min_flow_slots(B) == pipeline.min_flow_slots(B, 1) == per_batch * B + const
        for depth in (2, 3):
            assert pipeline.min_flow_slots(B, depth) - pipeline.min_flow_slots(B, depth - 1) == B
