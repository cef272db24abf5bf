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

The modes that read FRAME slots behind a batch (pass1_pairs' with_frames hook: weights="residual" | "texture", their
combination, track["match"]) and the track add three ledgers.  Frames: upload_frames records which frame a frame slot holds,
and residual_weights, texture_weights, track_match and track_template assert that slot k still holds frame js[k] (f0) or
js[k] + 1 (f1) of the pair whose flow slot, map address and record address they are given -- a slot re-staged too early, or a
hook handed another batch's slots, shows as the wrong frame.  Maps: a state machine per pair, unwritten -> residual (from a
field with no fit and no subtraction) -> texture combined (gate = out, behind the residual write); "texture" alone and the
ROI map are one write; motion_fit, pass1_weighted and the weighted window forms meet a map only in its final state.  Track: one
counter "next pair to advance"; track_advance takes consecutive raw pairs from it and writes at first * 48 * T, track_template
runs at most once, before the first advance, on the slot of frame 0; the records' match runs on the f0 slots of records
advanced and not yet matched, the state's match is one item on the slot of frame last + 1 straight behind it, roi_weights
comes after both; the fit under a track is unweighted; the window forms about the track buffer (base lo * 48 * T, stride
48 * T) find every pair of their seq advanced, matched and mapped.  With track["match"]["redetect"] track_redetect is one item
on the slot of frame last + 1 about the state tensor (stride 48 * T) with the chunk's templates, straight behind the state's
match of the batch just advanced and at most once per batch -- every advance but the first finds one re-detection per batch
before it --, its trigger is the span the state's match of THIS batch wrote (a mark the next advance clears), write_back is
true, and its 48 * T bytes go to record `last` of redetect_out, each record written at most once per chunk and no other record
ever; roi_weights then comes behind it.

The cross product n x B x depth x spare slots x schedule x entry point x keyword set x flows_out layout x engine flavour is
some 10^6 chunks; every AXIS is swept whole, the product is trimmed: every (n, B, depth, spare) context runs a rotating
choice of five keyword sets (PER_CONTEXT; four reached every axis value while there were thirteen sets, not with
twenty-seven; five still do with thirty-one), each on a rotating schedule, entry point, layout and flavour, and the test
asserts that every keyword set met every n, every B, every (depth, spare), both schedules, every entry point and every layout.
12309 chunks; the file takes 12 to 17 s on the CPU where its thirteen sets in 9936 chunks took 8: the chunks grew by a quarter,
and a chunk of the new sets issues up to five more calls per batch (template, advance, two matches, ROI map), each with its
own address lookups -- nothing in the profile stands out, the time is spread over the same functions as before.  With the four
re-detection sets the chunk count stays (PER_CONTEXT did not have to rise: the rotation spreads the same contexts over more
sets) and the file takes 14.2 s where its twenty-seven sets took 11.4 s on the same machine: about one chunk in eight now
runs a re-detection set, the sets with the most calls per batch.

What turns these tests red, tried with pipeline.py edited by hand, one edit at a time (every keyword set the edit reaches
goes red; none of the eleven stays green):
 1. _ChunkResidual.with_frames takes its flow slots % (flow_slots - 1) -- residual, residual-gate, residual-texture,
    compensate-residual, compensate-residual-texture (once the ring wraps: the slot holds another pair, or a fitted field);
 2. its maps slice is js[0]:js[-1] -- the same five sets, every chunk: one map too few for the batch;
 3. the texture combine queued ahead of the residual call -- residual-texture, compensate-residual-texture: the combination
    meets an unwritten map;
 4. _chain(comp.behind, trk.behind) -- compensate-track-roi-match: the fit runs before the advance of its pairs (and the
    advance would meet a fitted field);
 5. _chunk_motion given the ROI maps -- compensate-track-roi-match: a weighted fit under a track;
 6. the records' match on f1 -- track-match, track-match-capture, track-roi-match, compensate-track-roi-match: frame j + 1
    where pair j needs frame j;
 7. the state's match on f0[-1] -- the same four: frame last where the state stands in frame last + 1;
 8. roi_weights queued ahead of track_match -- track-roi-match, compensate-track-roi-match: the map is made behind the
    advance, not behind the state's match;
 9. self.capture never cleared -- track-match-capture, track-roi-match, compensate-track-roi-match, from the second batch
    on: track_template a second time;
10. centres() with an item of 48 -- track3-home, track-match, track-roi-match (the sets with T > 1): the stride is not 48 * T;
11. with_frames handed the previous batch's f0 / f1 -- every frame-reading set (the seven residual / texture sets and the
    four match sets), from the second batch on: the slots hold the previous pairs' frames.
Six more, on the re-detection call of _ChunkTrack.behind, with the four re-detection sets (track-match-redetect,
track-roi-match-redetect, compensate-track-roi-match-redetect, track-match-redetect-dict); none stays green:
 a. the re-detection on f0[-1] -- all four, every chunk: frame last where the state stands in frame last + 1;
 b. its output at ls[0] -- all four, in every chunk with a batch of two pairs or more: not the batch's last record;
 c. its trigger the batch's match_out span instead of state_match -- all four, every chunk: not what the state's match of
    this batch wrote;
 d. the re-detection queued ahead of the state's match -- all four, every chunk: behind the records' match;
 e. its centres the batch's records -- all four, every chunk: not the state tensor;
 f. _ChunkTrack.with_frames handed the previous batch's f0 / f1 -- all four and the four match sets, from the second batch
    on (the records' match meets the wrong frames first)."""
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
        self.uploaded, self.zeroed = [], []     # tensors made by torch.from_numpy(...).to(device) and by torch.zeros

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

    class Host:
        """torch.from_numpy(array): all that is asked of it is .to(device)"""

        def __init__(self, array):
            self.array = array

        def to(self, device):
            dt = next(d for d in DTYPES.values() if d.typestr == self.array.dtype.str)
            arena.uploaded.append(FakeTensor(arena.take(self.array.nbytes), self.array.shape, dt))
            return arena.uploaded[-1]

    def zeros(*size, dtype=None, device=None):
        arena.zeroed.append(empty(*size, dtype=dtype, device=device))
        return arena.zeroed[-1]

    t.empty, t.zeros, t.from_numpy = empty, zeros, Host
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
    flows_out ((tensor, layout) or None), motion (tensor or None), item, axes, pov, thr, src (the source arrays of process_flows),
    frame_maps (None | dict(mode, texture, gate, params): weights="residual" | "texture"), track (None | dict(T, state, on_cut,
    roi, gate, match, capture, templates, p, track_out, match_out, redetect, redetect_params, redetect_out): center="track"; a
    tensor the caller did not give is None)."""

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
        # the maps a mode makes behind a batch, per pair: [] unwritten -> ["residual"] -> ["residual", "texture"], ["texture"], ["roi"]
        self.made = [[] for _ in range(n)]
        self.advanced, self.matched = [0] * n, [0] * n
        self.next_advance = self.templates = self.state_matches = self.redetects = 0
        self.redetected = [0] * n               # writes per record of redetect_out
        self.state_written = None               # the span the state's match of THIS batch wrote; the next advance clears it
        self.last = None                        # the latest call queued behind a batch

    # -- helpers
    def _frames(self, fslots, first, who, shift=0):
        """frame slot k still holds frame first + k + shift of the chunk"""
        for k, s in enumerate(fslots):
            assert 0 <= s < self.frame_slots, f"{who}: frame slot {s} out of range"
            assert self.frames.get(s) == first + k + shift, \
                f"{who}: frame slot {s} holds frame {self.frames.get(s)}, pair {first + k} needs frame {first + k + shift} there"

    def _map_index(self, out, count, who):
        """the pair whose map `out` -- a slice of the chunk's (n, H, W) tensor -- starts at; it holds `count` maps"""
        kind = self.want["maps"]
        assert isinstance(out, FakeTensor) and kind is not None and kind[0] == "pair", who
        assert out.shape == (count, H, W) and out.stride() == (kind[2], W, 1), f"{who}: {out.shape[0]} maps for {count} pairs"
        j, rest = divmod(out.data_ptr() - kind[1], kind[2])
        assert rest == 0 and 0 <= j and j + count <= self.want["n"], f"{who}: maps outside the chunk's tensor"
        return j

    def _final(self, first, count, who):
        """a reader of the maps a mode makes meets them complete: written once, and combined where the chunk combines"""
        w = self.want
        if w["frame_maps"] is None and not (w["track"] and w["track"]["roi"]):
            return
        final = (["roi"] if w["track"] else ["texture"] if w["frame_maps"]["mode"] == "texture" else
                 ["residual", "texture"] if w["frame_maps"]["texture"] else ["residual"])
        for p in range(first, first + count):
            assert self.made[p] == final, f"{who}: the map of pair {p} is {self.made[p] or 'unwritten'}, meant {final}"

    def _gate(self, gate, want, who):
        if want is None:
            assert gate is None, f"{who}: a gate nobody gave"
        else:
            assert isinstance(gate, _capi.DevWeights) and (gate.base, gate.item_stride) == (want.data_ptr(), 0), f"{who}: not the static gate"

    def _raw(self, slots, who):
        for s in slots:
            assert (self.slots[s].fits, self.slots[s].subtractions, self.slots[s].weighted) == (0, 0, 0), \
                f"{who}: the field of pair {self.slots[s].pair} is not raw"

    def _tracked(self, first, count, who, maps=False):
        """records (and ROI maps) of pairs a centre reader meets: advanced, corrected where the chunk matches, written once"""
        t = self.want["track"]
        for p in range(first, first + count):
            assert self.advanced[p] == 1, f"{who}: the record of pair {p} was advanced {self.advanced[p]} times"
            assert self.matched[p] == (1 if t["match"] else 0), f"{who}: the record of pair {p} was matched {self.matched[p]} times"
            if maps:
                assert self.made[p] == ["roi"], f"{who}: the ROI map of pair {p} is {self.made[p] or 'unwritten'}"

    def _track_records(self, centres, who):
        """(buffer, byte stride) about the chunk's track records: the pair the span starts at and the pairs it holds"""
        t = self.want["track"]
        assert isinstance(centres, tuple) and len(centres) == 2 and centres[1] == 48 * t["T"], f"{who}: a stride of {centres[1:]}, meant 48 * T = {48 * t['T']}"
        ptr, nbytes = _capi._device_span(centres[0])
        assert nbytes % (48 * t["T"]) == 0, who
        return self._where("track", ptr, 48 * t["T"], t["track_out"]), nbytes // (48 * t["T"])

    def _state(self, obj, who):
        t = self.want["track"]
        made = self.arena.uploaded
        want = t["state"] if t["state"] is not None else made[0] if len(made) == 1 else None
        assert want is not None and obj is want, f"{who}: not the chunk's state tensor"

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
        self.last = "motion_fit"
        if self.want["track"] is not None:     # the ROI maps say where the subject is, not what is reliable
            assert weights is None, "motion_fit: weighted under a track"
            self._tracked(first, len(slots), "motion_fit (behind the advance)")
        else:
            self._maps(weights, first, "motion_fit")
            self._final(first, len(slots), "motion_fit")
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
        self._final(first, len(slots), "pass1_weighted")
        self.last = "pass1_weighted"
        if self.want["track"] is not None:
            self._tracked(first, len(slots), "pass1_weighted", maps=True)
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

    # -- maps made from the batch's frame slots (pass1_pairs' with_frames hook)
    def residual_weights(self, fslot0, fslot1, flow_slots, out, params=None, gate=None, stream=None):
        self._stream(stream)
        fm = self.want["frame_maps"]
        assert fm is not None and fm["mode"] == "residual" and isinstance(params, _capi.ResidualParams)
        assert len(fslot0) == len(fslot1) == len(flow_slots)
        first = self._held(flow_slots, who="residual_weights")
        self._raw(flow_slots, "residual_weights")            # before the fit: the maps are those of the estimator's field
        assert self._map_index(out, len(flow_slots), "residual_weights") == first, "residual_weights: the maps of other pairs"
        self._frames(fslot0, first, "residual_weights (f0)")
        self._frames(fslot1, first, "residual_weights (f1)", shift=1)
        self._gate(gate, fm["gate"], "residual_weights")
        if fm["params"] is not None:
            assert {k: pytest.approx(v) for k, v in fm["params"].items()} == {k: params.as_dict()[k] for k in fm["params"]}
        for p in range(first, first + len(flow_slots)):
            assert self.made[p] == [], f"residual_weights: the map of pair {p} is already {self.made[p]}"
            self.made[p].append("residual")
        self.last = "residual_weights"

    def texture_weights(self, fslots, out, params=None, gate=None, stream=None):
        self._stream(stream)
        fm = self.want["frame_maps"]
        assert fm is not None and isinstance(params, _capi.TextureParams)
        first = self._map_index(out, len(fslots), "texture_weights")
        self._frames(fslots, first, "texture_weights")      # frame 0 of the pair the map belongs to
        if fm["mode"] == "residual":     # the combination: in place, behind the residual call
            assert fm["texture"], "texture_weights without texture="
            assert isinstance(gate, FakeTensor) and (gate.data_ptr(), gate.shape, gate.stride()) == (out.data_ptr(), out.shape, out.stride()), \
                "texture_weights: the combination is gate = out"
            before = ["residual"]
        else:
            self._gate(gate, fm["gate"], "texture_weights")
            before = []
        for p in range(first, first + len(fslots)):
            assert self.made[p] == before, f"texture_weights: the map of pair {p} is {self.made[p] or 'unwritten'}, meant {before or 'unwritten'}"
            self.made[p].append("texture")
        self.last = "texture_weights"

    # -- the track
    def track_template(self, fslot, centres, templates, p=None, tracks=None, stream=None):
        self._stream(stream)
        t = self.want["track"]
        assert t is not None and t["match"] and t["capture"], "track_template without capture"
        assert self.templates == 0, "track_template a second time"
        assert self.next_advance == 0 and self.last is None, "track_template behind an advance"
        self._frames([fslot], 0, "track_template")
        self._state(centres, "track_template")
        self._templates(templates, "track_template")
        assert (p, tracks) == (t["p"], t["T"])
        self.templates += 1

    def _templates(self, templates, who):
        t = self.want["track"]
        made = self.arena.zeroed
        want = t["templates"] if t["templates"] is not None else made[0] if len(made) == 1 else None
        assert want is not None and templates is want, f"{who}: not the chunk's templates"

    def track_advance(self, seq_slots, state, out, params=None, weights=None, stream=None):
        self._stream(stream)
        t = self.want["track"]
        assert t is not None and weights is None and isinstance(params, _capi.TrackParams)
        assert params.as_dict()["on_cut"] == t["on_cut"] and params.cut_threshold == np.float32(self.want["thr"])
        first = self._held(seq_slots, self.next_advance, who="track_advance")
        self._raw(seq_slots, "track_advance")               # rule Q5's cut is the raw whole-frame mean magnitude
        self._state(state, "track_advance")
        ptr, nbytes = _capi._device_span(out)
        assert self._where("track", ptr, 48 * t["T"], t["track_out"]) == first, "track_advance: its records are not at first * 48 * T"
        assert nbytes == len(seq_slots) * 48 * t["T"]
        assert self.templates == (1 if t["match"] and t["capture"] else 0), "track_advance: the template is captured before the first advance, or never"
        batches = -(-first // self.max_batch)
        assert self.redetects == (batches if t["redetect"] else 0), f"track_advance of batch {batches}: {self.redetects} re-detections so far"
        self.state_written = None
        for p in range(first, first + len(seq_slots)):
            self.advanced[p] += 1
        self.next_advance += len(seq_slots)
        self.last = ("track_advance", first, len(seq_slots))

    def track_match(self, fslots, templates, centres, out, params=None, tracks=1, write_back=True, stream=None):
        self._stream(stream)
        t = self.want["track"]
        assert t is not None and t["match"] and isinstance(params, _capi.MatchParams) and write_back is True
        assert (params.p, tracks) == (t["p"], t["T"])
        self._templates(templates, "track_match")
        assert isinstance(centres, tuple) and len(centres) == 2
        if isinstance(centres[0], FakeTensor) and self.arena.find(centres[0].data_ptr()) == self.arena.find(self._state_ptr()):
            # about the state: one item on the frame the state stands in, straight behind the records' match of the batch
            self._state(centres[0], "track_match (state)")
            assert centres[1] == 48 * t["T"] and len(fslots) == 1
            assert self.last is not None and self.last[0] == "records_match" and self.last[1] + self.last[2] == self.next_advance, \
                f"track_match (state): behind {self.last}, not behind the records' match of its batch"
            self._frames(fslots, self.next_advance, "track_match (state)")       # frame last + 1
            assert self.arena.find(span(out))[0] not in (self.buffers.get("track"), self.buffers.get("match"), self.buffers.get("redetect")), \
                "track_match (state): its records go to a buffer of their own"
            assert _capi._device_span(out)[1] == 48 * t["T"]
            self.state_matches += 1
            self.state_written = _capi._device_span(out)
            self.last = ("state_match",)
            return
        first, count = self._track_records(centres, "track_match")
        assert count == len(fslots), f"track_match: {len(fslots)} frame slots for the records of {count} pairs"
        assert self.last == ("track_advance", first, count), f"track_match of pairs {first}..{first + count - 1}: behind {self.last}, not behind their advance"
        self._frames(fslots, first, "track_match")          # the f0 slots: a record is the track's place in frame 0 of its pair
        ptr, nbytes = _capi._device_span(out)
        assert self._where("match", ptr, 48 * t["T"], t["match_out"]) == first and nbytes == count * 48 * t["T"]
        for p in range(first, first + count):
            assert (self.advanced[p], self.matched[p]) == (1, 0), f"track_match: pair {p} advanced {self.advanced[p]}, matched {self.matched[p]} times"
            self.matched[p] += 1
        self.last = ("records_match", first, count)

    def track_redetect(self, fslots, templates, centres, out, params=None, tracks=1, trigger=None, write_back=True, stream=None):
        self._stream(stream)
        t = self.want["track"]
        assert t is not None and t["match"] and t["redetect"], "track_redetect without track['match']['redetect']"
        assert isinstance(params, _capi.RedetectParams) and write_back is True and (params.p, tracks) == (t["p"], t["T"])
        got = params.as_dict()
        assert {k: got[k] for k in t["redetect_params"]} == t["redetect_params"], f"track_redetect: parameters {got}, meant {t['redetect_params']}"
        # one item, straight behind the state's match of the batch just advanced, once per batch
        assert len(fslots) == 1, f"track_redetect: {len(fslots)} items"
        assert self.last == ("state_match",), f"track_redetect: behind {self.last}, not behind the state's match of its batch"
        last = self.next_advance - 1
        self._frames(fslots, last + 1, "track_redetect")                   # the frame the state stands in
        assert isinstance(centres, tuple) and len(centres) == 2 and isinstance(centres[0], FakeTensor), "track_redetect: not the state tensor"
        self._state(centres[0], "track_redetect")
        assert centres[1] == 48 * t["T"]
        self._templates(templates, "track_redetect")
        assert self.templates == (1 if t["capture"] else 0)
        assert trigger is not None and self.state_written is not None and _capi._device_span(trigger) == self.state_written, \
            "track_redetect: the trigger is not what the state's match of this batch wrote"
        ptr, nbytes = _capi._device_span(out)
        at = self._where("redetect", ptr, 48 * t["T"], t["redetect_out"])
        assert at == last and nbytes == 48 * t["T"], f"track_redetect: {nbytes} bytes at record {at}, meant {48 * t['T']} at the batch's last pair {last}"
        assert self.arena.find(ptr)[0] not in (self.buffers.get("track"), self.buffers.get("match"), self.arena.find(self.state_written[0])[0])
        self.redetected[at] += 1
        assert self.redetected[at] == 1, f"track_redetect: record {at} written a second time"
        self.redetects += 1
        self.last = ("redetect",)

    def _state_ptr(self):
        t = self.want["track"]
        return (t["state"] if t["state"] is not None else self.arena.uploaded[0]).data_ptr()

    def roi_weights(self, n, centres, out, params=None, gate=None, stream=None):
        self._stream(stream)
        t = self.want["track"]
        assert t is not None and t["roi"] and isinstance(params, _capi.RoiParams)
        first, count = self._track_records(centres, "roi_weights")
        assert count == n and self._map_index(out, n, "roi_weights") == first, "roi_weights: the maps of other pairs"
        assert self.last == (("redetect",) if t["redetect"] else ("state_match",) if t["match"] else ("track_advance", first, n)), \
            f"roi_weights of pairs {first}..{first + n - 1}: behind {self.last}"
        self._tracked(first, n, "roi_weights")
        self._gate(gate, t["gate"], "roi_weights")
        for p in range(first, first + n):
            assert self.made[p] == [], f"roi_weights: the map of pair {p} is already written"
            self.made[p].append("roi")
        self.last = "roi_weights"

    # -- the window calls
    def _window(self, form, seq, first, count, out, radius, thr, pov, stream, weights=None, centres=None):
        self._stream(stream)
        w, n = self.want, self.want["n"]
        want_form = ("weighted_centres" if w["track"] and w["track"]["roi"] else "centres" if w["variance"] or w["track"] else
                     "weighted" if w["maps"] is not None else "axes" if w["axes"] else "plain")
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
        self.last = "window"
        if form in ("weighted", "weighted_centres"):
            self._maps(weights, j0, "radial_window_axes_" + form)
            self._final(j0, count, "radial_window_axes_" + form)
        if w["track"] is not None:      # about the track buffer: base lo * 48 * T, stride 48 * T, every pair of the seq complete
            got = self._track_records(centres, "radial_window_axes_" + form)
            assert got == (lo, len(seq)), f"radial_window_axes_{form}: centres of pairs {got[0]}.. for a seq of pairs {lo}.."
            self._tracked(lo, len(seq), "radial_window_axes_" + form, maps=bool(w["track"]["roi"]))
        elif form == "centres":
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

    def radial_window_axes_weighted_centres(self, seq, first, n, weights, centres, out, radius=6, thr=7.0, pov=False, stream=None):
        return self._window("weighted_centres", seq, first, n, out, radius, thr, pov, stream, weights=weights, centres=centres)

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
        t, fm = w["track"], w["frame_maps"]
        assert self.advanced == (ones if t else [0] * n), f"pairs advanced {self.advanced}"
        assert self.matched == (ones if t and t["match"] else [0] * n), f"pairs matched {self.matched}"
        assert self.next_advance == (n if t else 0)
        assert self.state_matches == (-(-n // self.max_batch) if t and t["match"] else 0), f"{self.state_matches} state matches"
        assert self.templates == (1 if t and t["match"] and t["capture"] and n else 0), f"{self.templates} template captures"
        batches = -(-n // self.max_batch)
        assert self.redetects == (batches if t and t["redetect"] else 0), f"{self.redetects} re-detections"
        assert self.redetected == [int(bool(t and t["redetect"]) and (p + 1 == n or (p + 1) % self.max_batch == 0)) for p in range(n)]
        if t or fm:
            self._final(0, n, "the chunk's end")
        else:
            assert self.made == [[] for _ in range(n)]
        if t and n:
            for role, given in (("track", t["track_out"]), ("match", t["match_out"] if t["match"] else None),
                                ("redetect", t["redetect_out"] if t["redetect"] else None)):
                if given is not None:
                    assert self.buffers[role] == self.arena.find(given.data_ptr())[0], f"{role}_out is not the caller's buffer"
            assert ("match" in self.buffers) == bool(t["match"]) and ("redetect" in self.buffers) == bool(t["redetect"])
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


def frame_maps(arena, n, mode="residual", texture=False, gate=False):
    """weights="residual" | "texture"; gate=True: a static gate, the caller's own weights_out and explicit parameters"""
    kw, want = {"weights": mode}, {"frame_maps": {"mode": mode, "texture": texture, "gate": None, "params": None}}
    if texture:
        kw["texture"] = True if not gate else {"radius": 3, "tau": 40.0}
    if gate:
        kw["weights_gate"] = want["frame_maps"]["gate"] = tensor(arena, (H, W))
        kw["weights_out"] = tensor(arena, (n, H, W))
        if mode == "residual":
            kw["residual"] = want["frame_maps"]["params"] = {"alpha": 0.75, "beta": 3.0, "soft": 0}
    return kw, want


def track(arena, n, T=1, state=False, on_cut="hold", roi=False, match=None, out=False, redetect=None):
    """center="track": T tracks from `start`, or from a state tensor of the caller's; roi: maps with a static gate into the
    caller's weights_out; match: None, "templates" (the caller's, capture off) or "capture"; out: the caller's track_out
    (and match_out, redetect_out); redetect: None, True or the dict form of track["match"]["redetect"]"""
    tr = {"on_cut": on_cut, "radius": 5}
    want = {"T": T, "state": None, "on_cut": on_cut, "roi": roi, "gate": None, "match": match is not None, "capture": False,
            "templates": None, "p": None, "track_out": None, "match_out": None, "redetect": redetect is not None,
            "redetect_params": None, "redetect_out": None}
    if state:
        tr["state"] = want["state"] = tensor(arena, (T * _capi.TRACK_STATE_DTYPE.itemsize,))
    else:
        tr["start"] = [(20.0 + 7 * t, 30.0 - 5 * t) for t in range(T)] if T > 1 else (20.0, 30.0)
    kw = {"center": "track", "track": tr}
    if roi:
        tr["roi"] = (12.0, 9.0)
        kw["weights_gate"] = want["gate"] = tensor(arena, (H, W))
        kw["weights_out"] = tensor(arena, (n, H, W))
    if match is not None:
        tr["match"] = {"p": 6, "s": 4}
        want["p"], want["capture"] = 6, match == "capture"
        if match == "templates":
            tr["match"]["templates"] = want["templates"] = tensor(arena, (T, 13, 13))
        if redetect is not None:     # p, mode and thresholds are the match's; exclude defaults to p, reach to the whole frame, the mask to POOR
            tr["match"]["redetect"] = redetect
            r = {} if redetect is True else redetect
            want["redetect_params"] = {"p": 6, "mode": "zssd", "exclude": r.get("exclude", 6), "reach": r.get("reach", 0),
                                       "trigger_mask": r.get("mask", 2), "max_mse": 400.0, "ratio": 0.8}
    if out:
        kw["track_out"] = want["track_out"] = tensor(arena, (max(n, 1) * T * 48 + 16,))
        if match is not None:
            kw["match_out"] = want["match_out"] = tensor(arena, (max(n, 1) * T * 48,))
        if redetect is not None:
            kw["redetect_out"] = want["redetect_out"] = tensor(arena, (max(n, 1) * T * 48 + 48,))
    return kw, {"track": want}


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
    "residual": frame_maps,
    "residual-gate": lambda arena, n: frame_maps(arena, n, gate=True),
    "texture": lambda arena, n: frame_maps(arena, n, "texture"),
    "residual-texture": lambda arena, n: frame_maps(arena, n, texture=True),
    "compensate-residual": both(lambda arena, n: compensate(arena, n, "similarity"), frame_maps),
    "compensate-texture": both(lambda arena, n: compensate(arena, n, "rigid", out=False), lambda arena, n: frame_maps(arena, n, "texture", gate=True)),
    "compensate-residual-texture": both(compensate, lambda arena, n: frame_maps(arena, n, texture=True, gate=True)),
    "track": track,
    "track3-home": lambda arena, n: track(arena, n, T=3, state=True, on_cut="home", out=True),
    "track-roi": lambda arena, n: track(arena, n, roi=True),
    "track-match": lambda arena, n: track(arena, n, T=2, match="templates", out=True),
    "track-match-capture": lambda arena, n: track(arena, n, match="capture"),
    "track-roi-match": lambda arena, n: track(arena, n, T=2, state=True, roi=True, match="capture", out=True),
    "compensate-track-roi-match": both(lambda arena, n: compensate(arena, n, "affine"), lambda arena, n: track(arena, n, roi=True, match="capture")),
    "track-match-redetect": lambda arena, n: track(arena, n, T=2, match="templates", out=True, redetect=True),
    "track-roi-match-redetect": lambda arena, n: track(arena, n, T=2, state=True, roi=True, match="capture", redetect=True),
    "compensate-track-roi-match-redetect": both(lambda arena, n: compensate(arena, n, "affine"),
                                                lambda arena, n: track(arena, n, roi=True, match="capture", out=True, redetect=True)),
    "track-match-redetect-dict": lambda arena, n: track(arena, n, T=3, state=True, match="capture", out=True,
                                                        redetect={"reach": 20, "exclude": 4, "mask": 6}),
}
FRAME_READERS = tuple(k for k in KEYWORDS if "residual" in k or "texture" in k or "match" in k)      # process_chunk only
ENTRIES = ("chunk", "flows", "segments")
PER_CONTEXT = 5                                 # keyword sets every (n, B, depth, spare) context runs
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
        forced = any(k in want for k in ("maps", "variance", "cons", "frame_maps", "track"))      # these run the device schedule whatever post_out says
        want = {"n": n, "comp": False, "maps": None, "variance": False, "grid": None, "cons": None, "flows_out": None, "motion": None,
                "axes": False, "post": None, "src": (), "pov": pov, "thr": thr, "frame_maps": None, "track": None, **want}
        want["device"] = device or forced
        want["axes"] = want["axes"] or forced
        want["item"] = (_capi.PASS2_AXES_DTYPE if want["axes"] else _capi.PASS2_DTYPE).itemsize
        if device:
            kw["post_out"] = True
            if turn % 2:
                kw["post_out"] = want["post"] = tensor(arena, (max(n, 1) * want["item"] + 16,))
        if want["cons"] is not None or want["frame_maps"] is not None or (want["track"] is not None and want["track"]["roi"]):
            own = kw.get("weights_out")             # the chunk's maps: the caller's tensor, or one the schedule makes
            want["maps"] = ("pair", own.data_ptr(), H * W) if own is not None else ("pair-unknown",)
            if own is None:
                real = sys.modules["torch"].empty

                def empty(*size, dtype=None, device=None):
                    t = real(*size, dtype=dtype, device=device)
                    if t.shape == (max(n, 0), H, W):
                        want["maps"] = ("pair", t.data_ptr(), H * W)
                    return t
                sys.modules["torch"].empty = empty
        if entry == "chunk":
            if layout is not None:
                t = tensor(arena, (n, H, W, 2) if layout == "nhwc" else (n, 2, H, W), "float32")
                kw["flows_out"], want["flows_out"] = t, (t, layout)
            ctx.begin(want)
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
    if name in FRAME_READERS:
        return entry == "chunk"                     # process_flows has no frames
    if "pair-maps" in name:
        return n >= 1                               # (0, H, W) is no tensor of maps
    return True


def test_every_schedule_keeps_every_slot_live_for_its_readers():
    names = list(KEYWORDS)
    seen = {k: set() for k in ("n", "B", "ctx", "device", "entry", "layout", "flavour")}
    chunks = 0
    for c, (n, B, depth, spare) in enumerate(itertools.product(NS, BS, DEPTHS, SPARE)):
        for i in range(PER_CONTEXT):
            t = c * PER_CONTEXT + i
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
        assert {v for k, v in seen["entry"] if k == name} == ({"chunk"} if cons or name in FRAME_READERS else set(ENTRIES)), name
        assert {v for k, v in seen["layout"] if k == name} == set(LAYOUTS), name
        assert {v for k, v in seen["flavour"] if k == name} == set(FLAVOURS), name
    assert chunks > 12000


@pytest.mark.parametrize("entry", ENTRIES)
def test_a_chunk_without_pairs_under_a_track_with_roi(entry):
    """the ROI maps are the schedule's own (0, H, W) tensor: process_flows once looked at it and refused the chunk, where
    process_chunk returned the empty result (the sweep above meets n = 0 under every set, but not under every entry point)"""
    for name in ("track", "track-roi"):
        run_chunk(0, 3, 1, 0, True, entry, name, None, "tuned")


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
