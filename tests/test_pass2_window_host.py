"""Host side of the device pass 2, no GPU: the record layout of ffl_pass2_record as numpy sees it,
and pipeline.window_calls -- the schedule of Context.radial_window calls a streaming chunk issues -- against the rule it
restates (_ChunkPost._finalize) and against smooth_centers."""
import os
import re

import numpy as np
import pytest

from funscript_flow_amd import _capi, pipeline

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_PAIRS = [1, 2, 6, 7, 13, 40, 300]
BATCHES = [1, 5, 16]
RADII = [0, 1, 6]


def test_record_dtype_matches_header():
    dt = _capi.PASS2_DTYPE
    assert dt.itemsize == 48
    text = open(os.path.join(ROOT, "include", "ffl.h")).read()
    body = re.search(r"typedef struct ffl_pass2_record \{(.*?)\} ffl_pass2_record;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"double": 8, "float": 4, "int32_t": 4}
    kind = {"double": "<f8", "float": "<f4", "int32_t": "<i4"}
    off, seen = 0, []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = decl.split(None, 1)
        for name in (n.strip() for n in names.split(",")):
            off = -(-off // size[ctype]) * size[ctype]       # natural alignment, as the C compiler lays it out
            assert dt.fields[name] == (np.dtype(kind[ctype]), off), name
            seen.append(name)
            off += size[ctype]
    assert off == 48 and tuple(seen) == dt.names
    assert int(re.search(r"#define FFL_MAX_RADIUS (\d+)", text).group(1)) == _capi.FFL_MAX_RADIUS
    assert "ffl_radial_window" in _capi.EXPORTS


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", N_PAIRS)
def test_window_calls(n, B, radius):
    calls = pipeline.window_calls(n, B, radius)
    issued = np.zeros(n, int)
    pos = np.random.default_rng(n * 100 + B * 10 + radius).integers(0, 300, (n, 2))
    want = pipeline.smooth_centers(pos, radius)
    last_batch = -1
    for lo, hi, first, count, after in calls:
        assert 0 <= lo < hi <= n and 1 <= count <= B and first >= 0 and first + count <= hi - lo
        assert hi - lo <= B + 2 * radius
        assert after >= last_batch                                   # issue order follows the batches
        last_batch = after
        # nothing of the call's seq is later than the batch it is issued after ...
        assert hi <= min((after + 1) * B, n)
        for j in range(lo + first, lo + first + count):
            issued[j] += 1
            w0, w1 = max(0, j - radius), min(n, j + radius + 1)    # the pair's window, clipped by the chunk alone
            assert lo <= w0 and w1 <= hi                             # ... and the whole of it lies in seq
            # ... and the call is not issued before the batch that completes the window
            assert after >= (w1 - 1) // B
            # the window as ffl_radial_window clips it at the ends of seq is the chunk's window
            k = j - lo
            s0, s1 = max(0, k - radius), min(hi - lo - 1, k + radius)
            assert (lo + s0, lo + s1 + 1) == (w0, w1)
            got = pos[lo + s0:lo + s1 + 1].sum(axis=0) / float(s1 - s0 + 1)
            assert got.tobytes() == want[j].tobytes()
    assert (issued == 1).all()


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("n", N_PAIRS)
def test_window_calls_follow_the_host_schedule(n, B):
    """the calls are the pass-2 calls _ChunkPost issues: same pairs, same moments"""
    log = []

    class Ctx:
        flow_slots = 10 ** 6

        def radial(self, slots, cs, cuts, pov):
            log.append((slots[0], len(slots), batch[0]))
            return [0.0] * len(slots)

    batch = [0]
    post = pipeline._ChunkPost(Ctx(), n, B, False)
    for k, j0 in enumerate(range(0, n, B)):
        batch[0] = k
        js = list(range(j0, min(j0 + B, n)))
        post.add(js, [(1, 2, 0.0, 0.0, False)] * len(js))
    post.finish()
    assert log == [(lo + first, count, after) for lo, hi, first, count, after in pipeline.window_calls(n, B)]


# ---- the release schedule of process_chunk(post_out=) over a prefetch ring, against stand-ins -----------------------------
class RingCtx:
    """Stands in for the device under the device pass 2.  An upload only REMEMBERS the host array; its pixels are read ("the
    H2D transfer runs") at the latest moment the real one may still be reading page-locked memory: when something on the
    host has waited for the batch -- an event recorded behind a window call whose seq holds one of the batch's slots, or
    sync() -- or, failing that, after the whole run.  A ring slot recycled before that shows up as a wrong pair."""

    def __init__(self, max_batch, frame_slots, flow_slots):
        self.max_batch, self.frame_slots, self.flow_slots, self.device = max_batch, frame_slots, flow_slots, 0
        self.slot_upload, self.batches, self.slot_batch, self.calls, self.syncs = {}, [], {}, [], 0

    def pinned_frames(self, n, channels=1, size=None):
        return np.zeros((n, size[1], size[0], 3), np.uint8)

    def upload_frames(self, first, frames):
        for k, f in enumerate(frames):
            self.slot_upload[first + k] = {"host": f, "device": None}

    def flow_pairs(self, f0, f1, slots, pov):
        self.batches.append({"ops": [(self.slot_upload[a], self.slot_upload[b]) for a, b in zip(f0, f1)], "done": False})
        for s in slots:
            self.slot_batch[s] = len(self.batches) - 1

    def radial_window(self, seq, first, n, out, radius, thr, pov, stream):
        assert len(set(seq)) == len(seq) and stream == "side"      # the engine's own stream, never the caller's
        self.calls.append({self.slot_batch[s] for s in seq})      # the batches this call waits for on the device
        return out

    def complete(self, k):
        b = self.batches[k]
        if not b["done"]:
            b["done"] = True
            for up in (u for pair in b["ops"] for u in pair):
                if up["device"] is None:
                    up["device"] = int(up["host"][0, 0, 0]) | (int(up["host"][0, 0, 1]) << 8)

    def sync(self):
        self.syncs += 1
        for k in range(len(self.batches)):
            self.complete(k)

    def pass1_results(self, slots, thr):
        raise AssertionError("the device pass 2 never collects records")

    def pairs_seen(self):
        return [(a["device"], b["device"]) for bt in self.batches for a, b in bt["ops"]]


class RingEvent:
    """an event behind every window call issued so far; it is complete only once somebody waits for it"""

    def __init__(self, ctx, stream):
        assert stream == "side"                                    # recorded behind the window calls, on their stream
        self.ctx, self.n_calls = ctx, len(ctx.calls)

    def query(self):
        return False

    def synchronize(self):
        for waited in self.ctx.calls[:self.n_calls]:
            for k in waited:
                self.ctx.complete(k)


class HostSpan:
    __cuda_array_interface__ = {"version": 2, "data": (4096, False), "shape": (1 << 20,), "strides": None, "typestr": "|u1"}


@pytest.mark.parametrize("B,depth", [(4, 1), (4, 2), (8, 2), (16, 2)])
def test_ring_frames_are_released_only_behind_their_batches(monkeypatch, B, depth):
    """B = 4 is shorter than the window's radius (the first batch of a chunk has no window call behind it: the sync
    fallback); the ring holds 3B + 1 frames, fewer than a chunk, so slots are recycled inside every chunk.  Every batch
    must have seen its own frames, whenever its transfers ran."""
    import test_prefetch_host as tp
    from funscript_flow_amd import postchain, prefetch
    monkeypatch.setattr(pipeline, "_stream_event", RingEvent)
    monkeypatch.setattr(pipeline, "_side_stream", lambda ctx: "side")
    monkeypatch.setattr(pipeline._DevicePost, "finish", lambda self: None)      # joins two torch streams: no device here
    n_frames, bracket = 120, 50
    cap = tp.FakeCapture(n_frames, 30.0)
    _, _, indices = postchain.sampling(30.0, n_frames)
    ctx = RingCtx(B, pipeline.min_frame_slots(B, depth), pipeline.min_flow_slots(B, depth))
    ring = prefetch.PrefetchRing(ctx, cap, indices, bracket, 3 * B + 1)
    eng = pipeline.PairEngine(ctx, depth=depth)
    try:
        for view, fidx in ring.chunks():
            out = HostSpan()
            assert eng.process_chunk(view, post_out=out) is out
            # nothing of this chunk may still be in flight: the next chunk's decoding overwrites the ring
            assert all(b["done"] for b in ctx.batches), "process_chunk returned before the chunk's last transfer"
    finally:
        ring.close()
    for k in range(len(ctx.batches)):      # whatever was never waited for runs now, after the ring has been overwritten
        ctx.complete(k)
    want = [(i, i + 1) for c in range(0, n_frames, bracket) for i in range(c, min(c + bracket, n_frames) - 1)]
    assert ctx.pairs_seen() == want
    assert ring.max_outstanding <= 3 * B + 1 and cap.reads == n_frames
    assert (ctx.syncs > 0) == (B <= pipeline.SMOOTH_RADIUS)      # the fallback only where a batch has no call behind it
