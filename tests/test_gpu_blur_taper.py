"""k_blur_solve with a tapered launch plan ("blur_taper_pairs": the pairs dealt last walk shorter strips, ffl_blur_plan): a
speed option, so flows, pass-1 records and pass-2 scalars must be the bits of the same context with taper off, and the
oracle's.  Batches of 1, 2 and 3 pairs with one pair per taper segment run without a bulk, with one taper and with all
three segments; the strip lengths cover 1 tile (all segments alike), 3 (2 + 1), 8 (4 + 2) and 17 (9 + 5) against heights
of 2 to 35 tile rows.

What this file can and cannot see: a workgroup that walks too FEW rows leaves tiles unwritten and fails here (the tapered
run writes flow slots of its own, and a batch of other pairs first overwrites them and the lane's level buffers, so nothing
stale can pass for a result).  A workgroup that walks too MANY rows -- the last segment taking the bulk's strip length --
recomputes tiles a neighbour also writes, with the same bits: no result changes and no GPU test can notice.  That mapping
is single-sourced (ffl_blur_block) and held exactly, strip by strip, by tests/test_blur_plan_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as orc
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

SIZES = [(250, 131), (96, 80), (64, 256), (80, 560), (17, 19)]
KNOBS = {"blur_taper_pairs": 0, "blur_taper": 1, "blur_rows": 0, "fuse_first": 10000}   # the defaults, restored in finally


def run(ctx, nB, first_slot=0, reverse=False):
    """nB pairs of a stream (reverse: each pair backwards, another result) through the flow, pass 1 and pass 2, into flow
    slots first_slot .. -> (flows, records, scalars)"""
    slots = list(range(first_slot, first_slot + nB))
    f0, f1 = list(range(nB)), list(range(1, nB + 1))
    ctx.flow_pairs(*((f1, f0) if reverse else (f0, f1)), slots)
    recs = ctx.pass1_results(slots, 7.0)
    centers = pipeline.smooth_centers([(r[0], r[1]) for r in recs])
    dots = ctx.radial(slots, centers, [r[4] for r in recs], False)
    return [ctx.download_flow(j) for j in slots], [tuple(r) for r in recs], dots


@pytest.mark.parametrize("w,h", SIZES)
def test_tapered_launches_change_no_bit(w, h):
    fr = sine_translate_frames(4, w, h, seed=w + h, amp=(2.0, 3.0), period=5, zoom=0.02)
    want = orc.farneback(fr[1], fr[2])            # pair 1: the last pair of B = 2, inside B = 3
    _capi.set_option("lanes", 1)                  # one lane: the scrub batch dirties the buffers the tapered run uses
    try:
        ctx = _capi.Context(w, h, max_batch=3, frame_slots=5, flow_slots=6)
    finally:
        _capi.set_option("lanes", 2)
    with ctx:
        ctx.upload_frames(0, list(fr))
        try:
            for nB in (1, 2, 3):
                for rows in (1, 3, 8, 17):
                    for fuse in (0, 1):
                        ctx.set_option("blur_rows", rows)
                        ctx.set_option("fuse_first", fuse)
                        ctx.set_option("blur_taper_pairs", 0)
                        ctx.set_option("blur_taper", 0)
                        off = run(ctx, nB)
                        scrub = run(ctx, nB, 3, reverse=True)
                        ctx.set_option("blur_taper_pairs", 1)
                        on = run(ctx, nB, 3)
                        case = (nB, rows, fuse)
                        assert not np.array_equal(scrub[0][0], off[0][0]), case
                        assert all(np.array_equal(a, b) for a, b in zip(on[0], off[0])), case
                        assert on[1] == off[1] and on[2] == off[2], case
                        if case == (2, 8, 1):
                            assert np.array_equal(on[0][1], want)
            assert ctx.graph_stats()["capture_failures"] == 0
        finally:
            for k, v in KNOBS.items():
                ctx.set_option(k, v)


def test_tapered_graph_replay_two_lanes():
    """64 x 64, B = 4 on two lanes: each lane captures the tapered launches once and replays them; every run gives the
    flows of the plain launches.  The last two visits leave the taper to the automatic rule (one pair per segment here)."""
    w, h, B = 64, 64, 4
    fr = sine_translate_frames(B + 1, w, h, seed=7, amp=(2.0, 1.0), period=5)
    try:
        _capi.set_option("lanes", 2)
        _capi.set_option("blur_rows", 4)          # 4 tile rows: strips of 4, 2 and 1 tiles
        _capi.set_option("blur_taper", 0)
        with _capi.Context(w, h, max_batch=B, frame_slots=B + 2, flow_slots=3 * B) as ctx:   # slots 0 .. B-1 keep the plain flows
            ctx.upload_frames(0, list(fr))
            f0, f1 = list(range(B)), list(range(1, B + 1))
            ctx.flow_pairs(f0, f1, list(range(B)))
            plain = [ctx.download_flow(j) for j in range(B)]
            recs = [tuple(r) for r in ctx.pass1_results(list(range(B)), 7.0)]
            assert np.array_equal(plain[B - 1], orc.farneback(fr[B - 1], fr[B]))
            ctx.set_option("blur_taper_pairs", 1)
            before = ctx.graph_stats()
            for visit in range(6):                # lanes 0, 1 capture, then both replay
                if visit == 4:
                    assert _capi.blur_plan(1, 4, B, 1024, blur_rows=4, blur_taper=1, blocks=False)[0] == [(0, 0, 2, 4, 1), (16, 2, 1, 2, 2), (24, 3, 1, 1, 4)]
                    ctx.set_option("blur_taper_pairs", 0)
                    ctx.set_option("blur_taper", 1)
                slots = [(1 + visit % 2) * B + j for j in range(B)]
                ctx.flow_pairs(f0, f1, slots)
                assert [tuple(r) for r in ctx.pass1_results(slots, 7.0)] == recs, visit
                assert all(np.array_equal(ctx.download_flow(s), p) for s, p in zip(slots, plain)), visit
            after = ctx.graph_stats()
            assert after["capture_failures"] == 0 and after["replayed"] - before["replayed"] >= 2, (before, after)
    finally:
        _capi.set_option("lanes", 2)
        _capi.set_option("blur_rows", 0)
        _capi.set_option("blur_taper", 1)
        _capi.set_option("blur_taper_pairs", 0)
