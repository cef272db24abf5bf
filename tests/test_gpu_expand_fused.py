"""Level 0 blurred inside PolyExp (option fuse_l0_blur, default 1): in the merged frame expansion PolyExp's tile loader forms
level 0's image -- the 3-tap REFLECT_101 blur of the gray frame -- at the positions its own REPLICATE clamp picks, and the
level-0 image plane is neither written nor read.  Everything is compared bit for bit: the stage dumps against the oracle's
(oracle.farneback_dbg), and the option on against the option off.

The library's domain starts at 16x16 (ffl_create refuses smaller frames), so the shapes 13x11 and 8x8 can reach no kernel:
for them the tests assert the refusal, and 16x16 and 19x17 (the smallest legal frame, and an odd one next to it -- both
narrower than one tile, 19x17 unaligned with rows that start on any byte) probe what they were meant to."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import oracle as orc
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

# (w, h): what the shape probes in the 64x16-tile loader (halo 5 + 1 for the blur's taps)
SHAPES = [(64, 16),    # exactly one tile: every halo position is clamped
          (72, 24),    # partial tiles; the blur's reflection and PolyExp's clamp meet in one tile
          (200, 40),   # interior tile columns with no border
          (13, 11),    # below the domain (see the module docstring)
          (66, 18),    # unaligned: byte-wise staging
          (8, 8),      # below the domain
          (16, 16),    # the smallest legal frame: narrower than the tile, as high as it
          (19, 17)]    # odd and unaligned, one row and three columns past a tile boundary of neither axis
CONTENTS = ["random", "checker", "constant255", "corners"]


@functools.lru_cache(maxsize=None)
def frames(w, h, content):
    """three frames of a stream (pairs 0-1 and 1-2 share frame 1)"""
    rng = np.random.default_rng(1000 * w + h)
    y, x = np.mgrid[0:h, 0:w]
    if content == "random":
        fr = [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(3)]
    elif content == "checker":
        c = (((x + y) & 1) * 255).astype(np.uint8)
        fr = [c, np.roll(c, 1, axis=1), c]
    elif content == "constant255":
        fr = [np.full((h, w), 255, np.uint8)] * 3
    else:
        a = np.zeros((h, w), np.uint8)
        a[0, 0] = a[0, w - 1] = a[h - 1, 0] = a[h - 1, w - 1] = 255
        b = a.copy()
        b[1, 1] = b[1, w - 2] = b[h - 2, 1] = b[h - 2, w - 2] = 255
        fr = [a, b, a]
    return tuple(np.ascontiguousarray(f) for f in fr)


@functools.lru_cache(maxsize=None)
def oracle_dbg(w, h, content, level):
    fr = frames(w, h, content)
    return orc.farneback_dbg(fr[0], fr[1], level, 0)


@functools.lru_cache(maxsize=None)
def oracle_flows(w, h, content):
    fr = frames(w, h, content)
    return tuple(orc.farneback(fr[j], fr[j + 1]).tobytes() for j in range(2))


def same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def refused(w, h):
    if w >= 16 and h >= 16:
        return False
    with pytest.raises(_capi.FFLError):
        _capi.Context(w, h, max_batch=1)
    return True


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_level0_expansion_one_pair(w, h, content):
    """B = 1, through the stage capture: level-0 R0 / R1 with the option on equal the oracle's and those with the option
    off; the capture still returns level 0's I (the pyramid keeps that job while a capture runs), equal to the oracle's."""
    if refused(w, h):
        return
    fr = frames(w, h, content)
    o = oracle_dbg(w, h, content, 0)
    with _capi.Context(w, h, max_batch=1) as ctx:
        assert ctx.get_option("fuse_l0_blur") == 1 and ctx.get_option("merge_expand") == 1
        ctx.upload_frame(0, fr[0])
        ctx.upload_frame(1, fr[1])
        on = ctx.debug_pair(0, 1, 0, 0)
        ctx.set_option("fuse_l0_blur", 0)
        off = ctx.debug_pair(0, 1, 0, 0)
    for key in ("R0", "R1"):
        assert same(on[key], o[key]), f"{key}: fused PolyExp differs from the oracle, max abs {np.abs(on[key] - o[key]).max()}"
        assert same(on[key], off[key]), f"{key}: option on differs from option off"
    for key in ("I0", "I1"):
        assert same(on[key], o[key]) and same(off[key], o[key]), key
    assert same(on["out"], o["out"]) and same(off["out"], o["out"])


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("w,h", SHAPES)
def test_level0_expansion_stream_of_two_pairs(w, h, content):
    """B = 2 in stream form (three unique frames, the middle one shared) on a fresh context, whose level-0 image plane was
    never written: both flow fields equal the oracle's, and those with the option off."""
    if refused(w, h):
        return
    fr = frames(w, h, content)
    want = oracle_flows(w, h, content)
    with _capi.Context(w, h, max_batch=2) as ctx:
        for i in range(3):
            ctx.upload_frame(i, fr[i])
        ctx.flow_pairs([0, 1], [1, 2], [0, 1])
        on = [ctx.download_flow(j).tobytes() for j in range(2)]
        ctx.set_option("fuse_l0_blur", 0)
        ctx.flow_pairs([0, 1], [1, 2], [0, 1])
        off = [ctx.download_flow(j).tobytes() for j in range(2)]
        assert ctx.graph_stats()["capture_failures"] == 0
    for j in range(2):
        assert on[j] == want[j], f"pair {j}: fused expansion differs from the oracle"
        assert on[j] == off[j], f"pair {j}: option on differs from option off"


# 128x64 and 136x72 have one coarser level (x1/2); the x1/4 and x1/8 levels exist from 256 pixels a side on, so 256x256 (2 x 4
# whole tiles of the one-pass coarse kernel) and 288x264 (partial tiles in both axes, every level's width a multiple of 4 so
# that the merged launches run) carry levels 2 and 3
@pytest.mark.parametrize("w,h", [(128, 64), (136, 72), (256, 256), (288, 264)])
def test_coarser_level_images_and_expansions(w, h):
    """levels 1..3 with the option on: I and R of both frames equal the oracle's"""
    fr = frames(w, h, "random")
    with _capi.Context(w, h, max_batch=1) as ctx:
        ctx.upload_frame(0, fr[0])
        ctx.upload_frame(1, fr[1])
        assert ctx.num_levels() == orc.num_levels(w, h) >= 1
        for level in range(1, ctx.num_levels() + 1):
            g = ctx.debug_pair(0, 1, level, 0)
            o = oracle_dbg(w, h, "random", level)
            for key in ("I0", "I1", "R0", "R1"):
                assert same(g[key], o[key]), f"{key} differs at level {level}"


def test_whole_results_do_not_depend_on_the_form():
    """256x144, B = 3: records, scalars and every flow field by their bytes -- fuse_l0_blur on / off, graph replay / eager
    launches"""
    w, h, B = 256, 144, 3
    fr = sine_translate_frames(B + 1, w, h, seed=11, amp=(3.0, 2.0), period=6)

    def run(**opts):
        with _capi.Context(w, h, max_batch=B, frame_slots=B + 2, flow_slots=B) as ctx:
            for k, v in opts.items():
                ctx.set_option(k, v)
            ctx.upload_frames(0, list(fr))
            slots = list(range(B))
            for _ in range(2):   # the second call replays the graph the first one captured
                ctx.flow_pairs(slots, list(range(1, B + 1)), slots)
            recs = ctx.pass1_results(slots, 7.0)
            dots = ctx.radial(slots, [(w / 2.0, h / 2.0)] * B, [False] * B, False)
            flows = [ctx.download_flow(j).tobytes() for j in slots]
            gs = ctx.graph_stats()
        assert gs["capture_failures"] == 0 and (gs["replayed"] > 0) == bool(opts.get("graph", 1)), gs
        return ([np.asarray(r, np.float64).tobytes() for r in recs], np.asarray(dots, np.float64).tobytes(), flows)

    ref = run()
    assert ref[2][0] == orc.farneback(fr[0], fr[1]).tobytes()
    for opts in ({"fuse_l0_blur": 0}, {"graph": 0}, {"graph": 0, "fuse_l0_blur": 0}):
        assert run(**opts) == ref, opts
