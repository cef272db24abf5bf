"""Hostile frame content on the launch shapes the library ships: 1920x1080 and 3840x2160 at B = 32 with library-default
options (folded first launch on levels 0-1, automatic strip length, graph replay, one and two lanes), and the same content
through the general Farneback kernels and DIS.  Uniform noise, a 1-px checkerboard and its roll, constants, a 40-px jump and
a rotation-plus-zoom about an off-centre point (warps leave the image along two borders, every lane of a wave has its own
sub-pixel offset), with the cross-kind pairs a cyclic stream brings.  Every flow is compared bit for bit with a live run
of the CPU oracle / restatement of its pair; the records and radial values with the exact references of tests/post_ref.py."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dis_ref
import fb_general_ref
import oracle as orc
import post_ref as pr
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

# FflOptions' initialisers (ffl_kernels.h) and the fixed "run_ahead" and "merge_expand"; "lanes" is the one knob a test
# here chooses
DEFAULTS = dict(run_ahead=0, fuse_first=10000, merge_expand=1, graph=1, copy_threads=4, blur_rows=0, blur_min_wgs=3500,
                tile_order=0, pyr_coarse=1, fb_general=0)


def rotate_zoom(img, degrees, zoom, about):
    """img turned by `degrees` and magnified by `zoom` about the point `about`: inverse mapping, bilinear, edge-clamped"""
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    c, s = math.cos(math.radians(degrees)) / zoom, math.sin(math.radians(degrees)) / zoom
    sx = about[0] + c * (x - about[0]) + s * (y - about[1])
    sy = about[1] - s * (x - about[0]) + c * (y - about[1])
    sx, sy = np.clip(sx, 0, w - 1), np.clip(sy, 0, h - 1)
    x0, y0 = np.minimum(sx.astype(np.int64), w - 2), np.minimum(sy.astype(np.int64), h - 2)
    fx, fy = sx - x0, sy - y0
    g = img.astype(np.float64)
    out = (g[y0, x0] * (1 - fx) + g[y0, x0 + 1] * fx) * (1 - fy) + (g[y0 + 1, x0] * (1 - fx) + g[y0 + 1, x0 + 1] * fx) * fy
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def kinds(w, h):
    """the distinct frames, by name"""
    rng = np.random.default_rng(w * 31 + h)
    y, x = np.mgrid[0:h, 0:w]
    checker = (((x + y) & 1) * 255).astype(np.uint8)
    wide = sine_translate_frames(1, w + 40, h, seed=6)[0]
    sine = np.ascontiguousarray(wide[:, :w])
    return {"noise_a": rng.integers(0, 256, (h, w), dtype=np.uint8), "noise_b": rng.integers(0, 256, (h, w), dtype=np.uint8),
            "checker": checker, "checker_roll": np.roll(checker, 1, axis=1),
            "c77": np.full((h, w), 77, np.uint8), "c79": np.full((h, w), 79, np.uint8),
            "jump40": np.ascontiguousarray(wide[:, 40:40 + w]), "sine": sine,
            "sine_rot": rotate_zoom(sine, 3.0, 1.04, (0.365 * w, 0.278 * h))}


# nine frames in a cycle: the five pairs of a kind (noise a/b, checkerboard / roll, 77 / 79, the 40-px jump, rotation + zoom)
# and the four pairs that cross kinds (noise -> checkerboard, checkerboard -> constant, constant -> texture, texture -> noise)
FULL = ["noise_a", "noise_b", "checker", "checker_roll", "c77", "c79", "jump40", "sine", "sine_rot"]
SHORT = ["noise_a", "noise_b", "sine", "sine_rot"]      # 3840x2160: noise, rotation and their two cross pairs

_frames, _refs = {}, {}


def stream(w, h, cycle, n):
    if (w, h) not in _frames:
        _frames[(w, h)] = kinds(w, h)
    names = [cycle[i % len(cycle)] for i in range(n)]
    return names, [_frames[(w, h)][k] for k in names]


def reference(tag, w, h, a, b, fn):
    """fn(frame a, frame b), run once per distinct pair and estimator"""
    key = (tag, w, h, a, b)
    if key not in _refs:
        ref = fn(_frames[(w, h)][a], _frames[(w, h)][b])
        assert np.isfinite(ref).all(), key
        _refs[key] = ref
    return _refs[key]


def run_pairs(ctx, frames, launch):
    n = len(frames) - 1
    for i, f in enumerate(frames):
        ctx.upload_frame(i, f)
    launch(list(range(n)), list(range(1, n + 1)), list(range(n)))
    return ctx.pass1_results(list(range(n)))


def check_batch(ctx, names, recs, tag, fn, post=True):
    """every flow bit-identical to the reference of its pair and to its other occurrences in the batch; records and radial
    against the exact references on the first occurrence of each pair, bit-equal on the others"""
    w, h = ctx.width, ctx.height
    c = (0.37 * w + 0.25, 0.41 * h + 0.5)
    n = len(recs)
    rad = ctx.radial(list(range(n)), [c] * n, [False] * n, False)
    pov = ctx.radial(list(range(n)), [c] * n, [False] * n, True)
    first = {}
    for j in range(n):
        pair = (names[j], names[j + 1])
        ref = reference(tag, w, h, *pair, fn)
        got = ctx.download_flow(j)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            f"{tag} {w}x{h} pair {j} {pair}: {np.count_nonzero(got != ref)} values differ, max |diff| {np.abs(got - ref).max()}"
        if pair in first:
            k = first[pair]
            assert repr(recs[j]) == repr(recs[k]) and rad[j] == rad[k] and pov[j] == pov[k], (j, k, pair)
            continue
        first[pair] = j
        if post:
            x, y, v, mm, cut = recs[j]
            rx, ry, rv = pr.argmax_ref(got)
            assert (x, y) == (rx, ry) and np.float32(v).tobytes() == np.float32(rv).tobytes(), (j, pair)
            pr.check_mean_mag(mm, got)
            assert cut is bool(np.float32(mm) > np.float32(7.0))
            pr.check_radial(rad[j], got, c, False)
            pr.check_radial(pov[j], got, c, True)
    return first


@pytest.mark.parametrize("config,lanes", [("default", 1), ("default", 2), ("fuse_first=1", 2), ("fuse_first=0", 2)])
def test_1080p_b32(config, lanes):
    """the path bench.py and every 1080p user takes.  "default": no option touched, the step captured and replayed;
    fuse_first = 1 folds the first launch on every level, 0 on none: the same bits."""
    W, H, B = 1920, 1080, 32
    names, frames = stream(W, H, FULL, B + 1)
    launch_opts = dict(DEFAULTS)
    try:
        _capi.set_option("lanes", lanes)
        if config != "default":
            launch_opts["fuse_first"] = int(config.split("=")[1])
            _capi.set_option("fuse_first", launch_opts["fuse_first"])
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
            assert {k: ctx.get_option(k) for k in DEFAULTS} == launch_opts and ctx.get_option("lanes") == lanes
            recs = run_pairs(ctx, frames, ctx.flow_pairs)
            first = check_batch(ctx, names, recs, "farneback", orc.farneback, post=config == "default")
            assert len(first) == len(FULL)
            recs2 = run_pairs(ctx, frames, ctx.flow_pairs)            # the same step again: replayed from the graph
            assert repr(recs2) == repr(recs)
            for j in (0, 7, B - 1):
                assert np.array_equal(ctx.download_flow(j), reference("farneback", W, H, names[j], names[j + 1], orc.farneback))
            gs = ctx.graph_stats()
            assert gs["capture_failures"] == 0 and gs["captured"] >= 1 and gs["replayed"] == 2, gs
    finally:
        _capi.set_option("lanes", 2)
        _capi.set_option("fuse_first", 10000)


def test_4k_b32_default_options():
    """3840x2160 picks other strips and tiles: noise and rotation pairs and their cross pairs, B = 32, nothing overridden but
    the lane count (one lane, as bench.py runs)"""
    W, H, B = 3840, 2160, 32
    names, frames = stream(W, H, SHORT, B + 1)
    try:
        _capi.set_option("lanes", 1)
        with _capi.Context(W, H, frame_slots=B + 2, flow_slots=B, max_batch=B) as ctx:
            assert {k: ctx.get_option(k) for k in DEFAULTS} == DEFAULTS
            recs = run_pairs(ctx, frames, ctx.flow_pairs)
            first = check_batch(ctx, names, recs, "farneback", orc.farneback)
            assert len(first) == len(SHORT)
            gs = ctx.graph_stats()
            assert gs["capture_failures"] == 0 and gs["captured"] >= 1, gs
    finally:
        _capi.set_option("lanes", 2)


@pytest.mark.parametrize("w,h", [(640, 360), (333, 197)])
@pytest.mark.parametrize("over", [dict(winsize=31), dict(pyr_scale=0.7, levels=6)], ids=["winsize31", "scale0.7_levels6"])
def test_general_farneback(over, w, h):
    B = 8
    names, frames = stream(w, h, FULL, B + 1)
    p = _capi.FarnebackParams(**over)
    tag = "general " + ",".join(f"{k}={v}" for k, v in over.items())
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        recs = run_pairs(ctx, frames, lambda a, b, s: ctx.flow_pairs_farneback(a, b, s, False, p))
        first = check_batch(ctx, names, recs, tag, lambda a, b: fb_general_ref.flow(a, b, fb_general_ref.params(**over)))
        assert len(first) == B


@pytest.mark.parametrize("w,h,B", [(256, 256, 32), (512, 512, 9)])
def test_dis(w, h, B):
    names, frames = stream(w, h, FULL, B + 1)
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        recs = run_pairs(ctx, frames, ctx.flow_pairs_dis)
        first = check_batch(ctx, names, recs, "dis", lambda a, b: dis_ref.flow(a, b, dis_ref.fast_params()))
        assert len(first) == len(FULL)
