"""GPU tests of Farneback with caller-chosen parameters (ffl_flow_pairs_farneback): the
general kernels are bit-identical to the oracle at the reference's values (forced through them with the context option
"fb_general") and to the plain-C restatement (tests/fb_general_ref) under every fixture parameter set; pass-1 argmax records
are exact, mean magnitudes and radial scalars within the tolerances the other GPU tests use (their reductions sum in another
order) and within the derived bounds of tests/post_ref.py.  Parity with cv2 itself is unpinned."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fb_general_ref as fbr
import gen_fb_params_golden as gen
import oracle as orc
import post_ref as pr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

CASES = {c[0]: c for c in gen.CASES}


def _stream(w, h, n_frames, distinct=3, seed=21):
    """n_frames frames cycling through `distinct` textured frames: consecutive pairs share frames and repeat, so a big
    batch needs only `distinct` restatement pairs"""
    fr = sine_translate_frames(distinct + 1, w, h, seed=seed, amp=(2.5, 1.5), period=6, zoom=0.02)
    return [np.ascontiguousarray(fr[i % distinct]) for i in range(n_frames)]


def _run(ctx, frames, params, pov=False, force=None):
    """upload frames, one batch of the stream's pairs (frame j, j+1) -> flow slot j"""
    n = len(frames) - 1
    ctx.upload_frames(0, frames)
    if force is not None:
        ctx.set_option("fb_general", force)
    ctx.flow_pairs_farneback(list(range(n)), list(range(1, n + 1)), list(range(n)), pov, params)
    return ctx.pass1_results(list(range(n)))


def _check(ctx, frames, recs, want_of, pov=False):
    """every pair's flow bit-identical to want_of(f0, f1) (cached per distinct pair), records exact"""
    cache = {}
    for j, r in enumerate(recs):
        key = (id(frames[j]), id(frames[j + 1]))
        if key not in cache:
            ref = want_of(frames[j], frames[j + 1])
            cache[key] = (ref, orc.max_divergence_np(ref), float(orc.mean_mag_np(ref)))
        ref, (ox, oy, ov), rm = cache[key]
        got = ctx.download_flow(j)
        assert np.array_equal(got, ref), f"pair {j}: max |diff| {np.abs(got - ref).max()}"
        x, y, v, mm, _ = r
        if not pov:
            assert (x, y) == (ox, oy) and np.float32(v) == np.float32(ov), j
        assert abs(float(mm) - rm) <= 1e-4 * max(rm, 1e-6), j
        pr.check_mean_mag(mm, ref)


@pytest.mark.parametrize("w,h,scales", [(16, 16, 1),      # no coarser level
                                        (64, 64, 2),      # exactly one: 32 passes min_size, 16 does not
                                        (63, 65, 1),      # 31.5 columns: just under that boundary on one side
                                        (130, 66, 2),     # 65 x 33, then 32.5 x 16.5 is refused
                                        (258, 257, 4)])   # 129 x 128 (128.5 rounds to even), 64 x 64, 32 x 32
def test_context_level_geometry_equals_the_restatement_at_the_defaults(w, h, scales):
    """The levels a context of the tuned path is built with (ffl_num_levels, ffl_level_size) are the ones the plain-C
    restatement derives for the reference's parameters: the tuned and the general plan come from one level rule."""
    assert fbr.geometry(w, h) == scales
    with _capi.Context(w, h, max_batch=1) as ctx:
        assert ctx.num_levels() == scales - 1
        assert [ctx.level_size(k) for k in range(scales)] == [fbr.level_params(w, h, None, k)[:2] for k in range(scales)]


@pytest.mark.parametrize("w,h,B", [(256, 256, 64), (640, 360, 8), (333, 197, 4), (1920, 1080, 32)])
def test_general_kernels_at_the_defaults_equal_the_oracle(w, h, B):
    frames = _stream(w, h, B + 1)
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        recs = _run(ctx, frames, _capi.FarnebackParams(), force=1)
        _check(ctx, frames, recs, lambda a, b: orc.farneback(a, b))
        assert ctx.graph_stats()["captured"] == 0          # the general batch was launched eagerly


def _case_batch(name, B):
    _, w, h, over = CASES[name]
    f0, f1 = gen.frames(w, h)
    frames = [f0 if j % 2 == 0 else f1 for j in range(B + 1)]     # pairs alternate (f0, f1) and (f1, f0): shared frames
    return w, h, over, frames


@pytest.mark.parametrize("name,B", [(c[0], 256 if c[1] == 256 else 8) for c in gen.CASES])
def test_every_fixture_case_matches_the_restatement_and_the_fixtures(name, B, golden_dir):
    w, h, over, frames = _case_batch(name, B)
    p = _capi.FarnebackParams(**over)
    g = np.load(f"{golden_dir}/fb_params_golden.npz")
    i = list(g["names"]).index(name)
    assert json.loads(str(g["params"][i])) == over
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        recs = _run(ctx, frames, p, force=1)
        _check(ctx, frames, recs, lambda a, b: fbr.flow(a, b, over))
        assert gen.sha(ctx.download_flow(0)) == g["flow_sha256"][i]
        x, y, v, mm, _ = recs[0]
        assert (x, y) == tuple(g["pass1_xy"][i]) and np.float32(v) == g["pass1_div"][i]
        ref0 = fbr.flow(frames[0], frames[1], over)          # the restatement's field of pair 0, not the device's own
        for k, pov in enumerate((False, True)):
            got = ctx.radial([0], [gen.gen_dis_golden.center(w, h)], [False], pov)[0]
            want = float(g["radial"][i][k])
            assert abs(got - want) <= 1e-6 * max(abs(want), 1e-9), (pov, got, want)
            pr.check_radial(got, ref0, gen.gen_dis_golden.center(w, h), pov)
        # pov on: the same flow, no argmax record
        recs = _run(ctx, frames, p, pov=True)
        _check(ctx, frames, recs, lambda a, b: fbr.flow(a, b, over), pov=True)
        assert ctx.graph_stats()["capture_failures"] == 0 and ctx.graph_stats()["captured"] == 0


def test_pair_engine_chunk_with_hip_farneback_equals_the_restatement():
    w = h = 256
    over = {"winsize": 21, "poly_n": 7, "poly_sigma": 1.5}
    frames = sine_translate_frames(30, w, h, seed=4, amp=(2.0, 1.0), period=6, zoom=0.01)
    frames = [np.ascontiguousarray(f) for f in frames]
    B = 8
    with _capi.Context(w, h, frame_slots=4 * B + 4, flow_slots=4 * B + 16, max_batch=B) as ctx:
        eng = pipeline.PairEngine(ctx)
        fb = _capi.farneback_choice({"hip_farneback": over})
        dots, recs = eng.process_chunk(frames, farneback=fb)
        for j in range(len(frames) - 1):
            ref = fbr.flow(frames[j], frames[j + 1], over)
            ox, oy, ov = orc.max_divergence_np(ref)
            assert (recs[j][0], recs[j][1]) == (ox, oy) and np.float32(recs[j][2]) == np.float32(ov), j
        # the last pairs' flows are still resident: bit-identical fields
        n = len(frames) - 1
        for j in range(n - 4, n):
            assert np.array_equal(ctx.download_flow(j % ctx.flow_slots), fbr.flow(frames[j], frames[j + 1], over)), j


def test_default_and_general_batches_interleaved_leave_the_defaults_unchanged():
    w = h = 256
    B = 16
    frames = _stream(w, h, B + 1)
    over = {"levels": 5, "winsize": 9}
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=2 * B, max_batch=B) as ctx:
        ctx.upload_frames(0, frames)
        f0, f1 = list(range(B)), list(range(1, B + 1))
        ctx.flow_pairs_farneback(f0, f1, list(range(B)), False, None)          # defaults: the tuned path, captured
        ctx.pass1_results(list(range(B)))
        first = [ctx.download_flow(j) for j in range(B)]
        captured = ctx.graph_stats()["captured"]
        assert captured >= 1
        for rnd in range(3):
            ctx.flow_pairs_farneback(f0, f1, list(range(B, 2 * B)), False, _capi.FarnebackParams(**over))
            ctx.flow_pairs(f0, f1, list(range(B)), False)
            ctx.pass1_results(list(range(2 * B)))
            for j in range(B):
                assert np.array_equal(ctx.download_flow(j), first[j]), (rnd, j)
        ref = fbr.flow(frames[0], frames[1], over)
        assert np.array_equal(ctx.download_flow(B), ref)
        assert np.array_equal(first[0], orc.farneback(frames[0], frames[1]))
        st = ctx.graph_stats()
        assert st["capture_failures"] == 0 and st["captured"] == captured   # no general batch was captured


def test_a_working_set_beyond_the_lane_buffers_runs_in_the_general_work_area():
    w = h = 256
    B = 8
    over = {"pyr_scale": 0.9, "levels": 12}
    p = _capi.FarnebackParams(**over)
    assert _capi.farneback_extra_bytes(w, h, B, p) > 0
    frames = _stream(w, h, B + 1)
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        recs = _run(ctx, frames, p)
        _check(ctx, frames, recs, lambda a, b: fbr.flow(a, b, over))
        recs = _run(ctx, frames, p)                # the area is reused
        _check(ctx, frames, recs, lambda a, b: fbr.flow(a, b, over))
