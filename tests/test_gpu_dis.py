"""GPU tests of the DIS path (ffl_flow_pairs_dis, the reference's "DNN" backend, FF:948-980): flows are bit-identical
to the plain-C restatement (tests/dis_ref), pass-1 records exact, mean magnitudes and radial scalars
within the 1e-4 relative tolerance of the first GPU tests and within the derived bounds of tests/post_ref.py.  Parity with
cv2.DISOpticalFlow itself is unpinned (no cv2 here)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dis_ref
import gen_dis_golden
import oracle as orc
import post_ref as pr
from funscript_flow_amd import _capi, backend, pipeline
from funscript_flow_amd.synth import gray_to_bgr, sine_translate_frames


_contents = gen_dis_golden.contents


def _ref_pair(f0, f1, p):
    rp = dis_ref.fast_params(**p.as_dict()) if p is not None else dis_ref.fast_params()
    return dis_ref.flow(f0, f1, rp)


def _check_batch(ctx, pairs, p=None, pov=False):
    """pairs: list of (f0, f1) arrays; uploads 2 frames per pair, one DIS batch, every flow and record checked"""
    n = len(pairs)
    frames = [f for pr in pairs for f in pr]
    ctx.upload_frames(0, frames)
    ctx.flow_pairs_dis(list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), list(range(n)), pov, p)
    recs = ctx.pass1_results(list(range(n)))
    for i, (f0, f1) in enumerate(pairs):
        ref = _ref_pair(f0, f1, p)
        got = ctx.download_flow(i)
        assert np.array_equal(got, ref), f"pair {i}: max |diff| {np.abs(got - ref).max()}"
        x, y, v, mm, cut = recs[i]
        if not pov:
            ox, oy, ov = orc.max_divergence_np(ref)
            assert (x, y) == (ox, oy) and np.float32(v) == np.float32(ov)
        rm = float(orc.mean_mag_np(ref))
        assert abs(float(mm) - rm) <= 1e-4 * max(rm, 1e-6)
        pr.check_mean_mag(mm, ref)
    return recs


@pytest.mark.parametrize("B", [1, 32, 256])
def test_batches_bit_identical_to_restatement(B):
    w = h = 256
    cont = _contents(w, h)
    pairs = [cont[i % len(cont)][1:] for i in range(B)]
    if B == 256:   # the big batch checks a sample against the restatement (one C pair is ~10 ms) and the rest for equality
        with _capi.Context(w, h, frame_slots=2 * B, flow_slots=B, max_batch=B) as ctx:
            ctx.upload_frames(0, [f for pr in pairs for f in pr])
            ctx.flow_pairs_dis(list(range(0, 2 * B, 2)), list(range(1, 2 * B, 2)), list(range(B)))
            refs = {i: _ref_pair(*cont[i][1:], None) for i in range(len(cont))}
            want = {i: (orc.max_divergence_np(r), float(orc.mean_mag_np(r))) for i, r in refs.items()}
            recs = ctx.pass1_results(list(range(B)))
            for i in range(B):
                assert np.array_equal(ctx.download_flow(i), refs[i % len(cont)]), i
                (ox, oy, ov), rm = want[i % len(cont)]
                x, y, v, mm, _ = recs[i]
                assert (x, y) == (ox, oy) and np.float32(v) == np.float32(ov), i
                assert abs(float(mm) - rm) <= 1e-4 * max(rm, 1e-6), i
                pr.check_mean_mag(mm, refs[i % len(cont)])
            assert ctx.graph_stats()["capture_failures"] == 0
        return
    with _capi.Context(w, h, frame_slots=2 * B, flow_slots=B, max_batch=B) as ctx:
        _check_batch(ctx, pairs)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_constant_and_identical_frames_give_zero_flow():
    w = h = 256
    cont = {n: (a, b) for n, a, b in _contents(w, h)}
    with _capi.Context(w, h, max_batch=2) as ctx:
        _check_batch(ctx, [cont["constant"], cont["identical"]])
        assert not ctx.download_flow(0).any() and not ctx.download_flow(1).any()


def test_radial_matches_restatement_field():
    w = h = 256
    cont = _contents(w, h)
    with _capi.Context(w, h, max_batch=8) as ctx:
        recs = _check_batch(ctx, [c[1:] for c in cont], pov=False)
        c = np.array([130.5, 120.25])
        for pov in (False, True):
            got = ctx.radial(list(range(len(cont))), [c] * len(cont), [False] * len(cont), pov)
            for i, (_, f0, f1) in enumerate(cont):
                want = float(orc.radial_np(_ref_pair(f0, f1, None), c, False, pov))
                assert abs(got[i] - want) <= 1e-4 * max(abs(want), 1e-3)
                pr.check_radial(got[i], _ref_pair(f0, f1, None), c, pov)


def test_parameter_variants_and_512():
    cont = _contents(256, 256)
    with _capi.Context(256, 256, max_batch=4) as ctx:
        for over in ({"stripes": 8}, {"stripes": 1}, {"var_refine_iters": 0}, {"use_spatial_prop": 0},
                     {"use_mean_norm": 0}):
            _check_batch(ctx, [c[1:] for c in cont[:3]], _capi.DisParams(**over))
    fr = sine_translate_frames(2, 512, 512, seed=9, amp=(4.0, 3.0), zoom=0.03)
    with _capi.Context(512, 512, max_batch=1) as ctx:
        _check_batch(ctx, [(fr[0], fr[1])])


def test_vr_input_through_raw_upload():
    src = sine_translate_frames(2, 640, 480, seed=6, amp=(5.0, 3.0))
    bgr = [np.ascontiguousarray(gray_to_bgr(f, (1.0, 0.9, 1.1))) for f in src]
    with _capi.Context(256, 256, max_batch=1) as ctx:
        ctx.upload_frames_raw(0, bgr, (512, 512), (0, 256))
        g0, g1 = ctx.download_frame(0), ctx.download_frame(1)
        assert np.array_equal(g0, orc.frontend(bgr[0], vr_mode=True))
        ctx.flow_pairs_dis([0], [1], [0])
        assert np.array_equal(ctx.download_flow(0), _ref_pair(g0, g1, None))


@pytest.mark.parametrize("scale", [2, 3])
def test_debug_stages_match_restatement(scale):
    f0, f1 = _contents(256, 256)[1][1:]
    with _capi.Context(256, 256, max_batch=1) as ctx:
        ctx.upload_frames(0, [f0, f1])
        for name, st in _capi.DIS_STAGES.items():
            got = ctx.debug_dis_pair(0, 1, scale, name)
            _, want = dis_ref.flow(f0, f1, dis_ref.fast_params(), dbg=(scale, st))
            assert got.shape == want.shape and np.array_equal(got, want), (scale, name)
        assert np.array_equal(ctx.download_flow(0), _ref_pair(f0, f1, None))


def test_unsupported_sizes_are_refused():
    for w, h in ((640, 360), (1920, 1080)):
        with _capi.Context(w, h, max_batch=1) as ctx:
            ctx.upload_frames(0, [np.zeros((h, w), np.uint8)] * 2)
            with pytest.raises(_capi.FFLError, match="ffl error 1"):
                ctx.flow_pairs_dis([0], [1], [0])
    with _capi.Context(256, 256, max_batch=1) as ctx:
        ctx.upload_frames(0, [np.zeros((256, 256), np.uint8)] * 2)
        with pytest.raises(_capi.FFLError, match="patch_size"):
            ctx.flow_pairs_dis([0], [1], [0], params=_capi.DisParams(patch_size=12, finest_scale=1))


def test_mixed_dis_and_farneback_batches_on_two_lanes():
    """DIS and Farneback batches alternate over shared frame slots on a two-lane context; each result equals the pair
    computed alone (restatement / oracle), slots recycled across algorithms"""
    w = h = 256
    fr = sine_translate_frames(9, w, h, seed=11, amp=(3.0, 2.0), zoom=0.02)
    with _capi.Context(w, h, frame_slots=9, flow_slots=8, max_batch=4) as ctx:
        assert ctx.get_option("lanes") == 2
        ctx.upload_frames(0, list(fr))
        # round 0: DIS pairs 0..3 -> slots 0..3, Farneback pairs 0..3 -> slots 4..7
        # round 1: Farneback pairs 4..7 -> slots 0..3, DIS pairs 4..7 -> slots 4..7 (every slot recycled)
        for rnd in range(2):
            lo = 4 * rnd
            first, second = (ctx.flow_pairs_dis, ctx.flow_pairs) if rnd == 0 else (ctx.flow_pairs, ctx.flow_pairs_dis)
            first(list(range(lo, lo + 4)), list(range(lo + 1, lo + 5)), [0, 1, 2, 3])
            second(list(range(lo, lo + 4)), list(range(lo + 1, lo + 5)), [4, 5, 6, 7])
            recs = ctx.pass1_results(list(range(8)))
            for s in range(8):
                a = lo + s % 4
                dis = (s < 4) == (rnd == 0)
                want = _ref_pair(fr[a], fr[a + 1], None) if dis else orc.farneback(fr[a], fr[a + 1])
                assert np.array_equal(ctx.download_flow(s), want), (rnd, s)
                assert recs[s][:2] == orc.max_divergence_np(want)[:2]
        assert ctx.graph_stats()["capture_failures"] == 0


def test_pair_engine_dis_recycles_slots_at_depth_2():
    w = h = 256
    fr = sine_translate_frames(40, w, h, seed=12, amp=(3.0, 2.0), zoom=0.03)
    B = 8
    ctx = _capi.Context(w, h, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2),
                        max_batch=B)
    eng = pipeline.PairEngine(ctx, depth=2, flow="dis")
    dots, recs = eng.process_chunk(list(fr))
    for j in (0, 17, 38):
        ref = _ref_pair(fr[j], fr[j + 1], None)
        ox, oy, _ = orc.max_divergence_np(ref)
        assert recs[j][:2] == (ox, oy)
    centers = pipeline.smooth_centers(np.array([r[:2] for r in recs]))
    for j in (0, 17, 38):
        want = float(orc.radial_np(_ref_pair(fr[j], fr[j + 1], None), centers[j], recs[j][4], False))
        assert abs(dots[j] - want) <= 1e-4 * max(abs(want), 1e-3)
        assert not recs[j][4], j                  # a 3 % zoom is no cut: the exact check below runs for every sampled pair
        pr.check_radial(dots[j], _ref_pair(fr[j], fr[j + 1], None), centers[j], False)
    assert ctx.graph_stats()["capture_failures"] == 0
    ctx.close()


def test_drop_ins_on_a_zoom_clip():
    w = h = 256
    fr = sine_translate_frames(600, w, h, seed=13, amp=(2.0, 1.5), zoom=0.04, period=24)
    frames = list(fr)
    pairs = list(zip(frames[:-1], frames[1:]))
    params = {"backend": "HIP", "hip_flow": "dis"}
    pre = backend.precompute_all(pairs, params)
    centers = pipeline.smooth_centers(np.array([p["pos_center"] for p in pre]))
    dots = backend.radial_all(pre, centers)
    # the restatement-driven chain, on a sample of pairs (full pass-1 records for all of them)
    rx, exact = [], 0
    for j in range(len(pairs)):
        ref = _ref_pair(pairs[j][0], pairs[j][1], None)
        ox, oy, _ = orc.max_divergence_np(ref)
        assert (int(pre[j]["pos_center"][0]), int(pre[j]["pos_center"][1])) == (ox, oy), j
        rx.append(float(orc.radial_np(ref, centers[j], pre[j]["cut"], False)))
        if j % 25 == 0 and not pre[j]["cut"]:
            pr.check_radial(dots[j], ref, centers[j], False)
            exact += 1
    assert exact >= 12, exact                      # of the 24 sampled pairs; a cut's scalar is 0.0 by definition
    rx = np.array(rx)
    assert np.all(np.abs(np.array(dots) - rx) <= 1e-4 * np.maximum(np.abs(rx), 1e-3))
    # DIS against Farneback about one fixed centre (the argmax centres of two algorithms need not agree, so the per-pair
    # scalars of the two chains are not comparable): a forgotten x4 or a flipped sign would show here
    mid = [(w / 2.0, h / 2.0)] * len(pairs)
    ddots, flow5, c5 = backend.radial_all(pre, mid), np.asarray(pre[5]["flow"]), pre[5]["pos_center"]
    far = backend.precompute_all(pairs, {"backend": "HIP"})     # reuses the chunk's flow slots: `pre` goes stale
    fdots = backend.radial_all(far, mid)
    assert np.corrcoef(ddots, fdots)[0, 1] > 0.9
    scale = np.sum(np.abs(ddots)) / np.sum(np.abs(fdots))
    assert 0.5 < scale < 2.0, scale
    # precompute_flow_info with hip_flow="dis" gives the same record as the batched drop-in
    info = backend.precompute_flow_info(pairs[5][0], pairs[5][1], params)
    assert info["pos_center"] == c5 and np.array_equal(np.asarray(info["flow"]), flow5)
    backend.release_contexts()


def test_committed_fixtures():
    """the device reproduces tests/golden/dis_golden.npz (written from the restatement by tests/gen_dis_golden.py): flow
    SHA-256, pass-1 records exact, radial scalars within 1e-4, the 64x64 finest-scale refined fields bit for bit"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dis_golden.npz"))
    cases = gen_dis_golden.cases()
    assert [c[0] for c in cases] == list(g["names"])
    ctxs = {}
    try:
        for k, (name, f0, f1, over) in enumerate(cases):
            h, w = f0.shape
            assert gen_dis_golden.sha(f0) + gen_dis_golden.sha(f1) == g["frames_sha256"][k], f"{name}: inputs drifted"
            assert json.loads(str(g["params"][k])) == over
            ctx = ctxs.get((w, h)) or ctxs.setdefault((w, h), _capi.Context(w, h, max_batch=1))
            p = _capi.DisParams(**over)
            ctx.upload_frames(0, [f0, f1])
            ctx.flow_pairs_dis([0], [1], [0], False, p)
            x, y, v, mm, _ = ctx.pass1_result(0)
            flow = ctx.download_flow(0)
            assert gen_dis_golden.sha(flow) == g["flow_sha256"][k], name
            assert (x, y) == tuple(g["pass1_xy"][k]) and np.float32(v) == g["pass1_div"][k], name
            want_mm = float(g["pass1_mean_mag"][k])
            assert abs(float(mm) - want_mm) <= 1e-4 * max(want_mm, 1e-6), name
            pr.check_mean_mag(mm, flow)
            c = gen_dis_golden.center(w, h)
            for pov, want in zip((False, True), g["radial"][k]):
                got = ctx.radial([0], [c], [False], pov)[0]
                assert abs(got - want) <= 1e-4 * max(abs(want), 1e-3), (name, pov)
                pr.check_radial(got, flow, c, pov)
            if "finest_" + name in g:
                fin = ctx.debug_dis_pair(0, 1, 2, "refined", p)
                assert np.array_equal(fin, g["finest_" + name]), name
            assert ctx.graph_stats()["capture_failures"] == 0
    finally:
        for ctx in ctxs.values():
            ctx.close()
