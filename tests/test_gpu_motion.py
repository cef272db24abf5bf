"""GPU side of the global-motion fit and compensation (ffl_motion_fit, ffl_motion_subtract; DESIGN.md section 19, appendix
C), everything through the C ABI via _capi and on fields placed with import_flows.

The twelve sums are held against the exact sums of the restated terms (tests/motion_ref.py, whose docstring derives the
bound); the record against ffl_motion_solve of the device's own sums, bit for bit -- the host function compiles the source
of the device's solve; the subtraction against rule C8 bit for bit and its records against upload_flow's.

The shapes are the smallest that cross every boundary of the walk: 16x16 (the minimum), 19x17 (odd, narrower than a strip, an
odd pixel count: the subtraction's one-pixel path), 127x33 and 129x17 (a strip of 128 -+ 1, a row group of 16 +- 1), 258x35
(three strips, a ragged last row group)."""
import functools
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import golden_check
import motion_ref as mr
import post_ref as pr
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
SIZES = [(16, 16), (19, 17), (127, 33), (129, 17), (258, 35)]
NS = (1, 3)
REC = _capi.MOTION_DTYPE.itemsize
NAN, INF = float("nan"), float("inf")
BIG = 1e30   # a cut threshold nothing reaches
PRIORS = np.array([[0.5, 0.0, 0.0, -0.25, 0.0, 0.0], [0.1, 0.002, -0.003, 0.2, 0.003, 0.002], [-1.0, 0.0, 0.01, 0.75, -0.01, 0.0]])


def gid(s):
    return f"{s[0]}x{s[1]}"


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


def context(w, h, mb=8, slots=None):
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=slots or 2 * mb)


@functools.lru_cache(maxsize=None)
def field(w, h, seed):
    """a pan, a slow rotation and zoom and noise of order 1: every sum of rule C4 is far from zero"""
    rng = np.random.default_rng(seed)
    xc, yc = mr.coords(w, h)
    f = rng.standard_normal((h, w, 2)) * 0.8
    f[..., 0] += 1.5 + 0.01 * xc - 0.02 * yc
    f[..., 1] += -0.75 + 0.02 * xc + 0.015 * yc
    f = f.astype(np.float32)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def random_map(w, h, seed):
    """random 1..255 with about a third zeros"""
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    m[rng.random((h, w)) < 1 / 3] = 0
    m.setflags(write=False)
    return m


def padded(maps):
    """(n, h, w) maps as a device view with a padded row pitch and item stride"""
    n, h, w = maps.shape
    big = torch.full((n, h + 2, w + 13), 0x5A, dtype=torch.uint8, device=DEV)
    view = big[:, 1:h + 1, 5:5 + w]
    view.copy_(dev(maps))
    return view


def records(buf, n):
    return np.frombuffer(buf.cpu().numpy().tobytes(), _capi.MOTION_DTYPE, n)


def fit(ctx, slots, model="translation", iterations=1, tau=1.0, weights=None, prior=None):
    """(records, sums float64[n, 12]) of one motion_fit call into poisoned buffers"""
    n = len(slots)
    out = torch.full((n * REC,), 0xA5, dtype=torch.uint8, device=DEV)
    sums = torch.full((n, 12), NAN, dtype=torch.float64, device=DEV)
    ctx.motion_fit(slots, model, iterations, tau, weights=weights, prior=prior, out=out, sums_out=sums)
    return records(out, n), sums.cpu().numpy()


def check_items(ctx, fields, slots, maps=None, prior=None, tau=1.0):
    """the sums of every item against the restatement, and the record of every model against ffl_motion_solve of those sums"""
    worst, sums0 = 0.0, None
    for model in mr.MODELS:
        rec, sums = fit(ctx, slots, model, 1, tau, None if maps is None else maps[0], None if prior is None else dev(prior))
        if sums0 is None:
            sums0 = sums
            for i, f in enumerate(fields):
                W = None if maps is None else maps[1][i if maps[1].ndim == 3 else ...]
                worst = max(worst, mr.check_sums(sums[i], f, W, None if prior is None else prior[i], tau))
        assert sums.tobytes() == sums0.tobytes(), model                       # the sums do not depend on the model
        for i in range(len(fields)):
            assert rec[i].tobytes() == _capi.motion_solve(sums[i], model).tobytes(), (model, i, rec[i])
    return worst


# ---- 1. sums and models ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_sums_match_the_restatement_and_records_the_host_solve(size, n, capsys):
    w, h = size
    slots = list(range(2, 2 + n))
    fields = [field(w, h, 10 * w + i) for i in range(n)]
    maps = np.stack([random_map(w, h, 10 * w + i) for i in range(n)])
    hostile = [f.copy() for f in fields]
    for i, f in enumerate(hostile):                       # NaN and inf in the flow, all under zero weights
        zy, zx = np.nonzero(maps[i] == 0)
        f[zy[0], zx[0]] = (NAN, 1.0)
        f[zy[1], zx[1]] = (2.0, -INF)
        f[zy[-1], zx[-1]] = (INF, NAN)
    loud = [f.copy() for f in fields]
    full = np.full((n, h, w), 255, np.uint8)
    for i, f in enumerate(loud):                          # a non-finite pixel under weight 255: excluded all the same
        f[h // 2, w // 3] = (NAN, 0.5)
        f[h - 1, w - 1] = (0.5, INF)
    with context(w, h) as ctx:
        ctx.import_flows(dev(np.stack(fields)), slots)
        worst = [check_items(ctx, fields, slots)]                                                   # no map, no prior
        worst.append(check_items(ctx, fields, slots, prior=PRIORS[:n], tau=1.5))                    # a given prior
        worst.append(check_items(ctx, fields, slots, maps=(dev(maps[0]), maps[0])))                 # item_stride = 0
        ctx.import_flows(dev(np.stack(hostile)), slots)
        worst.append(check_items(ctx, hostile, slots, maps=(padded(maps), maps)))                   # per-item maps, padded pitch
        worst.append(check_items(ctx, hostile, slots, maps=(padded(maps), maps), prior=PRIORS[:n], tau=0.5))
        ctx.import_flows(dev(np.stack(loud)), slots)
        worst.append(check_items(ctx, loud, slots, maps=(dev(full), full)))
        worst.append(check_items(ctx, loud, slots, prior=PRIORS[:n]))
        assert ctx.graph_stats()["capture_failures"] == 0
    with capsys.disabled():
        print(f"\n  {w}x{h} n={n}: worst sum error {max(worst):.2f} u*A, bound {pr.radial_depth(w, h)}")


@pytest.mark.parametrize("size", [(19, 17), (129, 17)], ids=gid)
def test_empty_and_degenerate_fits(size):
    w, h = size
    f = [field(w, h, 5), field(w, h, 6), field(w, h, 7)]
    maps = np.zeros((3, h, w), np.uint8)                  # item 0: an empty map
    maps[1, 9, :] = 200                                   # item 1: all the weight on one row (AFFINE degenerates)
    maps[2, 4, 3] = 7                                     # item 2: one pixel (RIGID and SIMILARITY degenerate too)
    with context(w, h) as ctx:
        ctx.import_flows(dev(np.stack(f)), [0, 1, 2])
        for model in mr.MODELS:
            for prior in (None, dev(PRIORS)):
                rec, sums = fit(ctx, [0, 1, 2], model, 1, 1.0, dev(maps), prior)
                for i in range(3):
                    assert rec[i].tobytes() == _capi.motion_solve(sums[i], model).tobytes(), (model, i)
                assert rec["status"][0] == mr.EMPTY and sums[0].tobytes() == np.zeros(12).tobytes() and mr.six(rec[0]) == [0.0] * 6
                assert rec["status"][1] == (mr.DEGENERATE if model == "affine" else mr.OK)
                assert rec["status"][2] == (mr.OK if model == "translation" else mr.DEGENERATE)
                if prior is None:
                    assert (rec["a0"][2], rec["b0"][2]) == (float(f[2][4, 3, 0]), float(f[2][4, 3, 1]))
        # everything excluded without a map: a field of NaN
        ctx.upload_flow(3, np.full((h, w, 2), NAN, np.float32))
        rec, sums = fit(ctx, [3], "affine", 3)
        assert rec["status"][0] == mr.EMPTY and rec[0].tobytes() == _capi.motion_solve(np.zeros(12), "affine").tobytes()


# ---- 2. iterations ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(19, 17), (258, 35)], ids=gid)
def test_three_iterations_are_three_chained_calls(size):
    w, h = size
    n = 3
    fields = np.stack([field(w, h, 40 + i) for i in range(n)])
    fields[1, :h // 2, :w // 2] += np.float32(6.0)        # a block of outliers for the robust weight to work on
    maps = dev(np.stack([random_map(w, h, 40 + i) for i in range(n)]))
    slots = [5, 1, 3]
    with context(w, h) as ctx:
        ctx.import_flows(dev(fields), slots)
        for model in mr.MODELS:
            for wts, prior in ((None, None), (maps, None), (maps, dev(PRIORS))):
                rec3, sums3 = fit(ctx, slots, model, 3, 2.0, wts, prior)
                buf = torch.full((n * REC,), 0xA5, dtype=torch.uint8, device=DEV)
                sums = torch.full((n, 12), NAN, dtype=torch.float64, device=DEV)
                ctx.motion_fit(slots, model, 1, 2.0, weights=wts, prior=prior, out=buf, sums_out=sums)
                first = records(buf, n)
                for _ in range(2):                        # its own records as the prior, in place (stride 64)
                    ctx.motion_fit(slots, model, 1, 2.0, weights=wts, prior=buf, out=buf, sums_out=sums)
                assert records(buf, n).tobytes() == rec3.tobytes() and sums.cpu().numpy().tobytes() == sums3.tobytes(), model
                assert first.tobytes() != rec3.tobytes()
                # the last pass against the restatement with pass 2's record as its prior
                two = fit(ctx, slots, model, 2, 2.0, wts, prior)[0]
                for i in range(n):
                    W = None if wts is None else wts[i].cpu().numpy()
                    mr.check_sums(sums3[i], fields[i], W, mr.six(two[i]), 2.0)


# ---- 2b. the fit's sums and pass 2's are one walk --------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(16, 16), (129, 17), (258, 35)], ids=gid)
def test_motion_sums_are_pass2_sums(size):
    """An exact relation between the two families that run the strip-sum walk, so that an edit to one policy that reorders its
    sums is seen.  In POV mode pass 2's quadrant weights are 1.0, so its shift_x term is (u * 1) * 1 [* p] and the fit's,
    without a prior, (p * 1) * u: the same products of the same pixels, which both add pixel x, then x + 1, row by row, through
    one wave tree, one LDS order and one collect.  An excluded pixel adds +0.0 in pass 2 and +-0.0 in the fit, neither of which
    changes a bit of a sum that started at +0.0; one IEEE division on either side.  The fields mix two scales, 1 and 2^30, under
    random signs: with flow of one magnitude every float64 addition here is exact and no order could be seen, and without
    cancellation a lane's rounding is lost in the total.  129x17: a last strip of one column and a last row group of one row;
    258x35: three strips and three row groups."""
    w, h = size
    n = 3
    rng = np.random.default_rng(w)
    scale = rng.choice([-1.0, 1.0], (n, h, w, 2)) * np.exp2(rng.choice([0, 30], (n, h, w, 2)))
    fields = np.stack([field(w, h, 70 + i) for i in range(n)]) * scale.astype(np.float32)
    fields[1][rng.random((h, w, 2)) < 0.05] = np.float32(-0.0)
    assert np.isfinite(fields).all() and np.signbit(fields[1][fields[1] == 0]).any()
    slots, centres = [4, 0, 2], [(0.0, 0.0), (w / 3.0, h / 2.0), (w - 1.0, 5.5)]
    S, SU, SV = (_capi.MOTION_SUMS.index(k) for k in ("S", "Su", "Sv"))
    bits = lambda a: np.ascontiguousarray(a, np.float64).tobytes()

    def window(maps):
        out = torch.full((n * _capi.PASS2_AXES_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device=DEV)
        ctx.radial_window_axes_weighted(slots, 0, n, maps, out, 1, BIG, True)
        return np.frombuffer(out.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)

    with context(w, h) as ctx:
        ctx.import_flows(dev(fields), slots, pov_mode=True)
        sums = fit(ctx, slots)[1]
        axes = ctx.radial_axes(slots, centres, [False] * n, pov_mode=True)
        npx = np.float64(w) * np.float64(h)
        assert bits(sums[:, S]) == bits(np.full(n, w * h))
        assert bits(axes[:, 2]) == bits(sums[:, SU] / npx)
        assert bits(axes[:, 3]) == bits(sums[:, SV] / npx)
        per_item = np.stack([random_map(w, h, 70), np.zeros((h, w), np.uint8), random_map(w, h, 72)])
        for maps, live in ((padded(per_item), [0, 2]), (dev(random_map(w, h, 73)), [0, 1, 2])):
            sums = fit(ctx, slots, weights=maps)[1]
            rec = window(maps)
            assert not rec["cut"].any() and (sums[live, S] > 0).all()
            assert bits(rec["shift_x"][live]) == bits(sums[live, SU] / sums[live, S])
            assert bits(rec["shift_y"][live]) == bits(sums[live, SV] / sums[live, S])
            if len(live) < n:                             # the all-zero map: rule W5
                assert bits(sums[1]) == bits(np.zeros(12))
                assert bits([rec["shift_x"][1], rec["shift_y"][1]]) == bits(np.zeros(2))


# ---- 3. the subtraction ---------------------------------------------------------------------------------------------------------
def rec_bytes(recs):
    return [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in recs]


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("size", SIZES, ids=gid)
def test_subtract_is_rule_c8_and_its_records_are_upload_flows(size, n):
    w, h = size
    src, dst = list(range(n)), list(range(4, 4 + n))
    fields = np.stack([field(w, h, 70 + 10 * w + i) for i in range(n)])
    fields[0, 2, 3] = (NAN, INF)                          # non-finite samples follow IEEE
    models = np.array([[1.5, 0.01, -0.02, -0.75, 0.02, 0.015], [3.25, 0.0, 0.0, -1.5, 0.0, 0.0], [0.0] * 6])[:n]
    want = [mr.subtract(fields[i], models[i]) for i in range(n)]
    own = np.zeros(n, _capi.MOTION_DTYPE)                 # the same six numbers in 64-byte records
    for k, name in enumerate(("a0", "a1", "a2", "b0", "b1", "b2")):
        own[name] = models[:, k]
    own["sw"], own["status"] = NAN, 2                     # neither is read
    with context(w, h) as ctx, context(w, h) as ref:
        for pov in (False, True):
            for m in (dev(models), dev(own.view(np.uint8))):                      # stride 48 and stride 64
                ctx.import_flows(dev(fields), src, pov)
                ctx.motion_subtract(src, dst, m, pov)
                got = [ctx.download_flow(s) for s in dst]
                for i in range(n):
                    assert got[i].tobytes() == want[i].tobytes(), (i, pov)
                    assert ctx.download_flow(src[i]).tobytes() == fields[i].tobytes()   # the src is intact
                    ref.upload_flow(0, want[i], pov)
                    assert rec_bytes(ctx.pass1_results([dst[i]], 1.0)) == rec_bytes(ref.pass1_results([0], 1.0)), (i, pov)
                ctx.motion_subtract(src, src, m, pov)                             # in place: the same bits
                for i in range(n):
                    assert ctx.download_flow(src[i]).tobytes() == want[i].tobytes(), (i, pov)
                assert rec_bytes(ctx.pass1_results(src, 1.0)) == rec_bytes(ctx.pass1_results(dst, 1.0))
        if n == 3:
            assert want[2].tobytes() == fields[2].tobytes()                       # an all-zero model is a copy
            ctx.import_flows(dev(fields), src)                                    # mixed: item 1 in place, the others moved
            ctx.motion_subtract(src, [6, 1, 7], dev(models))
            assert [ctx.download_flow(s).tobytes() for s in (6, 1, 7)] == [x.tobytes() for x in want]
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    W, H = 130, 17
    INVALID, STATE = _capi.FFL_ERR_INVALID, _capi.FFL_ERR_STATE
    slots = list(range(3, 8))
    fields = np.stack([field(W, H, 90 + i) for i in range(5)])
    with _capi.Context(W, H, max_batch=8, frame_slots=2, flow_slots=16) as ctx:
        ctx.import_flows(dev(fields), slots)
        before = rec_bytes(ctx.pass1_results(slots, 1.0))
        out = torch.full((8 * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        sums = torch.full((8, 12), NAN, dtype=torch.float64, device=DEV)
        prior = dev(np.zeros((8, 6)))
        one = dev(random_map(W, H, 1))
        L, h = ctx.L, ctx._h

        def refused(match, code, call, fn):
            with pytest.raises(_capi.FFLError, match=match) as e:
                call()
            assert e.value.code == code and fn in str(e.value)

        def fit_raw(s, prm=None, w=None, prior_ptr=None, pstride=0, out_ptr=out.data_ptr(), sums_ptr=None, stream=None):
            ps, keep = _capi._iarr(s)
            prm = prm or _capi.MotionParams()
            return lambda: ctx._chk(L.ffl_motion_fit(h, len(keep), ps, _capi.C.byref(prm), None if w is None else _capi.C.byref(w),
                                                     prior_ptr, pstride, out_ptr, sums_ptr, _capi.stream_handle(stream, 0)))

        def sub_raw(s, d, ptr=prior.data_ptr(), stride=48, stream=None):
            (ps, k1), (pd, k2) = _capi._iarr(s), _capi._iarr(d)
            return lambda: ctx._chk(L.ffl_motion_subtract(h, len(k1), ps, pd, ptr, stride, 0, _capi.stream_handle(stream, 0)))

        FIT, SUB = "ffl_motion_fit", "ffl_motion_subtract"
        refused(r"n = 0 slots outside 1\.\.8", INVALID, fit_raw([]), FIT)
        refused(r"n = 9 slots outside 1\.\.8", INVALID, fit_raw(list(range(9))), FIT)
        refused(r"flow slot 16 out of range", INVALID, fit_raw([16]), FIT)
        refused(r"flow slot 5 repeated in one call", INVALID, fit_raw([4, 5, 5]), FIT)
        refused(r"flow slot 2 holds no flow", STATE, fit_raw([2, 3]), FIT)
        refused(r"rule C7: iterations = 9 outside", INVALID, fit_raw(slots, _capi.MotionParams(iterations=9)), FIT)
        refused(r"rule C3: tau = 0 outside", INVALID, fit_raw(slots, _capi.MotionParams(tau=0.0)), FIT)
        bad = _capi.MotionParams()
        bad.model = 7
        refused(r"rule C2: model = 7", INVALID, fit_raw(slots, bad), FIT)
        refused(r"overlap: weight row pitch 129 below the width 130", INVALID, fit_raw(slots, w=_capi.DevWeights(one.data_ptr(), 0, W - 1)), FIT)
        refused(r"NULL weight base", INVALID, fit_raw(slots, w=_capi.DevWeights(0, 0, W)), FIT)
        pin = ctx.pinned_frames(1, channels=1)
        assert pin.size >= max(W * H, 5 * REC)
        refused(r"the weight maps is page-locked host memory", INVALID, fit_raw(slots, w=_capi.DevWeights(pin.ctypes.data, 0, W)), FIT)
        refused(r"models_dev is page-locked host memory", INVALID, fit_raw(slots, out_ptr=pin.ctypes.data), FIT)
        refused(r"NULL models_dev", INVALID, fit_raw(slots, out_ptr=None), FIT)
        refused(r"models_dev and sums_dev must be 8-byte aligned", INVALID, fit_raw(slots, out_ptr=out.data_ptr() + 4), FIT)
        refused(r"models_dev and sums_dev must be 8-byte aligned", INVALID, fit_raw(slots, sums_ptr=sums.data_ptr() + 4), FIT)
        refused(r"prior_dev must be 8-byte aligned", INVALID, fit_raw(slots, prior_ptr=prior.data_ptr() + 4, pstride=48), FIT)
        refused(r"prior_dev stride 40: a multiple of 8 bytes, at least 48", INVALID, fit_raw(slots, prior_ptr=prior.data_ptr(), pstride=40), FIT)
        refused(r"prior_dev stride 52", INVALID, fit_raw(slots, prior_ptr=prior.data_ptr(), pstride=52), FIT)
        torch.cuda.empty_cache()
        big = torch.empty(18 << 20, dtype=torch.uint8, device=DEV)            # an allocation of its own
        end = big.data_ptr() + big.numel()
        refused(rf"models_dev spans {5 * REC} bytes, {REC} more than its allocation holds", INVALID, fit_raw(slots, out_ptr=end - 4 * REC), FIT)
        refused(r"sums_dev spans 480 bytes, 96 more", INVALID, fit_raw(slots, sums_ptr=end - 4 * 96), FIT)
        refused(r"prior_dev spans 240 bytes, 48 more", INVALID, fit_raw(slots, prior_ptr=end - 4 * 48, pstride=48), FIT)
        refused(r"rule C7: overlap: models_dev .* and prior_dev .* share memory with iterations = 3", INVALID,
                fit_raw(slots, prior_ptr=out.data_ptr(), pstride=64), FIT)
        fit_raw(slots, _capi.MotionParams(iterations=1), prior_ptr=out.data_ptr(), pstride=64)()   # one pass in place is the chain
        refused(r"n = 0 items outside 1\.\.8", INVALID, sub_raw([], []), SUB)
        refused(r"flow slot 16 out of range", INVALID, sub_raw([3], [16]), SUB)
        refused(r"flow slot 4 repeated among the src slots", INVALID, sub_raw([4, 4], [8, 9]), SUB)
        refused(r"flow slot 9 repeated among the dst slots", INVALID, sub_raw([3, 4], [9, 9]), SUB)
        refused(r"dst flow slot 4 is another item's src slot", INVALID, sub_raw([3, 4], [4, 9]), SUB)
        refused(r"flow slot 2 holds no flow", STATE, sub_raw([2], [2]), SUB)
        refused(r"NULL models_dev", INVALID, sub_raw([3], [3], ptr=None), SUB)
        refused(r"models_dev must be 8-byte aligned", INVALID, sub_raw([3], [3], ptr=prior.data_ptr() + 4), SUB)
        refused(r"models_dev stride 16", INVALID, sub_raw([3], [3], stride=16), SUB)
        refused(r"models_dev is page-locked host memory", INVALID, sub_raw([3], [3], ptr=pin.ctypes.data), SUB)
        refused(r"models_dev spans 96 bytes, 48 more", INVALID, sub_raw([3, 4], [3, 4], ptr=end - 48), SUB)
        with pytest.raises(ValueError, match="2 weight maps for 5 items"):
            ctx.motion_fit(slots, weights=dev(np.ones((2, H, W), np.uint8)))
        with pytest.raises(ValueError, match="motion_fit: out holds 64 bytes, 5 records need 320"):
            ctx.motion_fit(slots, out=out[:64])
        with pytest.raises(ValueError, match=r"float64 shape \(4, 6\)"):
            ctx.motion_fit(slots, prior=prior[:4])
        with pytest.raises(ValueError, match="2 src slots for 1 dst slots"):
            ctx.motion_subtract([3, 4], [3], prior)
        x = torch.zeros(16, device=DEV)
        g = torch.cuda.CUDAGraph()
        codes = []
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            for call in (fit_raw(slots[:1], stream=torch.cuda.current_stream()), sub_raw([3], [3], stream=torch.cuda.current_stream())):
                try:
                    call()
                except _capi.FFLError as err:
                    codes.append((err.code, "capturing" in str(err)))
            x += 1
        g.replay()
        torch.cuda.synchronize()
        assert codes == [(STATE, True)] * 2 and float(x.sum()) == 16.0
        # nothing was queued by a refused call: fields and records are what they were, slots 8.. still hold nothing
        assert rec_bytes(ctx.pass1_results(slots, 1.0)) == before
        assert [ctx.download_flow(s).tobytes() for s in slots] == [f.tobytes() for f in fields]
        refused(r"flow slot 9 holds no flow", STATE, fit_raw([9]), FIT)
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 5. ordering ----------------------------------------------------------------------------------------------------------------
def test_a_fit_behind_a_kernel_that_still_writes_the_map_needs_no_host_sync():
    w, h, n = 258, 35, 3
    fields = [field(w, h, 120 + i) for i in range(n)]
    maps = np.stack([random_map(w, h, 120 + i) for i in range(n)])
    side = torch.cuda.Stream(device=DEV)
    with context(w, h) as ctx:
        ctx.import_flows(dev(np.stack(fields)), [0, 1, 2])
        m = torch.zeros((n, h, w), dtype=torch.uint8, device=DEV)
        out = torch.full((n * REC,), 0xA5, dtype=torch.uint8, device=DEV)
        sums = torch.full((n, 12), NAN, dtype=torch.float64, device=DEV)
        busy = torch.ones(1 << 27, device=DEV)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                m.zero_()
                for _ in range(8):
                    busy.mul_(1.0001)                     # 1 GiB of traffic each: the stream is busy ahead of the map's writer
                m.copy_(dev(maps), non_blocking=True)     # the map's writer, queued and not waited for
                ctx.motion_fit([0, 1, 2], "affine", 2, 1.0, weights=m, out=out, sums_out=sums, stream=side)
                m.zero_()                                 # runs behind the call's reads of the map
                rec, got = records(out, n), sums.cpu().numpy()   # run behind the call's writes
                first = fit(ctx, [0, 1, 2], "affine", 1, 1.0, dev(maps))[0]
                for i in range(n):
                    mr.check_sums(got[i], fields[i], maps[i], mr.six(first[i]), 1.0)
                    assert rec[i].tobytes() == _capi.motion_solve(got[i], "affine").tobytes()
                out.fill_(0xA5)
        torch.cuda.current_stream().wait_stream(side)
        assert ctx.graph_stats()["capture_failures"] == 0


# ---- 6. the schedule ------------------------------------------------------------------------------------------------------------
SW, SH, SB = 256, 256, 8


def engine_ctx():
    return _capi.Context(SW, SH, max_batch=SB, frame_slots=pipeline.min_frame_slots(SB, 2), flow_slots=pipeline.min_flow_slots(SB, 2))


def axes_records(t, n):
    return np.frombuffer(t.cpu().numpy().tobytes(), _capi.PASS2_AXES_DTYPE, n)


def test_process_chunk_with_compensation_is_the_hand_made_sequence():
    n = 19
    fr = list(sine_translate_frames(n + 1, SW, SH, seed=3))
    with engine_ctx() as ctx:
        eng = pipeline.PairEngine(ctx)
        mo = pipeline.motion_buffer(ctx, n)
        flows = torch.empty((n, SH, SW, 2), dtype=torch.float32, device=DEV)
        buf = eng.process_chunk(fr, False, 7.0, post_out=True, axes=True, compensate="translation", motion_out=mo, flows_out=flows)
        got, models = axes_records(buf, n), pipeline.motion_records(mo, n)
        comps, recs = eng.process_chunk(fr, False, 7.0, axes=True, compensate="translation")     # the host schedule
        assert np.ascontiguousarray(comps).tobytes() == np.stack([got[k] for k in ("dot", "tangential", "shift_x", "shift_y")], axis=1).tobytes()
        assert ctx.graph_stats()["capture_failures"] == 0
    assert (models["status"] == mr.OK).all() and (models["model"] == 0).all() and (models["sw"] > 0).all()
    # by hand: every pair's raw field, then fit -> subtract in place -> the window call over the whole chunk
    with _capi.Context(SW, SH, max_batch=32, frame_slots=n + 1, flow_slots=32) as one:
        one.upload_frames(0, fr)
        slots = list(range(n))
        one.flow_pairs(list(range(n)), list(range(1, n + 1)), slots)
        raw = [one.download_flow(s) for s in slots]
        m2 = one.motion_fit(slots, "translation", 3, 1.0)
        one.motion_subtract(slots, slots, m2)
        want = torch.empty(n * 80, dtype=torch.uint8, device=DEV)
        one.radial_window_axes(slots, 0, n, want, 6, 7.0, False)
        assert records(m2, n).tobytes() == models.tobytes()
        assert axes_records(want, n).tobytes() == got.tobytes()
        assert rec_bytes(one.pass1_results(slots, 7.0)) == rec_bytes(recs)
        for j in (0, 7, 8, n - 1):                        # flows_out holds the compensated fields
            assert flows[j].cpu().numpy().tobytes() == one.download_flow(j).tobytes() == mr.subtract(raw[j], mr.six(models[j])).tobytes()
    # the fitted pan is the synthetic clip's: the texture moves by (dx_t - dx_{t+1}) and the flow is its negative
    assert np.abs(models["a0"]).max() < 4.0 and np.abs(models["a0"]).max() > 0.5


def test_process_chunk_without_the_keyword_is_todays():
    """the committed 256x256 golden (64 pairs of seed 1, made by the CPU oracle) through a B = 8 engine, and the bytes of the
    call with compensate=None"""
    n = 64
    fr = sine_translate_frames(n + 1, SW, SH, seed=1)
    gold = golden_check.load_golden(SW, SH, n, 1)
    assert gold is not None
    with engine_ctx() as ctx:
        eng = pipeline.PairEngine(ctx)
        dots, recs = eng.process_chunk(list(fr))
        d2, r2 = eng.process_chunk(list(fr), compensate=None)
        assert np.asarray(dots).tobytes() == np.asarray(d2).tobytes() and rec_bytes(recs) == rec_bytes(r2)
        with pytest.raises(ValueError, match="motion_out needs compensate="):
            eng.process_chunk(list(fr), motion_out=pipeline.motion_buffer(ctx, n))
        with pytest.raises(ValueError, match="compensate= together with weights='consistency' is not supported"):
            eng.process_chunk(list(fr), weights="consistency", compensate="translation")
        for run in (pipeline.process_chunk_sharded, pipeline.process_chunk_sharded_halo):
            with pytest.raises(ValueError, match="the sharded schedules run on the raw fields"):
                run(None, list(fr), 0, 1, lambda o: [o], compensate="translation")
        with pytest.raises(ValueError, match="the sharded schedules run on the raw fields"):
            pipeline.process_chunk_local_ranks([None], list(fr), compensate="translation")
        assert ctx.graph_stats()["capture_failures"] == 0
    status, detail = golden_check.check_batch(gold, fr, recs, dots)
    if status is None:
        pytest.skip(f"golden comparison not possible here: {detail}")
    assert status is True, detail


def test_process_flows_takes_a_pan_out_of_the_shift_components():
    """Fields k_j * (xc, yc) + (3.25, -1.5), k_j = (j + 1) / 64: every sample is a multiple of 1 / 128 that float32 holds exactly.

    Pass 1 of the fit has exact sums (multiples of 2^-7 far below 2^46), the zoom part cancels by symmetry, and a0 = 3.25 *
    N / N exactly.  A later pass weights with rho and its terms round: with depth = post_ref.radial_depth, S and Su are within
    depth * u and (depth + 1) * u of their exact values relative to sum |term|, the quotient adds u, and the exact quotient is
    3.25 when the prior is (the zoom part still cancels: rho is even), so |a0 - 3.25| <= E = (2 * depth + 2) * u * max|u|.  A
    prior off by e moves the exact quotient by at most 2 e (|d rho / d ru * ru| <= 2 rho), so three passes stay within 7 E,
    about 1e-12 here.  float32(u - a0) is then the pan-free sample itself wherever 7 E is below a quarter of its float32
    spacing; the smallest sample is 2^-7 with spacing 2^-30, so every compensated field IS the pan-free field, and the
    bound on shift_x and shift_y against the pan-free run is zero: the same bits.  The uncompensated run in pov_mode (wx =
    wy = 1) differs from it by the mean of the pan itself, within the summation bound of the two means."""
    n = 11
    xc, yc = mr.coords(SW, SH)
    free = np.stack([np.stack([np.broadcast_to(xc * ((j + 1) / 64.0), (SH, SW)), np.broadcast_to(yc * ((j + 1) / 64.0), (SH, SW))], axis=-1)
                     for j in range(n)]).astype(np.float32)
    pan = np.array([3.25, -1.5], np.float32)
    moved = free + pan
    assert np.array_equal(moved.astype(np.float64), free.astype(np.float64) + pan.astype(np.float64))
    depth = pr.radial_depth(SW, SH)
    E = (2 * depth + 2) * pr.U * float(np.abs(moved).max())
    assert 7 * E < 2.0 ** -33
    with engine_ctx() as ctx:
        eng = pipeline.PairEngine(ctx)
        mo = pipeline.motion_buffer(ctx, n)
        a, _ = pipeline.post_records(eng.process_flows(dev(moved), True, BIG, post_out=True, axes=True, compensate="translation", motion_out=mo), axes=True)
        b, _ = pipeline.post_records(eng.process_flows(dev(free), True, BIG, post_out=True, axes=True), axes=True)
        c, _ = pipeline.post_records(eng.process_flows(dev(moved), True, BIG, post_out=True, axes=True), axes=True)
        a_host, _ = eng.process_flows(dev(moved), True, BIG, axes=True, compensate={"model": "translation", "iterations": 3, "tau": 1.0})
        models = pipeline.motion_records(mo, n)
        assert ctx.graph_stats()["capture_failures"] == 0
    assert np.abs(models["a0"] - 3.25).max() <= 7 * E and np.abs(models["b0"] + 1.5).max() <= 7 * E, models
    assert a.tobytes() == b.tobytes() == np.ascontiguousarray(a_host).tobytes()
    for j in range(n):
        for col, p in ((2, 3.25), (3, -1.5)):
            bound = pr.sum_bound(1, depth) * (float(np.abs(moved[j, ..., col - 2]).mean()) + float(np.abs(free[j, ..., col - 2]).mean()))
            assert abs((c[j, col] - b[j, col]) - p) <= bound, (j, col, c[j, col], b[j, col])
            assert abs(a[j, col] - b[j, col]) == 0.0 and abs(c[j, col] - b[j, col]) > 1.0


def test_precompute_all_under_hip_compensate():
    """the drop-in call: every dict and its "flow" are those of the compensated field"""
    from funscript_flow_amd import backend
    w, h, n = 64, 48, 5
    fr = list(sine_translate_frames(n + 1, w, h, seed=2))
    pairs = list(zip(fr[:-1], fr[1:]))
    raw = [np.asarray(r["flow"]).copy() for r in backend.precompute_all(pairs, {"backend": "HIP"})]
    got = backend.precompute_all(pairs, {"backend": "HIP", "hip_compensate": {"model": "rigid", "iterations": 2, "tau": 0.5}})
    flows = [np.asarray(r["flow"]).copy() for r in got]
    with context(w, h) as one:
        slots = list(range(n))
        one.import_flows(dev(np.stack(raw)), slots)
        models = one.motion_fit(slots, "rigid", 2, 0.5)
        one.motion_subtract(slots, slots, models)
        want = one.pass1_results(slots, 7.0)
        for j in range(n):
            assert flows[j].tobytes() == one.download_flow(j).tobytes() != raw[j].tobytes(), j
            x, y, d, mm, cut = want[j]
            assert (int(got[j]["pos_center"][0]), int(got[j]["pos_center"][1]), bool(got[j]["cut"])) == (x, y, cut), j
            assert np.float32(got[j]["mean_mag"]).tobytes() == np.float32(mm).tobytes(), j
    with pytest.raises(ValueError, match="motion model must be one of"):
        backend.precompute_all(pairs, {"backend": "HIP", "hip_compensate": "zoom"})
