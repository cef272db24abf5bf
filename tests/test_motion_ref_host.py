"""Host side of the global-motion fit: ffl_motion_solve -- the source the device's solve
kernel compiles -- bit for bit against the restated solve of tests/motion_ref.py, known answers on the restatement, and the
host checks of the C ABI.  No device is needed."""
import math

import numpy as np
import pytest

import motion_ref as mr
from funscript_flow_amd import _capi
from post_ref import P2_STRIP, ROW_GROUP

NAN = float("nan")


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def field_sums(w, h, seed, weighted=True):
    """the exact sums of a random field under a random map: a well-conditioned system"""
    rng = np.random.default_rng(seed)
    f = rng.standard_normal((h, w, 2)).astype(np.float32) * 3
    W = rng.integers(0, 256, (h, w)).astype(np.uint8) if weighted else None
    return [s for s, _ in mr.sums_exact(f, W)]


# ---- the solve, bit for bit ---------------------------------------------------------------------------------------------------
def test_the_binding_and_the_restatement_agree_on_the_record():
    assert _capi.MOTION_DTYPE == mr.RECORD and _capi.MOTION_DTYPE.itemsize == 64
    assert _capi.MOTION_MODELS == mr.MODELS and _capi.MOTION_SUMS == mr.SUMS and len(mr.SUMS) == 12
    assert _capi.MOTION_STATUS.index("ok") == mr.OK and _capi.MOTION_STATUS.index("empty") == mr.EMPTY
    assert _capi.MOTION_STATUS.index("degenerate") == mr.DEGENERATE


@pytest.mark.parametrize("model", mr.MODELS)
def test_solve_matches_the_restatement_on_well_conditioned_sums(model):
    for seed, (w, h) in enumerate([(16, 16), (19, 17), (64, 48), (129, 17), (33, 127)] * 4):
        s = field_sums(w, h, seed, weighted=seed % 3 != 0)
        got, want = _capi.motion_solve(s, model), mr.solve(s, model)
        assert same(got, want), (model, w, h, got, want)
        assert got["status"] == mr.OK and got["model"] == mr.MODELS.index(model) and got["sw"] == s[0]
    rng = np.random.default_rng(7)   # sums that come from no field at all: the arithmetic is still the same
    for _ in range(200):
        s = rng.standard_normal(12) * 10.0 ** rng.integers(-3, 6)
        s[[0, 3, 5]] = np.abs(s[[0, 3, 5]]) + 1.0
        assert same(_capi.motion_solve(s, model), mr.solve(s, model)), (model, s)


@pytest.mark.parametrize("model", mr.MODELS)
def test_solve_of_an_empty_fit(model):
    for s in (np.zeros(12), np.array([0.0] + [3.0] * 11), np.array([-0.0] + [NAN] * 11)):
        got = _capi.motion_solve(s, model)
        assert same(got, mr.solve(s, model))
        assert got["status"] == mr.EMPTY and mr.six(got) == [0.0] * 6
        assert all(math.copysign(1.0, v) == 1.0 for v in mr.six(got))   # +0.0


@pytest.mark.parametrize("model", mr.MODELS)
def test_solve_of_collinear_support(model):
    """All the weight on one row: yc is constant on the support, so AFFINE's third pivot vanishes and the translation comes
    out.  RIGID and SIMILARITY stay determined -- a rotation and a zoom show in how v and u change ALONG the row, and their
    pivot D = sum omega * ((xc - mean)^2 + (yc - mean)^2) keeps the row's spread in x -- and degenerate only when the support
    is a single point (below)."""
    f = np.random.default_rng(3).standard_normal((17, 40, 2)).astype(np.float32)
    W = np.zeros((17, 40), np.uint8)
    W[5, :] = 200
    s = [v for v, _ in mr.sums_exact(f, W)]
    got, tr = _capi.motion_solve(s, model), _capi.motion_solve(s, "translation")
    assert same(got, mr.solve(s, model))
    if model == "affine":
        assert got["status"] == mr.DEGENERATE and mr.six(got) == mr.six(tr) and got["a1"] == got["a2"] == got["b1"] == got["b2"] == 0.0
    else:
        assert got["status"] == mr.OK
    if model in ("rigid", "similarity"):   # a known rotation (and zoom) is read off the one row exactly
        mm = [0.5, 0.0, -0.25, -1.5, 0.25, 0.0] if model == "rigid" else [0.5, 0.125, -0.25, -1.5, 0.25, 0.125]
        mu, mv = mr.model_flow(mm, 40, 17)
        g = np.stack([mu, mv], axis=-1).astype(np.float32)
        rec = _capi.motion_solve([v for v, _ in mr.sums_exact(g, W)], model)
        assert rec["status"] == mr.OK and mr.six(rec) == mm
    W = np.zeros((17, 40), np.uint8)
    W[5, 7] = 1                                         # one pixel: every second moment about the mean is zero
    s = [v for v, _ in mr.sums_exact(f, W)]
    got = _capi.motion_solve(s, model)
    assert same(got, mr.solve(s, model)) and got["status"] == (mr.OK if model == "translation" else mr.DEGENERATE)
    assert (got["a0"], got["b0"]) == (float(f[5, 7, 0]), float(f[5, 7, 1]))


@pytest.mark.parametrize("model", mr.MODELS)
def test_solve_of_nan_and_inf_sums(model):
    base = field_sums(64, 48, 11)
    for k in range(12):
        for bad in (NAN, math.inf, -math.inf):
            s = list(base)
            s[k] = bad
            got = _capi.motion_solve(s, model)
            assert same(got, mr.solve(s, model)), (model, k, bad, got)
    got = _capi.motion_solve([NAN] * 12, model)
    assert got["status"] == (mr.OK if model == "translation" else mr.DEGENERATE) and math.isnan(got["a0"]) and math.isnan(got["b0"])
    assert got["a1"] == got["a2"] == got["b1"] == got["b2"] == 0.0


def test_solve_refusals():
    with pytest.raises(ValueError, match="motion model must be one of"):
        _capi.motion_solve(np.zeros(12), "zoom")
    with pytest.raises(ValueError, match="12 sums are needed"):
        _capi.motion_solve(np.zeros(11), "affine")
    L = _capi.load()
    out = np.zeros((), _capi.MOTION_DTYPE)
    s = np.zeros(12)
    assert L.ffl_motion_solve(s.ctypes.data_as(_capi._dp), 4, out.ctypes.data) == _capi.FFL_ERR_INVALID
    assert b"rule C2: model = 4" in L.ffl_last_error(None)
    assert L.ffl_motion_solve(None, 0, out.ctypes.data) == _capi.FFL_ERR_INVALID
    assert L.ffl_motion_solve(s.ctypes.data_as(_capi._dp), 0, None) == _capi.FFL_ERR_INVALID


# ---- known answers on the restatement -----------------------------------------------------------------------------------------
def affine_field(w, h, m):
    """an exactly affine float32 field: coefficients in eighths and half-integer coordinates make every sample a multiple of
    1/16 below 2^10, which float32 holds exactly"""
    mu, mv = mr.model_flow(m, w, h)
    f = np.stack([mu, mv], axis=-1).astype(np.float32)
    assert np.array_equal(f[..., 0].astype(np.float64), mu) and np.array_equal(f[..., 1].astype(np.float64), mv)
    return f


@pytest.mark.parametrize("size", [(16, 16), (19, 17), (129, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_an_exactly_affine_field_returns_its_six_numbers(size):
    w, h = size
    m = [1.25, 0.125, -0.25, -2.5, 0.375, 0.5]
    f = affine_field(w, h, m)
    W = np.random.default_rng(w).integers(1, 256, (h, w)).astype(np.uint8)   # an asymmetric map: Sx, Sy, Sxy are not zero
    s = [v for v, _ in mr.sums_exact(f, W)]
    assert s[1] != 0.0 and s[2] != 0.0 and s[4] != 0.0
    rec = mr.solve(s, "affine")
    tol = mr.affine_tolerance(s, m)
    assert rec["status"] == mr.OK and tol < 1e-9
    assert max(abs(a - b) for a, b in zip(mr.six(rec), m)) <= tol, (mr.six(rec), m, tol)
    assert same(rec, _capi.motion_solve(s, "affine"))
    # without a map the centred coordinates decouple the system (Sx = Sy = Sxy = 0 exactly) and every quotient is exact
    s = [v for v, _ in mr.sums_exact(f)]
    assert s[1] == s[2] == s[4] == 0.0 and mr.six(mr.solve(s, "affine")) == m
    # the sub-models return theirs: a rotation plus a pan is RIGID's, with a zoom SIMILARITY's
    for model, mm in (("rigid", [0.5, 0.0, -0.25, -1.5, 0.25, 0.0]), ("similarity", [0.5, 0.125, -0.25, -1.5, 0.25, 0.125])):
        assert mr.six(mr.solve([v for v, _ in mr.sums_exact(affine_field(w, h, mm))], model)) == mm


def test_iterations_pull_the_pan_out_from_under_a_block_of_outliers():
    w, h = 64, 48
    pan = (3.25, -1.5)
    f = np.empty((h, w, 2), np.float32)
    f[...] = pan
    f[:h // 2, :w // 2] = (-8.0, 6.0)                   # a quarter of the frame moves otherwise
    recs = mr.fit(f, "translation", 3, 1.0)
    err = [math.hypot(r["a0"] - pan[0], r["b0"] - pan[1]) for r in recs]
    assert err[0] > 1.0 and err[2] < err[1] < err[0], err
    W = np.full((h, w), 255, np.uint8)
    W[:h // 2, :w // 2] = 0                             # a zero-weight map over the block: the pan, exactly
    for r in mr.fit(f, "translation", 3, 1.0, W):
        assert (r["a0"], r["b0"]) == pan and r["sw"] == 255.0 * (w * h * 3 // 4)


def test_a_nan_changes_nothing_under_any_weight():
    rng = np.random.default_rng(5)
    w, h = 40, 19
    f = rng.standard_normal((h, w, 2)).astype(np.float32)
    W = rng.integers(1, 256, (h, w)).astype(np.uint8)
    prior = [0.25, 0.0, 0.0, -0.5, 0.0, 0.0]
    hole = W.copy()
    hole[7, 11] = 0
    want = [s for s, _ in mr.sums_exact(f, hole, prior, 2.0)]
    for bad in (NAN, math.inf, -math.inf):
        for comp in (0, 1):
            g = f.copy()
            g[7, 11, comp] = bad
            assert [s for s, _ in mr.sums_exact(g, hole, prior, 2.0)] == want      # under a zero weight
            assert [s for s, _ in mr.sums_exact(g, W, prior, 2.0)] == want         # under a non-zero weight: excluded all the same
            assert all(np.isfinite(t).all() for t in mr.terms(g, W, prior, 2.0))


def test_subtracting_a_zero_model_is_a_copy_and_one_rounding():
    rng = np.random.default_rng(9)
    f = rng.standard_normal((17, 19, 2)).astype(np.float32)
    f[3, 4] = (NAN, math.inf)
    assert same(mr.subtract(f, [0.0] * 6), f)
    m = [3.25, 0.0, 0.0, -1.5, 0.0, 0.0]
    g = mr.subtract(f, m)
    assert g[0, 0, 0] == np.float32(np.float64(f[0, 0, 0]) - 3.25) and math.isnan(g[3, 4, 0]) and g[3, 4, 1] == math.inf


# ---- host checks ----------------------------------------------------------------------------------------------------------------
def test_default_params_are_rule_c9():
    p = _capi.MotionParams()
    assert p.as_dict() == {"model": "translation", "iterations": 3, "tau": 1.0}
    _capi.motion_params_check(p)
    for model in _capi.MOTION_MODELS:
        for it in (1, 8):
            for tau in (1e-6, 1.0, 1e6):
                _capi.motion_params_check(_capi.MotionParams(model=model, iterations=it, tau=tau))
    assert _capi.motion_choice("rigid").as_dict()["model"] == "rigid"
    assert _capi.motion_choice({"model": "affine", "tau": 2.0}).as_dict() == {"model": "affine", "iterations": 3, "tau": 2.0}


@pytest.mark.parametrize("kw, rule", [
    ({"iterations": 0}, r"rule C7: iterations = 0 outside 1\.\.8"),
    ({"iterations": 9}, r"rule C7: iterations = 9 outside 1\.\.8"),
    ({"tau": 0.0}, r"rule C3: tau = 0 outside 0 < tau <= 1e6"),
    ({"tau": -1.0}, r"rule C3: tau = -1 outside"),
    ({"tau": 2e6}, r"rule C3: tau = 2e\+06 outside"),
    ({"tau": NAN}, r"rule C3: tau = nan outside"),
    ({"tau": math.inf}, r"rule C3: tau = inf outside"),
])
def test_params_check_names_its_rule(kw, rule):
    with pytest.raises(ValueError, match=rule) as e:
        _capi.motion_params_check(_capi.MotionParams(**kw))
    assert "ffl_motion_params_check" in str(e.value)


def test_params_check_refuses_an_unknown_model_and_null():
    p = _capi.MotionParams()
    for bad in (-1, 4):
        p.model = bad
        with pytest.raises(ValueError, match=rf"rule C2: model = {bad} is none of"):
            _capi.motion_params_check(p)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.motion_params_check(None)
    with pytest.raises(ValueError, match="motion model must be one of"):
        _capi.MotionParams(model="zoom")
    with pytest.raises(ValueError, match="unknown motion parameter"):
        _capi.MotionParams(sigma=1.0)


def test_extra_bytes_is_twelve_partials_per_workgroup_of_the_radial_grid():
    def blocks(w, h):   # ffl_radial_blocks
        return -(-(-(-w // P2_STRIP) * -(-h // ROW_GROUP)) // 4)
    for w, h in ((16, 16), (19, 17), (256, 256), (1920, 1080), (3840, 2160)):
        assert _capi.motion_extra_bytes(w, h) == 12 * blocks(w, h) * 8 * _capi.FFL_MAX_BATCH
        assert _capi.motion_extra_bytes(w, h) == 3 * _capi.axes_extra_bytes(w, h)
    with pytest.raises(_capi.FFLError, match="ffl_motion_extra_bytes failed"):
        _capi.motion_extra_bytes(8, 8)


def test_the_symbols_are_exported():
    L = _capi.load()
    for name in ("ffl_motion_default_params", "ffl_motion_params_check", "ffl_motion_solve", "ffl_motion_extra_bytes",
                 "ffl_motion_fit", "ffl_motion_subtract"):
        assert name in _capi.EXPORTS and hasattr(L, name)


def test_the_schedule_keywords_are_checked_without_a_device():
    from funscript_flow_amd import pipeline
    assert pipeline.compensate_kwargs({}) == {} and pipeline.compensate_kwargs({"hip_compensate": None}) == {}
    assert pipeline.compensate_kwargs({"hip_compensate": "rigid"})["compensate"].as_dict() == {"model": "rigid", "iterations": 3, "tau": 1.0}
    got = pipeline.compensate_kwargs({"hip_compensate": {"model": "affine", "iterations": 1, "tau": 0.5}})["compensate"]
    assert got.as_dict() == {"model": "affine", "iterations": 1, "tau": 0.5}
    with pytest.raises(ValueError, match=r"rule C3: tau = 0 outside"):
        pipeline.compensate_kwargs({"hip_compensate": {"tau": 0.0}})
    with pytest.raises(ValueError, match="motion model must be one of"):
        pipeline.compensate_kwargs({"hip_compensate": "zoom"})
    frames = [None] * 4
    for run in (pipeline.process_chunk_sharded, pipeline.process_chunk_sharded_halo):
        with pytest.raises(ValueError, match="the sharded schedules run on the raw fields"):
            run(None, frames, 0, 1, lambda o: [o], compensate="translation")
    with pytest.raises(ValueError, match="the sharded schedules run on the raw fields"):
        pipeline.process_chunk_local_ranks([None], frames, compensate="translation")
