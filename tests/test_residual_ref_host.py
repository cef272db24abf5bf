"""Host side of the photometric-residual maps: known answers of the numpy restatement
tests/residual_ref.py, the conditions the GPU tests' synthetic inputs must meet, and what needs no device of the binding and
the schedule -- ffl_residual_params_check, the exports, MAP_MODES and the params keys."""
import ctypes as C

import numpy as np
import pytest

import residual_ref as rr
from funscript_flow_amd import _capi, pipeline

F32 = np.float32
SEEDS = rr.SEEDS   # the seeds the GPU tests use at every size of rr.SIZES (n = 5 items)


def gid(s):
    return f"{s[0]}x{s[1]}"


# ---- the conditions on the synthetic inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_synthetic_inputs_exercise_every_outcome(size, seed):
    w, h = size
    I0, I1, F = rr.synthetic(w, h, seed)
    assert I0.dtype == np.uint8 and I1.dtype == np.uint8 and F.dtype == F32 and F.shape == (h, w, 2)
    W, outside = rr.residual(I0, I1, F, with_outside=True)
    out_share, zero_inside = float(outside.mean()), float(((W == 0) & ~outside).mean())
    full, distinct = float((W == 255).mean()), len(np.unique(W))
    print(f"{w}x{h} seed {seed}: outside {100 * out_share:.1f} %, inside with 0 {100 * zero_inside:.1f} %, 255 {100 * full:.1f} %, "
          f"{distinct} distinct values")
    assert 0.03 <= out_share <= 0.40
    assert zero_inside >= 0.02
    assert full >= 0.05
    assert distinct >= 64
    H = rr.residual(I0, I1, F, soft=0)
    assert set(np.unique(H)) == {0, 255}


@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_hostile_inputs_hold_what_they_claim(size):
    w, h = size
    I0, I1, F = rr.hostile(w, h, SEEDS[0])
    assert np.isnan(F).any() and np.isposinf(F).any() and np.isneginf(F).any() and (np.abs(F[np.isfinite(F)]) >= 1e30).any()
    assert (F == F32(rr.DENORMAL)).any() and 0 < float(F32(rr.DENORMAL)) < np.finfo(F32).tiny
    W, outside = rr.residual(I0, I1, F, with_outside=True)
    for y, x in ((1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (2, 4), (3, 1), (3, 2), (3, 3)):
        assert outside[y, x] and W[y, x] == 0
    y, x = np.mgrid[0:h, 0:w]
    px, py = x.astype(F32) + F[..., 0], y.astype(F32) + F[..., 1]
    assert ((px == w - 1) & (py == h - 1)).sum() >= 2                       # the far corner, exactly
    assert ((px == w - 1) & (py != np.floor(py)) & ~outside).any()          # the last column, a fractional row
    assert ((py == h - 1) & (px != np.floor(px)) & ~outside).any()          # the last row, a fractional column
    assert ((px > 0) & (px < np.finfo(F32).tiny)).any()                     # column 0 with ax a denormal
    for edge in (I0[:, 0], I0[:, w - 1], I0[0, :], I0[h - 1, :]):
        assert (edge == 0).any() or (edge == 255).any()
    assert (I1 == 0).any() and (I1 == 255).any()


# ---- known answers, exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("size", rr.SIZES, ids=gid)
def test_true_integer_flow_is_255_exactly_where_it_lands_inside(size, soft):
    w, h = size
    dx, dy = 3, -2
    I0 = rr.to_u8(rr.texture(w, h, 11))
    I1 = rr.displaced(I0, dx, dy)
    F = np.zeros((h, w, 2), F32)
    F[...] = (dx, dy)
    W, outside = rr.residual(I0, I1, F, soft=soft, with_outside=True)
    y, x = np.mgrid[0:h, 0:w]
    inside = (x + dx >= 0) & (x + dx <= w - 1) & (y + dy >= 0) & (y + dy <= h - 1)
    assert (outside == ~inside).all() and ((W == 255) == inside).all() and ((W == 0) == ~inside).all()
    assert int((W == 255).sum()) == (w - dx) * (h + dy)
    W0 = rr.residual(I0, I1, np.zeros((h, w, 2), F32), soft=soft)
    print(f"{w}x{h} soft {soft}: mean W under the true flow {W.mean():.1f}, under zero flow {W0.mean():.1f}")
    assert W0.mean() < W.mean()


def test_interpolation_rounding_and_threshold_by_hand():
    """A 16x16 frame of I0 = 100 everywhere (g = 0, thr = beta = 4) and I1 = 100 but for I1[3][5] = 108.
    F[3][4] = (0.5, 0): ic = 100 + 0.5 * 8 = 104, a = 4, q = 1 - 4 / 4 = 0 -> 0; hard: 4 < 4 fails -> 0.
    F[3][5] = (0, 0): a = 8 -> 0.  F[3][6] = (-0.75, 0) and F[3][7] = (-1.75, 0): px = 5.25, ic = 108 + 0.25 * (100 - 108) = 106,
    a = 6 -> 0.  F[4][5] = (0, -0.25): py = 3.75, t = 108 (row 3), s = 100 (row 4), ic = 108 + 0.75 * (100 - 108) = 102, a = 2,
    q = 0.5, q * 255 + 0.5 = 128 -> 128; hard: 255.  F[2][5] = (0, 0.125): t = 100, s = 108, ic = 101, a = 1, q = 0.75,
    191.25 + 0.5 -> 191; hard: 255.  Every other pixel reads 100 against 100: 255."""
    w, h = 16, 16
    I0 = np.full((h, w), 100, np.uint8)
    I1 = I0.copy()
    I1[3, 5] = 108
    F = np.zeros((h, w, 2), F32)
    F[3, 4], F[3, 6], F[3, 7], F[4, 5], F[2, 5] = (0.5, 0), (-0.75, 0), (-1.75, 0), (0, -0.25), (0, 0.125)
    W = rr.residual(I0, I1, F, alpha=0.5, beta=4.0, soft=1)
    H = rr.residual(I0, I1, F, alpha=0.5, beta=4.0, soft=0)
    want = {(4, 3): (0, 0), (5, 3): (0, 0), (6, 3): (0, 0), (7, 3): (0, 0), (5, 4): (128, 255), (5, 2): (191, 255)}
    for (x, y), (s, hard) in want.items():
        assert (W[y, x], H[y, x]) == (s, hard), (x, y, W[y, x], H[y, x])
    rest = np.delete(W.ravel(), [y * w + x for x, y in want])
    assert (rest == 255).all()


def test_gradient_scales_the_threshold_and_alpha_zero_is_beta():
    """thr = alpha * (|gx| + |gy|) + beta with clamped central differences: on a ramp I0[y][x] = 10 * x + 3 * y, gx = 20 inside and
    10 in the first and last column, gy = 6 inside and 3 in the first and last row."""
    w, h = 16, 16
    y, x = np.mgrid[0:h, 0:w]
    I0 = (10 * x + 3 * y).astype(np.uint8)
    thr = rr.threshold(I0, 0.5, 4.0)
    assert thr.dtype == F32
    assert thr[5, 5] == 0.5 * 26 + 4 and thr[5, 0] == 0.5 * 16 + 4 and thr[5, w - 1] == 0.5 * 16 + 4
    assert thr[0, 5] == 0.5 * 23 + 4 and thr[h - 1, 5] == 0.5 * 23 + 4 and thr[0, 0] == 0.5 * 13 + 4
    assert (rr.threshold(I0, 0.0, 7.5) == F32(7.5)).all()
    for seed in SEEDS[:2]:
        I0, I1, F = rr.synthetic(130, 17, seed)
        a0 = rr.residual(I0, I1, F, alpha=0.0, beta=9.0, soft=0)
        flat = rr.residual(np.full_like(I0, 7), I1, F, alpha=16.0, beta=9.0, soft=0)   # g = 0 everywhere: thr = beta again
        ref = rr.residual(np.full_like(I0, 7), I1, F, alpha=0.0, beta=9.0, soft=0)
        assert (flat == ref).all() and set(np.unique(a0)) <= {0, 255}


@pytest.mark.parametrize("soft", [1, 0])
def test_gate_is_min(soft):
    w, h = 130, 17
    I0, I1, F = rr.synthetic(w, h, 1)
    g = np.random.default_rng(5).integers(0, 256, (h, w)).astype(np.uint8)
    W = rr.residual(I0, I1, F, soft=soft)
    G = rr.residual(I0, I1, F, soft=soft, gate=g)
    assert (G == np.minimum(W, g)).all() and (G != W).any() and (G != g).any()
    assert (rr.residual(I0, I1, F, soft=soft, gate=np.full((h, w), 255, np.uint8)) == W).all()
    assert (rr.residual(I0, I1, F, soft=soft, gate=np.zeros((h, w), np.uint8)) == 0).all()


# ---- the binding and the schedule, without a device ----------------------------------------------------------------------------
def test_exports_defaults_and_record():
    L = _capi.load()
    for name in ("ffl_residual_default_params", "ffl_residual_params_check", "ffl_residual_weights"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    p = _capi.ResidualParams()
    assert C.sizeof(p) == 12 and p.as_dict() == {"alpha": 0.5, "beta": 4.0, "soft": 1}
    assert (F32(p.alpha), F32(p.beta), p.soft) == (rr.ALPHA, rr.BETA, rr.SOFT)
    assert _capi.RECORDS["ffl_residual_params"] is _capi.ResidualParams
    assert L.ffl_residual_default_params(None) == _capi.FFL_ERR_INVALID
    with pytest.raises(ValueError, match="unknown residual parameter 'gamma'"):
        _capi.ResidualParams(gamma=1)


def test_params_check_accepts_and_refuses_as_the_abi_says():
    ok = [{}, {"alpha": 0.0}, {"alpha": 16.0}, {"beta": 255.0}, {"beta": 1e-6}, {"soft": 0}, {"alpha": 3.0, "beta": 10.0, "soft": 0}]
    for kw in ok:
        p = _capi.residual_choice(kw)
        assert isinstance(p, _capi.ResidualParams)
        _capi.residual_params_check(p)
    assert _capi.residual_choice(None).as_dict() == _capi.ResidualParams().as_dict()
    given = _capi.ResidualParams(soft=0)
    assert _capi.residual_choice(given) is given
    bad = [({"alpha": -0.001}, r"alpha = -0\.001 outside 0\.\.16"), ({"alpha": 16.5}, r"alpha = 16\.5 outside 0\.\.16"),
           ({"alpha": float("nan")}, r"alpha = nan outside"), ({"alpha": float("inf")}, r"alpha = inf outside"),
           ({"beta": 0.0}, r"beta = 0 outside 0 < beta <= 255"), ({"beta": -1.0}, r"beta = -1 outside"),
           ({"beta": 255.5}, r"beta = 255\.5 outside 0 < beta <= 255"), ({"beta": float("nan")}, r"beta = nan outside"),
           ({"beta": float("inf")}, r"beta = inf outside"), ({"soft": 2}, r"soft = 2 is neither"), ({"soft": -1}, r"soft = -1 is neither")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_residual_params_check: " + match):
            _capi.residual_choice(kw)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.residual_params_check(None)


def test_pipeline_keys_without_a_device():
    assert pipeline.MAP_MODES == ("consistency", "residual") and pipeline.WEIGHT_MODES == ("consistency",)
    assert pipeline.consistency_kwargs(None, {"hip_weights": "residual"}) == {"weights": "residual", "residual": None, "weights_gate": None}
    assert pipeline.consistency_kwargs(None, {"hip_weights": "residual", "hip_residual": {"soft": 0}}) == {
        "weights": "residual", "residual": {"soft": 0}, "weights_gate": None}
    with pytest.raises(ValueError, match="hip_residual needs hip_weights = 'residual'"):
        pipeline.consistency_kwargs(None, {"hip_residual": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_residual needs hip_weights = 'residual', got 'consistency'"):
        pipeline.consistency_kwargs(None, {"hip_weights": "consistency", "hip_residual": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_consistency needs hip_weights = 'consistency', got 'residual'"):
        pipeline.consistency_kwargs(None, {"hip_weights": "residual", "hip_consistency": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_center together with hip_weights"):
        pipeline.center_kwargs({"hip_center": "variance", "hip_weights": "residual"})
    with pytest.raises(ValueError, match="flows_to_actions: hip_weights = 'residual' needs the frames.*Context.residual_weights"):
        pipeline.flows_to_actions(None, [], 30.0, 10, {"hip_weights": "residual"})
    with pytest.raises(ValueError, match="0 chunks of flows for a plan of 1 chunks"):   # a map is no mode name: not refused as one
        pipeline.flows_to_actions(None, [], 30.0, 10, {"hip_weights": np.ones((4, 4), np.uint8)})
    for fn, args in ((pipeline.process_chunk_sharded, (None, [], 0, 1, None)), (pipeline.process_chunk_sharded_halo, (None, [], 0, 1, None)),
                     (pipeline.process_chunk_local_ranks, ([], []))):
        with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
            fn(*args, weights="residual")
