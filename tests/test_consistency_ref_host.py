"""Host side of the forward-backward consistency maps: known answers of the numpy
restatement tests/consistency_ref.py computed by hand, the conditions the GPU tests' synthetic inputs must meet, and the
refusals that need no device -- ffl_consistency_params_check and the descriptor rules through the library."""
import ctypes as C

import numpy as np
import pytest

import consistency_ref as cr
from funscript_flow_amd import _capi, pipeline

F32 = np.float32
SEEDS = (0, 1, 2)   # the seeds the GPU tests use at every size of cr.SIZES
SCHEDULE_SIZE = (64, 48)


def zeros(w, h):
    return np.zeros((h, w, 2), F32)


@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("size", cr.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_fields_are_fully_consistent(size, soft):
    w, h = size
    W = cr.consistency(zeros(w, h), zeros(w, h), soft=soft)
    assert W.dtype == np.uint8 and W.shape == (h, w) and (W == 255).all()


@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("a,b", [(3, 0), (0, -2), (-5, 4), (1, 1), (129, 0), (0, 17)])
def test_integer_translation_is_255_exactly_where_it_lands_inside(a, b, soft):
    w, h = 130, 17
    F, B = zeros(w, h), zeros(w, h)
    F[...] = (a, b)
    B[...] = (-a, -b)
    W, outside = cr.consistency(F, B, soft=soft, with_outside=True)
    y, x = np.mgrid[0:h, 0:w]
    inside = (x + a >= 0) & (x + a <= w - 1) & (y + b >= 0) & (y + b <= h - 1)
    assert ((W == 255) == inside).all() and ((W == 0) == ~inside).all() and (outside == ~inside).all()
    assert int((W == 255).sum()) == max(0, w - abs(a)) * max(0, h - abs(b))


def test_rounding_on_both_sides_of_a_half():
    """F = 0, B = (bu, 0) at the pixel itself, alpha = 0, beta = 2: e2 = bu * bu, thr = 2, q = 1 - e2 / 2.
    bu = 1: q = 0.5, q * 255 = 127.5 exactly, + 0.5 = 128 -> 128.
    bu = 1 + 2^-10: e2 = 1 + 2^-9 + 2^-20 (exact in float32), q * 255 = 127.2508..., + 0.5 -> 127.
    bu = 1 - 2^-10: e2 = 1 - 2^-9 + 2^-20, q * 255 = 127.7489..., + 0.5 -> 128.
    bu = 0.5: q = 0.875, q * 255 = 223.125 -> 223.  bu = 1.5: e2 = 2.25 > thr, q < 0 -> 0.  bu = 0.0625: q * 255 = 254.50195.. -> 255."""
    w, h = 16, 16
    F, B = zeros(w, h), zeros(w, h)
    cases = {(2, 3): (1.0, 128), (4, 3): (1.0 + 2.0 ** -10, 127), (6, 3): (1.0 - 2.0 ** -10, 128), (8, 3): (0.5, 223),
             (10, 3): (1.5, 0), (12, 3): (0.0625, 255)}
    for (x, y), (bu, _) in cases.items():
        B[y, x, 0] = bu
    W = cr.consistency(F, B, alpha=0.0, beta=2.0, soft=1)
    H = cr.consistency(F, B, alpha=0.0, beta=2.0, soft=0)
    for (x, y), (bu, want) in cases.items():
        assert W[y, x] == want, (bu, W[y, x], want)
        assert H[y, x] == (255 if bu * bu < 2.0 else 0)
    assert (np.delete(W.ravel(), [y * w + x for x, y in cases]) == 255).all()


def test_landing_on_the_last_column_and_row_clamps_the_second_corner():
    """px = w - 1 exactly: x0 = w - 1, x1 = min(w, w - 1) = x0 and ax = 0; the same in y.  Nothing outside B is indexed
    (numpy would raise), and the sample is B's last pixel itself."""
    w, h = 16, 16
    F, B = zeros(w, h), zeros(w, h)
    F[5, w - 2] = (1, 0)
    F[h - 2, 7] = (0, 1)
    F[h - 3, w - 4] = (3, 2)
    B[5, w - 1] = (-1, 0)
    B[h - 1, 7] = (0, -1)
    B[h - 1, w - 1] = (-3, -2)
    W = cr.consistency(F, B, soft=0)
    assert W[5, w - 2] == 255 and W[h - 2, 7] == 255 and W[h - 3, w - 4] == 255
    # the pixels that now find a foreign backward flow under themselves: e2 = 1 (resp. 13) against thr = 0.51 (0.63)
    assert W[5, w - 1] == 0 and W[h - 1, 7] == 0 and W[h - 1, w - 1] == 0
    assert int((W == 255).sum()) == w * h - 3
    F[5, w - 2] = (1 + 2.0 ** -20, 0)   # 14 + u rounds to 15 + 2^-20, one ulp beyond the last column: outside
    assert cr.consistency(F, B, soft=0)[5, w - 2] == 0
    F[5, w - 2] = (1 + 2.0 ** -22, 0)   # 14 + u rounds to 15 exactly: inside, and e2 = 2^-44 < thr
    assert cr.consistency(F, B, soft=0)[5, w - 2] == 255


@pytest.mark.parametrize("soft", [1, 0])
def test_hostile_values_in_the_forward_field_and_in_a_corner(soft):
    w, h = 16, 16
    F, B = zeros(w, h), zeros(w, h)
    nan, inf, big, den = np.nan, np.inf, 1e30, cr.DENORMAL
    for i, val in enumerate([(nan, 0), (0, nan), (inf, 0), (0, -inf), (big, 0), (0, -big)]):
        F[1, 1 + i] = val                      # NaN fails K1's test; inf and 1e30 land outside
    F[3, 3] = (den, -den)                      # absorbed by the coordinate: lands on itself, e2 = 0
    F[5, 0] = (den, 0)                         # px = a denormal, ax = that denormal; B = 0 all round
    F[8, 4] = (0.5, 0.5)
    B[9, 5] = (nan, 0)                         # one NaN corner: the whole chain is NaN -> 0
    F[8, 8] = (0.5, 0.5)
    B[9, 9] = (big, 0)                         # bu = 2.5e29: e2 = inf and thr = inf, e2 / thr = NaN -> 0; inf < inf is false
    F[8, 12] = (0.5, 0.5)
    B[9, 13] = (0, inf)                        # bv = inf: the same
    F[12, 4] = (0.5, 0.5)
    B[13, 5] = (den, den)                      # bu = bv = a quarter denormal: e2 = 0.5, thr = 0.505: q*255 + .5 = 3.02 -> 3
    B[12, 9] = (inf, 0)                        # F = 0 there: ax = 0, t = inf + 0 * (0 - inf) = NaN -> 0
    W = cr.consistency(F, B, soft=soft)
    for i in range(6):
        assert W[1, 1 + i] == 0
    assert W[3, 3] == 255 and W[5, 0] == 255
    assert W[8, 4] == 0 and W[8, 8] == 0 and W[8, 12] == 0 and W[12, 9] == 0
    assert W[12, 4] == (3 if soft else 255)
    # with alpha = 0 the bound is 0 * inf + beta = NaN: still 0
    assert cr.consistency(F, B, alpha=0.0, soft=soft)[8, 8] == 0
    # A zero-flow pixel whose right, lower or lower-right neighbour in B is inf or NaN multiplies it by ax = 0 or ay = 0:
    # 0 * inf = NaN, so it is 0 too (the IEEE result of K2 as written); 1e30 is finite and 0 * 1e30 = 0.
    nan_neighbours = {(9, 4), (8, 5), (9, 12), (8, 13), (12, 8), (11, 9), (11, 8)}
    for y, x in nan_neighbours:
        assert W[y, x] == 0, (x, y)
    assert W[9, 8] == 255 and W[8, 9] == 255
    # the corners' own pixels (F = 0 on a hostile B) are 0; everything else is untouched
    touched = nan_neighbours | {(1, 1 + i) for i in range(6)} | {(3, 3), (5, 0), (8, 4), (8, 8), (8, 12), (12, 4), (12, 9), (9, 5),
                                                                   (9, 9), (9, 13), (13, 5)}
    for y in range(h):
        for x in range(w):
            if (y, x) not in touched:
                assert W[y, x] == 255, (x, y)
    assert W[9, 5] == 0 and W[9, 9] == 0 and W[9, 13] == 0 and W[13, 5] == 255


def test_gate_is_a_minimum():
    w, h = 130, 17
    F, B = cr.synthetic_pair(w, h, 0)
    rng = np.random.default_rng(5)
    S = rng.integers(0, 256, (h, w)).astype(np.uint8)
    S[rng.random((h, w)) < 0.3] = 0
    for soft in (1, 0):
        W, outside = cr.consistency(F, B, soft=soft, with_outside=True)
        G = cr.consistency(F, B, soft=soft, gate=S)
        assert (G == np.minimum(W, S)).all()
        assert (G[(S == 0) | outside] == 0).all()
    assert (cr.consistency(F, B, gate=np.full((h, w), 255, np.uint8)) == cr.consistency(F, B)).all()


@pytest.mark.parametrize("size", cr.SIZES + [SCHEDULE_SIZE], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("seed", SEEDS)
def test_synthetic_inputs_exercise_every_branch(size, seed):
    """what the GPU tests rely on: the soft reference map of each synthetic pair has >= 10 % zeros, >= 10 % 255s, >= 25 %
    strictly between, and >= 2 % of the pixels land outside"""
    w, h = size
    W, outside = cr.consistency(*cr.synthetic_pair(w, h, seed), with_outside=True)
    n = W.size
    assert (W == 0).sum() >= 0.10 * n
    assert (W == 255).sum() >= 0.10 * n
    assert ((W > 0) & (W < 255)).sum() >= 0.25 * n
    assert outside.sum() >= 0.02 * n


def test_hostile_pairs_stay_defined():
    for w, h in cr.SIZES:
        F, B = cr.hostile_pair(w, h, 0)
        assert not np.isfinite(F).all() and not np.isfinite(B).all()
        for soft in (1, 0):
            W = cr.consistency(F, B, soft=soft)
            assert W[1, 1] == 0 and W[2, 2] == 0 and W[3, 1] == 0
            assert W[h // 2 - 3, w // 2 - 1] == 255


# ---- the library's pure host checks -------------------------------------------------------------------------------------------
def test_default_params():
    p = _capi.ConsistencyParams()
    assert (p.alpha, p.beta, p.soft) == (F32(0.01), F32(0.5), 1)
    assert (cr.ALPHA, cr.BETA, cr.SOFT) == (p.alpha, p.beta, p.soft)
    _capi.consistency_params_check(p)
    for kw in (dict(alpha=0.0), dict(alpha=1.0), dict(beta=1e-30), dict(beta=1e6), dict(soft=0)):
        _capi.consistency_params_check(_capi.ConsistencyParams(**kw))
    assert _capi.consistency_choice({"alpha": 0.25, "soft": 0}).as_dict() == {"alpha": 0.25, "beta": 0.5, "soft": 0}
    with pytest.raises(ValueError, match="unknown consistency parameter 'gamma'"):
        _capi.ConsistencyParams(gamma=1)


@pytest.mark.parametrize("kw,rule", [
    (dict(alpha=-1e-6), r"alpha = -1e-06 outside 0\.\.1"),
    (dict(alpha=1.0001), r"alpha = 1\.0001 outside 0\.\.1"),
    (dict(alpha=np.nan), r"alpha = nan outside 0\.\.1"),
    (dict(alpha=np.inf), r"alpha = inf outside 0\.\.1"),
    (dict(beta=0.0), r"beta = 0 outside 0 < beta <= 1e6"),
    (dict(beta=-0.5), r"beta = -0\.5 outside 0 < beta <= 1e6"),
    (dict(beta=1.1e6), r"beta = 1\.1e\+06 outside 0 < beta <= 1e6"),
    (dict(beta=np.nan), r"beta = nan outside"),
    (dict(beta=np.inf), r"beta = inf outside"),
    (dict(soft=2), r"soft = 2 is neither 0 \(hard\) nor 1 \(soft\)"),
    (dict(soft=-1), r"soft = -1 is neither"),
])
def test_params_check_names_its_rule(kw, rule):
    with pytest.raises(ValueError, match=rule) as e:
        _capi.consistency_params_check(_capi.ConsistencyParams(**kw))
    assert "ffl_consistency_params_check" in str(e.value)
    with pytest.raises(ValueError, match=rule):
        _capi.consistency_choice(kw)


def test_params_check_refuses_null():
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.consistency_params_check(None)
    assert _capi.load().ffl_consistency_default_params(None) == _capi.FFL_ERR_INVALID


def desc(base=0x1000, item=0, pitch=0):
    return _capi.DevWeights(base, item, pitch)


@pytest.mark.parametrize("n,size,d,rule", [
    (1, (130, 17), None, "NULL weight descriptor"),
    (1, (130, 17), desc(base=0, pitch=130), "NULL weight base"),
    (0, (130, 17), desc(pitch=130), r"n = 0 weight maps"),
    (1, (1, 17), desc(pitch=130), r"size 1x17 outside 2\.\.32768"),
    (1, (130, 40000), desc(pitch=130), r"size 130x40000 outside 2\.\.32768"),
    (1, (130, 17), desc(pitch=-130), "negative weight stride"),
    (2, (130, 17), desc(item=-1, pitch=130), "negative weight stride"),
    (1, (130, 17), desc(pitch=(1 << 40) + 1), r"beyond 2\^40"),
    (1, (130, 17), desc(pitch=129), "overlap: weight row pitch 129 below the width 130"),
    (3, (130, 17), desc(item=16 * 136 + 129, pitch=136), "overlap: weight item stride 2305 below one map's extent 2306"),
])
def test_descriptor_rules_name_themselves(n, size, d, rule):
    """the rules `out` and `gate` of ffl_consistency_weights are held to (ffl_dev_weights_check), with no device"""
    with pytest.raises(ValueError, match=rule):
        _capi.dev_weights_check(n, size[0], size[1], d)


def test_exports():
    L = _capi.load()
    for name in ("ffl_consistency_default_params", "ffl_consistency_params_check", "ffl_consistency_weights"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    p = _capi.ConsistencyParams()
    assert C.sizeof(p) == 12


def test_pipeline_keys_without_a_device():
    assert pipeline.WEIGHT_MODES == ("consistency",)
    assert pipeline.consistency_kwargs(None, {}) == {}
    assert pipeline.consistency_kwargs(None, {"hip_weights": np.ones((4, 4), np.uint8)}) == {}
    assert pipeline.consistency_kwargs(None, {"hip_weights": "consistency", "hip_consistency": {"soft": 0}}) == {
        "weights": "consistency", "consistency": {"soft": 0}, "weights_gate": None}
    for key in ("hip_consistency", "hip_weights_gate"):
        with pytest.raises(ValueError, match=f"{key} needs hip_weights = 'consistency'"):
            pipeline.consistency_kwargs(None, {key: {"soft": 0}})
    with pytest.raises(ValueError, match="hip_center together with hip_weights"):
        pipeline.center_kwargs({"hip_center": "variance", "hip_weights": "consistency"})
    with pytest.raises(ValueError, match="flows_to_actions: hip_weights = 'consistency' needs the backward fields"):
        pipeline.flows_to_actions(None, [], 30.0, 10, {"hip_weights": "consistency"})
    for fn, args in ((pipeline.process_chunk_sharded, (None, [], 0, 1, None)), (pipeline.process_chunk_sharded_halo, (None, [], 0, 1, None)),
                     (pipeline.process_chunk_local_ranks, ([], []))):
        with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
            fn(*args, weights="consistency")
