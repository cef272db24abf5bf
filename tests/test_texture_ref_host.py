"""Host side of the texture (structure-tensor) maps: known answers of the numpy restatement
tests/texture_ref.py, the conditions the GPU tests' synthetic inputs must meet, what needs no device of the binding and the
schedule -- ffl_texture_params_check, the exports, the mode names and the params keys -- and the scene the map is for: a
camera fit that a flat wall drags to "no motion" and the map sets right."""
import ctypes as C

import numpy as np
import pytest

import motion_ref as mr
import texture_ref as tr
from funscript_flow_amd import _capi, pipeline


def gid(s):
    return f"{s[0]}x{s[1]}"


# ---- known answers, exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [1, 0])
@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_a_constant_frame_is_zero_in_both_modes(size, soft):
    w, h = size
    for r in tr.RADII:
        assert (tr.texture_map(tr.constant(w, h), r, soft=soft) == 0).all()   # tr == 0: no division, and T5 gives 0 too
    assert (tr.texture_map(tr.constant(w, h, 0), 8, tau=1e-3, soft=soft) == 0).all()


@pytest.mark.parametrize("soft", [1, 0])
def test_pure_stripes_are_zero_away_from_the_band_edges(soft):
    """horizontal stripes: gx = 0 everywhere, so Sxx = Sxy = 0 and det = 0 whatever Syy is -- the aperture problem"""
    w, h = 130, 40
    y = np.mgrid[0:h, 0:w][0]
    I = tr.residual_ref.to_u8(128.0 + 40.0 * np.sin(2 * np.pi * y / 9.0))
    for r in tr.RADII:
        c, det, t = tr.cornerness(I, r)
        assert (det == 0).all() and t.max() > 0
        assert (tr.texture_map(I, r, soft=soft) == 0).all()
    I = tr.thirds(w, h, 1)   # as a band of thirds(): 0 wherever the window stays inside the band
    a, b = w // 3, (2 * w) // 3
    for r in (1, 3, 7):
        W = tr.texture_map(I, r, soft=soft)
        assert (W[:, a + r + 1:b - r - 1] == 0).all()


def test_the_checkerboard_is_255_inside_and_the_trap_for_a_32_bit_product():
    for w, h in tr.SIZES[1:]:
        I = tr.checkerboard(w, h)
        gx, gy = tr.gradients(I)
        assert (np.abs(gx[1:-1, 1:-1]) == 255).all() and (np.abs(gy[1:-1, 1:-1]) == 255).all()
        for r in tr.RADII:
            N = (2 * r + 1) ** 2
            Sxx, Sxy, Syy = tr.window_sums(I, r)
            inner = (slice(r + 1, h - r - 1), slice(r + 1, w - r - 1))
            if Sxx[inner].size:
                assert (Sxx[inner] == N * 65025).all() and (Syy[inner] == N * 65025).all()
                for soft in (1, 0):
                    assert (tr.texture_map(I, r, soft=soft)[inner] == 255).all()
    Sxx, Sxy, Syy = tr.window_sums(tr.checkerboard(257, 40), 8)
    assert int((Sxx * Syy).max()) > 2 ** 32 and int((Sxx * Syy).max()) == (289 * 65025) ** 2
    wrapped = (Sxx * Syy) % 2 ** 32 - (Sxy * Sxy) % 2 ** 32   # what a 32-bit multiply would leave
    assert (wrapped != Sxx * Syy - Sxy * Sxy).any()


def test_a_single_bright_pixel_by_hand():
    """I = 0 but for I[8][8] = 255 on 16x16: gx = +255 at (7, 8), -255 at (9, 8); gy = +255 at (8, 7), -255 at (8, 9); gx * gy = 0
    everywhere.  At radius 1 the window of pixel (8, 8) holds all four: Sxx = Syy = 2 * 65025, Sxy = 0, det / tr = 65025,
    N = 9, tau = 16: q = 65025 / 144 > 1 -> 255.  The window of (6, 8) holds (7, 8) only: Syy = 0 -> det = 0 -> 0."""
    I = tr.single_pixel(16, 16)
    Sxx, Sxy, Syy = tr.window_sums(I, 1)
    assert (Sxx[8, 8], Sxy[8, 8], Syy[8, 8]) == (2 * 65025, 0, 2 * 65025)
    assert (Sxx[8, 6], Syy[8, 6]) == (65025, 0)
    for soft in (1, 0):
        W = tr.texture_map(I, 1, soft=soft)
        assert W[8, 8] == 255 and W[8, 6] == 0 and W[0, 0] == 0
    # the ramp: tau = 14450 gives tn = 130050 = 2 * 65025 exactly, q = 1/2 at (8, 8), W = (int)(127.5 + 0.5) = 128
    assert tr.texture_map(I, 1, tau=14450.0, soft=1)[8, 8] == 128


def test_window_sums_clamp_the_position_not_the_image():
    """rule T2 at a border: the offsets that leave the frame repeat the border pixel's gradient (which is not 0)"""
    I = np.zeros((16, 16), np.uint8)
    I[:, 1:] = 200                      # gx at column 0 is I[.][1] - I[.][0] = 200, at column 1 200, else 0
    Sxx, Sxy, Syy = tr.window_sums(I, 2)
    assert Sxx[8, 0] == 5 * (3 * 40000 + 40000)   # columns -2, -1, 0 (all column 0) and 1, five rows
    assert Sxx[8, 3] == 5 * 40000 and Sxx[8, 4] == 0


@pytest.mark.parametrize("soft", [1, 0])
def test_gate_is_min(soft):
    w, h = 130, 17
    I = tr.thirds(w, h, 1)
    g = np.random.default_rng(5).integers(0, 256, (h, w)).astype(np.uint8)
    W = tr.texture_map(I, 3, soft=soft)
    G = tr.texture_map(I, 3, soft=soft, gate=g)
    assert (G == np.minimum(W, g)).all() and (G != W).any() and (G != g).any()


# ---- the conditions on the synthetic inputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", tr.SEEDS)
@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_thirds_holds_every_class_of_weight(size, seed):
    w, h = size
    I = tr.thirds(w, h, seed)
    assert I.dtype == np.uint8 and I.shape == (h, w)
    for r in tr.RADII:
        if (w, h) == (16, 16) and r != 1:
            continue   # wider windows cover that whole frame
        W = tr.texture_map(I, r, tau=16.0, soft=1)
        zero, mid, full = float((W == 0).mean()), float(((W > 0) & (W < 255)).mean()), float((W == 255).mean())
        print(f"{w}x{h} seed {seed} r {r}: 0 {100 * zero:.1f} %, between {100 * mid:.1f} %, 255 {100 * full:.1f} %")
        assert zero >= 0.03 and mid >= 0.03 and full >= 0.03
        assert set(np.unique(tr.texture_map(I, r, tau=16.0, soft=0))) == {0, 255}


@pytest.mark.parametrize("size", tr.SIZES, ids=gid)
def test_hostile_frames_hold_what_they_claim(size):
    w, h = size
    e = tr.edge_steps(w, h)
    for edge in (e[0, :], e[h - 1, :], e[:, 0], e[:, w - 1]):
        assert (edge == 0).any() and (edge == 255).any()
    assert tr.single_pixel(w, h).sum() == 255
    assert set(np.unique(tr.checkerboard(w, h))) == {0, 255}
    Sxx, Sxy, Syy = tr.window_sums(tr.checkerboard(w, h), 8)
    assert int((Sxx * Syy).max()) > 2 ** 32   # at every size, 16x16 included


# ---- the binding and the schedule, without a device ----------------------------------------------------------------------------
def test_exports_defaults_and_record():
    L = _capi.load()
    for name in ("ffl_texture_default_params", "ffl_texture_params_check", "ffl_texture_weights"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    p = _capi.TextureParams()
    assert C.sizeof(p) == 12 and p.as_dict() == {"radius": 7, "tau": 16.0, "soft": 1}
    assert (p.radius, np.float32(p.tau), p.soft) == (tr.RADIUS, tr.TAU, tr.SOFT)
    assert _capi.RECORDS["ffl_texture_params"] is _capi.TextureParams
    assert L.ffl_texture_default_params(None) == _capi.FFL_ERR_INVALID
    with pytest.raises(ValueError, match="unknown texture parameter 'sigma'"):
        _capi.TextureParams(sigma=1)
    assert hasattr(_capi.Context, "texture_weights")


def test_params_check_accepts_and_refuses_as_the_abi_says():
    ok = [{}, {"radius": 1}, {"radius": 8}, {"tau": 65025.0}, {"tau": 1e-6}, {"soft": 0}, {"radius": 3, "tau": 100.0, "soft": 0}]
    for kw in ok:
        p = _capi.texture_choice(kw)
        assert isinstance(p, _capi.TextureParams)
        _capi.texture_params_check(p)
    assert _capi.texture_choice(None).as_dict() == _capi.TextureParams().as_dict()
    assert _capi.texture_choice(True).as_dict() == _capi.TextureParams().as_dict()
    given = _capi.TextureParams(soft=0)
    assert _capi.texture_choice(given) is given
    bad = [({"radius": 0}, r"radius = 0 outside 1\.\.8"), ({"radius": 9}, r"radius = 9 outside 1\.\.8"),
           ({"radius": -1}, r"radius = -1 outside 1\.\.8"), ({"tau": 0.0}, r"tau = 0 outside 0 < tau <= 65025"),
           ({"tau": -1.0}, r"tau = -1 outside"), ({"tau": 65026.0}, r"tau = 65026 outside 0 < tau <= 65025"),
           ({"tau": float("nan")}, r"tau = nan outside"), ({"tau": float("inf")}, r"tau = inf outside"),
           ({"soft": 2}, r"soft = 2 is neither"), ({"soft": -1}, r"soft = -1 is neither")]
    for kw, match in bad:
        with pytest.raises(ValueError, match="ffl_texture_params_check: " + match):
            _capi.texture_choice(kw)
    with pytest.raises(ValueError, match="NULL parameters"):
        _capi.texture_params_check(None)


def test_pipeline_keys_without_a_device():
    assert pipeline.MAP_MODES == ("consistency", "residual") and pipeline.WEIGHT_MODES == ("consistency",)   # the pinned names
    assert pipeline.FRAME_MAP_MODES == ("residual", "texture")
    assert pipeline.ALL_MAP_MODES == ("consistency", "residual", "texture")
    kw = pipeline.consistency_kwargs
    assert kw(None, {"hip_weights": "texture"}) == {"weights": "texture", "texture": None, "weights_gate": None}
    assert kw(None, {"hip_weights": "texture", "hip_texture": {"radius": 3}}) == {
        "weights": "texture", "texture": {"radius": 3}, "weights_gate": None}
    assert kw(None, {"hip_weights": "residual", "hip_texture": True}) == {
        "weights": "residual", "residual": None, "texture": True, "weights_gate": None}
    assert kw(None, {"hip_weights": "residual", "hip_residual": {"soft": 0}, "hip_texture": {"radius": 3}}) == {
        "weights": "residual", "residual": {"soft": 0}, "texture": {"radius": 3}, "weights_gate": None}
    with pytest.raises(ValueError, match="hip_texture needs hip_weights = 'texture'"):
        kw(None, {"hip_texture": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_texture needs hip_weights = 'texture', got 'consistency'"):
        kw(None, {"hip_weights": "consistency", "hip_texture": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_residual needs hip_weights = 'residual', got 'texture'"):
        kw(None, {"hip_weights": "texture", "hip_residual": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_consistency needs hip_weights = 'consistency', got 'texture'"):
        kw(None, {"hip_weights": "texture", "hip_consistency": {"soft": 0}})
    with pytest.raises(ValueError, match="hip_center together with hip_weights"):
        pipeline.center_kwargs({"hip_center": "variance", "hip_weights": "texture"})
    with pytest.raises(ValueError, match="flows_to_actions: hip_weights = 'texture' needs the frames.*Context.texture_weights"):
        pipeline.flows_to_actions(None, [], 30.0, 10, {"hip_weights": "texture"})
    for fn, args in ((pipeline.process_chunk_sharded, (None, [], 0, 1, None)), (pipeline.process_chunk_sharded_halo, (None, [], 0, 1, None)),
                     (pipeline.process_chunk_local_ranks, ([], []))):
        with pytest.raises(ValueError, match="the sharded schedules run unweighted"):
            fn(*args, weights="texture")


# ---- what the map is for ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [3, 7])
@pytest.mark.parametrize("seed", tr.SEEDS)
@pytest.mark.parametrize("size", [(64, 64), (130, 72), (257, 40)], ids=gid)
def test_the_map_frees_the_camera_fit_from_a_flat_wall(size, seed, radius):
    """the left 3/5 of the frame is a wall that reports zero flow, the rest moves by (3, -2): the Cauchy-weighted translation
    fit locks on to the wall unless the texture map weights it"""
    w, h = size
    I, F = tr.wall_scene(w, h, seed)
    plain = mr.fit(F, "translation", 3, 1.0)[-1]
    W = tr.texture_map(I, radius)
    weighted = mr.fit(F, "translation", 3, 1.0, W=W)[-1]
    da, db = float(weighted["a0"]) - tr.MOVE[0], float(weighted["b0"]) - tr.MOVE[1]
    print(f"{w}x{h} seed {seed} r {radius}: unweighted ({float(plain['a0']):.3f}, {float(plain['b0']):.3f}), weighted off by "
          f"({da:.3f}, {db:.3f})")
    assert abs(float(plain["a0"])) < 1.0
    assert abs(da) <= 0.15 and abs(db) <= 0.15
