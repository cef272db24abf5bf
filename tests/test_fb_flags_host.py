"""CPU side of general Farneback's two modes: the restatement tests/fb_flags_ref against
tests/fb_general_ref, against whole-array numpy restatements written from the rules (bit for bit: both are float32 in the
same order), against closed forms; the refusals and the routing of the Python binding.  No GPU."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import fb_flags_ref as ffr
import fb_general_ref as fbr
import param_domain as pd
from funscript_flow_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the composed driver --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(130, 66), (257, 255)])
def test_the_composed_driver_without_a_mode_is_fb_general_ref(w, h):
    fr = pd.fb_frames(w, h)
    for over in ({}, {"winsize": 33, "iterations": 2}):
        assert np.array_equal(bits(ffr.flow(fr[0], fr[1], over)), bits(fbr.flow(fr[0], fr[1], over)))


# ---- F.7 ------------------------------------------------------------------------------------------------------------
def np_taps(winsize):
    m = winsize // 2
    sigma, s = m * 0.3, 1.0
    k = np.empty(m + 1, f32)
    k[0] = 1.0
    for i in range(1, m + 1):
        k[i] = f32(math.exp(-(i * i) / (2 * sigma * sigma)))
        s += 2.0 * float(k[i])
    inv = 1.0 / s
    for i in range(m + 1):
        k[i] = f32(float(k[i]) * inv)
    return k


def np_gauss_solve(M, winsize):
    """F.7 on whole arrays: every line is one float32 (or, in the solve, float64) operation of the rule"""
    m, k = winsize // 2, np_taps(winsize)
    M = np.ascontiguousarray(M, f32)
    _, h, w = M.shape
    P = np.pad(M, ((0, 0), (m, m), (0, 0)), mode="edge")
    v = P[:, m:m + h] * k[0]
    for i in range(1, m + 1):
        v = v + (P[:, m + i:m + i + h] + P[:, m - i:m - i + h]) * k[i]
    V = np.pad(v, ((0, 0), (0, 0), (m, m)), mode="edge")
    g = V[:, :, m:m + w] * k[0]
    for i in range(1, m + 1):
        g = g + k[i] * (V[:, :, m - i:m - i + w] + V[:, :, m + i:m + i + w])
    assert g.dtype == f32
    g11, g12, g22, h1, h2 = g.astype(np.float64)
    idet = 1.0 / (g11 * g22 - g12 * g12 + 1e-3)
    return np.stack([((g11 * h2 - g12 * h1) * idet).astype(f32), ((g22 * h1 - g12 * h2) * idet).astype(f32)], -1)


@pytest.mark.parametrize("winsize", [3, 5, 15, 33, 63])
def test_taps(winsize):
    k = ffr.taps(winsize)
    assert np.array_equal(bits(k), bits(np_taps(winsize)))
    full = np.concatenate([k[:0:-1], k]).astype(np.float64)      # the symmetric window k[m] .. k[1], k[0], k[1] .. k[m]
    assert len(full) == winsize and np.array_equal(full, full[::-1]) and (full > 0).all() and (np.diff(k) < 0).all()
    assert abs(full.sum() - 1.0) <= 1e-6, full.sum() - 1.0


@pytest.mark.parametrize("winsize", [3, 5, 15, 33, 63])
@pytest.mark.parametrize("w,h", [(16, 16), (65, 17), (130, 66), (20, 300)])
def test_gauss_solve_equals_the_numpy_restatement_bit_for_bit(w, h, winsize):
    rng = np.random.default_rng(w * 31 + h + winsize)
    A = rng.standard_normal((2, h, w))
    # a positive semi-definite G and an h of like size, as UpdateMatrices produces them
    M = np.stack([A[0] ** 2 + 0.1, A[0] * A[1], A[1] ** 2 + 0.1, rng.standard_normal((h, w)), rng.standard_normal((h, w))]).astype(f32)
    assert np.array_equal(bits(ffr.gauss_solve(M, winsize)), bits(np_gauss_solve(M, winsize)))


@pytest.mark.parametrize("winsize", [3, 15, 63])
def test_a_constant_M_gives_the_closed_form_solve_everywhere(winsize):
    h, w, m = 40, 70, winsize // 2
    c = np.array([2.0, 0.5, 3.0, 1.0, -1.0])
    M = np.broadcast_to(c[:, None, None], (5, h, w)).astype(f32)
    got = ffr.gauss_solve(M, winsize)
    det = c[0] * c[2] - c[1] ** 2 + 1e-3
    want = np.array([(c[0] * c[4] - c[1] * c[3]) / det, (c[2] * c[3] - c[1] * c[4]) / det])
    # each pass is m + 1 products and m sums in float32 of taps that sum to 1 within 1e-6: a blurred value is c (1 + e),
    # |e| <= 2 (2 m + 1) 2^-24 + 2e-6; the solve's terms are of one sign pattern with det = 5.75, so the quotient moves by at
    # most 4 e
    e = 2 * (2 * m + 1) * 2.0 ** -24 + 2e-6
    assert np.allclose(got, want, rtol=4 * e + 2.0 ** -23, atol=0), np.abs(got / want - 1).max()


def _quadratic(h, w, coef, shift=(0.0, 0.0)):
    a, bx, by, cxx, cyy, cxy = coef
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - shift[0], y - shift[1]
    return (a + bx * x + by * y + cxx * x * x + cyy * y * y + cxy * x * y).astype(f32)


@pytest.mark.parametrize("d", [(1.5, -0.75), (-2.25, 0.5), (0.0, 3.0), (0.4, 0.0)])
def test_exact_quadratic_pair_gives_the_displacement_under_the_gaussian_window(d):
    """the construction and tolerance of tests/test_oracle_farneback.py: M is constant in the interior, so the Gaussian
    window (taps summing to one) leaves it unchanged and the solve returns d * det / (det + 1e-3)"""
    h, w = 72, 88
    coef = (40.0, 0.7, -0.4, 0.11, 0.07, 0.05)
    coef = coef[:3] + tuple(c * 6.0 for c in coef[3:])
    I0, I1 = _quadratic(h, w, coef), _quadratic(h, w, coef, shift=d)
    M = fbr.update_matrices(fbr.polyexp(I0), fbr.polyexp(I1), np.zeros((h, w, 2), f32))
    flow = ffr.gauss_solve(M, 15)
    cxx, cyy, r6 = coef[3], coef[4], coef[5] / 2
    det = (cxx * cyy - r6 * r6) ** 2
    want = np.array(d) * det / (det + 1e-3)
    inner = flow[20:-20, 20:-20]
    assert np.allclose(inner[..., 0], want[0], rtol=2e-4, atol=2e-4), (inner[..., 0].mean(), want[0])
    assert np.allclose(inner[..., 1], want[1], rtol=2e-4, atol=2e-4), (inner[..., 1].mean(), want[1])


# ---- F.8 ------------------------------------------------------------------------------------------------------------
def np_area_table(S, D):
    s = S / D
    out = []
    for d in range(D):
        f1 = d * s
        f2 = f1 + s
        cw = min(s, S - f1)
        s1, s2 = math.ceil(f1), min(math.floor(f2), S - 1)
        s1 = min(s1, s2)
        if s1 - f1 > 1e-3:
            out.append((d, s1 - 1, f32((s1 - f1) / cw)))
        out += [(d, q, f32(1.0 / cw)) for q in range(s1, s2)]
        if f2 - s2 > 1e-3:
            out.append((d, s2, f32(min(min(f2 - s2, 1.0), cw) / cw)))
    return out


def np_area_init(seed, lw, lh, scale):
    """F.8 from the rule; ((lh, lw, 2) float32, path)"""
    seed = np.ascontiguousarray(seed, f32)
    H, W = seed.shape[:2]
    fs = f32(scale)
    if (lw, lh) == (W, H):
        return seed * fs, "a"
    sx, sy = W / lw, H / lh
    ix, iy = round(sx), round(sy)
    if abs(sx - ix) < np.finfo(np.float64).eps and abs(sy - iy) < np.finfo(np.float64).eps:
        blocks = seed.reshape(lh, iy, lw, ix, 2)
        acc = np.zeros((lh, lw, 2), f32)
        for j in range(iy):
            for i in range(ix):
                acc = acc + blocks[:, j, :, i]
        return acc * f32(f32(1.0) / f32(ix * iy)) * fs, "b"
    xt, yt = np_area_table(W, lw), np_area_table(H, lh)
    out = np.empty((lh, lw, 2), f32)
    first = set()
    for dy, syi, beta in yt:
        buf = np.zeros((lw, 2), f32)
        for dx, sxi, alpha in xt:
            buf[dx] = buf[dx] + seed[syi, sxi] * alpha
        if dy not in first:
            out[dy] = beta * buf
            first.add(dy)
        else:
            out[dy] = out[dy] + beta * buf
    return out * fs, "c"


# (W, H, overrides) -> the coarsest level and its F.8 path
AREA_CASES = [
    (16, 16, {}, "a"), (300, 20, {}, "a"), (40, 40, {"pyr_scale": 0.99, "levels": 1}, "a"),
    (130, 66, {}, "b"), (64, 64, {}, "b"), (256, 256, {}, "b"),
    (127, 129, {"levels": 1}, "c"), (128, 127, {"levels": 1}, "c"), (257, 255, {"levels": 2}, "c"),
    (257, 255, {"pyr_scale": 0.8, "levels": 12}, "c"),
]


def coarsest(W, H, over):
    K = fbr.geometry(W, H, over) - 1
    lw, lh, _, _ = fbr.level_params(W, H, over, K)
    return lw, lh, ffr.level_scale(over, K)


@pytest.mark.parametrize("W,H,over,path", AREA_CASES, ids=[f"{c[3]}_{c[0]}x{c[1]}" for c in AREA_CASES])
def test_area_init_paths_against_the_numpy_restatement(W, H, over, path):
    lw, lh, scale = coarsest(W, H, over)
    rng = np.random.default_rng(W * 31 + H)
    seed = (rng.standard_normal((H, W, 2)) * 3).astype(f32)
    seed[0, 0, 0] = -0.0                                        # (a) keeps the sign of a zero
    got, took = ffr.area_init(seed, lw, lh, scale)
    want, np_took = np_area_init(seed, lw, lh, scale)
    assert took == np_took == path
    assert np.array_equal(bits(got), bits(want))
    # a constant seed comes back as constant x scale: (a) and (b) exactly (sums of up to 64 equal small integers and a
    # power-of-two block), (c) within the tables' deviation from a unit sum (1e-6 per axis) and five float32 roundings
    const = np.broadcast_to(f32([3.0, -5.0]), (H, W, 2))
    out, _ = ffr.area_init(const, lw, lh, scale)
    target = np.broadcast_to(f32([3.0, -5.0]) * f32(scale), out.shape)
    if path == "c":
        assert np.allclose(out, target, rtol=2e-6 + 5 * 2.0 ** -24, atol=0)
    else:
        assert np.array_equal(bits(out), bits(target))


@pytest.mark.parametrize("S,D", [(127, 64), (129, 64), (255, 64), (257, 64), (257, 34), (255, 34), (128, 64)])
def test_area_tables(S, D):
    di, si, al = ffr.area_table(S, D)
    want = np_area_table(S, D)
    assert [(int(d), int(s)) for d, s in zip(di, si)] == [(d, s) for d, s, _ in want]
    assert np.array_equal(bits(al), bits(np.array([a for _, _, a in want], f32)))
    assert si.min() >= 0 and si.max() <= S - 1 and (al > 0).all() and len(di) <= S + 2 * D
    sums = np.zeros(D)
    np.add.at(sums, di, al.astype(np.float64))
    assert np.abs(sums - 1.0).max() <= 1e-6
    assert sorted(set(di.tolist())) == list(range(D))          # every destination has an entry


def test_the_tables_of_127x129_hold_126_partial_x_entries():
    di, si, al = ffr.area_table(127, 64)
    whole = f32(1.0 / (127 / 64))
    assert np.count_nonzero(al != whole) == 126


# ---- the seed reaches the output ------------------------------------------------------------------------------------
SEED_REACH = [(16, 16, {}), (300, 20, {}), (130, 66, {}), (64, 64, {}), (127, 129, {"levels": 1}), (128, 127, {"levels": 1})]


@pytest.mark.parametrize("window", ["box", "gaussian"])
@pytest.mark.parametrize("w,h,over", SEED_REACH, ids=[f"{w}x{h}" for w, h, _ in SEED_REACH])
def test_the_seed_reaches_the_output(w, h, over, window):
    """with at most two scales a seeded flow differs from the unseeded one nearly everywhere: a comparison of final flows
    (tests/test_gpu_fb_flags.py) sees the area stage.  Deeper pyramids forget the seed and decide nothing here.  The content
    is a translated broadband texture, the seed its true flow plus noise (measured: 99.1 - 100 % of the values change).  How
    much is kept depends on the content: on the smooth pattern of param_domain.fb_frames, locally the exact quadratic whose
    update does not depend on the start, 82 - 95 % of the values changed under the box and 96 - 100 % under the Gaussian
    window, whatever the seed."""
    assert fbr.geometry(w, h, over) <= 2
    f0, f1 = ffr.textured_frames(w, h, 2)
    rng = np.random.default_rng(w * 31 + h)
    seed = (f32(ffr.TEXTURE_FLOW) + 0.25 * rng.standard_normal((h, w, 2))).astype(f32)
    cache = {}
    plain = ffr.flow(f0, f1, over, window, rcache=cache)
    seeded = ffr.flow(f0, f1, over, window, seed, rcache=cache)
    changed = np.mean(bits(plain) != bits(seeded))
    print(f"{w}x{h} {window}: {100 * changed:.1f} % of the values change; median flow {np.median(plain[..., 0]):.2f}, "
          f"{np.median(plain[..., 1]):.2f}")
    assert changed >= 0.9, changed


# ---- refusals and routing -------------------------------------------------------------------------------------------
def test_window_names():
    assert _capi.farneback_mode({}) == "box" and _capi.farneback_mode({"hip_farneback_window": "box"}) == "box"
    assert _capi.farneback_mode({"hip_farneback_window": "gaussian", "hip_farneback": {"winsize": 21}}) == "gaussian"
    with pytest.raises(ValueError, match="hann"):
        _capi.farneback_mode({"hip_farneback_window": "hann"})
    with pytest.raises(ValueError, match="hip_farneback_window.*dis"):
        _capi.farneback_mode({"hip_farneback_window": "gaussian", "hip_flow": "dis"})
    with pytest.raises(ValueError, match="hip_farneback_window.*dis"):
        _capi.farneback_mode({"hip_farneback_window": "box", "hip_flow": "dis"})
    # farneback_choice is as it was: the window is no Farneback parameter, and the two flags stay refused as parameters
    assert _capi.farneback_choice({"hip_farneback_window": "gaussian"}) is None
    for flags in (4, 256):
        with pytest.raises(ValueError):
            _capi.farneback_choice({"hip_farneback": {"flags": flags}})


def test_an_unknown_mode_bit_is_refused_by_name():
    L = _capi.load()
    for mode in (1, 2, 8, 512, 256 | 2, 1 << 31):
        assert L.ffl_flow_pairs_farneback_ex(None, 1, None, None, None, 0, None, mode) == _capi.FFL_ERR_INVALID
        msg = L.ffl_last_error(None).decode()
        assert "unknown mode bit" in msg and hex(mode & ~260) in msg, msg


def test_the_abi_exports_and_declares_the_new_entry_point():
    L = _capi.load()
    assert hasattr(L, "ffl_flow_pairs_farneback_ex") and "ffl_flow_pairs_farneback_ex" in _capi.EXPORTS
    header = open(os.path.join(ROOT, "include", "ffl.h")).read()
    assert re.search(r"#define FFL_FB_USE_INITIAL_FLOW\s+4u", header) and re.search(r"#define FFL_FB_GAUSSIAN_WINDOW\s+256u", header)
    assert (_capi.FFL_FB_USE_INITIAL_FLOW, _capi.FFL_FB_GAUSSIAN_WINDOW) == (4, 256)


class _Recorder:
    """stands in for the library behind a Context: records which symbol a call reaches"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return _capi.FFL_OK
        return call


def test_only_a_mode_reaches_the_new_symbol():
    ctx = object.__new__(_capi.Context)
    ctx.L, ctx._h = _Recorder(), None
    p = _capi.FarnebackParams(winsize=21)
    ctx.flow_pairs_farneback([0], [1], [0], False, p)
    ctx.flow_pairs_farneback([0], [1], [0], False, None, window="box", initial_flow=False)
    assert [c[0] for c in ctx.L.calls] == ["ffl_flow_pairs_farneback"] * 2
    ctx.L.calls.clear()
    ctx.flow_pairs_farneback([0], [1], [0], True, p, window="gaussian")
    ctx.flow_pairs_farneback([0], [1], [0], False, None, initial_flow=True)
    ctx.flow_pairs_farneback([0], [1], [0], False, None, window="gaussian", initial_flow=True)
    assert [(c[0], c[1][-1]) for c in ctx.L.calls] == [("ffl_flow_pairs_farneback_ex", m) for m in (256, 4, 260)]
    with pytest.raises(ValueError, match="hann"):
        ctx.flow_pairs_farneback([0], [1], [0], False, None, window="hann")
    ctx._h = None   # nothing to destroy


class _Ctx:
    """a recording stand-in for the context behind a PairEngine"""

    def __init__(self, B=8, frame_slots=64, flow_slots=64, w=256, h=256):
        self.max_batch, self.frame_slots, self.flow_slots, self.width, self.height = B, frame_slots, flow_slots, w, h
        self.calls = []

    def upload_frames(self, first, frames):
        pass

    def flow_pairs(self, f0, f1, slots, pov):
        self.calls.append(("tuned", None, "box"))

    def flow_pairs_farneback(self, f0, f1, slots, pov, params=None, window="box", initial_flow=False):
        assert not initial_flow                         # nothing in the pipeline seeds a batch
        self.calls.append(("general", params.as_dict() if params is not None else None, window))

    def pass1_results(self, slots, thr):
        return [(0, 0, 0.0, 0.0, False)] * len(slots)

    def radial(self, slots, centers, cuts, pov):
        return np.zeros(len(slots))


def test_the_pipeline_passes_the_window_wherever_hip_farneback_goes(monkeypatch):
    from funscript_flow_amd import pipeline, postchain
    monkeypatch.setattr(postchain, "actions_from_scalars", lambda *a: [])
    frames = [np.zeros((256, 256), np.uint8)] * 40
    ctx = _Ctx()
    eng = pipeline.PairEngine(ctx, depth=1)
    pipeline.frames_to_actions(eng, frames, 30.0, {"hip_farneback_window": "gaussian"})
    assert ctx.calls and all(c == ("general", None, "gaussian") for c in ctx.calls)    # the default numbers, general path
    assert eng.window == "box"
    ctx.calls.clear()
    pipeline.frames_to_actions(eng, frames, 30.0, {"hip_farneback_window": "gaussian", "hip_farneback": {"winsize": 21}})
    assert ctx.calls and all(c[0] == "general" and c[1]["winsize"] == 21 and c[2] == "gaussian" for c in ctx.calls)
    ctx.calls.clear()
    pipeline.frames_to_actions(eng, frames, 30.0, {})
    assert ctx.calls and all(c[0] == "tuned" for c in ctx.calls)
    ctx.calls.clear()
    own = pipeline.PairEngine(ctx, depth=1, window="gaussian", farneback=_capi.FarnebackParams(levels=5))
    own.process_chunk(frames[:9])
    assert ctx.calls and all(c[0] == "general" and c[1]["levels"] == 5 and c[2] == "gaussian" for c in ctx.calls)
    ctx.calls.clear()
    own.process_chunk(frames[:9], window="box", farneback=None)                          # per call: the tuned path
    assert ctx.calls and all(c[0] == "tuned" for c in ctx.calls)
    with pytest.raises(ValueError, match="hann"):
        pipeline.PairEngine(ctx, window="hann")
    with pytest.raises(ValueError):
        pipeline.PairEngine(ctx, flow="dis", window="gaussian")
    for bad in ({"hip_farneback_window": "hann"}, {"hip_farneback_window": "gaussian", "hip_flow": "dis"}):
        with pytest.raises(ValueError, match="hip_farneback_window|hann"):
            pipeline.frames_to_actions(eng, frames, 30.0, bad)
