"""Host side of the weight maps: the restatement tests/weights_ref.py against the unweighted
restatements and integer closed forms, and the refusals that need no device -- ffl_dev_weights_check through _capi.load()
and _capi.device_weights."""
import numpy as np
import pytest

import axes_ref as ar
import post_ref as pr
import weights_ref as wr
from funscript_flow_amd import _capi

SIZES = [(16, 16), (130, 17), (257, 40)]


def field(w, h, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((h, w, 2)) * 1.5).astype(np.float32)


def random_map(w, h, seed):
    rng = np.random.default_rng(seed)
    W = rng.integers(1, 256, (h, w)).astype(np.uint8)
    W[rng.random((h, w)) < 1 / 3] = 0
    return W


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_all_ones_map_is_the_unweighted_restatement(size):
    w, h = size
    f, ones = field(w, h, w), np.ones((h, w), np.uint8)
    assert wr.total_weight(ones) == w * h
    x, y, d = wr.argmax_weighted(f, ones)
    x0, y0, d0 = pr.argmax_ref(f)
    assert (x, y) == (x0, y0) and np.float32(d).tobytes() == np.float32(d0).tobytes()
    assert wr.mag_exact_weighted(f, ones) == pr.mag_exact(f)[0]
    assert wr.mean_mag_accepted(f, ones) == pr.mean_mag_accepted(f)
    for pov in (False, True):
        for centre in ((0.37 * w + 0.25, 0.41 * h + 0.5), (0.0, 0.0), (w + 4.5, -3.0)):
            got = wr.axes_exact_weighted(f, centre, ones, pov)
            want = ar.axes_exact(f, centre, pov)
            assert got == want                                               # value for value, S included
            for a, b in zip(wr.weighted_terms(f, centre, ones, pov), ar.axes_terms(f, centre, pov)):
                assert a.tobytes() == np.ascontiguousarray(np.broadcast_to(b, a.shape)).tobytes()   # x 1.0 is exact
    assert wr.axes_bound(w, h, 1.0) == ar.axes_bound(w, h, 1.0)
    # a bool map is the same map
    assert wr.axes_exact_weighted(f, (3.0, 4.0), np.ones((h, w), bool)) == wr.axes_exact_weighted(f, (3.0, 4.0), ones)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_closed_forms(size):
    w, h = size
    centre = (w // 3, h // 4)
    known = ar.known_fields(w, h, centre)
    ones, W = np.ones((h, w), np.uint8), random_map(w, h, 7)
    sw = wr.total_weight(W)
    dx = np.arange(w, dtype=np.int64)[None, :] - centre[0] + np.zeros((h, 1), np.int64)
    dy = np.arange(h, dtype=np.int64)[:, None] - centre[1] + np.zeros((1, w), np.int64)
    q = W.astype(np.int64)
    for name, (f, want) in known.items():
        assert wr.known_weighted(f, centre, ones) == want, name             # axes_ref's closed forms
        got = wr.known_weighted(f, centre, W)
        exact = [m for m, _ in wr.axes_exact_weighted(f, centre, W, True)]
        assert got == exact, name                                            # integer terms: the exact sum IS the value
    k, a, b = 3, 5, -2
    r2 = int(((dx * dx + dy * dy) * q).sum())
    sx, sy = int((dx * q).sum()), int((dy * q).sum())
    m = lambda t: float(t) / float(sw)
    assert wr.known_weighted(known["rotation"][0], centre, W) == [0.0, m(k * r2), m(-k * sy), m(k * sx)]
    assert wr.known_weighted(known["expansion"][0], centre, W) == [m(k * r2), 0.0, m(k * sx), m(k * sy)]
    assert wr.known_weighted(known["uniform"][0], centre, W) == [m(a * sx + b * sy), m(b * sx - a * sy), float(a), float(b)]
    # a single weighted pixel: the components are that pixel's terms, whatever its weight
    one = np.zeros((h, w), np.uint8)
    one[h - 2, w - 3] = 200
    f = known["expansion"][0]
    px, py = w - 3 - centre[0], h - 2 - centre[1]
    assert wr.known_weighted(f, centre, one) == [float(k * (px * px + py * py)), 0.0, float(k * px), float(k * py)]


def test_masked_argmax_mean_and_empty_map():
    w, h = 130, 17
    f, W = field(w, h, 3), random_map(w, h, 4)
    div = np.abs(pr.divergence(f))
    x, y, d = wr.argmax_weighted(f, W)
    assert W[y, x] > 0 and abs(d) == div[W > 0].max()
    first = np.flatnonzero((div == abs(d)).ravel() & (W.ravel() > 0))[0]
    assert (y, x) == divmod(int(first), w)
    # the unmasked maximum is excluded when its weight is 0, and only then
    x0, y0, _ = pr.argmax_ref(f)
    W2 = np.ones((h, w), np.uint8)
    W2[y0, x0] = 0
    assert wr.argmax_weighted(f, W2)[:2] != (x0, y0)
    # a NaN outside the map is invisible, one inside wins
    g = f.copy()
    g[5, 60, 0] = np.nan
    W3 = np.full((h, w), 9, np.uint8)
    W3[3:8, 57:64] = 0
    assert np.float32(wr.argmax_weighted(g, W3)[2]).tobytes() == np.float32(wr.argmax_weighted(np.nan_to_num(g), W3)[2]).tobytes()
    assert wr.mag_exact_weighted(g, W3) == wr.mag_exact_weighted(np.nan_to_num(g), W3)
    assert wr.axes_exact_weighted(g, (1.0, 2.0), W3) == wr.axes_exact_weighted(np.nan_to_num(g), (1.0, 2.0), W3)
    W3[4, 60] = 1                                                            # div at (60, 4) reads u of row 5
    assert np.isnan(wr.argmax_weighted(g, W3)[2]) and wr.argmax_weighted(g, W3)[:2] == (60, 4)
    # the mean: weights scale out
    assert wr.mag_exact_weighted(f, np.full((h, w), 255, np.uint8)) == pytest.approx(pr.mag_exact(f)[0], rel=1e-15)
    empty = np.zeros((h, w), np.uint8)
    assert wr.argmax_weighted(f, empty) is None
    rec = wr.pass1_record(f, empty)
    assert rec[:2] == (w // 2, h // 2) and np.float32(rec[2]).tobytes() == np.float32(0).tobytes() and rec[3:] == (0.0, False)
    assert wr.pass1_record(f, empty, pov=True)[:2] == (w // 2, h // 2)
    assert wr.axes_exact_weighted(f, (1.0, 2.0), empty) == [(0.0, 0.0)] * 4 and wr.known_weighted(np.zeros((h, w, 2)), (1, 2), empty) == [0.0] * 4
    assert wr.pass1_record(f, W, pov=True)[:3] == (w // 2, h - 1, np.float32(0.0))


# ---- ffl_dev_weights_check (pure host) ----------------------------------------------------------------------------------
def desc(base=4096, item=0, pitch=130):
    return _capi.DevWeights(base, item, pitch)


def test_dev_weights_check_accepts():
    w, h = 130, 17
    for n, d in ((1, desc()), (5, desc()),                                       # one shared map
                 (5, desc(item=h * w)), (5, desc(item=(h - 1) * 200 + w, pitch=200)),   # packed, padded pitch
                 (3, desc(base=4097, item=h * 131 + 3, pitch=131)),                  # an odd base, odd pitch and item stride
                 (2, desc(item=1 << 40, pitch=1 << 30))):                            # the largest strides
        _capi.dev_weights_check(n, w, h, d)
    _capi.dev_weights_check(1, 2, 2, desc(pitch=2))
    _capi.dev_weights_check(1, 32768, 32768, desc(pitch=32768))


@pytest.mark.parametrize("n,size,d,rule", [
    (1, (130, 17), None, "NULL weight descriptor"),
    (1, (130, 17), desc(base=0), "NULL weight base"),
    (0, (130, 17), desc(), r"n = 0 weight maps \(>= 1\)"),
    (-3, (130, 17), desc(), r"n = -3 weight maps"),
    (1, (1, 17), desc(), r"size 1x17 outside 2\.\.32768"),
    (1, (130, 32769), desc(), r"size 130x32769 outside 2\.\.32768"),
    (2, (130, 17), desc(item=-1), r"negative weight stride \(item -1, row 130\)"),
    (2, (130, 17), desc(pitch=-130), r"negative weight stride"),
    (2, (130, 17), desc(item=(1 << 40) + 1), r"weight stride beyond 2\^40"),
    (2, (130, 17), desc(pitch=(1 << 40) + 1), r"weight stride beyond 2\^40"),
    (2, (130, 17), desc(pitch=129), r"overlap: weight row pitch 129 below the width 130"),
    (2, (130, 17), desc(item=17 * 130 - 1), r"overlap: weight item stride 2209 below one map's extent 2210"),
    (2, (130, 17), desc(item=1), r"overlap: weight item stride 1 below"),
    (1, (130, 17), desc(item=16 * 200 + 129, pitch=200), r"overlap: weight item stride 3329 below one map's extent 3330"),
])
def test_dev_weights_check_names_its_rule(n, size, d, rule):
    with pytest.raises(ValueError, match=rule) as e:
        _capi.dev_weights_check(n, size[0], size[1], d)
    assert "ffl_dev_weights_check" in str(e.value)


def test_device_weights_refusals_name_their_rule():
    torch = pytest.importorskip("torch")
    w, h = 130, 17
    for obj, rule in ((np.ones((h, w), np.uint8), "not device memory: weight maps are torch device tensors, got ndarray"),
                      (torch.ones((h, w), dtype=torch.float32), r"dtype torch\.float32 is not supported: weight maps are uint8 or bool"),
                      (torch.ones((h, w), dtype=torch.int32), "uint8 or bool"),
                      (torch.ones((w,), dtype=torch.uint8), r"shape: weight maps are \(H, W\) or \(n, H, W\)"),
                      (torch.ones((2, 1, h, w), dtype=torch.uint8), r"shape: weight maps are \(H, W\) or \(n, H, W\)"),
                      (torch.ones((w, h), dtype=torch.uint8), r"size: a map of 17x130 does not match the context's 130x17"),
                      (torch.ones((3, h, w + 1), dtype=torch.bool), r"size: a map of 131x17 does not match"),
                      (torch.ones((h, 2 * w), dtype=torch.uint8)[:, ::2], "pixel stride: the pixels of a row must be contiguous, the stride is 2"),
                      (torch.ones((3, w, h), dtype=torch.uint8).transpose(1, 2), "pixel stride"),
                      (torch.ones((0, h, w), dtype=torch.uint8), r"shape: no maps"),
                      (torch.ones((h, w), dtype=torch.uint8), "not device memory: a CPU tensor"),
                      (torch.ones((2, h, w), dtype=torch.bool), "not device memory: a CPU tensor")):
        with pytest.raises(ValueError, match=rule):
            _capi.device_weights(obj, w, h)


def test_exports_and_scratch_size():
    L = _capi.load()
    for name in ("ffl_dev_weights_check", "ffl_pass1_weighted", "ffl_radial_window_axes_weighted", "ffl_weights_extra_bytes"):
        assert name in _capi.EXPORTS and hasattr(L, name)
    # FFL_N_AXES + 1 partials per workgroup of the radial grid, 256 items, 8 bytes each
    blocks = lambda w, h: -(-(-(-w // 128) * -(-h // 16)) // 4)
    for w, h in ((16, 16), (257, 40), (1920, 1080), (3840, 2160)):
        assert _capi.weights_extra_bytes(w, h) == 5 * blocks(w, h) * 256 * 8
        assert _capi.weights_extra_bytes(w, h) * 4 == _capi.axes_extra_bytes(w, h) * 5
    with pytest.raises(_capi.FFLError, match="unsupported frame size"):
        _capi.weights_extra_bytes(8, 8)
