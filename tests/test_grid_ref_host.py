"""Host side of the per-cell statistics grid and the variance centre: the numpy
restatement tests/grid_ref.py against the fixtures the reference's own center_of_mass_variance produced
(tests/golden/grid_golden.npz, written by tests/gen_grid_golden.py), against hand-computed answers and against numpy's own
means; rule G6 against np.mean over the list FF:1205-1213 builds; and the refusals that need no device."""
import os

import numpy as np
import pytest

import grid_ref as gr
from funscript_flow_amd import _capi, pipeline

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "grid_golden.npz")


@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def test_fields_are_closed_form():
    """the generator's bytes: a hash of integers, float32 products and sums -- pinned by a few values and a checksum"""
    f = gr.field(53, 37, seed=2)
    assert f.dtype == np.float32 and f.shape == (37, 53, 2)
    assert np.array_equal(f, gr.field(53, 37, seed=2)) and not np.array_equal(f, gr.field(53, 37, seed=3))
    u = gr._unit(8, 4, 0, 0)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
    assert np.array_equal(u * np.float32(2.0 ** 24), np.round(u * np.float32(2.0 ** 24)))   # 24 exact bits
    m = gr.magnitude(f)
    assert np.median(m) < 0.02 and m.max() > 1.5        # near-zero background, px-sized noise and blob
    y, x = np.mgrid[0:37, 0:53]
    far = ((x - 35) ** 2 + (y - 12) ** 2 >= 49) & ~((x >= 6) & (x < 19) & (y >= 18) & (y < 30))
    assert m[far].max() < 0.015


def test_centres_match_the_reference_function(golden):
    """the bound is DESIGN.md section 17's: the reference's variance is float32 np.var, rule G4's is float64"""
    assert [tuple(c) for c in golden["cases"]] == gr.GOLDEN_CASES
    worst = 0.0
    for k, (w, h, G) in enumerate(gr.GOLDEN_CASES):
        cx, cy, T, empty = gr.centre(gr.field(w, h, seed=k), G)
        dist = float(np.hypot(cx - golden["centres"][k, 0], cy - golden["centres"][k, 1]))
        print(f"{w}x{h} G={G}: ({cx!r}, {cy!r}) against the reference's {tuple(golden['centres'][k])}: {dist:.3e} px")
        assert empty == 0 and T > 0
        worst = max(worst, dist)
        assert dist <= gr.CENTRE_BOUND, (w, h, G, dist)
    assert worst <= gr.CENTRE_BOUND and float(golden["max_distance"]) <= gr.CENTRE_BOUND


def test_constant_field_takes_the_default_centre(golden):
    w, h, G = (int(v) for v in golden["constant_case"])
    f = np.empty((h, w, 2), np.float32)
    f[..., 0], f[..., 1] = np.float32(1.25), np.float32(-0.75)
    cx, cy, T, empty = gr.centre(f, G)
    assert (cx, cy, empty) == (w // 2, h // 2, 1) and T.tobytes() == np.float64(0.0).tobytes()
    assert tuple(golden["constant_centre"]) == (w // 2, h // 2)


def test_a_field_constant_per_cell_has_zero_variance_exactly():
    w, h, G = 53, 37, 5
    gw, gh = gr.geometry(w, h, G)
    rng = np.random.default_rng(3)
    per_cell = rng.standard_normal((G, G, 2)).astype(np.float32) * np.float32(1e4)
    f = rng.standard_normal((h, w, 2)).astype(np.float32)      # the margin is noise: it belongs to no cell
    f[:G * gh, :G * gw] = np.repeat(np.repeat(per_cell, gh, axis=0), gw, axis=1)
    rec = gr.cell_records(f, G)
    assert rec[..., 3].tobytes() == np.zeros((G, G)).tobytes()  # +0.0, bit for bit
    assert gr.centre(f, G)[:2] == (w // 2, h // 2) and gr.centre(f, G)[3] == 1
    assert np.array_equal(rec[..., 0], per_cell[..., 0].astype(np.float64))
    assert np.array_equal(rec[..., 2], gr.magnitude(per_cell).astype(np.float64))


def test_one_two_valued_cell_by_hand():
    """cell (1, 2) of a 4 x 4 grid on 40x24: 60 pixels, 15 of magnitude 5 (flow (3, 4)) and 45 of magnitude 1 (flow (0, 1)),
    every other cell constant.  mean = 2, variance = (15 * 9 + 45 * 1) / 60 = 3 -- all exact in binary."""
    w, h, G = 40, 24, 4
    gw, gh = gr.geometry(w, h, G)
    assert (gw, gh) == (10, 6)
    f = np.zeros((h, w, 2), np.float32)
    f[..., 1] = 1.0
    f[gh:2 * gh, 2 * gw:3 * gw][:, :, :] = (0.0, 1.0)
    cell = f[gh:2 * gh, 2 * gw:3 * gw]
    cell[1:4, 2:7] = (3.0, 4.0)
    rec = gr.cell_records(f, G)
    want = np.zeros((G, G))
    want[1, 2] = 3.0
    assert np.array_equal(rec[..., 3], want)
    assert rec[1, 2].tolist() == [15 * 3.0 / 60, (15 * 4.0 + 45 * 1.0) / 60, 2.0, 3.0]
    cx, cy, T, empty = gr.centre(f, G)
    assert (cx, cy, T, empty) == (2 * gw + gw / 2.0, 1 * gh + gh / 2.0, 3.0, 0)
    assert 2 * gw <= cx < 3 * gw and gh <= cy < 2 * gh          # the centre lies in that cell


@pytest.mark.parametrize("case", gr.GOLDEN_CASES, ids=lambda c: f"{c[0]}x{c[1]}-G{c[2]}")
def test_means_against_numpy(case):
    """mean_u, mean_v and mean_mag against np.mean of the float64 cell: a sum of n terms in another order, n * 2^-53 relative
    to the sum of absolute values at the most; the variance against np.var of the float64 magnitudes likewise (its terms
    are squares of differences from a mean that itself carries such an error)"""
    w, h, G = case
    f = gr.field(w, h, seed=11)
    gw, gh = gr.geometry(w, h, G)
    rec = gr.cell_records(f, G)
    m = gr.magnitude(f).astype(np.float64)
    n = gw * gh
    for i in range(G):
        for j in range(G):
            sl = (slice(i * gh, (i + 1) * gh), slice(j * gw, (j + 1) * gw))
            for k, plane in enumerate((f[..., 0].astype(np.float64), f[..., 1].astype(np.float64), m)):
                tol = (n + 2) * 2.0 ** -53 * float(np.abs(plane[sl]).sum()) / n + 2.0 ** -52 * abs(float(plane[sl].mean()))
                if k == 2:   # S_d is summed about K: its terms are |m - K| <= 2 max m
                    tol = (n + 2) * 2.0 ** -53 * 2 * float(plane[sl].max()) + 2.0 ** -52 * abs(float(plane[sl].mean()))
                assert abs(rec[i, j, k] - plane[sl].mean()) <= tol, (i, j, k)
            var = float(np.var(m[sl]))
            span = float(m[sl].max() - m[sl].min())
            assert rec[i, j, 3] >= 0 and abs(rec[i, j, 3] - var) <= (4 * n + 8) * 2.0 ** -53 * max(4 * span * span, var), (i, j)


def test_remainder_margin_is_never_read():
    w, h, G = 53, 37, 5
    f = gr.field(w, h, seed=4)
    g = f.copy()
    g[35:, :] = np.nan
    g[:, 50:] = 1e30
    assert gr.cell_records(f, G).tobytes() == gr.cell_records(g, G).tobytes()
    g[7, 10] = np.nan   # cell (1, 1)
    rec, ref = gr.cell_records(g, G), gr.cell_records(f, G)
    assert np.isnan(rec[1, 1, 3]) and np.isnan(gr.centre(g, G)[0]) and np.isnan(gr.centre(g, G)[2]) and gr.centre(g, G)[3] == 0
    keep = np.ones((G, G), bool)
    keep[1, 1] = False
    assert rec[keep].tobytes() == ref[keep].tobytes()


def test_block_order_is_part_of_the_rule():
    """a cell that crosses column 256 is the sum of two block partials, not one left-to-right sum"""
    w, h, G = 600, 16, 1
    f = gr.field(w, h, seed=5) + np.float32(100.0)
    K, Su, *_ = gr.cell_sums(f, G)
    col = np.zeros(w)
    for r in range(h):
        col = col + f[r, :, 0].astype(np.float64)
    parts = []
    for b in range(3):
        p = 0.0
        for x in range(b * 256, min(w, b * 256 + 256)):
            p = p + col[x]
        parts.append(p)
    assert Su[0, 0] == (0.0 + parts[0] + parts[1]) + parts[2]


@pytest.mark.parametrize("radius", [0, 1, 6, 32])
@pytest.mark.parametrize("n_seq", [1, 2, 7, 13, 14, 40])
def test_window_is_numpys_mean_of_the_list(n_seq, radius):
    """rule G6 against np.mean(center_list, axis=0) with the list built as FF:1205-1213 builds it, bit for bit, every j"""
    rng = np.random.default_rng(100 * n_seq + radius)
    cen = [tuple(c) for c in rng.uniform(-50, 300, (n_seq, 2))]
    got = gr.window(cen, radius)
    for j in range(n_seq):
        center_list = [cen[j]]
        for i in range(1, radius + 1):
            if j - i >= 0:
                center_list.append(cen[j - i])
            if j + i < n_seq:
                center_list.append(cen[j + i])
        want = np.mean(np.array(center_list), axis=0)
        assert got[j].tobytes() == want.tobytes(), (j, got[j], want)


def test_window_mean_equals_the_sequential_sum_on_random_lists():
    rng = np.random.default_rng(7)
    for _ in range(2000):
        k = int(rng.integers(1, 14))
        lst = rng.uniform(-1e3, 1e3, (k, 2)) * 10.0 ** rng.integers(-3, 4)
        acc = lst[0].copy()
        for row in lst[1:]:
            acc = acc + row
        assert (acc / np.float64(k)).tobytes() == np.mean(lst, axis=0).tobytes()


def test_grid_check_refusals_need_no_device():
    assert _capi.cell_grid(53, 37, 5) == (10, 7) and _capi.cell_grid(1920, 1080, 32) == (60, 33)
    assert _capi.cell_grid(16, 16, 16) == (1, 1) and _capi.cell_grid(192, 136, 64) == (3, 2)
    assert _capi.FFL_MAX_CELLS == gr.MAX_CELLS == 64
    for (w, h, G), rule in (((64, 64, 0), r"rule G1: cells = 0 outside 1\.\.64"), ((256, 256, 65), r"rule G1: cells = 65 outside 1\.\.64"),
                            ((53, 37, 40), r"rule G1: cells = 40 exceeds min\(width, height\) of 53x37")):
        with pytest.raises(_capi.FFLError, match=rule) as e:
            _capi.cell_grid(w, h, G)
        assert e.value.code == _capi.FFL_ERR_INVALID and "ffl_cell_grid_check" in str(e.value)
        with pytest.raises(ValueError, match="rule G1"):
            gr.geometry(w, h, G)
        with pytest.raises(_capi.FFLError, match="rule G1"):
            _capi.cells_extra_bytes(w, h, G)
    assert _capi.cells_extra_bytes(1920, 1080, 32) == 2 * 64 * 256 * 8
    assert _capi.CELL_DTYPE.itemsize == 32 and _capi.GRID_CENTRE_DTYPE.itemsize == 32
    assert _capi.GRID_CENTRE_DTYPE.fields["cells"][1] == 24 and _capi.GRID_CENTRE_DTYPE.fields["empty"][1] == 28


def test_center_keywords_are_checked_on_the_host():
    assert pipeline.center_kwargs({}) == {} and pipeline.center_kwargs({"hip_center": None}) == {}
    assert pipeline.center_kwargs({"hip_center": "variance"}) == {"center": "variance", "cells": 32}
    assert pipeline.center_kwargs({"hip_center": "variance", "hip_center_cells": 8}) == {"center": "variance", "cells": 8}
    with pytest.raises(ValueError, match="hip_center together with hip_weights"):
        pipeline.center_kwargs({"hip_center": "variance", "hip_weights": np.ones((4, 4), np.uint8)})
    with pytest.raises(ValueError, match="center must be None or one of"):
        pipeline.center_kwargs({"hip_center": "argmax"})
    frames = [np.zeros((16, 16), np.uint8)] * 3
    for call in (lambda: pipeline.process_chunk_sharded(None, frames, 0, 1, None, center="variance"),
                 lambda: pipeline.process_chunk_sharded_halo(None, frames, 0, 1, None, center="variance"),
                 lambda: pipeline.process_chunk_local_ranks([None], frames, center="variance")):
        with pytest.raises(ValueError, match="sharded schedules take their centres from the |div| argmax".replace("|", r"\|")):
            call()
