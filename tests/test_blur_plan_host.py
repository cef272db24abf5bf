"""The launch plan of k_blur_solve (ffl_blur_plan) through ffl_debug_blur_plan, which enumerates a launch on the host with
the kernel's own workgroup mapping: whatever the taper does, every tile of every pair is walked exactly once, and with
taper off the launch is the one it always was.  No device is needed."""
import itertools

import numpy as np
import pytest

from funscript_flow_amd import _capi

TILES_Y = (1, 2, 3, 5, 9, 35, 68)
TILES_X = (1, 4, 5, 30)
PAIRS = (1, 2, 3, 32, 256)
PANEL_W = 4   # FFL_PANEL_W


def auto_rows(tiles_x, tiles_y, nB, min_wgs=3500):
    """ffl_blur_rows_per_wg, restated"""
    if nB > 32 and tiles_x * tiles_y >= 256:
        nB = 32
    for s in range(1, tiles_y + 1):
        nrb = -(-tiles_y // s)
        if nrb > 64:
            continue
        if tiles_x * -(-tiles_y // nrb) * nB >= min_wgs or nrb == 1:
            return nrb
    return 1


def uniform_launch(tiles_x, strips, nB, order):
    """the launch as it was before plans existed: ffl_tile_grid and ffl_tile_coord, restated -> (grid, {block: (pair, tile
    column, strip row)}) without the padding workgroups"""
    T = tiles_x * strips
    chunk = (T + 7) // 8
    grid = chunk * 8 * nB
    out = {}
    for blk in range(grid):
        if order == 0:
            b, l = divmod(blk, chunk * 8)
            t = (l & 7) * chunk + (l >> 3)
        else:
            tt, b = divmod(blk >> 3, nB)
            t = (blk & 7) * chunk + tt
        if t >= T:
            continue
        panel, within = divmod(t, PANEL_W * strips)
        pw = min(PANEL_W, tiles_x - panel * PANEL_W)
        sy, dx = divmod(within, pw)
        out[blk] = (b, panel * PANEL_W + dx, sy)
    return grid, out


def check_plan(tiles_x, tiles_y, nB, segments, grid, blocks):
    """the properties every plan has; returns the segments' strip lengths"""
    assert 1 <= len(segments) <= 3
    first, pair0 = 0, 0
    for (fb, fp, pairs, nrb, strips) in segments:
        assert pairs >= 1 and nrb >= 1 and strips == -(-tiles_y // nrb)
        assert fb == first and fb % 8 == 0 and fp == pair0
        first += -(-(tiles_x * strips) // 8) * 8 * pairs      # each segment padded to 8 per pair (ffl_tile_grid)
        pair0 += pairs
    assert grid == first == len(blocks) and pair0 == nB
    rows = [s[3] for s in segments]
    assert rows == sorted(rows, reverse=True)                 # strips never grow towards the launch's end
    # every (pair, tile column, tile row) exactly once
    blocks = np.asarray(blocks)
    live = np.flatnonzero(blocks[:, 0] >= 0)
    b, tx, r0, n = blocks[live].T
    seg = np.asarray(segments)[np.searchsorted([s[0] for s in segments], live, side="right") - 1]
    fp, pairs, nrb = seg[:, 1], seg[:, 2], seg[:, 3]
    assert ((fp <= b) & (b < fp + pairs) & (0 <= tx) & (tx < tiles_x) & (r0 % nrb == 0)).all()
    assert ((n == np.minimum(nrb, tiles_y - r0)) & (n >= 1)).all()
    cover = np.zeros((nB, tiles_x, tiles_y), np.int32)
    for k in range(int(n.max())):
        m = n > k
        np.add.at(cover, (b[m], tx[m], r0[m] + k), 1)
    assert (cover == 1).all()
    return rows


@pytest.mark.parametrize("tiles_x", TILES_X)
@pytest.mark.parametrize("tiles_y", TILES_Y)
def test_taper_off_is_the_launch_as_it_was(tiles_x, tiles_y):
    for nB, order, rows in itertools.product(PAIRS, (0, 1), (0, 3)):
        segments, grid, blocks = _capi.blur_plan(tiles_x, tiles_y, nB, 1024, blur_rows=rows, tile_order=order)
        nrb = rows or auto_rows(tiles_x, tiles_y, nB)
        strips = -(-tiles_y // nrb)
        want_grid, want = uniform_launch(tiles_x, strips, nB, order)
        assert segments == [(0, 0, nB, nrb, strips)] and grid == want_grid
        got = {blk: (b, tx, r0 // nrb) for blk, (b, tx, r0, n) in enumerate(blocks.tolist()) if b >= 0}
        assert got == want
        check_plan(tiles_x, tiles_y, nB, segments, grid, blocks)


@pytest.mark.parametrize("tiles_x", TILES_X)
@pytest.mark.parametrize("tiles_y", TILES_Y)
def test_forced_taper_covers_every_tile_once(tiles_x, tiles_y):
    for nB, P, rows, order in itertools.product(PAIRS, (1, 3), (0, 1, 3, 8, 17), (0, 1)):
        if order == 1 and (rows or nB == 256):
            continue   # tile-major: the automatic strips, small batches
        segments, grid, blocks = _capi.blur_plan(tiles_x, tiles_y, nB, 1024, blur_rows=rows, blur_taper_pairs=P, tile_order=order)
        got = check_plan(tiles_x, tiles_y, nB, segments, grid, blocks)
        nrb = rows or auto_rows(tiles_x, tiles_y, nB)
        p2 = min(P, nB)
        p1 = min(P, nB - p2)
        want = [(nB - p1 - p2, nrb), (p1, -(-nrb // 2)), (p2, max(1, -(-nrb // 4)))]
        assert [(s[2], s[3]) for s in segments] == [w for w in want if w[0]], (nB, P, rows)   # empty segments are left out
        assert got[-1] == max(1, -(-nrb // 4))


def test_no_bulk_left():
    """nB = 1 or 2 with P = 1: the taper takes every pair"""
    segments, grid, blocks = _capi.blur_plan(4, 9, 1, 1024, blur_rows=8, blur_taper_pairs=1)
    assert segments == [(0, 0, 1, 2, 5)] and grid == 24
    segments, grid, blocks = _capi.blur_plan(4, 9, 2, 1024, blur_rows=8, blur_taper_pairs=1)
    assert segments == [(0, 0, 1, 4, 3), (16, 1, 1, 2, 5)] and grid == 16 + 24
    check_plan(4, 9, 2, segments, grid, blocks)


@pytest.mark.parametrize("slots", (768, 1024))
@pytest.mark.parametrize("tiles_x", TILES_X)
@pytest.mark.parametrize("tiles_y", TILES_Y)
def test_automatic_taper(tiles_x, tiles_y, slots):
    """blur_taper = 1: levels whose bulk strips exceed 2 tiles get two taper segments of P pairs each, whose bulk
    workgroups would fill about half a round of the slots together and which never hold more than half the launch; where
    that rounds to no pair -- fewer than 4 pairs, or one pair alone exceeds half a round -- and on the other levels the
    launch is left alone"""
    for nB in PAIRS:
        segments, grid, blocks = _capi.blur_plan(tiles_x, tiles_y, nB, slots, blur_taper=1)
        check_plan(tiles_x, tiles_y, nB, segments, grid, blocks)
        nrb = auto_rows(tiles_x, tiles_y, nB)
        off = _capi.blur_plan(tiles_x, tiles_y, nB, slots, blocks=False)[0]
        per_pair = tiles_x * -(-tiles_y // nrb)
        P = min((slots + 2 * per_pair) // (4 * per_pair), nB // 4)
        if nrb <= 2 or nB < 4 or 2 * per_pair > slots:
            assert segments == off
            continue
        assert P >= 1 and [s[2] for s in segments] == [nB - 2 * P, P, P]
        assert 4 * P <= nB and 4 * P * per_pair <= slots + 2 * per_pair


def test_automatic_taper_leaves_small_batches_of_large_frames_alone():
    """3840 x 2160 with 2 pairs: one pair's 2040 workgroups are two rounds of the slots already"""
    for nB in (1, 2, 3, 4):
        on = _capi.blur_plan(60, 135, nB, 1024, blur_taper=1, blocks=False)
        assert on == _capi.blur_plan(60, 135, nB, 1024, blocks=False) and len(on[0]) == 1, nB


def test_the_flagship_level_0():
    """1080p, B = 32, level 0: 30 x 68 tiles; strips of 17 tiles, 120 workgroups per pair"""
    assert _capi.blur_plan(30, 68, 32, 1024, blocks=False)[:2] == ([(0, 0, 32, 17, 4)], 3840)
    segments, grid, _ = _capi.blur_plan(30, 68, 32, 1024, blur_taper=1, blocks=False)
    assert segments == [(0, 0, 28, 17, 4), (3360, 28, 2, 9, 8), (3840, 30, 2, 5, 14)] and grid == 3840 + 2 * 424
    segments, grid, _ = _capi.blur_plan(30, 68, 32, 768, blur_taper=1, blocks=False)
    assert [s[2] for s in segments] == [28, 2, 2]


def test_refusals():
    for bad in (dict(tiles_x=0), dict(n_pairs=0), dict(n_pairs=257), dict(slots=-1), dict(blur_rows=65), dict(blur_taper=2),
                dict(blur_taper_pairs=257), dict(tile_order=2), dict(blur_min_wgs=0)):
        kw = dict(tiles_x=4, tiles_y=9, n_pairs=2, slots=1024)
        kw.update(bad)
        with pytest.raises(ValueError):
            _capi.blur_plan(**kw)
