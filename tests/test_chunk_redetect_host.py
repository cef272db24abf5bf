"""The re-detection cases K13 and K14 of tests/test_gpu_chunk_compose.py on the CPU restatements alone (no GPU, no gpu mark): the
lost-and-found clip (chunk_by_hand.lost_clip of the suite's clip), oracle.farneback fields, chunk_by_hand.track_run.  The
device cases are only worth their time if the restatement itself skips, accepts and rejects searches at the batch borders of
both engine contexts (B = 3 and B = 4); here that is shown without a device, and the thresholds are derived.

    K13  threshold 0.614: the float32 mean magnitudes of the 41 oracle fields span 0.3983 .. 1.1835 with the median 0.6117; its
         neighbours are 0.6097 below and 0.6162 above, and 0.614 lies between the median and the pair above it, 0.002 from
         either (the median itself would sit ON a pair).  20 of 41 pairs are cut.
         borders / skipped / accepted onto the true centre / triggered and rejected (POOR | AMBIGUOUS):
         B = 3: 14 / 8 / 5 / 1,   B = 4: 11 / 4 / 5 / 2.
    K14  threshold 0.68: rule Q5 reads the raw means (0.6706 and 0.6844 are the neighbours; 14 of 41 cut), the window the means
         under the ROI maps (median 0.88; neighbours 0.649 and 0.733 at B = 3, 0.646 and 0.706 at B = 4; 28 and 29 of 41 cut) --
         at K13's 0.614 the window would cut 31 of 41, more than three quarters.  reach 20: the jump at frame 7 (some 16 px)
         lies inside it, the jumps at 22 and 30 (more than 30 px) outside.
         track 0 skipped / accepted and moved / rejected: B = 3: 5 / 3 / 6,   B = 4: 2 / 3 / 6;
         track 1 skipped: 12 of 14 and 10 of 11 borders, the others triggered and rejected as AMBIGUOUS."""
import functools

import numpy as np
import pytest

import chunk_by_hand as bh
import post_ref
import weights_ref
from funscript_flow_amd import _capi

W, H, N = 64, 48, 41
BATCHES = (3, 4)      # the B of the device suite's contexts R1 and R2
POOR, AMBIGUOUS = 2, 4


@functools.lru_cache(maxsize=None)
def scene():
    """(frames, oracle fields, float32 mean magnitudes)"""
    frames = bh.lost_clip(bh.suite_clip(N + 1, W, H))
    raw = bh.oracle_fields(frames)
    means = []
    for f in raw:
        mean, ok = post_ref.mean_mag_accepted(f)
        for thr in bh.LOST_THR.values():     # whatever float32 the device rounds the mean to, it lies on the same side
            assert len({bool(v > np.float32(thr)) for v in ok}) == 1
        means.append(np.float32(mean))
    for a in (frames, raw):
        a.setflags(write=False)
    return frames, raw, means


@functools.lru_cache(maxsize=None)
def run(case, batch, n=N):
    frames, raw, means = scene()
    gate = bh.random_map(W, H, bh.LOST_GATE_SEED) if bh.LOST_TRACKS[case].get("roi") else None
    return bh.track_run(frames[:n + 1], raw[:n], means[:n], bh.LOST_THR[case], bh.LOST_TRACKS[case], batch, gate)


def test_the_clip_is_the_recipe():
    frames, _, _ = scene()
    base, path = bh.suite_clip(N + 1, W, H), bh.lost_path(N + 1)
    assert path[0] == (14, 20) and path[6] == (20, 20) and path[7] == (34, 12) and path[27] == (55, 30) and path[28] == (54, 30)
    assert all(8 <= x <= 55 for x, _ in path)
    square = np.random.default_rng(1300).integers(0, 256, (13, 13)).astype(np.uint8)
    for k, (x, y) in enumerate(path):
        patch = frames[k, y - 6:y + 7, x - 6:x + 7]
        if k in (12, 28):
            assert frames[k].tobytes() == base[k].tobytes()
        else:
            assert patch.tobytes() == square.tobytes()
            rest = frames[k] != base[k]
            rest[y - 6:y + 7, x - 6:x + 7] = False
            assert not rest.any()


def test_the_thresholds_are_the_derived_ones():
    _, _, means = scene()
    s = np.sort(np.array(means))
    assert (round(float(s[0]), 4), round(float(s[-1]), 4), round(float(s[N // 2]), 4)) == (0.3983, 1.1835, 0.6117)
    thr = np.float32(bh.LOST_THR["K13"])
    assert s[N // 2] < thr < s[N // 2 + 1] and min(thr - s[N // 2], s[N // 2 + 1] - thr) > 0.002     # between two pairs
    assert int((s > thr).sum()) == 20
    thr = np.float32(bh.LOST_THR["K14"])
    assert np.abs(s - thr).min() > 0.004 and int((s > thr).sum()) == 14


@pytest.mark.parametrize("batch,table", [(3, (14, 8, 5, 1)), (4, (11, 4, 5, 2))])
def test_k13_skips_finds_and_rejects_at_the_borders(batch, table):
    res = run("K13", batch)
    (skipped, moved, rejected, statuses), = bh.check_redetect_conditions("K13", res["redetect"], res["track"], N, batch)
    assert (-(-N // batch), skipped, moved, rejected) == table and statuses == [POOR | AMBIGUOUS]
    # every accepted search puts the state onto the square's true centre, and the next batch starts from there
    rec = np.frombuffer(res["redetect"], _capi.MATCH_DTYPE).reshape(N, 1)
    path = bh.lost_path(N + 1)
    for lo in range(0, N, batch):
        hi = min(lo + batch, N)
        r = rec[hi - 1, 0]
        if r["status"] == 0:
            assert (r["x"], r["y"]) == path[hi] and r["cost"] == 0
        elif r["status"] != _capi.REDETECT_SKIPPED:
            assert hi in bh.LOST["absent"]      # rejected exactly where the square is not in the frame
    state = np.frombuffer(res["state"], _capi.TRACK_STATE_DTYPE)
    assert (state["x"][0], state["y"][0]) == path[N]


@pytest.mark.parametrize("batch,table", [(3, ((5, 3, 6), 12)), (4, ((2, 3, 6), 10))])
def test_k14_reach_and_a_second_track_with_its_own_trigger_words(batch, table):
    res = run("K14", batch)
    got = bh.check_redetect_conditions("K14", res["redetect"], res["track"], N, batch)
    assert (got[0][:3], got[1][0]) == table
    assert got[0][3] == [POOR | AMBIGUOUS] and got[1][1] == 0 and got[1][3] == [AMBIGUOUS]
    # a search that stays inside the reach never moves the state further than the reach
    rec = np.frombuffer(res["redetect"], _capi.MATCH_DTYPE).reshape(N, 2)[[min(lo + batch, N) - 1 for lo in range(0, N, batch)]]
    reach = bh.LOST_TRACKS["K14"]["match"]["redetect"]["reach"]
    ran = rec["status"] != _capi.REDETECT_SKIPPED
    assert ran.any() and (np.abs(rec["dx"][ran]) <= reach).all() and (np.abs(rec["dy"][ran]) <= reach).all()
    # the two thresholds K14's one value serves: rule Q5 on the raw means, the window on the means under the ROI maps
    _, raw, _ = scene()
    cut = (np.frombuffer(res["track"], _capi.TRACK_DTYPE).reshape(N, 2)["status"][:, 0] & 1) != 0
    assert int(cut.sum()) == 14
    maps = np.frombuffer(res["maps"], np.uint8).reshape(N, H, W)
    thr, window = np.float32(bh.LOST_THR["K14"]), 0
    for j in range(N):
        _, ok = weights_ref.mean_mag_accepted(raw[j], maps[j])
        assert len({bool(v > thr) for v in ok}) == 1
        window += bool(ok[0] > thr)
    assert N / 4 <= window <= 3 * N / 4 and window == {3: 28, 4: 29}[batch]


@pytest.mark.parametrize("n", [1, 5, 7, 13])
def test_short_chunks_write_one_record_per_border(n):
    res = run("K13", 3, n)
    got = bh.border_searches(res["redetect"], n, 1, 3)
    assert sum(got[0][:3]) <= -(-n // 3) and len(res["redetect"]) == n * 48


def test_a_state_carried_over_a_batch_border_is_the_one_chunk_run():
    """pairs 0 .. 20 capturing, pairs 21 .. 40 from the state and templates the first chunk left: records, state and templates
    are the one-chunk run's (21 is a border of B = 3)"""
    frames, raw, means = scene()
    whole, first = run("K13", 3), run("K13", 3, 21)
    track = dict(bh.LOST_TRACKS["K13"], state=np.frombuffer(first["state"], _capi.TRACK_STATE_DTYPE), capture=False,
                 templates=first["templates"])
    second = bh.track_run(frames[21:], raw[21:], means[21:], bh.LOST_THR["K13"], track, 3)
    for key in ("track", "match", "redetect"):
        assert first[key] + second[key] == whole[key], key
    assert second["state"] == whole["state"] and second["templates"] == first["templates"] == whole["templates"]
