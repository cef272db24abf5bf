"""The composed chunk schedules under slot recycling, on the device, against by-hand runs (tests/chunk_by_hand.py): bytes, no
tolerance anywhere.

One aperiodic clip -- 41 pairs of 64x48 whose period (53) is longer than the chunk, so no two pairs are the same bytes and a
read of a stale slot, of another pair's map or of another pair's centre cannot hide -- goes through two engine contexts that
both wrap their flow-slot ring:

    R1   B = 3, depth 1, 8 frame slots, 19 flow slots: 14 batches, a ragged last batch of 2, the ring wraps twice;
    R2   B = 4, depth 2, 15 frame slots, 25 flow slots: 11 batches, the last batch is one pair.

Every case of CASES runs through process_chunk (device schedule; the host schedule where the keywords allow one) and, K1-K5,
K10 and K12, through process_flows fed with the by-hand raw fields, once as one array and (but K12) once as segments (5, 1, 35).  Post records,
motion records, cell grids, ALL n flows_out fields and the pass-1 records are compared with by_hand's on bytes.

The cut thresholds put about half the pairs on either side of the cut test, so the cut path, its zero records and the uncut
path all run.  They come from CPU references (oracle.farneback, fb_flags_ref and dis_ref fields, motion_ref fits, the exact
mean of weights_ref), not from a device run: 0.44 for raw fields (CPU mean_mag 0.225 .. 0.629, median 0.441), 0.145 for
compensated ones (0.079 .. 0.205, medians 0.141 .. 0.150 over the four models and maps), 0.18 for compensated Gaussian-window
fields (median 0.180) and 0.10 for compensated DIS fields (median 0.1035).  The conditions themselves are asserted on the
by-hand result (test_the_clip_and_the_thresholds_do_their_work).

K7-K14 are the modes that make their maps or their centres behind a batch (DESIGN.md sections 18, 21-25), K7, K8, K11, K13 and
K14 from the batch's FRAME slots: K7 weights="residual" with texture=, a static gate and compensate="translation"; K8 weights="texture"
with explicit parameters and compensate="affine"; K9 weights="consistency" with a gate (the batch is halved: one pair per
batch on R1, two on R2, and the split ring wraps); K10 center="track", three tracks from a state tensor, on_cut="home", also
through process_flows; K11 center="track" with roi, a gate and match (p = 6, s = 4, accept-everything thresholds so that
every match is stored, capture on), on_cut="hold", against by_hand at the context's B; K12 one track under
compensate="rigid".  weights_out, track_out, the state tensor, match_out and the templates are compared on bytes as well, and
check_mode_anchors ties the by-hand maps, track records, state, match records and templates to the CPU restatements.
Where the records are weighted the threshold is the median weighted mean_mag of the 41 pairs, derived on the CPU
(oracle.farneback fields in both directions, the map restatements of chunk_by_hand.mode_maps, motion_ref fits under the maps,
the exact weighted mean of weights_ref): K7 0.139 (0.0761 .. 0.1909, median 0.1388, its neighbours 0.1386 and 0.1456), K8
0.139 (0.0845 .. 0.2054, median 0.1387, next 0.1423), K9 0.44 (0.2188 .. 0.6347, median 0.4413, the value below 0.4308).
K11's threshold serves two tests: rule Q5 of the track reads the RAW unweighted mean_mag (median 0.441) and the window the
mean under the ROI maps of chunk_by_hand.track_run (0.2653 .. 0.7451, median 0.545, the same to four digits at B = 3 and 4);
0.48 lies between the two medians and cuts 18 of 41 pairs for the track and 24 of 41 for the window.  K12 runs at 0.145: every
raw mean_mag lies above it, so the track, which reads the raw fields, must see EVERY pair as cut while the window cuts about
half -- an advance queued behind the subtraction would cut about half and change the bytes.

K13 and K14 are track["match"]["redetect"].  The suite's clip never loses its subject -- with a template
from frame 0 every search about the state reads OK and every re-detection is SKIPPED -- so they run on a clip of their own,
chunk_by_hand.lost_clip: the suite's clip with a 13x13 square of random bytes that walks 1 px per frame, jumps at frames 7, 16,
22, 30 and 37 and is absent from frames 12 and 28 (both batch borders of R1, and of R2).  K13: one track on the square, radius
9, on_cut="hold", match p = 6, s = 4 with the library's default thresholds, redetect=True, capture on; K14: the dict form
(reach 20, exclude 4), a second track on the background whose trigger words differ from track 0's, and roi with a static
gate.  redetect_out is pre-filled with 0xA5 and compared whole, so the records and "no other entry is written" are one
comparison.  What the CPU restatements give on this clip -- the counts of skipped, accepted and rejected searches on either
context, the thresholds 0.614 (K13: the raw means' median 0.6117 and its neighbour 0.6162 on either side) and 0.68 (K14: between
the raw median and the 0.88 of the means under the ROI maps, as K11's) -- is derived and asserted without a device in
tests/test_chunk_redetect_host.py; the conditions are asserted again here on the by-hand result
(chunk_by_hand.check_redetect_conditions).  K13 also runs as two chunks split at pair 21 with the state and the templates
carried over (test_a_carried_state_re_detects_as_the_one_chunk_run), and among the short chunks.

DIS refuses 64x48 (rule D2: the coarsest scale would lie below the finest), so its row runs the same clip at 128x96, the
smallest size of this aspect it accepts.

What turns these tests red, tried with pipeline.py edited by hand (plain Python, every slot index still checked by the
library): _ChunkMotion.behind taking its slots % (ring + 1) -- every compensated case, the library refuses slot `ring`;
_DevicePost._maps(j0) -> _maps(0) -- K3, K5 and the leak test on the bytes of nearly every record; the window calls queued
before cell_stats -- K4 on bytes (not on every context: the schedule's centre buffer may be handed the memory of the chunk
before it, with the same centres in it; the host ledger test sees it always); flows_out exported before the subtraction --
every flows_out of K1, K2, K4 and K6.  A flow ring ONE slot shorter than min_flow_slots changes no byte here: the bound has
that one slot to spare (test_chunk_schedule_host.py derives it), and a ring short enough to hand the device schedule's
window call a stale neighbour also repeats a slot inside that call's seq, which the library refuses.
The eleven hand edits that test_chunk_schedule_host.py's docstring lists, tried here on the device as well: the residual
hook's flow slots % (flow_slots - 1), its maps slice one short, the texture combine ahead of the residual call -- K7 (and the
leak test, as under every edit below); the fit chained ahead of the advance -- K12; the records' match on f1, the state's
match on f0[-1], roi_weights ahead of track_match, capture never cleared -- K11; centres() with an item of 48 -- K10 and K11;
with_frames handed the previous batch's slots -- K7, K8 and K11.  The fit handed the ROI maps under a track changes no byte
here (no case fits under a track WITH roi); the host ledger's compensate-track-roi-match set sees it.
Four of the six edits of the re-detection call that the host file lists, tried here as well; the library refuses none of them
(every slot, span and stride is a valid one), the bytes show each: (a) the re-detection on f0[-1] -- K13 and K14 on both
contexts from the first jump on (post records from pair 6, the track records of the batches behind a search that found the
square one frame early), K13 among the short chunks on the final state at n = 7, and the two-chunk run; (b) the output at
ls[0] -- the same tests on redetect_out alone: every batch's first record is written and its last keeps 0xA5 (the batches of
one pair agree); (c) the trigger the batch's match_out span -- the same tests, post records from pair 2 or 3 on and the state;
(e) the centres the batch's records -- the same tests, every post record, and redetect_out at n = 1.  Under each of the four
the leak test is red on both contexts as well, and nothing else of the file."""
import functools
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import chunk_by_hand as bh
from funscript_flow_amd import _capi, pipeline
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
W, H, N = 64, 48, 41
CELLS = 8
CONTEXTS = {"R1": dict(B=3, depth=1, frame_slots=2 * 3 + 2, flow_slots=pipeline.min_flow_slots(3)),
            "R2": dict(B=4, depth=2, frame_slots=pipeline.min_frame_slots(4, 2), flow_slots=pipeline.min_flow_slots(4, 2))}
RAW, COMP = 0.44, 0.145


# ---- the parameters of K7-K14 (plain data and host arrays: the thresholds below derive from them on the CPU, without a device;
# K13's and K14's tracks and thresholds are chunk_by_hand.LOST_TRACKS and LOST_THR, which the host test shares) ---------------------
def GATE7():
    return bh.random_map(W, H, 700)


def GATE9():
    return bh.random_map(W, H, 900)


def GATE11():
    return bh.random_map(W, H, 1100)


def GATE14():
    return bh.random_map(W, H, bh.LOST_GATE_SEED)


TEXTURE8 = {"radius": 3, "tau": 8.0, "soft": 1}
LOOSE = {"min_var": 0.0, "max_mse": 65025.0, "ratio": 1.0}          # accepts every match: the write-back always stores
TRACK10 = dict(state=pipeline.track_state_array([(40.0, 24.0), (5.0, 40.0), (33.0, 31.0)], home=[(32.0, 24.0)] * 3), radius=9,
               on_cut="home")
TRACK11 = dict(state=pipeline.track_state_array([(40.0, 24.0), (20.0, 30.0)]), radius=9, on_cut="hold", roi=(20.0, 12.0),
               match={"p": 6, "s": 4, "mode": "zssd", **LOOSE}, capture=True)
TRACK12 = dict(state=pipeline.track_state_array([(40.0, 24.0)]), radius=9, on_cut="hold")
# ---- the thresholds of K7-K11: see the module docstring ------------------------------------------------------------------------
THR7, THR8, THR9, THR11 = 0.139, 0.139, 0.44, 0.48
CASES = {
    "K0": dict(kw=dict(axes=True), thr=RAW, povs=(False, True), host=True, contexts=("R1", "R2")),
    "K1": dict(kw=dict(axes=True, compensate="translation"), flows_out="nhwc", thr=COMP, povs=(False, True), host=True, contexts=("R1", "R2")),
    "K2": dict(kw=dict(compensate={"model": "affine", "iterations": 2, "tau": 0.5}), maps="static", flows_out="nchw", thr=COMP,
               povs=(False, True), contexts=("R1", "R2")),
    "K3": dict(kw=dict(compensate="rigid"), maps="padded", thr=COMP, povs=(False,), contexts=("R1", "R2")),
    "K4": dict(kw=dict(compensate="similarity", center="variance", cells=CELLS), grid=True, flows_out="nhwc", thr=COMP,
               povs=(False, True), contexts=("R1", "R2")),
    "K5": dict(kw=dict(), maps="pair", thr=RAW, povs=(False, True), contexts=("R1", "R2")),
    "K6-dis": dict(kw=dict(axes=True, compensate="translation"), flows_out="nhwc", thr=0.10, povs=(False,), contexts=("R1",),
                   engine=dict(flow="dis"), size=(128, 96)),
    "K6-gaussian": dict(kw=dict(axes=True, compensate="translation"), flows_out="nhwc", thr=0.18, povs=(False,), contexts=("R1",),
                        engine=dict(window="gaussian")),
    "K7": dict(kw=dict(weights="residual", texture=True, compensate="translation"), gate=GATE7, flows_out="nhwc", thr=THR7,
               povs=(False, True), contexts=("R1", "R2")),
    "K8": dict(kw=dict(weights="texture", texture=TEXTURE8, compensate="affine"), flows_out="nchw", thr=THR8, povs=(False,),
               contexts=("R1", "R2")),
    "K9": dict(kw=dict(weights="consistency"), gate=GATE9, thr=THR9, povs=(False,), contexts=("R1", "R2")),
    "K10": dict(kw=dict(center="track"), track=TRACK10, thr=RAW, povs=(False,), contexts=("R1", "R2")),
    "K11": dict(kw=dict(center="track"), track=TRACK11, gate=GATE11, thr=THR11, povs=(False,), contexts=("R1", "R2")),
    "K12": dict(kw=dict(center="track", compensate="rigid"), track=TRACK12, thr=COMP, povs=(False,), contexts=("R1", "R2")),
    "K13": dict(kw=dict(center="track"), track=bh.LOST_TRACKS["K13"], clip="lost", thr=bh.LOST_THR["K13"], povs=(False,),
                contexts=("R1", "R2")),
    "K14": dict(kw=dict(center="track"), track=bh.LOST_TRACKS["K14"], clip="lost", gate=GATE14, thr=bh.LOST_THR["K14"], povs=(False,),
                contexts=("R1", "R2")),
}
FLOWS_CASES = {"K1": ("flows", "segments"), "K2": ("flows", "segments"), "K3": ("flows", "segments"), "K4": ("flows", "segments"),
               "K5": ("flows", "segments"), "K10": ("flows", "segments"), "K12": ("flows",)}
SHORT = (1, 5, 7, 13)      # one pair; shorter than the radius; radius + 1; exactly one full window


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to(DEV)


@functools.lru_cache(maxsize=None)
def clip(w=W, h=H):
    fr = sine_translate_frames(N + 1, w, h, seed=3, zoom=0.03, period=53, amp=(6.0, 3.0))
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def lost():
    """the clip of K13 and K14: the suite's with the lost-and-found square pasted in (chunk_by_hand.lost_clip)"""
    assert bh.suite_clip(N + 1, W, H).tobytes() == clip().tobytes()
    fr = bh.lost_clip(clip())
    fr.setflags(write=False)
    return fr


def frames_of(case):
    return lost() if CASES[case].get("clip") == "lost" else clip(*size_of(case))


@functools.lru_cache(maxsize=None)
def oracle_raw(kind=None):
    return bh.oracle_fields(lost() if kind == "lost" else clip())


def size_of(case):
    return CASES[case].get("size", (W, H))


@functools.lru_cache(maxsize=None)
def maps_of(kind, w, h, n):
    """the case's maps as a host array: one static map, or one per pair (a different seed each)"""
    m = bh.random_map(w, h, 500) if kind == "static" else bh.pair_maps(w, h, N, 600)[:n]
    m.setflags(write=False)
    return m


def device_maps(kind, w, h, n):
    if kind is None:
        return None
    m = maps_of(kind, w, h, n)
    return bh.padded(m, DEV) if kind == "padded" else dev(m)


def hand_kw(case):
    c, kw = CASES[case], dict(CASES[case]["kw"])
    kw.pop("axes", None)
    eng = c.get("engine", {})
    if "flow" in eng:
        kw["algo"] = (eng["flow"], None)
    if "window" in eng:
        kw["window"] = eng["window"]
    if "track" in c:
        kw["track"] = c["track"]
    return kw


def hand_batch(case, B):
    """The batch by_hand walks a track in.  The state's match happens at batch borders, so with a match it is the context's B;
    without one the records do not depend on it and one by-hand run (in batches of 5) serves both contexts."""
    track = CASES[case].get("track")
    if track is None:
        return None
    return B if track.get("match") is not None else 5


@functools.lru_cache(maxsize=None)
def hand(case, pov, n=N, batch=None):
    """by_hand of the case's first n pairs, computed once and left unchanged"""
    c = CASES[case]
    w, h = size_of(case)
    kw = hand_kw(case)
    with bh.hand_context(w, h, n, reverse=kw.get("weights") == "consistency") as one:
        kind = c.get("maps")
        if kind is not None:
            kw["weights"] = dev(maps_of(kind, w, h, n))        # contiguous here, whatever view the engine gets
        if "gate" in c:
            kw["gate"] = dev(c["gate"]())
        res = bh.by_hand(one, frames_of(case)[:n + 1], pov=pov, thr=c["thr"], batch=batch, **kw)
        assert one.graph_stats()["capture_failures"] == 0
    for v in (res["flows"], res["raw"]):
        v.setflags(write=False)
    return res


def engine_context(name, case):
    c = CONTEXTS[name]
    w, h = size_of(case)
    return _capi.Context(w, h, max_batch=c["B"], frame_slots=c["frame_slots"], flow_slots=c["flow_slots"])


def same(got, want, item, what):
    """bytes against bytes; names the records that differ"""
    if got == want:
        return
    assert len(got) == len(want), f"{what}: {len(got)} bytes, by hand {len(want)}"
    g, w = np.frombuffer(got, np.uint8).reshape(-1, item), np.frombuffer(want, np.uint8).reshape(-1, item)
    raise AssertionError(f"{what}: items {np.flatnonzero((g != w).any(axis=1)).tolist()} of {len(g)} differ from the by-hand run")


def run(eng, ctx, case, pov, schedule, entry, n=N):
    """one chunk through the engine, every output against by_hand's"""
    c, want = CASES[case], hand(case, pov, n, hand_batch(case, ctx.max_batch))
    w, h = size_of(case)
    what = f"{case} pov={pov} {schedule} {entry} n={n}"
    kw = dict(c["kw"])
    kind = c.get("maps")
    if kind is not None:
        kw["weights"] = device_maps(kind, w, h, n)
    mo = grid = T = None
    outs = {}       # the buffers a mode fills, by the key of by_hand's result: (tensor, item size)
    fill = lambda nbytes: torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)   # noqa: E731
    if "gate" in c:
        kw["weights_gate"] = dev(c["gate"]())
    track = c.get("track")
    if isinstance(kw.get("weights"), str) or (track is not None and track.get("roi") is not None):
        kw["weights_out"] = torch.full((n, h, w), 0xA5, dtype=torch.uint8, device=DEV)
        outs["maps"] = (kw["weights_out"], h * w)
    if track is not None:
        nt = len(track["state"]) * 48
        state = dev(np.array(track["state"]).view(np.uint8))
        kw["track"] = {"state": state, **{k: track[k] for k in ("radius", "on_cut", "roi") if k in track}}
        kw["track_out"] = fill(n * nt)
        outs["track"], outs["state"] = (kw["track_out"], nt), (state, nt)
        if track.get("match") is not None:
            assert entry == "chunk" and track["capture"]
            tmpl = pipeline.match_templates(ctx, len(track["state"]), track["match"]["p"])
            kw["track"]["match"] = {**track["match"], "templates": tmpl, "capture": True}
            kw["match_out"] = fill(n * nt)
            outs["match"], outs["templates"] = (kw["match_out"], nt), (tmpl, (2 * track["match"]["p"] + 1) ** 2)
            if track["match"].get("redetect"):      # pre-filled: the records that are no batch's last pair must stay untouched
                kw["redetect_out"] = fill(n * nt)
                outs["redetect"] = (kw["redetect_out"], nt)
    if "compensate" in kw:
        mo = kw["motion_out"] = torch.full((n * 64,), 0xA5, dtype=torch.uint8, device=DEV)
    if c.get("grid"):
        grid = kw["grid_out"] = torch.full((n * CELLS * CELLS * _capi.CELL_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device=DEV)
    if entry == "chunk":
        src = list(frames_of(case)[:n + 1])
        if c.get("flows_out"):
            T = kw["flows_out"] = torch.full((n, h, w, 2) if c["flows_out"] == "nhwc" else (n, 2, h, w), float("nan"), device=DEV)
        call = eng.process_chunk
    else:
        raw = dev(want["raw"])
        src = raw if entry == "flows" else [raw[:5], raw[5], raw[6:]]
        if entry == "segments":
            assert [len(raw[:5]), 1, len(raw[6:])] == [5, 1, 35]
        call = eng.process_flows
    item = _capi.PASS2_AXES_DTYPE.itemsize
    if schedule == "device":
        buf = call(src, pov, c["thr"], post_out=True, **kw)
        same(buf.cpu().numpy().tobytes(), want["post"], item, what + ": post records")
    else:
        comps, recs = call(src, pov, c["thr"], **kw)
        rec = bh.records(want["post"])
        cols = np.stack([rec[k] for k in ("dot", "tangential", "shift_x", "shift_y")], axis=1)
        same(np.ascontiguousarray(comps).tobytes(), np.ascontiguousarray(cols).tobytes(), 32, what + ": components")
        assert bh.rec_bytes(recs) == bh.rec_bytes(want["pass1"]), what + ": pass-1 records"
    if mo is not None:
        same(mo.cpu().numpy().tobytes(), want["motion"], 64, what + ": motion records")
    if grid is not None:
        same(grid.cpu().numpy().tobytes(), want["grid"], CELLS * CELLS * _capi.CELL_DTYPE.itemsize, what + ": cell grids")
    if T is not None:
        got = T.cpu().numpy() if c["flows_out"] == "nhwc" else T.permute(0, 2, 3, 1).contiguous().cpu().numpy()
        same(got.tobytes(), want["flows"].tobytes(), h * w * 8, what + ": flows_out")
    for key, (t, size) in outs.items():
        assert want[key] is not None, key
        same(t.cpu().numpy().tobytes(), want[key], size, f"{what}: {key}")


def plain_chunk(eng, case):
    return eng.process_chunk(list(clip(*size_of(case))), post_out=True, axes=True).cpu().numpy().tobytes()


def runs_of(case):
    c = CASES[case]
    runs = [(pov, "device", "chunk") for pov in c["povs"]]
    if c.get("host"):
        runs += [(pov, "host", "chunk") for pov in c["povs"]]
    if case in FLOWS_CASES:
        runs += [(pov, "device", entry) for pov in c["povs"] for entry in FLOWS_CASES[case]]
    random.Random(case).shuffle(runs)      # a fixed shuffled order
    return runs


def check_track_conditions(case, res, batch=None):
    """what the tracked cases were chosen for: K10, K11, K13 and K14 meet rule Q5's cut and the uncut step on at least a quarter
    of their records each; K11, K13 and K14 store matches on both sides of a cut; K12's track, which reads the RAW fields against
    the compensated threshold, sees every pair as cut (an advance queued behind the subtraction would see about half); K13 and
    K14 skip, accept and reject whole-frame searches at the borders of batches of `batch` pairs
    (chunk_by_hand.check_redetect_conditions)"""
    if res["track"] is None:
        return
    if res["redetect"] is not None:
        bh.check_redetect_conditions(case, res["redetect"], res["track"], N, batch)
    T = len(CASES[case]["track"]["state"])
    cut = (np.frombuffer(res["track"], _capi.TRACK_DTYPE).reshape(N, T)["status"] & 1) != 0
    if case == "K12":
        assert min(r[3] for r in res["raw_pass1"]) > COMP and cut.all()
        return
    assert cut.size / 4 <= int(cut.sum()) <= 3 * cut.size / 4
    if res["match"] is not None:
        stored = (np.frombuffer(res["match"], _capi.MATCH_DTYPE).reshape(N, T)["status"] == 0).any(axis=1)
        assert any(stored[:k].any() and stored[k + 1:].any() for k in np.flatnonzero(cut[:, 0])), "no cut with stored matches on both sides"


# ---- the by-hand runs themselves ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,pov", [(k, p) for k, c in CASES.items() for p in c["povs"]], ids=lambda v: str(v))
def test_the_clip_and_the_thresholds_do_their_work(case, pov, capsys):
    """the conditions the clip and the thresholds were chosen for, on the by-hand result, and its two CPU anchors"""
    c = CASES[case]
    tuned = "engine" not in c
    for batch in sorted({hand_batch(case, r["B"]) for r in CONTEXTS.values()}, key=str):
        res = hand(case, pov, N, batch)
        bh.check_anchors(res, oracle_raw(c.get("clip")) if tuned else None)
        bh.check_mode_anchors(res, frames_of(case), thr=c["thr"], gate=c["gate"]() if "gate" in c else None, track=c.get("track"),
                              batch=batch, **{k: v for k, v in c["kw"].items() if k in ("weights", "residual", "texture", "consistency", "center")})
        assert (res["redetect"] is not None) == (case in ("K13", "K14"))
        check_track_conditions(case, res, batch)
        rec = bh.records(res["post"])
        assert len(rec) == N
        assert len({f.tobytes() for f in res["raw"]}) == N and len({f.tobytes() for f in res["flows"]}) == N    # no two pairs alike
        centres = len(set(zip(rec["x"].tolist(), rec["y"].tolist())))
        cuts = int((rec["cut"] != 0).sum())
        with capsys.disabled():
            print(f"\n  {case} pov={pov} thr={CASES[case]['thr']}: {cuts} of {N} pairs cut, {centres} distinct centres, mean_mag "
                  f"{float(rec['mean_mag'].min()):.4f} .. {float(rec['mean_mag'].max()):.4f}")
        if not pov:
            assert centres >= N / 2
        assert N / 4 <= cuts <= 3 * N / 4
        if res["motion"] is not None:
            models = np.frombuffer(res["motion"], _capi.MOTION_DTYPE)
            assert (models["status"] == 0).all() and len({m.tobytes() for m in models}) == N


# ---- the engine against them ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,name", [(k, r) for k, c in CASES.items() for r in c["contexts"]], ids=lambda v: str(v))
def test_composed_chunk_on_a_wrapping_ring_is_the_by_hand_run(case, name):
    c = CONTEXTS[name]
    assert c["flow_slots"] < N and -(-N // c["B"]) == {"R1": 14, "R2": 11}[name] and N % c["B"] == {"R1": 2, "R2": 1}[name]
    with engine_context(name, case) as ctx:
        eng = pipeline.PairEngine(ctx, depth=c["depth"], **CASES[case].get("engine", {}))
        before = plain_chunk(eng, case)
        for pov, schedule, entry in runs_of(case):
            run(eng, ctx, case, pov, schedule, entry)
        assert plain_chunk(eng, case) == before
        assert ctx.graph_stats()["capture_failures"] == 0
    # the rings are the smallest the engine accepts: R1 wraps twice, R2 once and most of a second time
    assert (c["frame_slots"], c["flow_slots"]) == {"R1": (8, 19), "R2": (15, 25)}[name]


@pytest.mark.parametrize("name", list(CONTEXTS))
def test_cases_leave_nothing_behind_for_the_next(name):
    """every 64x48 case of the tuned engine on ONE context, in a fixed shuffled order; the plain chunk before and after"""
    c = CONTEXTS[name]
    runs = [(case, pov) for case in CASES if "engine" not in CASES[case] for pov in CASES[case]["povs"]]
    assert {case for case, _ in runs} == {f"K{i}" for i in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14)}
    random.Random(name).shuffle(runs)
    with engine_context(name, "K0") as ctx:
        eng = pipeline.PairEngine(ctx, depth=c["depth"])
        before = plain_chunk(eng, "K0")
        for i, (case, pov) in enumerate(runs):
            run(eng, ctx, case, pov, "device", ("chunk", "flows")[i % 2] if case in FLOWS_CASES else "chunk")
        assert plain_chunk(eng, "K0") == before
        assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("case", ["K1", "K4", "K7", "K11", "K13"])
def test_short_chunks(case):
    """one pair; shorter than the radius; radius + 1; exactly one full window -- none of them fills the ring"""
    c = CONTEXTS["R1"]
    with engine_context("R1", case) as ctx:
        eng = pipeline.PairEngine(ctx, depth=c["depth"])
        before = plain_chunk(eng, case)
        for n in SHORT:
            for pov in CASES[case]["povs"]:
                run(eng, ctx, case, pov, "device", "chunk", n)
                if case in FLOWS_CASES:
                    run(eng, ctx, case, pov, "device", "flows", n)
        assert plain_chunk(eng, case) == before
        assert ctx.graph_stats()["capture_failures"] == 0


def test_a_carried_state_re_detects_as_the_one_chunk_run():
    """K13 on R1 as two chunks split at pair 21, a batch border of B = 3: the first captures, the second gets the same state
    tensor and the templates with capture off, and both write into the two halves of the same track_out / match_out /
    redetect_out.  Track, match and re-detection records, the final state and the templates are the one-chunk by-hand run's on
    bytes (the post records are not: the smoothing window does not cross chunks)."""
    c, track, split = CONTEXTS["R1"], CASES["K13"]["track"], 21
    assert split % c["B"] == 0 and 0 < split < N
    want = hand("K13", False, N, c["B"])
    T, p = len(track["state"]), track["match"]["p"]
    nt = T * 48
    with engine_context("R1", "K13") as ctx:
        eng = pipeline.PairEngine(ctx, depth=c["depth"])
        state, tmpl = dev(np.array(track["state"]).view(np.uint8)), pipeline.match_templates(ctx, T, p)
        outs = {k: torch.full((N * nt,), 0xA5, dtype=torch.uint8, device=DEV) for k in ("track", "match", "redetect")}
        for lo, hi, capture in ((0, split, True), (split, N, False)):
            part = {k: t[lo * nt:hi * nt] for k, t in outs.items()}
            eng.process_chunk(list(lost()[lo:hi + 1]), False, CASES["K13"]["thr"], post_out=True, center="track",
                              track={"state": state, "radius": track["radius"], "on_cut": track["on_cut"],
                                     "match": {**track["match"], "templates": tmpl, "capture": capture}},
                              track_out=part["track"], match_out=part["match"], redetect_out=part["redetect"])
        for k, t in outs.items():
            same(t.cpu().numpy().tobytes(), want[k], nt, f"two chunks: {k}")
        same(state.cpu().numpy().tobytes(), want["state"], nt, "two chunks: state")
        same(tmpl.cpu().numpy().tobytes(), want["templates"], (2 * p + 1) ** 2, "two chunks: templates")
        assert ctx.graph_stats()["capture_failures"] == 0
