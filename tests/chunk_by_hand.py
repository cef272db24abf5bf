"""The composed chunk, stated once, without an engine (fixtures).

PairEngine.process_chunk / process_flows string the library's calls together per batch, on a ring of flow slots that later
batches recycle.  by_hand runs the same chunk on a context that holds every pair at once -- at least n flow slots and
max_batch >= n -- so nothing recycles and every step is ONE documented _capi.Context call over slots 0 .. n-1, in the order
process_chunk's docstring promises:

    1. the flow call (flow_pairs / flow_pairs_dis / flow_pairs_farneback(..., window=)), or import_flows of given fields;
       weights="consistency": the same call also queues the pairs reversed, into a second block of slots n .. 2n-1;
    1a. weights="residual" | "texture" | "consistency": residual_weights and / or texture_weights (the combination with gate =
        out, in place, behind the residual call) or consistency_weights over all n pairs, from the RAW fields;
    1b. center="track": track_template from frame 0 about the state when capturing; then per batch of `batch` pairs
        track_advance on the raw fields, with match track_match on the batch's f0 frames about its records and track_match
        with one item on the batch's last f1 frame about the state, with match["redetect"] track_redetect with one item on that
        same frame about the state, triggered by the records the state's match just wrote, with write-back, its T records at
        index hi - 1 of an (n x T)-record buffer pre-filled with 0xA5, with roi roi_weights.  The state's match and the
        re-detection happen at batch borders, so their outcome depends on the engine's B: by_hand takes batch=;
    2. compensate=: motion_fit (under the maps when there are maps, unweighted under a track), then motion_subtract in place;
    3. weights= (and the track's roi): pass1_weighted            -- or --   center="variance": cell_stats;
    4. one window call over the whole chunk (seq = range(n), first = 0, count = n, radius 6): radial_window[_axes],
       radial_window_axes_weighted, radial_window_axes_centres or radial_window_axes_weighted_centres.

One whole-chunk window call has the bits of the engine's chunked calls (pipeline.window_calls: every computed item's clipped
window lies inside its call's seq); the per-feature tests rely on that and so does this.

The helper is anchored to the CPU (check_anchors), so that by-hand and engine cannot agree on a wrong answer upstream: every
raw field of the tuned Farneback path is oracle.farneback of its pair, and every compensated field is
motion_ref.subtract(raw, model); the maps a mode makes are residual_ref / texture_ref / consistency_ref of the raw fields and
the clip's frames; track records and the final state are track_ref's over the raw fields, match records, corrected records
and templates match_ref's (corrected_batch per batch, template), re-detection records and the state they move redetect_ref's
(found_batch per batch; every record that is not a batch's last pair stays 0xA5), ROI maps track_ref's -- all on bytes, for
all n pairs.  No pytest marks: test_gpu_chunk_compose.py compares the engine with it on bytes, and
test_chunk_schedule_host.py holds the engine's schedules to the same order without a device."""
import numpy as np

from funscript_flow_amd import _capi, pipeline

RADIUS = pipeline.SMOOTH_RADIUS


def random_map(w, h, seed):
    """random 1..255 with about a third zeros (the generator of test_gpu_motion.random_map)"""
    rng = np.random.default_rng(1000 + seed)
    m = rng.integers(1, 256, (h, w)).astype(np.uint8)
    m[rng.random((h, w)) < 1 / 3] = 0
    return m


def pair_maps(w, h, n, seed):
    """(n, h, w): one map per pair, a different seed each"""
    return np.stack([random_map(w, h, seed + j) for j in range(n)])


def padded(maps, device):
    """(n, h, w) maps as a device view with a padded row pitch and item stride"""
    import torch
    n, h, w = maps.shape
    big = torch.full((n, h + 2, w + 13), 0x5A, dtype=torch.uint8, device=device)
    view = big[:, 1:h + 1, 5:5 + w]
    view.copy_(torch.from_numpy(np.array(maps, order="C")).to(device))
    return view


def suite_clip(frames, w, h):
    """the composed-chunk suites' clip: aperiodic over `frames` frames (period 53), so that no two pairs are the same bytes"""
    from funscript_flow_amd.synth import sine_translate_frames
    return sine_translate_frames(frames, w, h, seed=3, zoom=0.03, period=53, amp=(6.0, 3.0))


# The lost-and-found clip of the re-detection cases: a square of random bytes pasted over the suite's clip.  It walks + 1 px
# per frame in x and turns round at the ends of `span` (its centre's x), jumps to the centres of `jumps` at those frames and
# walks on from there in the direction it had, and is not pasted into the frames of `absent` (its walk goes on unseen).
LOST = dict(seed=1300, side=13, start=(14, 20), span=(8, 55), absent=(12, 28),
            jumps={7: (34, 12), 16: (12, 34), 22: (50, 30), 30: (20, 10), 37: (44, 36)})


def lost_path(frames, lost=LOST):
    """the square's centre (x, y) in every frame, the absent ones included"""
    (x, y), d, path = lost["start"], 1, []
    for k in range(frames):
        if k in lost["jumps"]:
            x, y = lost["jumps"][k]
        elif k:
            if not lost["span"][0] <= x + d <= lost["span"][1]:
                d = -d
            x += d
        path.append((x, y))
    return path


def lost_clip(base, lost=LOST):
    """`base` (frames, H, W) uint8 with the square pasted about lost_path's centres"""
    out, r = np.array(base), lost["side"] // 2
    square = np.random.default_rng(lost["seed"]).integers(0, 256, (lost["side"], lost["side"])).astype(np.uint8)
    for k, (x, y) in enumerate(lost_path(len(out), lost)):
        if k not in lost["absent"]:
            out[k, y - r:y + r + 1, x - r:x + r + 1] = square
    return out


def border_searches(redetect, n, T, batch):
    """What the re-detection did at the chunk's batch borders, from the bytes of by_hand's or track_run's `redetect`: per track
    (skipped, accepted and moved the state, triggered and rejected, the statuses of the rejected ones); the records of every
    pair that is not a batch's last must be untouched 0xA5 bytes."""
    rec = np.frombuffer(redetect, _capi.MATCH_DTYPE).reshape(n, T)
    last = [min(lo + int(batch), n) - 1 for lo in range(0, n, int(batch))]
    rest = np.delete(np.frombuffer(redetect, np.uint8).reshape(n, -1), last, axis=0)
    assert (rest == 0xA5).all(), "a re-detection record that is no batch's last pair was written"
    out = []
    for t in range(T):
        r = rec[last, t]
        ran = r["status"] != _capi.REDETECT_SKIPPED
        moved = (r["status"] == 0) & ((r["dx"] != 0) | (r["dy"] != 0))
        out.append((int((~ran).sum()), int(moved.sum()), int((ran & (r["status"] != 0)).sum()),
                    sorted({int(s) for s in r["status"][ran & (r["status"] != 0)]})))
    return out


# The two re-detection cases of test_gpu_chunk_compose.py on the lost-and-found clip (64x48, 41 pairs), as plain data: the host
# test test_chunk_redetect_host.py derives their thresholds and meets their conditions on the CPU restatements alone.
#   K13  one track on the square, the library's default thresholds, redetect=True (the whole frame);
#   K14  the dict form with a reach that some jumps exceed, a second track on the background whose trigger words differ from
#        track 0's, ROI maps about track 0 under a static gate.  Track 1 starts at (18, 32), not at the (20, 30) first meant
#        for it: a 13x13 template about (20, 30) holds a corner of the square in frame 0 (21 of its 169 pixels), follows the
#        square and is lost with it at the first jump -- on the restatements it was skipped at 3 of 14 (B = 3) and 2 of 11
#        (B = 4) borders, whatever the reach and wherever the jumps go.  (18, 32) is the nearest point on a 2 px grid whose
#        template is background only and which is still triggered at a border or two on either context.
LOST_TRACKS = {
    "K13": dict(state=pipeline.track_state_array([(14.0, 20.0)]), radius=9, on_cut="hold", match={"p": 6, "s": 4, "redetect": True},
                capture=True),
    "K14": dict(state=pipeline.track_state_array([(14.0, 20.0), (18.0, 32.0)]), radius=9, on_cut="hold", roi=(20.0, 12.0),
                match={"p": 6, "s": 4, "redetect": {"reach": 20, "exclude": 4}}, capture=True),
}
LOST_THR = {"K13": 0.614, "K14": 0.68}
LOST_GATE_SEED = 1400


def check_redetect_conditions(case, redetect, track, n, batch):
    """What K13 and K14 were chosen for, on a `redetect` buffer of n pairs (by_hand's or track_run's) and the `track` records:
    K13 at least 3 skipped searches, at least 3 accepted ones that move the state, at least 1 triggered and rejected, and rule
    Q5 cuts between a quarter and three quarters of the pairs; K14 track 0 at least 2 accepted ones that move the state and at
    least 1 triggered and rejected, track 1 skipped at three quarters of the borders or more."""
    T = len(LOST_TRACKS[case]["state"])
    got = border_searches(redetect, n, T, batch)
    borders = -(-n // int(batch))
    skipped, moved, rejected, _ = got[0]
    assert skipped + rejected + moved <= borders
    if case == "K13":
        assert skipped >= 3 and moved >= 3 and rejected >= 1, got
        cuts = int(((np.frombuffer(track, _capi.TRACK_DTYPE).reshape(n, T)["status"][:, 0] & 1) != 0).sum())
        assert n / 4 <= cuts <= 3 * n / 4, cuts
    else:
        assert moved >= 2 and rejected >= 1, got
        assert got[1][0] >= 3 * borders / 4, got
    return got


def hand_context(w, h, n, device=0, reverse=False):
    """a context on which a chunk of n pairs never recycles anything; reverse: with room for the n reversed pairs as well"""
    k = 2 if reverse else 1
    return _capi.Context(w, h, device=device, max_batch=k * max(n, 1), frame_slots=n + 1, flow_slots=k * max(n, 1))


def _fields(ctx, slots):
    return ctx.export_flows(slots).cpu().numpy()


def by_hand(ctx, frames_or_fields, *, pov, thr, axes=True, weights=None, center=None, cells=8, compensate=None, algo=None,
            window="box", residual=None, texture=None, consistency=None, gate=None, track=None, batch=None):
    """The chunk of `frames_or_fields` -- n + 1 gray frames (a list or an (n + 1, H, W) uint8 array), or the n pair fields as a
    device array (n, H, W, 2) -- on `ctx`, which holds it whole.  weights: None, an (H, W) / (n, H, W) uint8 device tensor, or
    "residual" | "texture" | "consistency" with residual= / texture= / consistency= (parameters; texture= next to "residual":
    the combination) and gate (the static gate, a device tensor); center: None, "variance" over cells x cells, or "track" with
    track = dict(state = (T,) TRACK_STATE_DTYPE host records, radius, on_cut, roi = (ax, ay) or None, roi_soft, match = a dict
    of MatchParams fields or None, next to them "redetect" = True or a dict as process_chunk takes it, capture, templates = host
    bytes when not capturing) and batch, the engine's B; compensate: as process_chunk takes it; algo: None (Farneback) or ("dis", DisParams or None); window: "box" or "gaussian".  Returns dict(post
    = the n records as bytes, motion = the n 64-byte records as bytes or None, grid = the cell records as bytes or None, flows =
    (n, H, W, 2) float32 as left in the slots, pass1 = pass1_results' tuples of the slots as left, raw = (n, H, W, 2) float32
    as the flow call left them, raw_pass1 = pass1_results of the raw fields, raw_bwd = the reversed pairs' raw fields or None,
    maps / track / state / match / templates / redetect = bytes or None)."""
    import torch
    dev = torch.device("cuda", ctx.device)
    given = not isinstance(frames_or_fields, (list, tuple)) and getattr(frames_or_fields, "ndim", 0) == 4
    n = len(frames_or_fields) - (0 if given else 1)
    mode = weights if isinstance(weights, str) else None
    k = 2 if mode == "consistency" else 1
    assert 1 <= n and k * n <= min(ctx.flow_slots, ctx.max_batch), "by_hand needs a context that holds the whole chunk"
    assert weights is None or center is None
    assert axes or (weights is None and center is None)
    assert mode is None or not given, "the modes that make maps read the frames"
    slots = list(range(n))
    f0, f1 = list(range(n)), list(range(1, n + 1))
    # 1. the flow call
    if given:
        ctx.import_flows(frames_or_fields, slots, pov)
    else:
        assert ctx.frame_slots >= n + 1
        ctx.upload_frames(0, [np.ascontiguousarray(f) for f in frames_or_fields])
        a, b, fl = (f0 + f1, f1 + f0, slots + [n + j for j in slots]) if k == 2 else (f0, f1, slots)
        if algo is not None and algo[0] == "dis":
            ctx.flow_pairs_dis(a, b, fl, pov, algo[1])
        elif window != "box":
            ctx.flow_pairs_farneback(a, b, fl, pov, None, window=window)
        else:
            ctx.flow_pairs(a, b, fl, pov)
    raw = _fields(ctx, slots)
    raw_pass1 = ctx.pass1_results(slots, thr)
    raw_bwd = _fields(ctx, [n + j for j in slots]) if k == 2 else None
    # 1a. the maps a mode makes, from the raw fields
    maps = None
    if mode is not None:
        maps = weights = torch.full((n, ctx.height, ctx.width), 0xA5, dtype=torch.uint8, device=dev)
        if mode == "residual":
            ctx.residual_weights(f0, f1, slots, maps, _capi.residual_choice(residual), gate)
            if texture is not None:
                ctx.texture_weights(f0, maps, _capi.texture_choice(texture), maps)
        elif mode == "texture":
            ctx.texture_weights(f0, maps, _capi.texture_choice(texture), gate)
        else:
            assert mode == "consistency" and compensate is None
            ctx.consistency_weights(slots, [n + j for j in slots], maps, _capi.consistency_choice(consistency), gate)
    # 1b. the track, on the raw fields
    trk = sd = mout = tmpl = rout = None
    if center == "track":
        T = len(track["state"])
        item = T * _capi.TRACK_DTYPE.itemsize
        sd = torch.from_numpy(np.array(track["state"], _capi.TRACK_STATE_DTYPE).view(np.uint8).copy()).to(dev)
        trk = torch.full((n * item,), 0xA5, dtype=torch.uint8, device=dev)
        tprm = {"radius": track.get("radius", 12), "on_cut": track.get("on_cut", "hold"), "cut_threshold": thr}
        prm = None
        if track.get("match") is not None:
            assert not given, "the match reads the frames"
            prm = _capi.match_choice({k: v for k, v in track["match"].items() if k in _capi.MATCH_FIELDS})
            rprm = None
            if track["match"].get("redetect") not in (None, False):
                rprm = pipeline.redetect_choice(prm, track["match"]["redetect"])
                rout = torch.full((n * item,), 0xA5, dtype=torch.uint8, device=dev)
            mout = torch.full((n * item,), 0xA5, dtype=torch.uint8, device=dev)
            sout = pipeline.match_buffer(ctx, 1, T)
            if track.get("capture", track.get("templates") is None):
                tmpl = pipeline.match_templates(ctx, T, prm.p)
                ctx.track_template(0, sd, tmpl, prm.p, T)
            else:
                tmpl = torch.from_numpy(np.frombuffer(track["templates"], np.uint8).copy()).to(dev)
        if track.get("roi") is not None:
            maps = weights = torch.full((n, ctx.height, ctx.width), 0xA5, dtype=torch.uint8, device=dev)
        for lo in range(0, n, int(batch)):
            hi = min(lo + int(batch), n)
            part = trk[lo * item:hi * item]
            ctx.track_advance(slots[lo:hi], sd, part, tprm)
            if prm is not None:
                ctx.track_match(f0[lo:hi], tmpl, (part, item), mout[lo * item:hi * item], prm, T, True)
                ctx.track_match([f1[hi - 1]], tmpl, (sd, item), sout, prm, T, True)
                if rprm is not None:
                    ctx.track_redetect([f1[hi - 1]], tmpl, (sd, item), rout[(hi - 1) * item:hi * item], rprm, T, sout, True)
            if maps is not None:
                ctx.roi_weights(hi - lo, (part, item), maps[lo:hi], {"ax": track["roi"][0], "ay": track["roi"][1],
                                                                     "soft": int(bool(track.get("roi_soft", True)))}, gate=gate)
    # 2. the fit, then the subtraction in place
    motion = None
    if compensate is not None:
        mo = pipeline.motion_buffer(ctx, n)
        ctx.motion_fit(slots, _capi.motion_choice(compensate), weights=None if trk is not None else weights, out=mo)
        ctx.motion_subtract(slots, slots, mo, pov)
        motion = mo.cpu().numpy().tobytes()
    # 3. the records under the maps, or the cell grid and its centres
    item = (_capi.PASS2_AXES_DTYPE if axes else _capi.PASS2_DTYPE).itemsize
    out = torch.full((n * item,), 0xA5, dtype=torch.uint8, device=dev)
    grid = None
    if trk is not None:
        centres = (trk, len(track["state"]) * _capi.TRACK_DTYPE.itemsize)
        if weights is not None:
            ctx.pass1_weighted(slots, weights, pov)
            ctx.radial_window_axes_weighted_centres(slots, 0, n, weights, centres, out, RADIUS, thr, pov)
        else:
            ctx.radial_window_axes_centres(slots, 0, n, centres, out, RADIUS, thr, pov)
    elif weights is not None:
        ctx.pass1_weighted(slots, weights, pov)
        ctx.radial_window_axes_weighted(slots, 0, n, weights, out, RADIUS, thr, pov)
    elif center is not None:
        assert center == "variance"
        cell_out = pipeline.grid_buffer(ctx, n, cells)
        centres = torch.full((n * _capi.GRID_CENTRE_DTYPE.itemsize,), 0xA5, dtype=torch.uint8, device=dev)
        ctx.cell_stats(slots, cells, cell_out, centres)
        ctx.radial_window_axes_centres(slots, 0, n, centres, out, RADIUS, thr, pov)
        grid = cell_out.cpu().numpy().tobytes()
    # 4. (the plain forms of) the one window call
    elif axes:
        ctx.radial_window_axes(slots, 0, n, out, RADIUS, thr, pov)
    else:
        ctx.radial_window(slots, 0, n, out, RADIUS, thr, pov)
    b = lambda t: None if t is None else t.cpu().numpy().tobytes()   # noqa: E731
    return dict(post=b(out), motion=motion, grid=grid, flows=_fields(ctx, slots), pass1=ctx.pass1_results(slots, thr), raw=raw,
                raw_pass1=raw_pass1, raw_bwd=raw_bwd, maps=b(maps), track=b(trk), state=b(sd), match=b(mout), templates=b(tmpl),
                redetect=b(rout))


def records(post, axes=True):
    """the post bytes of by_hand (or of an engine) as a numpy record array"""
    return np.frombuffer(post, _capi.PASS2_AXES_DTYPE if axes else _capi.PASS2_DTYPE)


def rec_bytes(recs):
    """pass1_results' tuples with their floats as bytes: NaN-safe equality"""
    return [(x, y, np.float32(d).tobytes(), np.float32(m).tobytes(), c) for x, y, d, m, c in recs]


def oracle_fields(frames):
    """(n, H, W, 2): oracle.farneback of every pair of `frames`, on the CPU"""
    import oracle as orc
    return np.stack([orc.farneback(frames[j], frames[j + 1]) for j in range(len(frames) - 1)])


def check_anchors(res, oracle=None):
    """The two CPU anchors of a by_hand result: with `oracle` (oracle_fields of the chunk's frames; the tuned Farneback path
    only) every raw field is the oracle's; with a fit, every field left in the slots is motion_ref.subtract(raw, the pair's
    model) -- for ALL n pairs, on bytes -- and without one it is the raw field."""
    import motion_ref as mr
    n = len(res["raw"])
    if oracle is not None:
        for j in range(n):
            assert res["raw"][j].tobytes() == oracle[j].tobytes(), f"raw field {j} is not the oracle's"
    if res["motion"] is None:
        assert res["flows"].tobytes() == res["raw"].tobytes()
        return
    models = np.frombuffer(res["motion"], _capi.MOTION_DTYPE, n)
    for j in range(n):
        assert res["flows"][j].tobytes() == mr.subtract(res["raw"][j], mr.six(models[j])).tobytes(), f"compensated field {j}"


def mode_maps(frames, raw, mode, residual=None, texture=None, consistency=None, gate=None, raw_bwd=None):
    """(n, H, W) uint8: the maps of weights=mode on the CPU -- residual_ref / texture_ref / consistency_ref of the raw fields and
    the frames, the combination as texture_ref under gate = the residual map; gate: the static gate as a host array or None"""
    import consistency_ref
    import residual_ref
    import texture_ref
    out = []
    for j in range(len(raw)):
        if mode == "residual":
            m = residual_ref.residual(frames[j], frames[j + 1], raw[j], gate=gate, **_capi.residual_choice(residual).as_dict())
            if texture is not None:
                m = texture_ref.texture_map(frames[j], gate=m, **_capi.texture_choice(texture).as_dict())
        elif mode == "texture":
            m = texture_ref.texture_map(frames[j], gate=gate, **_capi.texture_choice(texture).as_dict())
        else:
            m = consistency_ref.consistency(raw[j], raw_bwd[j], gate=gate, **_capi.consistency_choice(consistency).as_dict())
        out.append(m)
    return np.stack(out)


def track_run(frames, raw, mean_mag, thr, track, batch, gate=None):
    """The track of a chunk on the CPU: track_ref.advance over the raw fields, per batch of `batch` pairs, its cuts rule Q5 on the
    raw records' float32 mean magnitudes; with track["match"] match_ref.corrected_batch per batch and match_ref.template; with
    track["match"]["redetect"] redetect_ref.found_batch per batch instead: corrected_batch with the batch's cuts, then
    redetect_ref.redetect of the state on the batch's last f1 frame, triggered by the state's match records, with write-back.
    Returns dict(track, state, match, templates, maps, redetect) as bytes or None; redetect: (n, T) records, every index that
    is not a batch's last pair 0xA5 bytes."""
    import match_ref
    import redetect_ref
    import track_ref
    n, (h, w) = len(raw), raw[0].shape[:2]
    cuts = track_ref.mean_mag_cut(mean_mag, thr)
    st = np.array(track["state"], track_ref.STATE_DTYPE)
    radius, on_cut = track.get("radius", 12), _capi.TRACK_ON_CUT.index(track.get("on_cut", "hold"))
    prm = tm = rprm = rrecs = None
    if track.get("match") is not None:
        assert on_cut == track_ref.HOLD, "match_ref.corrected_batch advances with on_cut='hold'"
        choice = _capi.match_choice({k: v for k, v in track["match"].items() if k in _capi.MATCH_FIELDS})
        prm = choice.as_dict()
        prm["mode"] = _capi.MATCH_MODES.index(prm["mode"])
        if track["match"].get("redetect") not in (None, False):
            rprm = pipeline.redetect_choice(choice, track["match"]["redetect"]).as_dict()
            rprm["mode"] = _capi.MATCH_MODES.index(rprm["mode"])
            rrecs = np.full((n, len(st) * redetect_ref.RECORD_DTYPE.itemsize), 0xA5, np.uint8)
        if track.get("capture", track.get("templates") is None):
            tm = match_ref.template(frames[0], np.stack([st["x"], st["y"]], axis=-1), prm["p"])
        else:
            side = 2 * prm["p"] + 1
            tm = np.frombuffer(track["templates"], np.uint8).reshape(len(st), side, side)
    recs, mrecs = [], []
    for lo in range(0, n, int(batch)):
        hi = min(lo + int(batch), n)
        if prm is None:
            rec, st = track_ref.advance(raw[lo:hi], cuts[lo:hi], st, radius, on_cut)
        elif rprm is None:
            rec, mrec, _, st = match_ref.corrected_batch(track_ref, frames[lo:hi + 1], raw[lo:hi], st, tm, radius, prm, cuts[lo:hi])
            mrecs.append(mrec)
        else:
            rec, mrec, _, rrec, st = redetect_ref.found_batch(track_ref, frames[lo:hi + 1], raw[lo:hi], st, tm, radius, prm, rprm,
                                                              cuts[lo:hi])
            mrecs.append(mrec)
            rrecs[hi - 1] = np.frombuffer(rrec.tobytes(), np.uint8)
        recs.append(rec)
    rec = np.concatenate(recs)
    maps = None
    if track.get("roi") is not None:
        maps = track_ref.roi_maps(w, h, np.stack([rec["x"][:, 0], rec["y"][:, 0]], axis=-1), track["roi"][0], track["roi"][1],
                                  bool(track.get("roi_soft", True)), gate).tobytes()
    return dict(track=rec.tobytes(), state=st.tobytes(), match=np.concatenate(mrecs).tobytes() if mrecs else None,
                templates=None if tm is None else tm.tobytes(), maps=maps, redetect=None if rrecs is None else rrecs.tobytes())


def check_mode_anchors(res, frames, *, thr, weights=None, residual=None, texture=None, consistency=None, gate=None, center=None,
                       track=None, batch=None):
    """The CPU anchors of what by_hand made behind the flow call, on bytes, for all n pairs: the maps of a mode (mode_maps), and
    under a track its records, final state, match records, templates, re-detection records -- the whole (n, T) buffer, so the
    entries that are no batch's last pair are held to their 0xA5 fill -- and ROI maps (track_run).  `gate`: the host array."""
    if isinstance(weights, str):
        want = mode_maps(frames, res["raw"], weights, residual, texture, consistency, gate, res["raw_bwd"])
        got = np.frombuffer(res["maps"], np.uint8).reshape(want.shape)
        bad = [j for j in range(len(want)) if got[j].tobytes() != want[j].tobytes()]
        assert not bad, f"the {weights} maps of pairs {bad} are not the restatement's"
    if center == "track":
        want = track_run(frames, res["raw"], [r[3] for r in res["raw_pass1"]], thr, track, batch, gate)
        for key in ("templates", "match", "redetect", "track", "state", "maps"):
            assert (res[key] is None) == (want[key] is None), key
            assert res[key] == want[key], f"the track's {key} are not the restatement's"
