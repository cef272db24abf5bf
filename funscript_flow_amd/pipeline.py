"""Host-side schedule around the HIP pair kernels: the counterpart of the per-chunk section of
process_video (FunscriptFlow.pyw:1187-1242) for the "HIP" backend.

    pairs = zip(frames[:-1], frames[1:])                                   FF:1188
    pass 1  (flow, |div| argmax, mean magnitude, cut) for every pair       FF:1190-1191
    c_j = mean of pos_center over pairs j-6..j+6 inside the chunk          FF:1203-1214
    pass 2  radial_motion_weighted(flow_j, c_j, cut_j, pov_mode)            FF:1232-1236

Everything runs in the calling process (HIP state must not cross fork); flows never leave HBM.
Multi-GPU: pairs are sharded over the ranks either in contiguous blocks or round-robin in blocks of
`block` pairs (`shard_pairs`); the only exchange is a host all-gather of the 32-byte pass-1 records (no
RCCL collective) -- of ALL records under round-robin (`process_chunk_sharded`), of the <= 12 halo records per
rank under contiguous blocks (`process_chunk_sharded_halo`, the streaming form).
"""
import numpy as np

from . import _capi

SMOOTH_RADIUS = 6  # FF:1206 range(1, 7)


def smooth_centers(pos_centers, radius=SMOOTH_RADIUS):
    """FF:1203-1214: c_j = mean({p_i : |i-j| <= 6, 0 <= i < n}) as float64[2].

    The reference gathers the window's positions into a list and takes np.mean(..., axis=0) of the int64 pairs: an exact
    integer sum (far below 2^53) converted to float64 and divided by the count.  Window sums from a prefix sum give the
    same integers, hence the same float64 -- bit for bit (pinned by the chain captured from the real process_video,
    tests/test_host_side.py) -- without a Python loop over the chunk's 3000 pairs (13 ms -> 0.1 ms)."""
    p = np.asarray(pos_centers, np.int64).reshape(-1, 2)
    n = len(p)
    psum = np.zeros((n + 1, 2), np.int64)
    np.cumsum(p, axis=0, out=psum[1:])
    j = np.arange(n)
    lo, hi = np.maximum(0, j - radius), np.minimum(n, j + radius + 1)
    return (psum[hi] - psum[lo]) / (hi - lo)[:, None]


def min_flow_slots(max_batch, depth=1):
    """Flow slots a streaming two-pass schedule needs with `depth` + 1 batches in flight (depth = 1: the bound
    include/ffl.h documents for ffl_create)."""
    return (depth + 1) * max_batch + 2 * SMOOTH_RADIUS + 1


def min_frame_slots(max_batch, depth=1):
    """Frame slots for `depth` batches in flight + the one being staged, B + 1 frames each."""
    return (depth + 1) * (max_batch + 1)


def window_calls(n_pairs, B, radius=SMOOTH_RADIUS):
    """The Context.radial_window calls a streaming chunk of n_pairs pairs issues when its batches hold B pairs, as
    (seq_lo, seq_hi, first, count, after_batch) tuples in issue order: pairs seq_lo .. seq_hi-1 are the call's seq, items
    first .. first+count-1 of it (pairs seq_lo + first ...) are computed, and the call is issued once batch `after_batch`
    (0-based) has been queued.  _ChunkPost._finalize's rule: a pair is issued once its +-radius window is complete -- or at
    the chunk's end, where the window clips -- at most B pairs per call.  Every pair is issued exactly once; a call's seq
    holds its items' whole clipped windows and at most B + 2 * radius pairs, none of them later than batch after_batch.
    A pure function: no device."""
    calls, done = [], 0
    for k in range(-(-n_pairs // B)):
        j1 = min((k + 1) * B, n_pairs)                       # pairs queued so far
        limit = n_pairs if j1 == n_pairs else max(0, j1 - radius)
        while done < limit:
            c1 = min(done + B, limit)
            lo, hi = max(0, done - radius), min(n_pairs, c1 + radius)
            calls.append((lo, hi, done - lo, c1 - done, k))
            done = c1
    return calls


def _post_dtype(axes):
    """the record of a chunk's device pass 2: 48 bytes, or the 80 bytes of the four-component form (axes=True)"""
    return _capi.PASS2_AXES_DTYPE if axes else _capi.PASS2_DTYPE


def post_buffer(ctx, n, axes=False):
    """a device buffer for the n records of a chunk (torch uint8 on the context's device), as post_out= takes it"""
    import torch
    return torch.empty(n * _post_dtype(axes).itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def post_records(buf, n=None, device=None, axes=False):
    """The one device-to-host copy of a chunk whose pass 2 ran on the device (process_chunk / process_flows with
    post_out=): (dots float64[n], records) in the form process_chunk returns them; n defaults to the records `buf` holds.
    The copy runs on torch's current stream, behind the calls that filled `buf` there, and waits for them.  A torch
    tensor names its own device; for any other __cuda_array_interface__ object `device` is the context's (default: torch's
    current device).  axes=True: `buf` holds 80-byte records and the first item is comps float64[n, 4] (_capi.AXES)."""
    import torch
    if not isinstance(buf, torch.Tensor):
        buf = torch.as_tensor(buf, device=torch.device("cuda", torch.cuda.current_device() if device is None else device))
    dt = _post_dtype(axes)
    raw = buf.contiguous().view(torch.uint8).reshape(-1)
    n = raw.numel() // dt.itemsize if n is None else n
    raw = raw[:n * dt.itemsize].cpu().numpy()
    rec = np.frombuffer(raw.tobytes(), dt, n)
    records = list(zip(rec["x"].tolist(), rec["y"].tolist(), list(rec["div_val"]), list(rec["mean_mag"]),
                       (rec["cut"] != 0).tolist()))
    if axes:
        return np.stack([rec["dot"]] + [rec[k] for k in _capi.AXES[1:]], axis=1).astype(np.float64), records
    return rec["dot"].astype(np.float64), records


def grid_buffer(ctx, n, cells=32):
    """a device buffer for the n * cells * cells 32-byte cell records of a chunk (torch uint8 on the context's device), as
    grid_out= takes it: pair j's grid at byte 32 * cells * cells * j"""
    import torch
    return torch.empty(n * cells * cells * _capi.CELL_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def grid_records(buf, cells=32, n=None, device=None):
    """The cell records of a chunk run with grid_out= as a numpy array (n, cells, cells) of _capi.CELL_DTYPE (fields mean_u,
    mean_v, mean_mag, var_mag; [j, i, k] is cell row i, column k of pair j).  The copy runs on torch's current stream, behind
    the calls that filled `buf` there, and waits for them (see post_records for `device`)."""
    import torch
    if not isinstance(buf, torch.Tensor):
        buf = torch.as_tensor(buf, device=torch.device("cuda", torch.cuda.current_device() if device is None else device))
    item = cells * cells * _capi.CELL_DTYPE.itemsize
    raw = buf.contiguous().view(torch.uint8).reshape(-1)
    n = raw.numel() // item if n is None else n
    raw = raw[:n * item].cpu().numpy()
    return np.frombuffer(raw.tobytes(), _capi.CELL_DTYPE, n * cells * cells).reshape(n, cells, cells)


def motion_buffer(ctx, n):
    """a device buffer for the n 64-byte motion records of a chunk (torch uint8 on the context's device), as motion_out= and
    Context.motion_fit(out=) take it: pair j's record at byte 64 * j"""
    import torch
    return torch.empty(n * _capi.MOTION_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def motion_records(buf, n=None, device=None):
    """The motion records of a chunk run with motion_out= (or of Context.motion_fit) as a numpy array (n,) of
    _capi.MOTION_DTYPE (fields a0, a1, a2, b0, b1, b2 of rule C2, sw, model, status): the camera path, one model per pair.
    The copy runs on torch's current stream, behind the calls that filled `buf` there, and waits for them (see post_records
    for `device`)."""
    import torch
    if not isinstance(buf, torch.Tensor):
        buf = torch.as_tensor(buf, device=torch.device("cuda", torch.cuda.current_device() if device is None else device))
    item = _capi.MOTION_DTYPE.itemsize
    raw = buf.contiguous().view(torch.uint8).reshape(-1)
    n = raw.numel() // item if n is None else n
    raw = raw[:n * item].cpu().numpy()
    return np.frombuffer(raw.tobytes(), _capi.MOTION_DTYPE, n)


def track_buffer(ctx, n, tracks=1):
    """a device buffer for the n * tracks 48-byte track records of a chunk (torch uint8 on the context's device), as track_out=
    and Context.track_advance(out=) take it: record (pair j, track t) at byte 48 * (j * tracks + t)"""
    import torch
    return torch.empty(n * int(tracks) * _capi.TRACK_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def track_records(buf, tracks=1, n=None, device=None):
    """The track records of a chunk run with center="track" (or of Context.track_advance) as a numpy array (n, tracks) of
    _capi.TRACK_DTYPE (fields x, y -- the track's place in frame 0 of the pair --, du, dv, sw, count, status).  The copy runs on
    torch's current stream, behind the calls that filled `buf` there, and waits for them (see post_records for `device`)."""
    import torch
    if not isinstance(buf, torch.Tensor):
        buf = torch.as_tensor(buf, device=torch.device("cuda", torch.cuda.current_device() if device is None else device))
    item = int(tracks) * _capi.TRACK_DTYPE.itemsize
    raw = buf.contiguous().view(torch.uint8).reshape(-1)
    n = raw.numel() // item if n is None else n
    raw = raw[:n * item].cpu().numpy()
    return np.frombuffer(raw.tobytes(), _capi.TRACK_DTYPE, n * int(tracks)).reshape(n, int(tracks))


def match_buffer(ctx, n, tracks=1):
    """a device buffer for the n * tracks 48-byte match records of a chunk (torch uint8 on the context's device), as match_out=
    and Context.track_match(out=) take it: record (pair j, track t) at byte 48 * (j * tracks + t)"""
    import torch
    return torch.empty(n * int(tracks) * _capi.MATCH_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def match_records(buf, tracks=1, n=None, device=None):
    """The match records of a chunk run with track["match"] (or of Context.track_match) as a numpy array (n, tracks) of
    _capi.MATCH_DTYPE (fields x, y, dx, dy, cost, second, status, pad); the copy runs as track_records' does."""
    raw = track_records(buf, tracks, n, device)
    return np.frombuffer(raw.tobytes(), _capi.MATCH_DTYPE).reshape(raw.shape)


def match_templates(ctx, tracks=1, p=None):
    """a device tensor (torch uint8, (tracks, 2p+1, 2p+1)) for the templates of Context.track_template / track_match and
    track["match"]["templates"]; p None: the default of _capi.MatchParams"""
    import torch
    side = 2 * (_capi.MatchParams().p if p is None else int(p)) + 1
    return torch.zeros((int(tracks), side, side), dtype=torch.uint8, device=torch.device("cuda", ctx.device))


def track_state_array(points, home=None):
    """(T,) _capi.TRACK_STATE_DTYPE records on the host out of `points`, (x, y) or (T, 2): the tracks' positions; `home`
    (the same form, default: the points) is where on_cut="home" sends a track.  steps and lost_run start at 0."""
    p = np.asarray(points, np.float64).reshape(-1, 2)
    hm = p if home is None else np.asarray(home, np.float64).reshape(-1, 2)
    if not 1 <= len(p) <= _capi.FFL_MAX_TRACKS or hm.shape != p.shape:
        raise ValueError(f"track: {len(p)} points and {len(hm)} home points; 1..{_capi.FFL_MAX_TRACKS} (x, y) pairs, as many of each")
    st = np.zeros(len(p), _capi.TRACK_STATE_DTYPE)
    st["x"], st["y"], st["home_x"], st["home_y"] = p[:, 0], p[:, 1], hm[:, 0], hm[:, 1]
    return st


def track_state(ctx, points, home=None):
    """a device tensor (torch uint8, 48 bytes per track) of ffl_track_state records for Context.track_advance and
    track={"state": ...}: see track_state_array.  The library reads and writes it, so it carries a track from call to call and
    from chunk to chunk; a detector may overwrite it in between."""
    import torch
    st = track_state_array(points, home)
    return torch.from_numpy(st.view(np.uint8).copy()).to(torch.device("cuda", ctx.device))


def track_state_records(state):
    """the ffl_track_state records of a device state tensor as a numpy array (T,) of _capi.TRACK_STATE_DTYPE"""
    raw = state.contiguous().view(-1).cpu().numpy()
    return np.frombuffer(raw.tobytes(), _capi.TRACK_STATE_DTYPE)


def _stream_event(ctx, stream=None):
    """an event recorded on `stream` (None: torch's current stream of the context's device): query() / synchronize()"""
    import torch
    ev = torch.cuda.Event()
    ev.record(torch.cuda.current_stream(ctx.device) if stream is None else stream)
    return ev


def _side_stream(ctx):
    """The context's stream for the window calls of a chunk, made to wait for the work queued on torch's current stream.
    The calls make their stream wait for every batch they follow; on torch's current stream -- the default stream,
    which the device uploads join too -- that wait cost 0.3 ms of the device's time per call at 256x256 (DESIGN.md
    section 14), on a stream of their own nothing measurable."""
    import torch
    s = getattr(ctx, "_pass2_stream", None)
    if s is None:
        s = ctx._pass2_stream = torch.cuda.Stream(torch.device("cuda", ctx.device))
    s.wait_stream(torch.cuda.current_stream(ctx.device))
    return s


def shard_range(n_items, world, rank):
    """Contiguous block [lo, hi) of rank `rank`; block sizes differ by at most one."""
    base, rem = divmod(n_items, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def shard_pairs(n_items, world, rank, assign="contiguous", block=1):
    """Sorted pair indices owned by `rank`.

    "contiguous"   one block per rank (shard_range): consecutive pairs share a frame, so a rank uploads and
                   expands ~1 frame per pair, and the +-6 window of FF:1203-1214 stays local except at the two
                   block edges.  Needs the number of pairs up front.
    "round_robin"  blocks of `block` consecutive pairs dealt to ranks in turn (block k -> rank k % world):
                   BASELINE's "frame-pairs sharded round-robin" (block = 1), usable on a stream whose length is
                   not known when the first pairs are dispatched.  A rank expands (block + 1) / block frames
                   per pair (2 at block = 1, where no two of its pairs share a frame)."""
    if assign == "contiguous":
        lo, hi = shard_range(n_items, world, rank)
        return np.arange(lo, hi)
    if assign != "round_robin" or block < 1:
        raise ValueError(f"unknown pair assignment {assign!r} / block {block}")
    idx = np.arange(n_items)
    return idx[(idx // block) % world == rank]


OWN = object()   # pass1 / pass1_pairs / process_chunk `farneback` and `window` default: the engine's own


def farneback_kwargs(params, width, height):
    """{"farneback": FarnebackParams or None} when params names "hip_farneback" (checked against the frame size up front)
    and {"window": "box" | "gaussian"} when it names "hip_farneback_window", else {}: the per-call override of
    frames_to_actions and prefetch.video_to_actions."""
    kw = {}
    if "hip_farneback_window" in params:
        kw["window"] = _capi.farneback_mode(params)
    if "hip_farneback" in params:
        fb = _capi.farneback_choice(params)
        if fb is not None:
            _capi.farneback_geometry(width, height, fb)
        kw["farneback"] = fb
    return kw


class PairEngine:
    """Streams one chunk of frames through a device context in batches of `max_batch` pairs.

    Consecutive pairs share a frame, so every frame is uploaded and expanded once per batch it
    appears in.  Two batches are kept in flight; pass 2 for pair j is issued once the pass-1 records
    of pairs <= j+6 are known (or the chunk has ended), after which its flow slot is recycled.
    """

    def __init__(self, ctx, upload=None, depth=None, flow="farneback", dis=None, farneback=None, window="box"):
        """`upload(first_slot, frames)` puts a run of frames into consecutive frame slots; the default takes
        gray (or same-size BGR) operands, frontend.DecodedUploader takes frames as decoded (any size).
        `depth`: batches queued on the device before the oldest one's results are collected (default: 2 when the
        context has the slots for it -- 3B + 3 frame slots, 3B + 13 flow slots -- else 1).  With depth 2 the upload of
        batch s + 2 is already queued while batch s computes, so a slow transfer or a host hiccup does not idle the device;
        a third batch queued ahead measures within 1 % of two at 1080p and at 256x256 (profiles/r04_pcie_chunk_length.txt).
        Results do not depend on it.
        `flow`: "farneback" (ffl_flow_pairs) or "dis" (ffl_flow_pairs_dis with the _capi.DisParams `dis`, None = PRESET_FAST)
        for every batch the engine queues.
        `farneback`: _capi.FarnebackParams for the Farneback batches (ffl_flow_pairs_farneback; None: the reference's values
        through the tuned ffl_flow_pairs).
        `window`: "box" or "gaussian" (cv2.OPTFLOW_FARNEBACK_GAUSSIAN) for the Farneback batches; "gaussian" runs the general
        kernels, with `farneback`'s numbers or the reference's."""
        if flow not in _capi.FLOWS:
            raise ValueError(f"flow must be one of {_capi.FLOWS}, got {flow!r}")
        if farneback is not None and flow == "dis":
            raise ValueError("farneback parameters need flow='farneback'")
        if farneback is not None:
            _capi.farneback_geometry(ctx.width, ctx.height, farneback)
        _capi.farneback_window(window)
        if window != "box" and flow == "dis":
            raise ValueError("a Farneback window needs flow='farneback'")
        self.flow, self.dis, self.farneback, self.window = flow, dis, farneback, window
        self.ctx = ctx
        self.upload = upload or ctx.upload_frames
        self.B = ctx.max_batch
        if depth is None:
            depth = 2 if (ctx.frame_slots >= min_frame_slots(self.B, 2) and ctx.flow_slots >= min_flow_slots(self.B, 2)) else 1
        self.depth = int(depth)
        if self.depth > 1 and (ctx.frame_slots < min_frame_slots(self.B, self.depth) or ctx.flow_slots < min_flow_slots(self.B, self.depth)):
            raise ValueError(f"context too small for depth {self.depth}: need frame_slots >= {min_frame_slots(self.B, self.depth)} "
                             f"and flow_slots >= {min_flow_slots(self.B, self.depth)}")
        # frame slots: a batch's <= B+1 (stream) / 2B (arbitrary pairs) frames + the next batch's new ones;
        # flow slots: two batches in flight + the <= 6 pairs still waiting for their +-6 window (2B + 6 live
        # at most; 2B + 13 is the bound ffl.h documents and Context defaults to)
        if ctx.frame_slots < 2 * self.B + 2 or ctx.flow_slots < min_flow_slots(self.B):
            raise ValueError(f"context too small: need frame_slots >= 2B+2 = {2 * self.B + 2} and "
                             f"flow_slots >= 2B+13 = {min_flow_slots(self.B)}")

    def pass1(self, frames, pair_lo, pair_hi, pov_mode=False, cut_threshold=7.0, on_batch=None, algo=None, farneback=OWN,
              window=OWN, behind=None):
        """Run pass 1 for pairs [pair_lo, pair_hi) of `frames`; flows stay resident in slot
        (j - pair_lo) % flow_slots.  Returns the list of (x, y, val, mean_mag, cut)."""
        fs = self.ctx.flow_slots
        return self.pass1_pairs(frames, range(pair_lo, pair_hi), lambda l: l % fs, pov_mode, cut_threshold,
                                on_batch=(lambda ls, js, got: on_batch(js, got)) if on_batch else None, algo=algo,
                                farneback=farneback, window=window, behind=behind)

    def pass1_pairs(self, frames, pairs, slot_of, pov_mode=False, cut_threshold=7.0, on_batch=None, algo=None,
                    farneback=OWN, window=OWN, queued=None, batch=None, reverse_slot_of=None, behind=None, with_frames=None):
        """Pass 1 for an arbitrary ascending list of pair indices (pair j = frames[j], frames[j+1]) in batches of
        max_batch; the flow of the l-th listed pair stays resident in flow slot slot_of(l).  Frames go to the
        device once per run of batches that needs them: a ring over the frame slots, frames of the batch being
        assembled are never evicted, and runs of consecutive frames landing in consecutive slots go up with one
        H2D transfer.  (The library orders an upload into a recycled slot behind the batches that still read
        it.)  on_batch(local_indices, pair_indices, records) is called per finished batch.  `algo` = (flow, dis) as
        _capi.flow_choice returns it overrides the engine's own flow algorithm for this call only, and `farneback`
        (_capi.FarnebackParams, or None for the tuned path; as _capi.farneback_choice returns it) its Farneback parameters,
        `window` ("box" | "gaussian", as _capi.farneback_mode returns it) their window.
        `queued(local_indices, pair_indices)`: called straight after every batch has been QUEUED; the records are then never
        collected (no pass1_results, no on_batch, no frame release -- the device pass 2 of process_chunk) and the list
        returned holds None.
        `batch`: listed pairs per batch (default max_batch).  `reverse_slot_of(l)`: every batch is queued as ONE flow call of
        its pairs and then the same pairs reversed, (frames[j + 1], frames[j]) -> flow slot reverse_slot_of(l), so the
        frames' expansions are shared (2 * batch <= max_batch); records and callbacks are those of the forward pairs.
        `behind(local_indices, pair_indices)`: called straight after every batch has been queued and before anything reads
        its records or fields (queued= included): what it queues on the batch's slots -- the motion compensation of
        process_chunk -- is what every later reader sees.
        `with_frames(local_indices, pair_indices, fslot0, fslot1)`: called straight after every batch has been queued, ahead of
        behind=, with the frame slots the batch's pairs were queued from (frames[j] in fslot0, frames[j + 1] in fslot1): what
        reads the batch's frames next to its raw fields -- the residual maps of process_chunk.  The slots stay the frames'
        until a later batch is staged, and the library orders that upload behind whatever the hook queued on them."""
        ctx, B, S = self.ctx, (self.B if batch is None else int(batch)), self.ctx.frame_slots
        algo, dis = algo if algo is not None else (getattr(self, "flow", "farneback"), getattr(self, "dis", None))
        fb = getattr(self, "farneback", None) if farneback is OWN else farneback
        win = getattr(self, "window", "box") if window is OWN else window
        pairs = [int(j) for j in pairs]
        recs = [None] * len(pairs)
        resident, owner, state = {}, [None] * S, {"next": 0}

        def stage(ids):
            pinned = {resident[i] for i in ids if i in resident}
            placed = []
            for i in ids:
                if i in resident:
                    continue
                while state["next"] % S in pinned:
                    state["next"] += 1
                s = state["next"] % S
                state["next"] += 1
                if owner[s] is not None:
                    del resident[owner[s]]
                owner[s], resident[i] = i, s
                pinned.add(s)
                placed.append((i, s))
            k = 0
            while k < len(placed):  # runs of consecutive frames in consecutive slots: one transfer each
                n = 1
                while (k + n < len(placed) and placed[k + n][0] == placed[k + n - 1][0] + 1
                       and placed[k + n][1] == placed[k + n - 1][1] + 1):
                    n += 1
                self.upload(placed[k][1], [frames[i] for i, _ in placed[k:k + n]])
                k += n

        def enqueue(l0):
            ls = list(range(l0, min(l0 + B, len(pairs))))
            js = [pairs[l] for l in ls]
            stage(sorted({j for j in js} | {j + 1 for j in js}))
            f0, f1, fl = [resident[j] for j in js], [resident[j + 1] for j in js], [slot_of(l) for l in ls]
            if reverse_slot_of is not None:   # forward, then reversed
                f0, f1, fl = f0 + f1, f1 + f0, fl + [reverse_slot_of(l) for l in ls]
            if algo == "dis":
                ctx.flow_pairs_dis(f0, f1, fl, pov_mode, dis)
            elif win != "box":
                ctx.flow_pairs_farneback(f0, f1, fl, pov_mode, fb, window=win)
            elif fb is not None:
                ctx.flow_pairs_farneback(f0, f1, fl, pov_mode, fb)
            else:
                ctx.flow_pairs(f0, f1, fl, pov_mode)
            if with_frames is not None:
                with_frames(ls, js, f0[:len(ls)], f1[:len(ls)])
            if behind is not None:
                behind(ls, js)
            return ls, js

        release = getattr(frames, "release", None)  # prefetch.PrefetchRing views: frames may be recycled once consumed

        def collect(ls, js):
            got = ctx.pass1_results([slot_of(l) for l in ls], cut_threshold)  # one call per batch
            recs[ls[0]:ls[-1] + 1] = got
            if release:
                # this batch's kernels have run, so every transfer they waited for has left the host: frames up to
                # the batch's last one will not be read from host memory again (ascending pair lists only)
                release(js[-1] + 2)
            if on_batch:
                on_batch(ls, js, got)

        pending, depth = [], getattr(self, "depth", 1)
        if queued is not None:
            for l0 in range(0, len(pairs), B):
                queued(*enqueue(l0))
            return recs
        for l0 in range(0, len(pairs), B):
            pending.append(enqueue(l0))
            if len(pending) > depth:
                collect(*pending.pop(0))
        while pending:
            collect(*pending.pop(0))
        return recs

    def process_chunk(self, frames, pov_mode=False, cut_threshold=7.0, algo=None, farneback=OWN, flows_out=None, window=OWN,
                      post_out=None, axes=False, weights=None, center=None, cells=32, grid_out=None, consistency=None,
                      weights_out=None, weights_gate=None, compensate=None, motion_out=None, residual=None, texture=None,
                      track=None, track_out=None, match_out=None, redetect_out=None):
        """One whole chunk on one GPU: returns (dots float64[n], records) with n = len(frames)-1.  `algo`, `farneback`,
        `window`: see pass1_pairs (default: the engine's own flow algorithm, parameters and window).  `flows_out`: a float32 device array of
        (n, H, W, 2) or (n, 2, H, W) that receives every pair's flow field (Context.export_flows, on torch's current stream)
        as its batch finishes, before its slots can be recycled; records and dots are unchanged.
        `post_out`: device memory for n 48-byte records (_capi.PASS2_DTYPE), or True for a new buffer (post_buffer).  The centre window, the
        cut test and pass 2 are then queued on the device behind each batch (Context.radial_window on torch's current
        stream, the calls of window_calls); pass1_results is never called, nothing waits for the device, and the call
        returns post_out, which post_records reads.  Frames out of a prefetch.PrefetchRing are the one exception: its
        page-locked slots are read in place by the transfers, so they are released as events on the stream complete and
        the call returns once the chunk's last batch has run.
        `axes`: True returns (comps float64[n, 4], records) -- the four components of _capi.AXES (Context.radial_axes;
        column 0 has the bits of the dots) -- and with post_out a buffer of 80-byte records (_capi.PASS2_AXES_DTYPE,
        post_records(..., axes=True)).
        `weights`: a per-pixel weight map, a uint8 / bool device tensor (H, W) for every pair or
        (n, H, W), one map per pair.  The chunk then runs the device schedule: post_out defaults to a new buffer, the
        records are the 80-byte form whatever `axes` says, and behind each batch Context.pass1_weighted is queued on its
        slots, then its window calls as Context.radial_window_axes_weighted.  The flow (and flows_out) is unchanged.
        `center`: "variance" takes every pass-2 term about the reference's center_of_mass_variance (FF:721-746) over a
        `cells` x `cells` grid instead of the |div| argmax.  The chunk then runs the device schedule as
        with weights: post_out defaults to a new buffer, the records are the 80-byte form, and behind each batch
        Context.cell_stats is queued on its slots, then its window calls as Context.radial_window_axes_centres.  `grid_out`:
        device memory (grid_buffer) that receives every pair's cells x cells cell records.  Not combined with `weights`.
        `weights` = "consistency": the maps are made on the device by the forward-backward check of every pair (DESIGN.md
        section 18; `consistency`: a _capi.ConsistencyParams, a dict of its fields or None for the defaults; `weights_gate`:
        an (H, W) uint8 / bool device tensor, the static gate of rule K6).  A batch is then max_batch // 2 pairs, queued as
        one flow call of the pairs and the same pairs reversed; behind it Context.consistency_weights, then the calls of
        `weights`.  The chunk's maps live in one (n, H, W) uint8 device tensor: a new one, or `weights_out`, filled in
        place.  flows_out still receives the forward fields.
        `weights` = "residual": the maps are the photometric residual of every pair under its own forward field (DESIGN.md
        section 21; `residual`: a _capi.ResidualParams, a dict of its fields or None for the defaults, which are not tuned on
        footage; `weights_gate`: the static gate of rule P6; `weights_out` as above).  The batch stays max_batch pairs and the
        ring every flow slot, nothing is queued reversed: behind each batch's flow call Context.residual_weights writes the
        batch's maps from its frame slots and raw fields, then the calls of `weights` run.
        `weights` = "texture": the maps are the structure-tensor cornerness of every pair's frame 0 (DESIGN.md section 22;
        `texture`: a _capi.TextureParams, a dict of its fields or None for the defaults, which are not tuned on footage;
        `weights_gate`: the static gate of rule T6; `weights_out` as above) -- low on flat regions and pure stripes, where the
        flow is unconstrained and both checks above approve of it.  The schedule is that of "residual", with
        Context.texture_weights on the batch's f0 slots; it combines with compensate= in the same order.
        `weights` = "residual" with `texture` (parameters, or True for the defaults): both.  Behind each batch the residual
        maps are made from the raw fields, then Context.texture_weights min-combines frame 0's texture into them in place
        (gate = out = the batch's maps), then the fit, the subtraction and the calls of `weights` run.  `texture` is refused
        with weights="consistency" (that mode has no frames hook) and without a mode.
        `compensate`: a model name of _capi.MOTION_MODELS, a dict of _capi.MotionParams fields or a MotionParams (DESIGN.md
        section 19).  Behind each batch, and before anything reads its records or fields, Context.motion_fit is queued on the
        batch's slots -- under `weights` when that is a map -- and then Context.motion_subtract in place: pass 1, pass 2,
        cell_stats, pass1_weighted and the window calls all see the compensated fields, and flows_out RECEIVES THE COMPENSATED
        FIELDS.  "similarity" and "affine" contain a zoom term, which is the radial signal itself (rule C9).  `motion_out`:
        device memory for n 64-byte records (motion_buffer; motion_records reads it), the fitted model of every pair -- the
        camera path.  Not combined with weights="consistency" (the maps need both raw directions, and the ring holds the
        reversed pairs).  With weights="residual" the order behind a batch is: the maps from the raw fields, the fit (which
        the maps weight), the subtraction.  Without compensate= nothing of this runs.
        `center` = "track" (DESIGN.md section 23): every pass-2 term about a point that follows the flow from pair to pair.
        `track`: a dict -- "state" (a track_state tensor of 1..8 tracks, read and written: hand it to the next chunk) or "start"
        ((x, y) or (T, 2), with "home" alike); "radius" and "on_cut" ("hold" | "home") of _capi.TrackParams, whose cut
        threshold is the chunk's; "roi": None or the half-axes (ax, ay) of an elliptical map about the track, "roi_soft" its
        form.  The chunk runs the device schedule with 80-byte records.  Behind each batch Context.track_advance is queued on
        its slots in pair order -- on the raw fields, ahead of compensate='s fit and subtraction -- and writes into the
        chunk-long buffer of 48-byte records (`track_out`, a track_buffer, or a new one; track_records reads it).  Without
        "roi" the window calls are Context.radial_window_axes_centres about track 0's records; with it Context.roi_weights
        writes the batch's maps into an (n, H, W) tensor (`weights_out`, or a new one; `weights_gate`: the static gate of rule
        E5), Context.pass1_weighted follows and the window calls are Context.radial_window_axes_weighted_centres.  weights= of
        any form is refused next to it.
        track["match"]: a dict of _capi.MatchParams' fields ("p", "s", "mode", "min_var", "max_mse",
        "ratio"; the defaults are not tuned on footage), optionally "templates" (a match_templates tensor the caller carries
        from chunk to chunk) and "capture" (fill the templates from the chunk's first frame about the state; default: only
        when no "templates" are given).  Behind each batch, between track_advance and roi_weights, Context.track_match
        corrects the batch's records on their f0 frames and then the state on the batch's last f1 frame, both in place, so
        every centre read afterwards is a corrected one; `match_out` (a match_buffer, or a new one; match_records reads it)
        receives the n x T 48-byte match records of the first.  A rejected match (FLAT, POOR, AMBIGUOUS) leaves its centre
        alone: after a scene cut the template is stale, matches read POOR and the track is pure advection until the caller
        re-captures (Context.track_template).  Without the key the chunk queues exactly the calls it queued before.
        track["match"]["redetect"]: True, or a dict of "reach" (0: the whole frame), "exclude" and
        "mask" (the trigger mask; default MATCH_POOR) -- p, mode and the thresholds are the match's; the defaults are not
        tuned on footage.  Straight behind the batch's search about the state, Context.track_redetect is queued with one
        item on the same frame about the state, triggered by the status words of that search, with write-back: where the
        local search failed the whole frame is searched, and the next batch starts from a re-detected state (the batch
        already advanced keeps its records).  `redetect_out` (a match_buffer of n x T records) receives that call's T records
        at the index of the batch's last pair; its other entries are not written.  Whole pixels, no scale or rotation, no
        template update; after a scene cut a global search reads POOR as well.  Without the key nothing of this is queued."""
        ctx, B = self.ctx, self.B
        n = len(frames) - 1
        trk = _chunk_track(ctx, n, center, track, track_out, weights, weights_out, weights_gate, ctx.flow_slots, cut_threshold,
                           match_out, redetect_out=redetect_out)
        if trk is not None and trk.roi is not None:   # the keywords are the track's
            weights_out = weights_gate = None
        if compensate is not None and isinstance(weights, str) and weights == "consistency":
            raise ValueError(f"compensate= together with weights={weights!r} is not supported: the consistency maps need both "
                             "raw directions of every pair, and the slot ring holds the reversed pairs")
        resid = _chunk_residual(self, n, weights, residual, consistency, weights_out, weights_gate, texture)
        cons = None if resid is not None else _chunk_consistency(self, n, weights, consistency, weights_out, weights_gate)
        if cons is not None:
            weights, B = cons.maps, cons.B
        if resid is not None:
            weights = resid.maps
        if trk is not None:
            weights = trk.maps
        ring = ctx.flow_slots if cons is None else cons.ring
        maps = weights   # the tensor stays referenced while the calls that read it are queued
        post_out, axes, weights, grid = _chunk_post_args(ctx, n, post_out, axes, weights, center, cells, grid_out,
                                                         check_empty=False, device=trk is not None)
        # the ROI maps say where the subject is, not what is reliable, and are written behind the fit's place: it runs unweighted
        comp = _chunk_motion(ctx, n, compensate, motion_out, None if trk is not None else weights, ring, pov_mode)
        if n < 1:
            return (_no_scalars(axes), []) if post_out is None else post_out
        layout = None
        if flows_out is not None:
            shp = tuple(flows_out.shape)
            layout = ("nhwc" if shp == (n, ctx.height, ctx.width, 2) else
                      "nchw" if shp == (n, 2, ctx.height, ctx.width) else None)
            if layout is None:
                raise ValueError(f"flows_out must be ({n}, {ctx.height}, {ctx.width}, 2) or ({n}, 2, {ctx.height}, "
                                 f"{ctx.width}), got {shp}")
        if post_out is not None:
            post = _DevicePost(ctx, n, B, pov_mode, cut_threshold, post_out, axes, weights, grid, ring, cons, trk)
            release = getattr(frames, "release", None)
            marks = []   # (event, frames that have left the host once it completes), oldest first

            if comp is not None:
                comp.stream = post.stream
            if resid is not None:
                resid.stream = post.stream
            if trk is not None:
                trk.stream = post.stream

            def queued(ls, js):
                if layout is not None:   # before the window calls below let later batches recycle these slots
                    ctx.export_flows([j % ring for j in js], flows_out[js[0]:js[-1] + 1], layout)
                done = post.after_batch(js[0] // B)
                if release is None:
                    return
                if not done:   # batches no longer than the window's radius: no call has waited for this one yet
                    ctx.sync()
                    release(js[-1] + 2)
                    return
                # an event behind the window call, hence behind the batches of pairs < done: frames <= done have left the host
                marks.append((_stream_event(ctx, post.stream), done + 1))
                while marks and (marks[0][0].query() or len(marks) > getattr(self, "depth", 1)):
                    ev, upto = marks.pop(0)
                    ev.synchronize()
                    release(upto)

            self.pass1_pairs(frames, range(n), lambda l: l % ring, pov_mode, cut_threshold, algo=algo,
                             farneback=farneback, window=window, queued=queued,
                             **_chain(trk and trk.behind, comp and comp.behind),
                             **_frames_kw(trk if trk is not None and trk.match is not None else resid),
                             **({} if cons is None else {"batch": B, "reverse_slot_of": cons.bwd_slot}))
            if marks:
                marks[-1][0].synchronize()   # the ring's slots may be reused by the next chunk: every transfer is over
            post.finish()
            return post_out
        post = _ChunkPost(ctx, n, B, pov_mode, axes)

        def on_batch(js, got):
            if layout is not None:   # before pass 2 below lets later batches recycle these slots
                ctx.export_flows([j % ctx.flow_slots for j in js], flows_out[js[0]:js[-1] + 1], layout)
            post.add(js, got)

        self.pass1(frames, 0, n, pov_mode, cut_threshold, on_batch, algo=algo, farneback=farneback, window=window,
                   **_behind_kw(comp))
        return post.finish()

    def process_flows(self, flows, pov_mode=False, cut_threshold=7.0, post_out=None, axes=False, weights=None, center=None,
                      cells=32, grid_out=None, compensate=None, motion_out=None, track=None, track_out=None, weights_out=None,
                      weights_gate=None):
        """One whole chunk from flow fields the caller computed: returns (dots float64[n], records), the contract of
        process_chunk.  `flows` holds the chunk's n pair fields in device memory: one array (n, H, W, 2) or (n, 2, H, W)
        (float32, float16 or bfloat16, any strides; see _capi.device_flows) or a sequence of such arrays (single (H, W, 2)
        fields included), in pair order.  They are imported B at a time into the slot ring (Context.import_flows, on
        torch's current stream) with `depth` batches in flight; the +-6 window and pass 2 are process_chunk's own.
        `post_out`: as in process_chunk (a buffer, or True for a new one) -- pass 2 is queued on the device behind each
        import, nothing waits, and the buffer is returned for post_records.  `axes`, `weights`: as in process_chunk (with
        weights: the device schedule, 80-byte records, pass1_weighted behind each import).  `center`, `cells`, `grid_out`:
        as in process_chunk (center="variance": the device schedule, 80-byte records, cell_stats behind each import).
        `compensate`, `motion_out`: as in process_chunk -- motion_fit and motion_subtract in place behind each import, before
        anything reads the imported fields' records.  `center` = "track", `track`, `track_out`, and with track["roi"]
        `weights_out` and `weights_gate`: as in process_chunk -- track_advance behind each import, ahead of the fit."""
        ctx, B, fs = self.ctx, self.B, self.ctx.flow_slots
        if isinstance(weights, str) and weights == "residual":
            raise ValueError("process_flows: weights='residual' needs the frames, which a chunk of caller flows does not have; "
                             "Context.residual_weights serves callers who hold the frames in the context's frame slots")
        if isinstance(weights, str) and weights == "texture":
            raise ValueError("process_flows: weights='texture' needs the frames, which a chunk of caller flows does not have; "
                             "Context.texture_weights serves callers who hold the frames in the context's frame slots")
        if isinstance(weights, str):
            raise ValueError(f"process_flows: weights={weights!r} needs the backward fields, which a chunk of caller flows does "
                             "not have; Context.consistency_weights serves callers with their own estimator")
        segs = []   # (descriptor, dtype, first pair, count): one per source array
        n = 0
        for a in (flows if isinstance(flows, (list, tuple)) else [flows]):
            desc, dt, k = _capi.device_flows(a, ctx.width, ctx.height)
            segs.append((desc, dt, n, k))
            n += k
        trk = _chunk_track(ctx, n, center, track, track_out, weights, weights_out, weights_gate, fs, cut_threshold, frames=False)
        if trk is None and (weights_out is not None or weights_gate is not None):
            raise ValueError("process_flows: weights_out= and weights_gate= need center='track' with track['roi']")
        if trk is not None:
            weights = trk.maps
        maps = weights   # the tensor stays referenced while the calls that read it are queued
        # the ROI maps are the schedule's own tensor: a chunk without pairs has none to look at, as in process_chunk
        post_out, axes, weights, grid = _chunk_post_args(ctx, n, post_out, axes, weights, center, cells, grid_out,
                                                         check_empty=trk is None, device=trk is not None)
        if n < 1:
            return (_no_scalars(axes), []) if post_out is None else post_out
        post = (_ChunkPost(ctx, n, B, pov_mode, axes) if post_out is None else
                _DevicePost(ctx, n, B, pov_mode, cut_threshold, post_out, axes, weights, grid, track=trk))
        comp = _chunk_motion(ctx, n, compensate, motion_out, None if trk is not None else weights, fs, pov_mode)
        if comp is not None and post_out is not None:
            comp.stream = post.stream
        if trk is not None:
            trk.stream = post.stream

        def enqueue(j0):
            j1 = min(j0 + B, n)
            for desc, dt, first, k in segs:
                lo, hi = max(j0, first), min(j1, first + k)
                if lo >= hi:
                    continue
                part = _capi.DevFlow(desc.base + (lo - first) * desc.item_stride, desc.item_stride, desc.row_pitch,
                                     desc.pixel_stride, desc.channel_stride)
                ctx.import_flows_desc(part, dt, [j % fs for j in range(lo, hi)], pov_mode)
            js = list(range(j0, j1))
            if trk is not None:
                trk.behind(js, js)
            if comp is not None:
                comp.behind(js, js)
            return js

        def collect(js):
            post.add(js, ctx.pass1_results([j % fs for j in js], cut_threshold))

        if post_out is not None:
            for j0 in range(0, n, B):
                enqueue(j0)
                post.after_batch(j0 // B)
            post.finish()
            return post_out
        pending = []
        for j0 in range(0, n, B):
            pending.append(enqueue(j0))
            if len(pending) > self.depth:
                collect(pending.pop(0))
        while pending:
            collect(pending.pop(0))
        return post.finish()


def _no_scalars(axes):
    """the scalars of a chunk without pairs"""
    return np.zeros((0, len(_capi.AXES))) if axes else np.zeros(0)


def _chunk_weights(ctx, weights, n):
    """the _capi.DevWeights of a chunk of n pairs: `weights` is one (H, W) map for every pair or (n, H, W), one per pair"""
    desc, m = _capi.device_weights(weights, ctx.width, ctx.height)
    if m not in (0, n):
        raise ValueError(f"weights: {m} maps for a chunk of {n} pairs (one (H, W) map, or one per pair)")
    return desc


# weights= / params["hip_weights"] as a string: maps the library makes itself.  WEIGHT_MODES keeps the value its users know: the
# modes made from both flow directions of a pair, which halve the batch and exclude compensate=; MAP_MODES is every mode
WEIGHT_MODES = ("consistency",)
MAP_MODES = WEIGHT_MODES + ("residual",)
FRAME_MAP_MODES = ("residual", "texture")       # made behind a batch from its frame slots (pass1_pairs' with_frames hook)
ALL_MAP_MODES = MAP_MODES + ("texture",)        # every mode; MAP_MODES keeps the value its users know as well


class _ChunkConsistency:
    """What weights="consistency" adds to a chunk of n pairs on `engine`: B = max_batch // 2 pairs per
    batch; the forward fields keep a ring over the first `ring` = flow_slots - (depth + 1) * B flow slots, the backward field
    of the l-th pair goes to bwd_slot(l) in the region behind it; maps: the chunk's (n, H, W) uint8 device tensor; params: the
    checked _capi.ConsistencyParams; gate: the static gate's _capi.DevWeights or None (its tensor stays referenced)."""

    def __init__(self, engine, n, params, maps_out, gate):
        ctx = engine.ctx
        self.B = ctx.max_batch // 2
        if self.B < 1:
            raise ValueError("weights='consistency' needs max_batch >= 2: a batch is max_batch // 2 pairs, queued forward and reversed")
        self.params = _capi.consistency_choice(params)
        region = (getattr(engine, "depth", 1) + 1) * self.B
        self.ring = ctx.flow_slots - region   # >= (depth + 1) * B + 13 on any engine: min_flow_slots(max_batch, depth)
        self.bwd_slot = lambda l: self.ring + l % region
        self.maps = _chunk_maps(ctx, n, maps_out)
        self.gate_tensor, self.gate = gate, _static_gate(ctx, gate)


def _chunk_maps(ctx, n, maps_out):
    """the (n, H, W) uint8 device tensor a mode of MAP_MODES fills: weights_out, checked, or a new one"""
    import torch
    shape = (max(n, 0), ctx.height, ctx.width)
    if maps_out is None:
        return torch.empty(shape, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    if not isinstance(maps_out, torch.Tensor) or maps_out.dtype != torch.uint8 or tuple(maps_out.shape) != shape:
        raise ValueError(f"weights_out must be a uint8 device tensor of shape {shape}")
    return maps_out


def _static_gate(ctx, gate):
    """weights_gate= as a _capi.DevWeights: one static (H, W) map, or None"""
    if gate is None:
        return None
    desc, m = _capi.device_weights(gate, ctx.width, ctx.height)
    if m != 0:
        raise ValueError("weights_gate: one static (H, W) map")
    return desc


def _chunk_consistency(engine, n, weights, params, maps_out, gate):
    """None unless weights is a string, which must then name a mode of WEIGHT_MODES ("residual" never arrives here: _chunk_residual
    takes it first); the keywords that belong to a mode are refused without one"""
    if not isinstance(weights, str):
        if params is not None or maps_out is not None or gate is not None:
            raise ValueError("consistency=, weights_out= and weights_gate= need weights='consistency' (the latter two: or 'residual')")
        return None
    if weights not in WEIGHT_MODES:
        raise ValueError(f"weights must be a device tensor of maps or one of {WEIGHT_MODES}, got {weights!r}; or 'residual', the "
                         "mode that needs no backward flow")
    return _ChunkConsistency(engine, n, params, maps_out, gate)


class _ChunkResidual:
    """What weights="residual" adds to a chunk of n pairs on `engine`: nothing about its batches or its
    slot ring; with_frames(ls, js, f0, f1), pass1_pairs' hook, queues Context.residual_weights on the batch's frame slots and
    raw fields (the l-th pair in flow slot l % flow_slots), which writes the pairs' maps into the chunk's (n, H, W) uint8 device
    tensor `maps`.  params: the checked _capi.ResidualParams; gate: the static gate's _capi.DevWeights or None (its tensor
    stays referenced); stream: where the call is queued (the device schedule sets its side stream).  texture: None, or the
    checked _capi.TextureParams of the combination -- Context.texture_weights is then queued behind the
    residual call with gate = out = the batch's maps, which min-combines frame 0's texture into them in place."""

    def __init__(self, engine, n, params, maps_out, gate, texture=None):
        self.ctx = engine.ctx
        self.params = _capi.residual_choice(params)
        self.texture = None if texture is None else _capi.texture_choice(texture)
        self.maps = _chunk_maps(self.ctx, n, maps_out)
        self.gate_tensor, self.gate = gate, _static_gate(self.ctx, gate)
        self.stream = None

    def with_frames(self, ls, js, f0, f1):
        maps = self.maps[js[0]:js[-1] + 1]
        self.ctx.residual_weights(f0, f1, [l % self.ctx.flow_slots for l in ls], maps, self.params, self.gate, self.stream)
        if self.texture is not None:
            self.ctx.texture_weights(f0, maps, self.texture, maps, self.stream)


class _ChunkTexture:
    """What weights="texture" adds to a chunk of n pairs on `engine`: _ChunkResidual's form without a
    flow -- with_frames queues Context.texture_weights on the batch's f0 slots (the frame the flow is defined on), which writes
    the pairs' maps into `maps`.  params: the checked _capi.TextureParams; gate: the static gate of rule T6 or None."""

    def __init__(self, engine, n, params, maps_out, gate):
        self.ctx = engine.ctx
        self.params = _capi.texture_choice(params)
        self.maps = _chunk_maps(self.ctx, n, maps_out)
        self.gate_tensor, self.gate = gate, _static_gate(self.ctx, gate)
        self.stream = None

    def with_frames(self, ls, js, f0, f1):
        self.ctx.texture_weights(f0, self.maps[js[0]:js[-1] + 1], self.params, self.gate, self.stream)


def _chunk_residual(engine, n, weights, params, consistency, maps_out, gate, texture=None):
    """None unless weights is "residual" or "texture", the modes of FRAME_MAP_MODES; residual= is refused without "residual",
    texture= without either, and consistency= with both.  texture= next to "residual" (parameters, or True for the defaults) is
    the combination of the two maps."""
    mode = weights if isinstance(weights, str) and weights in FRAME_MAP_MODES else None
    if mode != "residual" and params is not None:
        raise ValueError("residual= needs weights='residual'")
    if mode is None:
        if texture is not None:
            raise ValueError("texture= needs weights='texture', or weights='residual' for the combination of the two maps"
                             + (" (weights='consistency' has no frames hook to queue it from)" if isinstance(weights, str) and weights == "consistency" else ""))
        return None
    if consistency is not None:
        raise ValueError(f"consistency= needs weights='consistency', not weights={mode!r} (its parameters are {mode}=)")
    if mode == "texture":
        return _ChunkTexture(engine, n, texture, maps_out, gate)
    return _ChunkResidual(engine, n, params, maps_out, gate, texture)


def _frames_kw(resid):
    """with_frames= only where there is something to queue: an engine without the keyword keeps serving the plain chunk"""
    return {} if resid is None else {"with_frames": resid.with_frames}


def chunk_center(center):
    """center= / params["hip_center"]: None (the |div| argmax of pass 1) or one of _capi.CENTERS"""
    if center is not None and center not in _capi.CENTERS:
        raise ValueError(f"center must be None or one of {_capi.CENTERS}, got {center!r}")
    return center


TRACK_KEYS = ("state", "start", "home", "radius", "on_cut", "roi", "roi_soft", "match")
MATCH_KEYS = _capi.MATCH_FIELDS + ("templates", "capture", "match_out", "redetect")
REDETECT_KEYS = ("reach", "exclude", "mask")


def _redetect_choice(match, r):
    """the RedetectParams of track["match"]["redetect"] = r (True or a dict of REDETECT_KEYS) next to the MatchParams `match`,
    whose p, mode and thresholds it takes; exclude defaults to p"""
    if r is True:
        r = {}
    unknown = [k for k in r if k not in REDETECT_KEYS] if isinstance(r, dict) else ["redetect"]
    if unknown:
        raise ValueError(f"track['match']['redetect']: True or a dict of {REDETECT_KEYS}; unknown key {unknown[0]!r}")
    over = {"exclude": match.p if r.get("exclude") is None else r["exclude"]}
    if r.get("reach") is not None:
        over["reach"] = r["reach"]
    if r.get("mask") is not None:
        over["trigger_mask"] = r["mask"]
    return _capi.redetect_choice({"p": match.p, "mode": match.mode, "min_var": match.min_var, "max_mse": match.max_mse,
                                  "ratio": match.ratio, **over})


redetect_choice = _redetect_choice   # the public name: callers who queue Context.track_redetect themselves form the same parameters


class _ChunkTrack:
    """center="track" of a chunk of n pairs: behind(ls, js) queues Context.track_advance on the slots of
    the chunk's pairs ls (the l-th pair in flow slot l % ring), in pair order, with the records of pair l at byte 48 * T * l of
    the chunk's buffer (track_out, or a new one) -- on the RAW fields, ahead of compensate='s fit and subtraction and of
    pass1_weighted, so rule Q5's cut is the unweighted whole-frame mean magnitude.  With roi, Context.roi_weights then writes
    the pairs' maps about track 0's records into the chunk's (n, H, W) uint8 tensor `maps` (weights_out, or a new one; gate:
    the static gate of rule E5).  state: the device tensor of T ffl_track_state records, read and written, which the caller
    carries to the next chunk.  stream: where the calls are queued (the device schedule sets its side stream).
    With track["match"] with_frames(ls, js, f0, f1), pass1_pairs' hook, keeps the batch's frame slots, and
    where the templates are to be captured queues Context.track_template on f0[0] about the state, once, before the first
    advance; behind() then queues, between track_advance and roi_weights, Context.track_match on the f0 slots about the batch's
    records and Context.track_match with one item on f1[last] about the state, both with write-back: the window calls and the
    ROI maps read corrected centres, and the next batch starts from a corrected state.  Without the key nothing of this is
    queued.
    With track["match"]["redetect"] behind() queues, straight after the search about the state,
    Context.track_redetect with one item on the same frame about the state, triggered by the status words of that search, with
    write-back; its T records go to redetect_out (or a new buffer) at the index of the batch's last pair."""

    def __init__(self, ctx, n, track, track_out, maps_out, gate, ring, cut_threshold, match_out=None, redetect_out=None):
        if not isinstance(track, dict) or not (("state" in track) ^ ("start" in track)):
            raise ValueError("center='track' needs track= {'state': a track_state tensor} or {'start': (x, y) or (T, 2)}, one of "
                             "the two")
        unknown = [k for k in track if k not in TRACK_KEYS]
        if unknown:
            raise ValueError(f"track=: unknown key {unknown[0]!r} (one of {TRACK_KEYS})")
        self.ctx, self.n, self.ring = ctx, n, int(ring)
        over = {k: track[k] for k in ("radius", "on_cut") if track.get(k) is not None}
        self.params = _capi.track_choice(_capi.TrackParams(cut_threshold=float(cut_threshold), **over))
        self.match, m = None, track.get("match")
        if m is not None:
            unknown = [k for k in m if k not in MATCH_KEYS] if isinstance(m, dict) else ["match"]
            if unknown:
                raise ValueError(f"track['match']: a dict of {MATCH_KEYS}; unknown key {unknown[0]!r}")
            self.match = _capi.match_choice({k: m[k] for k in _capi.MATCH_FIELDS if m.get(k) is not None})
        elif match_out is not None:
            raise ValueError("match_out= needs track['match'] with center='track'")
        self.redetect, r = None, m.get("redetect") if isinstance(m, dict) else None
        if r is not None and r is not False:
            self.redetect = _redetect_choice(self.match, r)
        elif redetect_out is not None:
            raise ValueError("redetect_out= needs track['match']['redetect'] with center='track'")
        if "state" in track:
            if "home" in track:
                raise ValueError("track=: 'home' goes with 'start' (a state carries its own home position)")
            self.state = track["state"]
        else:
            self.state = track_state(ctx, track["start"], track.get("home"))
        _, sbytes = _capi._device_span(self.state)
        item = _capi.TRACK_STATE_DTYPE.itemsize
        self.T = sbytes // item
        if sbytes % item or not 1 <= self.T <= _capi.FFL_MAX_TRACKS:
            raise ValueError(f"track=: the state holds {sbytes} bytes, 1..{_capi.FFL_MAX_TRACKS} records of {item} are needed")
        self.item = self.T * _capi.TRACK_DTYPE.itemsize
        self.out = track_buffer(ctx, max(n, 1), self.T) if track_out is None else track_out   # stays referenced
        self.base, nbytes = _capi._device_span(self.out)
        if nbytes < n * self.item:
            raise ValueError(f"track_out holds {nbytes} bytes, the chunk's {n} x {self.T} records need {n * self.item}")
        self.roi = self.maps = self.gate = self.gate_tensor = None
        if track.get("roi") is not None:
            ax, ay = track["roi"]
            self.roi = _capi.roi_choice({"ax": float(ax), "ay": float(ay), "soft": int(bool(track.get("roi_soft", True)))})
            self.maps = _chunk_maps(ctx, n, maps_out)
            self.gate_tensor, self.gate = gate, _static_gate(ctx, gate)
        elif maps_out is not None or gate is not None or track.get("roi_soft") is not None:
            raise ValueError("weights_out=, weights_gate= and track['roi_soft'] need track['roi'] = (ax, ay) with center='track'")
        self.stream = None
        self.templates = self.match_out = self.frames = None
        self.capture = False
        if self.match is not None:
            self.templates = m.get("templates")
            self.capture = bool(m.get("capture", self.templates is None))
            if self.templates is None:
                self.templates = match_templates(ctx, self.T, self.match.p)
            need = self.T * (2 * self.match.p + 1) ** 2
            if _capi._device_span(self.templates)[1] < need:
                raise ValueError(f"track['match']['templates'] holds {_capi._device_span(self.templates)[1]} bytes, {self.T} "
                                 f"templates of p = {self.match.p} need {need}")
            match_out = m.get("match_out") if match_out is None else match_out
            self.match_out = match_buffer(ctx, max(n, 1), self.T) if match_out is None else match_out   # stays referenced
            self.mbase, nbytes = _capi._device_span(self.match_out)
            if nbytes < n * self.item:
                raise ValueError(f"match_out holds {nbytes} bytes, the chunk's {n} x {self.T} records need {n * self.item}")
            self.state_match = match_buffer(ctx, 1, self.T)   # the records of the latest search about the state
        if self.redetect is not None:
            self.redetect_out = match_buffer(ctx, max(n, 1), self.T) if redetect_out is None else redetect_out   # stays referenced
            self.rbase, nbytes = _capi._device_span(self.redetect_out)
            if nbytes < n * self.item:
                raise ValueError(f"redetect_out holds {nbytes} bytes, the chunk's {n} x {self.T} records need {n * self.item}")

    def with_frames(self, ls, js, f0, f1):
        self.frames = (list(f0), list(f1))
        if self.capture:   # the first batch: the subject as the state sees it in the chunk's first frame
            self.ctx.track_template(f0[0], self.state, self.templates, self.match.p, self.T, self.stream)
            self.capture = False

    def centres(self, lo, hi):
        """the centres of pairs lo .. hi-1 for a window call: track 0's records, one every 48 * T bytes"""
        return _capi._DeviceSpan(self.base + lo * self.item, (hi - lo) * self.item), self.item

    def behind(self, ls, js):
        recs = _capi._DeviceSpan(self.base + ls[0] * self.item, len(ls) * self.item)
        self.ctx.track_advance([l % self.ring for l in ls], self.state, recs, self.params, None, self.stream)
        if self.match is not None:
            f0, f1 = self.frames
            out = _capi._DeviceSpan(self.mbase + ls[0] * self.item, len(ls) * self.item)
            self.ctx.track_match(f0, self.templates, (recs, self.item), out, self.match, self.T, True, self.stream)
            self.ctx.track_match([f1[-1]], self.templates, (self.state, self.item), self.state_match, self.match, self.T, True,
                                 self.stream)
            if self.redetect is not None:
                out = _capi._DeviceSpan(self.rbase + ls[-1] * self.item, self.item)
                self.ctx.track_redetect([f1[-1]], self.templates, (self.state, self.item), out, self.redetect, self.T,
                                        self.state_match, True, self.stream)
        if self.roi is not None:
            self.ctx.roi_weights(len(ls), (recs, self.item), self.maps[ls[0]:ls[-1] + 1], self.roi, self.gate, self.stream)


def _chunk_track(ctx, n, center, track, track_out, weights, maps_out, gate, ring, cut_threshold, match_out=None, frames=True,
                 redetect_out=None):
    """None unless center == "track" (track=, track_out= and match_out= are then refused), else the chunk's _ChunkTrack;
    weights= of any form is refused next to it, and track["match"] by a chunk without frames (frames=False)"""
    if center != "track":
        if track is not None or track_out is not None:
            raise ValueError("track= and track_out= need center='track'")
        if match_out is not None:
            raise ValueError("match_out= needs center='track' with track['match']")
        if redetect_out is not None:
            raise ValueError("redetect_out= needs center='track' with track['match']['redetect']")
        return None
    if not frames and isinstance(track, dict) and track.get("match") is not None:
        raise ValueError("process_flows: track['match'] needs the frames, which a chunk of caller flows does not have; "
                         "Context.track_match serves callers who hold frames in the context's frame slots")
    if weights is not None:
        raise ValueError("center='track' together with weights= (a map or a mode) is not supported: the region's own map is "
                         "track={'roi': (ax, ay)}, and weights_gate= is its static gate")
    if isinstance(track, dict) and "redetect" in track:
        raise ValueError("track=: 'redetect' is a key of track['match'] (it searches for the match's templates)")
    return _ChunkTrack(ctx, n, track, track_out, maps_out, gate, ring, cut_threshold, match_out, redetect_out)


def _chain(*hooks):
    """behind= of several parts of a chunk, in order; None without any"""
    hooks = [h for h in hooks if h is not None]
    if not hooks:
        return {}
    if len(hooks) == 1:
        return {"behind": hooks[0]}

    def behind(ls, js):
        for h in hooks:
            h(ls, js)
    return {"behind": behind}


def _chunk_grid(ctx, center, cells, grid_out, weights, n):
    """None without center=, else what _DevicePost needs for a chunk of n pairs about the variance centre: (cells, the chunk's
    centre records -- a new device buffer of n 32-byte records -- and grid_out's base address or None)"""
    if chunk_center(center) is None or center == "track":   # the tracked centres are _chunk_track's
        if grid_out is not None:
            raise ValueError("grid_out needs center='variance'")
        return None
    if weights is not None:
        raise ValueError("center='variance' together with weights= is not supported")
    cells = int(cells)
    _capi.cell_grid(ctx.width, ctx.height, cells)
    import torch
    centres = torch.empty(max(n, 1) * _capi.GRID_CENTRE_DTYPE.itemsize, dtype=torch.uint8, device=torch.device("cuda", ctx.device))
    base = None
    if grid_out is not None:
        base, nbytes = _capi._device_span(grid_out)
        need = n * cells * cells * _capi.CELL_DTYPE.itemsize
        if nbytes < need:
            raise ValueError(f"grid_out holds {nbytes} bytes, the chunk's {n} grids of {cells} x {cells} cells need {need}")
    return cells, centres, base


def _chunk_post_args(ctx, n, post_out, axes, weights, center, cells, grid_out, check_empty=True, device=False):
    """The keywords of process_chunk / process_flows as what the schedule of a chunk of n pairs needs: (post_out, axes, the
    chunk's _capi.DevWeights or None, _chunk_grid's tuple or None).  weights= and center= each put the chunk on the device
    schedule with 80-byte records: axes is True and post_out defaults to a new buffer; post_out=True is that buffer from
    here on (no records for a chunk without pairs, n <= 0).  check_empty=False: the maps of such a chunk are not looked at.
    device=True (center="track"): the device schedule with 80-byte records whether or not there are maps."""
    grid = _chunk_grid(ctx, center, cells, grid_out, weights, n)
    desc = _chunk_weights(ctx, weights, n) if weights is not None and (n >= 1 or check_empty) else None
    if grid is not None or weights is not None or device:
        axes, post_out = True, True if post_out is None else post_out
    if post_out is True:
        post_out = post_buffer(ctx, max(n, 0), axes)
    return post_out, axes, desc, grid


class _ChunkMotion:
    """compensate= of a chunk of n pairs: behind(ls, js) queues Context.motion_fit on the slots of the
    chunk's pairs ls (the l-th pair in flow slot l % ring) -- under the chunk's maps when it has any -- with pair l's record
    at byte 64 * l of the chunk's buffer (motion_out, or a new one), then Context.motion_subtract in place.  stream: where the
    calls are queued (None: torch's current stream; the device schedule sets its side stream)."""

    def __init__(self, ctx, n, params, out, weights, ring, pov_mode):
        self.ctx, self.params, self.weights, self.ring, self.pov_mode = ctx, params, weights, int(ring), pov_mode
        self.out = motion_buffer(ctx, max(n, 1)) if out is None else out   # stays referenced while the calls are queued
        self.base, nbytes = _capi._device_span(self.out)
        self.item = _capi.MOTION_DTYPE.itemsize
        if nbytes < n * self.item:
            raise ValueError(f"motion_out holds {nbytes} bytes, the chunk's {n} records need {n * self.item}")
        self.stream = None

    def behind(self, ls, js):
        slots, w = [l % self.ring for l in ls], self.weights
        maps = None if w is None else _capi.DevWeights(w.base + ls[0] * w.item_stride, w.item_stride, w.row_pitch)
        recs = _capi._DeviceSpan(self.base + ls[0] * self.item, len(ls) * self.item)
        self.ctx.motion_fit(slots, self.params, weights=maps, out=recs, stream=self.stream)
        self.ctx.motion_subtract(slots, slots, recs, self.pov_mode, self.stream)


def _chunk_motion(ctx, n, compensate, motion_out, weights, ring, pov_mode):
    """None without compensate= (motion_out= is then refused), else the chunk's _ChunkMotion; weights: the chunk's
    _capi.DevWeights or None"""
    if compensate is None:
        if motion_out is not None:
            raise ValueError("motion_out needs compensate=")
        return None
    return _ChunkMotion(ctx, n, _capi.motion_choice(compensate), motion_out, weights, ring, pov_mode)


def _behind_kw(comp):
    """behind= only where there is something to queue: an engine without the keyword keeps serving the plain chunk"""
    return {} if comp is None else {"behind": comp.behind}


def compensate_kwargs(params):
    """{"compensate": ...} when params names "hip_compensate" -- a model name of _capi.MOTION_MODELS or a dict of the three
    _capi.MotionParams fields -- else {}: the keyword of process_chunk / process_flows, checked here"""
    comp = params.get("hip_compensate")
    if comp is None:
        return {}
    return {"compensate": _capi.motion_choice(comp)}


def _no_sharded_compensate(compensate, who):
    if compensate is not None:
        raise ValueError(f"{who}: the sharded schedules run on the raw fields; compensate= needs PairEngine.process_chunk / "
                         "process_flows on one device")


def _no_sharded_weights(weights, who):
    if weights is not None:
        raise ValueError(f"{who}: the sharded schedules run unweighted; weights= (maps, 'consistency' or 'residual') needs "
                         "PairEngine.process_chunk on one device")


def _no_sharded_center(center, who):
    if center is not None:
        raise ValueError(f"{who}: the sharded schedules take their centres from the |div| argmax; center= needs "
                         "PairEngine.process_chunk / process_flows on one device")


class _ChunkPost:
    """The +-6 centre window and pass 2 of one chunk of n pairs (FF:1203-1236), shared by process_chunk and process_flows:
    add() takes a finished batch's pass-1 records in pair order and issues pass 2, B pairs per call, for every pair whose
    window is complete; finish() issues the rest and returns (dots, records).  Window means are exact integer prefix
    sums / counts, bit-identical to np.mean over the window.  axes=True: pass 2 is Context.radial_axes and the dots are
    float64[n, 4]."""

    def __init__(self, ctx, n, B, pov_mode, axes=False):
        self.ctx, self.n, self.B, self.pov_mode = ctx, n, B, pov_mode
        self.radial = ctx.radial_axes if axes else ctx.radial
        self.dots = np.zeros((n, len(_capi.AXES)) if axes else n, np.float64)
        self.psum = np.zeros((n + 1, 2), np.int64)   # prefix sums of pos_center
        self.cuts = np.zeros(n, bool)
        self.recs = [None] * n
        self.done = 0

    def _finalize(self, limit):
        ctx, n, B = self.ctx, self.n, self.B
        while self.done < limit:
            j0, j1 = self.done, min(self.done + B, limit)
            js = np.arange(j0, j1)
            lo, hi = np.maximum(0, js - SMOOTH_RADIUS), np.minimum(n, js + SMOOTH_RADIUS + 1)
            cs = (self.psum[hi] - self.psum[lo]) / (hi - lo)[:, None]
            self.dots[j0:j1] = self.radial(list(js % ctx.flow_slots), cs, self.cuts[j0:j1], self.pov_mode)
            self.done = j1

    def add(self, js, got):
        j0, j1 = js[0], js[-1] + 1
        self.recs[j0:j1] = got
        p = np.array([(r[0], r[1]) for r in got], np.int64)
        self.psum[j0 + 1:j1 + 1] = self.psum[j0] + np.cumsum(p, axis=0)
        self.cuts[j0:j1] = [r[4] for r in got]
        self._finalize(self.n if j1 == self.n else max(0, j1 - SMOOTH_RADIUS))

    def finish(self):
        self._finalize(self.n)
        return self.dots, self.recs


class _DevicePost:
    """_ChunkPost's schedule on the device: after_batch(k) queues the Context.radial_window calls window_calls lists for
    batch k (pair j in flow slot j % flow_slots, its record at byte 48 * j of `out`) on a stream of their own
    (_side_stream); finish() makes torch's current stream wait for them.  Nothing is read back.  axes=True: the calls are
    Context.radial_window_axes and the records 80 bytes.  weights (a _capi.DevWeights of the chunk's pairs, with axes):
    after_batch(k) first queues Context.pass1_weighted on batch k's slots, and its calls are
    Context.radial_window_axes_weighted with the maps of their computed pairs.  grid (_chunk_grid's, with axes): after_batch(k)
    first queues Context.cell_stats on batch k's slots, which writes the pairs' centre records into a chunk-long buffer at
    their absolute indices (and their cell records into grid_out), and its calls are Context.radial_window_axes_centres
    with the centres of their seq read from that buffer -- a neighbour's recycled slot is never re-read for its centre.
    ring: the length of the flow-slot ring the pairs live in (default: every flow slot of the context).  cons (a
    _ChunkConsistency, with weights = the descriptor of its maps): after_batch(k) first of all queues
    Context.consistency_weights, which writes batch k's maps from its forward slots and cons.bwd_slot's backward ones.
    track (a _ChunkTrack, with axes; its behind() hook has queued the batch's records, and with roi its maps, which are then
    `weights`): the calls are Context.radial_window_axes_centres about track 0's records of their seq, read from the track's
    chunk-long buffer, or with maps Context.radial_window_axes_weighted_centres."""

    def __init__(self, ctx, n, B, pov_mode, cut_threshold, out, axes=False, weights=None, grid=None, ring=None, cons=None,
                 track=None):
        self.ctx, self.pov_mode, self.cut_threshold, self.track = ctx, pov_mode, cut_threshold, track
        self.n, self.B, self.weights, self.grid = n, B, weights, grid
        self.ring, self.cons = (ctx.flow_slots if ring is None else int(ring)), cons
        self.window, self.item = (ctx.radial_window_axes if axes else ctx.radial_window), _post_dtype(axes).itemsize
        self.base, nbytes = _capi._device_span(out)
        if nbytes < n * self.item:
            raise ValueError(f"post_out holds {nbytes} bytes, the chunk's {n} records need {n * self.item}")
        self.stream = _side_stream(ctx)
        self.calls = {}
        for c in window_calls(n, B):
            self.calls.setdefault(c[4], []).append(c)

    def after_batch(self, k):
        """queue batch k's calls; returns the number of leading pairs whose batches these calls have waited for (0: none)"""
        fs, item, done = self.ring, self.item, 0
        if self.cons is not None:   # the batch's maps, before pass1_weighted reads them
            j0, j1 = k * self.B, min((k + 1) * self.B, self.n)
            self.ctx.consistency_weights([j % fs for j in range(j0, j1)], [self.cons.bwd_slot(j) for j in range(j0, j1)],
                                         self._maps(j0), self.cons.params, self.cons.gate, self.stream)
        if self.weights is not None:   # the batch's records under the maps, before any window call reads them
            j0, j1 = k * self.B, min((k + 1) * self.B, self.n)
            self.ctx.pass1_weighted([j % fs for j in range(j0, j1)], self._maps(j0), self.pov_mode, self.stream)
        if self.grid is not None:   # the batch's centres, before any window call reads them
            cells, centres, gbase = self.grid
            j0, j1 = k * self.B, min((k + 1) * self.B, self.n)
            citem, gitem = _capi.GRID_CENTRE_DTYPE.itemsize, cells * cells * _capi.CELL_DTYPE.itemsize
            self.ctx.cell_stats([j % fs for j in range(j0, j1)], cells,
                                None if gbase is None else _capi._DeviceSpan(gbase + j0 * gitem, (j1 - j0) * gitem),
                                _capi._DeviceSpan(centres.data_ptr() + j0 * citem, (j1 - j0) * citem), self.stream)
        for lo, hi, first, count, _ in self.calls.get(k, ()):
            out = _capi._DeviceSpan(self.base + (lo + first) * item, count * item)
            seq = [j % fs for j in range(lo, hi)]
            if self.track is not None and self.weights is not None:
                self.ctx.radial_window_axes_weighted_centres(seq, first, count, self._maps(lo + first), self.track.centres(lo, hi),
                                                             out, SMOOTH_RADIUS, self.cut_threshold, self.pov_mode, self.stream)
            elif self.track is not None:
                self.ctx.radial_window_axes_centres(seq, first, count, self.track.centres(lo, hi), out, SMOOTH_RADIUS,
                                                    self.cut_threshold, self.pov_mode, self.stream)
            elif self.grid is not None:
                citem = _capi.GRID_CENTRE_DTYPE.itemsize
                self.ctx.radial_window_axes_centres(seq, first, count,
                                                    _capi._DeviceSpan(self.grid[1].data_ptr() + lo * citem, (hi - lo) * citem), out,
                                                    SMOOTH_RADIUS, self.cut_threshold, self.pov_mode, self.stream)
            elif self.weights is not None:
                self.ctx.radial_window_axes_weighted(seq, first, count, self._maps(lo + first), out, SMOOTH_RADIUS,
                                                     self.cut_threshold, self.pov_mode, self.stream)
            else:
                self.window(seq, first, count, out, SMOOTH_RADIUS, self.cut_threshold, self.pov_mode, self.stream)
            done = hi
        return done

    def _maps(self, j):
        """the maps of pairs j, j + 1, ... (a static map: itself)"""
        w = self.weights
        return _capi.DevWeights(w.base + j * w.item_stride, w.item_stride, w.row_pitch)

    def finish(self):
        """the records are complete for work queued on torch's current stream from here on"""
        if self.stream is not None:
            import torch
            torch.cuda.current_stream(self.ctx.device).wait_stream(self.stream)


def _pass2_mode(params):
    """params["hip_pass2"]: "device" runs the window, the cut test and pass 2 on the device with one read per chunk; any
    other value, or none, is the host schedule"""
    return params.get("hip_pass2") == "device"


def pair_plan(fps, total_frames, params):
    """The sampled frame indices of every chunk frames_to_actions processes for a video of total_frames frames
    (FF:1127-1153; pairs never span chunks): chunk k's pairs are (plan[k][i], plan[k][i + 1]).  A caller with its own flow
    estimator computes those pairs' fields and hands them to flows_to_actions."""
    from . import postchain
    _, _, indices = postchain.sampling(fps, total_frames)
    bracket = int(params.get("batch_size", 3000.0))
    return [indices[cs:cs + bracket] for cs in range(0, len(indices), bracket) if len(indices[cs:cs + bracket]) >= 2]


def script_axes(params):
    """params["hip_axes"], a dict from file suffix to component name (_capi.AXES), e.g. {"roll": "tangential", "sway":
    "shift_x"}: [(suffix, column)] for the further scripts of frames_to_scripts / flows_to_scripts.  The library fixes no
    mapping of its own -- which device axis a component drives is the caller's convention.  An empty suffix (the main
    script's) and an unknown component are refused."""
    out = []
    for suffix, comp in dict(params.get("hip_axes") or {}).items():
        if not isinstance(suffix, str) or not suffix:
            raise ValueError(f"hip_axes: {suffix!r} is not a file suffix (the main script is the entry without one)")
        if comp not in _capi.AXES:
            raise ValueError(f"hip_axes[{suffix!r}]: unknown component {comp!r}, one of {_capi.AXES}")
        out.append((suffix, _capi.AXES.index(comp)))
    return out


def _scripts_from_chunks(chunks, extra, fps, params):
    """{suffix: actions} out of the chunks' (frame indices, comps float64[n, 4], records): "" from component 0 and one
    entry per (suffix, column) of `extra`, each through the post-chain with the chunks' cuts"""
    from . import postchain
    cuts = [bool(r[4]) for _, _, recs in chunks for r in recs]
    frame_idx = [i for idx, _, _ in chunks for i in idx]
    comps = np.concatenate([np.asarray(c, np.float64).reshape(-1, len(_capi.AXES)) for _, c, _ in chunks] or
                           [np.zeros((0, len(_capi.AXES)))], axis=0)
    return {suffix: postchain.actions_from_scalars([float(v) for v in comps[:, col]], cuts, frame_idx, fps, params)
            for suffix, col in [("", 0)] + extra}


def static_weights(engine, params):
    """params["hip_weights"], an (H, W) uint8 / bool numpy array or torch tensor, as a device tensor on the engine's
    device: the static weight map of every pair; None without the key."""
    return _static_map(engine, params, "hip_weights")


def _static_map(engine, params, key):
    """params[key] as an (H, W) uint8 / bool device tensor on the engine's device; None without the key"""
    w = params.get(key)
    if w is None:
        return None
    import torch
    t = w if isinstance(w, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(w))
    if t.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"{key}: dtype {t.dtype} is not supported, weight maps are uint8 or bool")
    ctx = engine.ctx
    if tuple(t.shape) != (ctx.height, ctx.width):
        raise ValueError(f"{key}: shape {tuple(t.shape)} is not (H, W) = ({ctx.height}, {ctx.width})")
    return t.to(torch.device("cuda", ctx.device)).contiguous()


def consistency_kwargs(engine, params):
    """The keywords of process_chunk when params["hip_weights"] names a mode of MAP_MODES -- params["hip_consistency"] (a dict
    of _capi.ConsistencyParams fields) and params["hip_weights_gate"] (a static (H, W) map) go with it -- else {}; the two
    further keys are refused without it.  With "residual" the parameters are params["hip_residual"] (a dict of
    _capi.ResidualParams fields), with "texture" params["hip_texture"] (a dict of _capi.TextureParams fields); each mode refuses
    the others' parameters, but for params["hip_texture"] next to "residual" (a dict, or True for the defaults): the
    combination of the two maps."""
    mode = params.get("hip_weights")
    if not isinstance(mode, str):
        for key, needs in (("hip_consistency", "'consistency'"), ("hip_residual", "'residual'"),
                           ("hip_texture", "'texture' (or 'residual', for the combination of the two maps)"),
                           ("hip_weights_gate", "'consistency' or 'residual'")):
            if params.get(key) is not None:
                raise ValueError(f"{key} needs hip_weights = {needs}")
        return {}
    own = mode if mode in FRAME_MAP_MODES else "consistency"
    for other in ("consistency", "residual", "texture"):
        if other != own and (own, other) != ("residual", "texture") and params.get("hip_" + other) is not None:
            raise ValueError(f"hip_{other} needs hip_weights = {other!r}, got {mode!r}")
    kw = {"weights": mode, own: params.get("hip_" + own), "weights_gate": _static_map(engine, params, "hip_weights_gate")}
    if own == "residual" and params.get("hip_texture") is not None:
        kw["texture"] = params["hip_texture"]
    return kw


def center_kwargs(params):
    """{"center": ..., "cells": ...} when params names "hip_center" (params["hip_center_cells"], default 32, its grid), else
    {}: the keywords of process_chunk / process_flows.  Together with "hip_weights" it is refused.  "hip_center" = "track":
    {"center": "track", "track": params["hip_track"]} (see process_chunk)."""
    center = chunk_center(params.get("hip_center"))
    if center is None:
        if params.get("hip_track") is not None:
            raise ValueError("hip_track needs hip_center = 'track'")
        return {}
    if params.get("hip_weights") is not None:
        raise ValueError("hip_center together with hip_weights is not supported")
    if center == "track":   # params["hip_track"]: the track= dict of process_chunk / process_flows
        track = params.get("hip_track")
        if not isinstance(track, dict):
            raise ValueError("hip_center = 'track' needs hip_track, a dict such as {'start': (x, y), 'radius': 12, 'roi': (48, 48)}")
        unknown = [k for k in track if k not in TRACK_KEYS]
        if unknown:
            raise ValueError(f"hip_track: unknown key {unknown[0]!r} (one of {TRACK_KEYS})")
        return {"center": center, "track": dict(track)}
    if params.get("hip_track") is not None:
        raise ValueError("hip_track needs hip_center = 'track'")
    return {"center": center, "cells": int(params.get("hip_center_cells", 32))}


def _track_carry(engine, params):
    """{"track_carry": the video's track state} with params["hip_center"] = "track" and a "start" in params["hip_track"], else
    {}: pairs never span chunks, but the subject does, so one state tensor serves every chunk of a video (a "state" of the
    caller's does so by itself); with a "match" in it that names no "templates", also {"match_carry": the video's templates
    and whether the next chunk captures them}: the first chunk does, every later one reuses them"""
    cen = center_kwargs(params)
    if cen.get("center") != "track":
        return {}
    track, carry = cen["track"], {}
    if "start" in track:
        carry["track_carry"] = track_state(engine.ctx, track["start"], track.get("home"))
    m = track.get("match")
    state = carry.get("track_carry", track.get("state"))
    if isinstance(m, dict) and m.get("templates") is None and state is not None:
        # the templates are the video's too: captured in the first chunk (unless "capture" says otherwise), carried to the rest
        tracks = _capi._device_span(state)[1] // _capi.TRACK_STATE_DTYPE.itemsize
        p = _capi.match_choice({k: m[k] for k in _capi.MATCH_FIELDS if m.get(k) is not None}).p
        carry["match_carry"] = {"templates": match_templates(engine.ctx, tracks, p), "capture": bool(m.get("capture", True))}
    return carry


def _weighted_scalars(buf, axes):
    """(dots or comps, records) out of a weighted chunk's buffer of 80-byte records"""
    comps, recs = post_records(buf, axes=True)
    return (comps if axes else comps[:, 0]), recs


def _axes_kw(axes):
    """axes=True only where it is asked for: an engine without the keyword keeps serving the single script"""
    return {"axes": True} if axes else {}


def _flow_chunks(engine, chunk_flows, fps, total_frames, params, axes, who):
    plan = pair_plan(fps, total_frames, params)
    if isinstance(params.get("hip_weights"), str) and params["hip_weights"] == "residual":
        raise ValueError(f"{who}: hip_weights = 'residual' needs the frames, which caller flows do not have; "
                         "Context.residual_weights serves callers who hold the frames in the context's frame slots")
    if isinstance(params.get("hip_weights"), str) and params["hip_weights"] == "texture":
        raise ValueError(f"{who}: hip_weights = 'texture' needs the frames, which caller flows do not have; "
                         "Context.texture_weights serves callers who hold the frames in the context's frame slots")
    if isinstance(params.get("hip_weights"), str):
        raise ValueError(f"{who}: hip_weights = {params['hip_weights']!r} needs the backward fields, which caller flows do not "
                         "have; Context.consistency_weights serves callers with their own estimator")
    if len(chunk_flows) != len(plan):
        raise ValueError(f"{who}: {len(chunk_flows)} chunks of flows for a plan of {len(plan)} chunks")
    if isinstance(params.get("hip_track"), dict) and params["hip_track"].get("match") is not None:
        raise ValueError(f"{who}: hip_track['match'] needs the frames, which caller flows do not have; Context.track_match "
                         "serves callers who hold the frames in the context's frame slots")
    out, carry = [], _track_carry(engine, params)
    for chunk, flows in zip(plan, chunk_flows):
        d, recs = _chunk_scalars(engine, flows, params, axes, run=engine.process_flows, **carry)
        if len(d) != len(chunk) - 1:
            raise ValueError(f"{who}: a chunk of {len(chunk)} frames needs {len(chunk) - 1} fields, got {len(d)}")
        out.append((chunk[:-1], d, recs))
    return out


def flows_to_actions(engine, chunk_flows, fps, total_frames, params):
    """.funscript actions from flow fields the caller computed: chunk_flows[k] holds the len(plan[k]) - 1 pair fields of
    chunk k of pair_plan(fps, total_frames, params) in device memory (see PairEngine.process_flows).  Everything after
    the flow -- pass 1, the +-6 window, pass 2, the post-chain -- is frames_to_actions' own."""
    from . import postchain
    dots, cuts, frame_idx = [], [], []
    for idx, d, recs in _flow_chunks(engine, chunk_flows, fps, total_frames, params, False, "flows_to_actions"):
        dots += [float(v) for v in d]
        cuts += [bool(r[4]) for r in recs]
        frame_idx += idx
    return postchain.actions_from_scalars(dots, cuts, frame_idx, fps, params)


def flows_to_scripts(engine, chunk_flows, fps, total_frames, params):
    """flows_to_actions for multi-axis scripts: {suffix: actions}, "" being flows_to_actions' own script (component 0) and
    one further entry per item of params["hip_axes"] (script_axes)."""
    extra = script_axes(params)
    return _scripts_from_chunks(_flow_chunks(engine, chunk_flows, fps, total_frames, params, True, "flows_to_scripts"), extra,
                                fps, params)


def _chunk_scalars(engine, items, params, axes=False, run=None, **kw):
    """(dots, records) of one chunk under params: `run` -- engine.process_chunk (the default; items: the chunk's frames) or
    engine.process_flows (its flow fields) -- or, with params["hip_pass2"] = "device", its device pass 2 with one buffer and
    one read for the chunk; axes=True: (comps float64[n, 4], records).  kw: further keywords of `run`."""
    run = run or engine.process_chunk
    pov, thr = bool(params.get("pov_mode", False)), float(params.get("cut_threshold", 7))
    kw.update(compensate_kwargs(params))   # params["hip_compensate"]: the fit and the subtraction behind every batch
    carry = kw.pop("track_carry", None)    # the video's track state, carried from chunk to chunk (_track_carry)
    cen = center_kwargs(params)
    mcarry = kw.pop("match_carry", None)   # the video's templates, likewise: the first chunk captures them
    if carry is not None:
        cen["track"] = {**{k: v for k, v in cen["track"].items() if k not in ("start", "home")}, "state": carry}
    if mcarry is not None:
        cen["track"] = {**cen["track"], "match": {**cen["track"]["match"], **mcarry}}
        mcarry["capture"] = False
    if cen:   # params["hip_center"]: the device schedule about that centre
        return _weighted_scalars(run(items, pov, thr, **cen, **kw), axes)
    ckw = consistency_kwargs(engine, params)
    if ckw:   # params["hip_weights"] = "consistency" / "residual": the device schedule under maps made from the chunk's own flow
        return _weighted_scalars(run(items, pov, thr, **ckw, **kw), axes)
    wts = static_weights(engine, params)
    if wts is not None:   # params["hip_weights"]: the device schedule under the static map
        return _weighted_scalars(run(items, pov, thr, weights=wts, **kw), axes)
    kw.update(_axes_kw(axes))
    if not _pass2_mode(params):
        return run(items, pov, thr, **kw)
    return post_records(run(items, pov, thr, post_out=True, **kw), **_axes_kw(axes))


def _frame_chunks(engine, frames, fps, params, axes):
    """[(frame indices, dots or comps, records)] of every chunk of pair_plan under params"""
    # params["hip_flow"] / ["hip_dis"] pick the flow algorithm for this call (the engine itself is left as it is); without
    # them the engine's own algorithm runs
    algo = _capi.flow_choice(params) if ("hip_flow" in params or "hip_dis" in params) else None
    # params["hip_farneback"] / ["hip_farneback_window"] likewise set the Farneback parameters and window of this call
    fbk = farneback_kwargs(params, frames[0].shape[1], frames[0].shape[0]) if len(frames) else {}
    out, carry = [], _track_carry(engine, params)
    for chunk in pair_plan(fps, len(frames), params):
        d, recs = _chunk_scalars(engine, [frames[i] for i in chunk], params, axes, **({"algo": algo} if algo is not None else {}),
                                 **fbk, **carry)
        out.append((chunk[:-1], d, recs))
    return out


def frames_to_actions(engine, frames, fps, params):
    """Gray (or BGR) frames of one video -> .funscript actions: the `process_video` body from frame
    sampling to keyframes (FF:1127-1385) with the HIP pair engine in the middle.  `frames` holds every
    decoded frame (any sequence); chunking follows FF:1145-1153 (pairs never span chunks, F10)."""
    from . import postchain
    dots, cuts, frame_idx = [], [], []
    for idx, d, recs in _frame_chunks(engine, frames, fps, params, False):
        dots += [float(v) for v in d]
        cuts += [bool(r[4]) for r in recs]
        frame_idx += idx
    return postchain.actions_from_scalars(dots, cuts, frame_idx, fps, params)


def frames_to_scripts(engine, frames, fps, params):
    """frames_to_actions for multi-axis scripts: {suffix: actions}.  "" is the main script, from
    component 0 -- action for action what frames_to_actions returns -- and every item of params["hip_axes"] (script_axes)
    adds one from its component, through the same post-chain with the same cuts.  postchain.write_funscripts writes them
    as base.funscript and base.<suffix>.funscript.  params["hip_pass2"] = "device" works as for the single script."""
    extra = script_axes(params)
    return _scripts_from_chunks(_frame_chunks(engine, frames, fps, params, True), extra, fps, params)


def _shard_pass1(engine, frames, mine, pov_mode, cut_threshold):
    recs = engine.pass1(frames, mine, pov_mode, cut_threshold) if len(mine) else []
    return np.array([[j, r[0], r[1], int(r[4])] for j, r in zip(mine, recs)], np.int64).reshape(-1, 4)


def _merge_records(parts, n):
    """every rank's (pair index, x, y, cut) rows -> (n, 3) array in pair order"""
    rows = np.concatenate([np.asarray(a, np.int64).reshape(-1, 4) for a in parts], axis=0)
    assert len(rows) == n and np.array_equal(np.sort(rows[:, 0]), np.arange(n)), "pairs lost or duplicated in the shard"
    allrecs = np.empty((n, 3), np.int64)
    allrecs[rows[:, 0]] = rows[:, 1:]
    return allrecs


def _shard_pass2(engine, mine, centers, allrecs, pov_mode):
    if not len(mine):
        return np.zeros((0, 2))
    local = engine.radial(list(range(len(mine))), centers[mine], allrecs[mine, 2].astype(bool), pov_mode)
    return np.stack([np.asarray(mine, np.float64), np.asarray(local, np.float64)], axis=1)


def _merge_dots(parts, n):
    rows = np.concatenate([np.asarray(p, np.float64).reshape(-1, 2) for p in parts], axis=0)
    dots = np.empty(n, np.float64)
    dots[rows[:, 0].astype(np.int64)] = rows[:, 1]
    return dots


def _no_sharded_axes(axes, who):
    if axes:
        raise ValueError(f"{who}: the sharded schedules compute the radial component alone; axes=True needs "
                         "PairEngine.process_chunk / process_flows on one device")


def process_chunk_sharded(engine, frames, rank, world, allgather, pov_mode=False, cut_threshold=7.0,
                          assign="contiguous", block=1, axes=False, center=None, weights=None, compensate=None):
    """Multi-GPU form of one chunk: rank r owns the pairs shard_pairs(n, world, r, assign, block).

    `engine` provides pass1(frames, pair_indices, pov_mode, cut_threshold) -> records (its l-th listed pair is
    local index l) and radial(local_indices, centers, cuts, pov_mode) -> floats on its own device;
    `allgather(obj)` returns the list of every rank's object (a host gather of ~32 B per pair: pair index, x, y,
    cut -- the only exchange).  Centres are smoothed over the WHOLE chunk (FF:1203-1214 needs pairs j+-6, which
    cross shard edges under either assignment).  Returns the full dots array and the (n, 3) records on every rank.
    axes=True is refused: the sharded schedules keep the single component."""
    _no_sharded_axes(axes, "process_chunk_sharded")
    _no_sharded_center(center, "process_chunk_sharded")
    _no_sharded_weights(weights, "process_chunk_sharded")
    _no_sharded_compensate(compensate, "process_chunk_sharded")
    n = len(frames) - 1
    mine = shard_pairs(n, world, rank, assign, block)
    allrecs = _merge_records(allgather(_shard_pass1(engine, frames, mine, pov_mode, cut_threshold)), n)
    centers = smooth_centers(allrecs[:, :2])
    return _merge_dots(allgather(_shard_pass2(engine, mine, centers, allrecs, pov_mode)), n), allrecs


def halo_rows(rows, radius=SMOOTH_RADIUS):
    """The part of a contiguous shard's pass-1 rows (pair index, x, y, cut; ascending) another rank can ever need: its
    first and last `radius` pairs.  A pair within `radius` of a foreign block lies within the first / last `radius` pairs
    of its own block, however short the blocks in between are."""
    rows = np.asarray(rows, np.int64).reshape(-1, 4)
    return rows if len(rows) <= 2 * radius else np.concatenate([rows[:radius], rows[-radius:]], axis=0)


def process_chunk_sharded_halo(engine, frames, rank, world, allgather, pov_mode=False, cut_threshold=7.0, axes=False,
                               center=None, weights=None, compensate=None):
    """Streaming multi-GPU form of one chunk for CONTIGUOUS blocks: the only exchange between the passes is the halo.

    process_chunk_sharded gathers every pass-1 record of the chunk before any pass 2 starts, so all ranks idle until the
    slowest has finished pass 1.  FF:1203-1214 only needs pairs j-6..j+6: with contiguous blocks a rank's interior pairs
    (window inside its own block, or clipped by the chunk's ends) depend on nobody else, and its <= 12 edge pairs on the
    neighbouring blocks' first / last 6 records ("block edges need a 6-pair halo of pass-1 scalars only").
    Schedule per rank:
        pass 1 over its block in batches; after every batch, pass 2 for all its pairs whose window is already known
        (runs on the device beside the next batch's pass 1, exactly as PairEngine.process_chunk does on one GPU);
        ONE all-gather of <= 12 halo rows (32 B each) per rank;
        pass 2 for the remaining edge pairs;
        ONE all-gather of the results (pair index, scalar, x, y, cut) -- the output, not a barrier between the passes.
    `engine.pass1` is called with on_batch= when it accepts one (HipShardEngine does); an engine without it still gives
    the same numbers, only without the overlap.  Window means are exact integer sums / counts, so the result is
    bit-identical to process_chunk_sharded's and to a single-GPU process_chunk.  Returns (dots, (n, 3) records) on every
    rank.  axes=True is refused, as in process_chunk_sharded."""
    _no_sharded_axes(axes, "process_chunk_sharded_halo")
    _no_sharded_center(center, "process_chunk_sharded_halo")
    _no_sharded_weights(weights, "process_chunk_sharded_halo")
    _no_sharded_compensate(compensate, "process_chunk_sharded_halo")
    n = len(frames) - 1
    R = SMOOTH_RADIUS
    lo, hi = shard_range(n, world, rank)
    mine = np.arange(lo, hi)
    pos = np.zeros((n, 2), np.int64)
    cuts = np.zeros(n, bool)
    known = np.zeros(n, bool)
    dots = np.zeros(hi - lo, np.float64)
    todo = list(range(lo, hi))                     # own pairs still waiting for pass 2, ascending

    def flush(final=False):
        ready, rest = [], []
        for j in todo:
            w0, w1 = max(0, j - R), min(n, j + R + 1)
            (ready if known[w0:w1].all() else rest).append(j)
        if final and rest:
            raise RuntimeError(f"rank {rank}: halo exchange left pairs {rest[:4]} without their +-{R} window")
        todo[:] = rest
        if ready:
            js = np.asarray(ready)
            w0, w1 = np.maximum(0, js - R), np.minimum(n, js + R + 1)
            psum = np.zeros((n + 1, 2), np.int64)
            psum[1:] = np.cumsum(pos, axis=0)
            centers = (psum[w1] - psum[w0]) / (w1 - w0)[:, None]
            dots[js - lo] = engine.radial(list(js - lo), centers, cuts[js], pov_mode)

    def take(js, got):
        js = np.asarray(js, np.int64)
        pos[js] = [(r[0], r[1]) for r in got]
        cuts[js] = [bool(r[4]) for r in got]
        known[js] = True

    def on_batch(ls, js, got):
        take(js, got)
        flush()

    if len(mine):
        import inspect
        if "on_batch" in inspect.signature(engine.pass1).parameters:
            recs = engine.pass1(frames, mine, pov_mode, cut_threshold, on_batch=on_batch)
        else:                                      # an engine without the streaming hook: same numbers, no overlap
            recs = engine.pass1(frames, mine, pov_mode, cut_threshold)
        take(mine, recs)
    own = np.concatenate([mine[:, None], pos[lo:hi], cuts[lo:hi, None].astype(np.int64)], axis=1) if len(mine) else np.zeros((0, 4), np.int64)
    for part in allgather(halo_rows(own)):         # the only exchange between pass 1 and pass 2
        part = np.asarray(part, np.int64).reshape(-1, 4)
        if len(part):
            pos[part[:, 0]] = part[:, 1:3]
            cuts[part[:, 0]] = part[:, 3].astype(bool)
            known[part[:, 0]] = True
    flush(final=True)
    out = np.concatenate([own.astype(np.float64), dots[:, None]], axis=1)          # (j, x, y, cut, dot)
    rows = np.concatenate([np.asarray(p, np.float64).reshape(-1, 5) for p in allgather(out)], axis=0)
    idx = rows[:, 0].astype(np.int64)
    assert len(rows) == n and np.array_equal(np.sort(idx), np.arange(n)), "pairs lost or duplicated in the shard"
    all_dots = np.empty(n, np.float64)
    allrecs = np.empty((n, 3), np.int64)
    all_dots[idx] = rows[:, 4]
    allrecs[idx] = rows[:, 1:4].astype(np.int64)
    return all_dots, allrecs


def process_chunk_local_ranks(engines, frames, pov_mode=False, cut_threshold=7.0, assign="contiguous", block=1, axes=False,
                              center=None, weights=None, compensate=None):
    """The same schedule with every rank driven from THIS process (one engine / context per device, or several
    contexts on one device): phase by phase, no process group.  Equivalent to world = len(engines) processes
    running process_chunk_sharded (axes=True is refused there and here)."""
    _no_sharded_axes(axes, "process_chunk_local_ranks")
    _no_sharded_center(center, "process_chunk_local_ranks")
    _no_sharded_weights(weights, "process_chunk_local_ranks")
    _no_sharded_compensate(compensate, "process_chunk_local_ranks")
    n, world = len(frames) - 1, len(engines)
    mine = [shard_pairs(n, world, r, assign, block) for r in range(world)]
    allrecs = _merge_records([_shard_pass1(e, frames, m, pov_mode, cut_threshold) for e, m in zip(engines, mine)], n)
    centers = smooth_centers(allrecs[:, :2])
    return _merge_dots([_shard_pass2(e, m, centers, allrecs, pov_mode) for e, m in zip(engines, mine)], n), allrecs


class HipShardEngine:
    """engine for process_chunk_sharded on one device: keeps the shard's flows resident (local pair l in flow
    slot l), so the context needs flow_slots >= the shard's pair count and frame_slots >= 2B + 2."""

    def __init__(self, ctx, upload=None):
        self.ctx = ctx
        B = ctx.max_batch
        if ctx.frame_slots < 2 * B + 2:
            # two frames of one batch in the same slot would silently compute the wrong flow
            raise ValueError(f"context too small for a shard engine: need frame_slots >= 2B+2 = {2 * B + 2}")
        self.inner = PairEngine.__new__(PairEngine)  # a shard's flow slots are bounded by its size, checked in pass1
        self.inner.ctx, self.inner.B, self.inner.upload = ctx, B, upload or ctx.upload_frames

    def pass1(self, frames, pair_indices, pov_mode, cut_threshold, on_batch=None):
        """on_batch(local_indices, pair_indices, records) after every finished batch (process_chunk_sharded_halo issues the
        pass 2 of pairs whose window is complete from it, beside the next batch's kernels)."""
        if len(pair_indices) > self.ctx.flow_slots:
            raise ValueError(f"shard of {len(pair_indices)} pairs does not fit the context's {self.ctx.flow_slots} flow slots")
        return self.inner.pass1_pairs(frames, pair_indices, lambda l: l, pov_mode, cut_threshold, on_batch=on_batch)

    def radial(self, local_indices, centers, cuts, pov_mode, axes=False):
        _no_sharded_axes(axes, "HipShardEngine.radial")
        out, B = [], self.ctx.max_batch
        for s in range(0, len(local_indices), B):
            sl = slice(s, s + B)
            out += self.ctx.radial(list(local_indices[sl]), list(centers[sl]), list(cuts[sl]), pov_mode)
        return out
