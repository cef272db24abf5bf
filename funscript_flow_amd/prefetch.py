"""Host-side decode / prefetch path of the HIP backend: the counterpart of

    AsyncVideoReader            FF:103-291   (<= 4 cv2.VideoCapture decoders, one SEEK per frame FF:173-189)
    fetch_frames_optimized      FF:1051-1091 (sub-batches of 50 frames, host resize + gray conversion)
    the chunk prefetch thread   FF:1156-1185 (one whole chunk of gray frames ahead, Queue(maxsize=1))

re-designed for a consumer that is ~100x faster than the reference's pool:

  * ONE capture, read strictly sequentially (grab() for the frames the 30-fps sampling skips, FF:1127-1129): no
    per-frame seeks, no decoder pool to keep in step;
  * decoded frames land directly in a ring of page-locked frames owned by the device context
    (Context.pinned_frames -> ffl_host_alloc): the H2D transfer reads them in place, resize / crop / gray happen
    on the device (frontend.DecodedUploader -> k_frontend), so the host never touches a pixel after the decoder;
  * back-pressure instead of whole-chunk buffering: the decoder thread blocks when the ring is full, the consumer
    releases a slot once the batch that uploaded it has returned its results -- memory is ring_frames decoded
    frames, not a chunk of 3000 (the reference's queue can also hand a stale chunk to a later iteration when a
    prefetch thread outlives its chunk, FF:1156-1185; there is no such queue here);
  * chunking as the reference does it: chunk c = indices[c*bracket : (c+1)*bracket], pairs never span chunks
    (FF:1145-1153, F10), chunks shorter than 2 frames are skipped.

Codec work itself stays with whatever `capture` is (cv2.VideoCapture in production); this module only needs its
read() / grab() / get() / release() methods, which is what the tests' fake capture provides.
"""
import threading

import numpy as np

from . import _capi, postchain

CAP_PROP_FRAME_COUNT, CAP_PROP_FPS, CAP_PROP_FRAME_WIDTH, CAP_PROP_FRAME_HEIGHT = 7, 5, 3, 4  # cv2.CAP_PROP_*


class DecodeError(RuntimeError):
    pass


class SequentialDecoder:
    """Decodes the frames `indices` (ascending) of `capture` in order, without seeking: frames between two wanted
    indices are skipped with grab() (demux + decode, no colour conversion / copy)."""

    def __init__(self, capture, indices):
        self.cap, self.indices = capture, list(indices)
        if any(b <= a for a, b in zip(self.indices, self.indices[1:])):
            raise ValueError("frame indices must be strictly ascending")
        self.pos = 0      # index of the frame the next read() / grab() returns
        self.k = 0        # next entry of `indices`

    def __len__(self):
        return len(self.indices)

    def read_into(self, dst):
        """Decode the next wanted frame into `dst` ((h, w, 3) uint8, or (3h/2, w) 4:2:0 of uint8 / uint16); returns its frame index, or None at
        the end."""
        if self.k >= len(self.indices):
            return None
        want = self.indices[self.k]
        while self.pos < want:
            if not self.cap.grab():
                raise DecodeError(f"capture ended at frame {self.pos}, frame {want} wanted")
            self.pos += 1
        try:
            ok, frame = self.cap.read(dst)            # cv2 decodes straight into a matching array
        except TypeError:
            ok, frame = self.cap.read()
        if not ok or frame is None:
            raise DecodeError(f"capture could not read frame {want}")
        if frame is not dst:
            if frame.shape != dst.shape:
                raise DecodeError(f"frame {want} is {frame.shape}, ring slots are {dst.shape}")
            np.copyto(dst, frame)
        self.pos += 1
        self.k += 1
        return want


class _ChunkView:
    """What PairEngine sees of one chunk: a sequence whose items appear as the decoder delivers them.  Item i of the
    chunk is frame `first + i` of the stream; release(n) tells the ring that items < n have left the host."""

    def __init__(self, ring, first, length):
        self.ring, self.first, self.length = ring, first, length

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        if isinstance(i, slice):
            raise TypeError("chunk views are indexed frame by frame")
        if i < 0:
            i += self.length
        if not 0 <= i < self.length:
            raise IndexError(i)
        return self.ring._wait_frame(self.first + i)

    def release(self, n_items):
        self.ring._release(self.first + min(n_items, self.length))


class PrefetchRing:
    """A decoder thread filling a ring of page-locked decoded frames, consumed chunk by chunk.

        ring = PrefetchRing(ctx, capture, indices, bracket, ring_frames=4 * B + 2)
        for view, frame_indices in ring.chunks():
            dots, recs = engine.process_chunk(view, ...)      # engine built with frontend.DecodedUploader(ctx)
        ring.close()

    `ctx` provides pinned_frames(n, channels=3, size=(w, h)) (a real Context, or anything with that method).
    ring_frames must cover what the engine keeps in flight: two batches + the one being staged = 3 * B + 1.
    yuv="i420" | "nv12": the capture's read() yields (3h/2, w) 4:2:0 frames (w, h still from CAP_PROP_FRAME_*), and the
    slots come from pinned_frames(n, size=(w, h), yuv=True); consume them with frontend.DecodedUploader(ctx, yuv=...).
    depth=9..16 beside yuv: read() yields uint16 frames, and the slots come from pinned_frames(..., yuv=True, depth=depth)
    -- the keyword is passed only then."""

    def __init__(self, ctx, capture, indices, bracket, ring_frames, frame_size=None, yuv=None, depth=8):
        self.decoder = SequentialDecoder(capture, indices)
        if frame_size is None:
            frame_size = (int(capture.get(CAP_PROP_FRAME_WIDTH)), int(capture.get(CAP_PROP_FRAME_HEIGHT)))
        self.bracket, self.n = int(bracket), len(self.decoder)
        if self.bracket < 2:
            raise ValueError("bracket (frames per chunk) must be >= 2")
        self.ring_frames = int(ring_frames)
        if yuv is None:
            if depth != 8:
                raise ValueError("depth describes 4:2:0 frames: it needs yuv=\"i420\" | \"nv12\"")
            self.slots = ctx.pinned_frames(self.ring_frames, channels=3, size=frame_size)
        else:
            _capi.yuv_layout(yuv)
            depth, _ = _capi.yuv_depth(depth)
            if frame_size[0] % 2 or frame_size[1] % 2:
                raise ValueError(f"4:2:0 frames need an even width and height, the capture reports {frame_size}")
            self.slots = ctx.pinned_frames(self.ring_frames, size=frame_size, yuv=True, **({"depth": depth} if depth != 8 else {}))
        self.cv = threading.Condition()
        self.decoded = 0       # stream positions [0, decoded) have been decoded (position = rank in `indices`)
        self.released = 0      # positions [0, released) may be overwritten
        self.error = None
        self.stop = False
        self.max_outstanding = 0
        self.thread = threading.Thread(target=self._run, name="ffl-decode", daemon=True)
        self.thread.start()

    # ---- decoder thread ------------------------------------------------------------------------------------
    def _run(self):
        try:
            while True:
                with self.cv:
                    while not self.stop and self.decoded - self.released >= self.ring_frames:
                        self.cv.wait()                      # back-pressure: every slot holds an unreleased frame
                    if self.stop or self.decoded >= self.n:
                        return
                    pos = self.decoded
                if self.decoder.read_into(self.slots[pos % self.ring_frames]) is None:
                    return
                with self.cv:
                    self.decoded = pos + 1
                    self.max_outstanding = max(self.max_outstanding, self.decoded - self.released)
                    self.cv.notify_all()
        except Exception as e:  # noqa: BLE001 -- handed to the consumer, which re-raises it
            with self.cv:
                self.error = e
                self.cv.notify_all()

    # ---- consumer side -------------------------------------------------------------------------------------
    def _wait_frame(self, pos):
        with self.cv:
            if pos < self.released:
                raise DecodeError(f"frame at stream position {pos} was already released (ring of {self.ring_frames})")
            if pos >= self.released + self.ring_frames:
                raise DecodeError(f"stream position {pos} is {pos - self.released} frames ahead of the oldest unreleased "
                                  f"one: the ring of {self.ring_frames} frames is too small for this consumer")
            while self.decoded <= pos and self.error is None:
                self.cv.wait()
            if self.decoded <= pos:
                raise DecodeError(f"decoder failed before stream position {pos}") from self.error
        return self.slots[pos % self.ring_frames]

    def _release(self, upto):
        with self.cv:
            if upto > self.released:
                self.released = upto
                self.cv.notify_all()

    def chunks(self):
        """Yields (chunk view, frame indices of the chunk's pairs = chunk[:-1]) per chunk with >= 2 frames, in stream
        order; a chunk's slots are released when the next one is requested."""
        idx = self.decoder.indices
        for s in range(0, self.n, self.bracket):
            length = min(self.bracket, self.n - s)
            if length < 2:
                self._release(s + length)
                continue
            yield _ChunkView(self, s, length), idx[s:s + length - 1]
            self._release(s + length)

    def close(self):
        with self.cv:
            self.stop = True
            self.cv.notify_all()
        self.thread.join()


def yuv_params(params):
    """(params["hip_yuv"], the depth and stream-metadata keywords of frontend.DecodedUploader): params["hip_yuv_depth"],
    the optional params["hip_yuv_msb"] and the stream's params["hip_rotate"] (0, 90, 180, 270), params["hip_mirror"] and
    params["hip_yuv_range"] ("limited" | "full"; DESIGN.md appendix Y, rules Y6 and Y7) travel only when they are set,
    so that without them nothing changes.  Nothing is read from the capture: the caller knows what its decoder delivers
    (PyAV / ffprobe report the rotation and range; a cv2.VideoCapture BGR frame is upright already).  The pinned ring stays
    sized by the stored frame."""
    deep = {}
    if params.get("hip_rotate") is not None:
        deep["rotate"] = int(params["hip_rotate"])
    if params.get("hip_mirror") is not None:
        deep["mirror"] = bool(params["hip_mirror"])
    if params.get("hip_yuv_range") is not None:
        deep["yuv_range"] = params["hip_yuv_range"]
    if params.get("hip_yuv_depth") is not None:
        deep["depth"] = int(params["hip_yuv_depth"])
    if params.get("hip_yuv_msb") is not None:
        deep["msb"] = bool(params["hip_yuv_msb"])
    return params.get("hip_yuv"), deep


VIEW_KEYS = ("projection", "fov", "yaw", "pitch", "roll", "stereo", "eye", "src_hfov", "src_vfov", "supersample")


def view_remap(ctx, capture, params):
    """params["hip_view"] -> the keyword of frontend.DecodedUploader that carries it ({} without the key, so that nothing
    changes): a dict with "projection" ("equirect" | "fisheye") and "fov" (degrees) and, optionally, "yaw", "pitch", "roll",
    "stereo" (None | "sbs" | "tb"), "eye" ("left" | "right"), "src_hfov", "src_vfov", "supersample" -- the pinhole view of
    frontend.view_map into one eye of the stream.  The map is built once, for the capture's stored
    size turned upright by params["hip_rotate"], and made resident in `ctx`, which is the caller's: whoever calls this
    destroys the map once the video is done (drop_remap), or a context reused over many videos runs out of maps.  Refused
    together with params["vr_mode"], which answers the same question by a crop (FF:1076-1079).  The values are the
    caller's: none is tuned on footage."""
    view = params.get("hip_view")
    if view is None:
        return {}
    from . import frontend
    if params.get("vr_mode"):
        raise ValueError("params[\"hip_view\"] and params[\"vr_mode\"] are two answers to one question: the view replaces the "
                         "reference's resize and quadrant crop (FF:1076-1079) -- set one of them")
    unknown = sorted(set(view) - set(VIEW_KEYS))
    if unknown or "projection" not in view or "fov" not in view:
        raise ValueError(f"params[\"hip_view\"] needs \"projection\" and \"fov\" and knows {VIEW_KEYS}; got {sorted(view)}")
    w, h = int(capture.get(CAP_PROP_FRAME_WIDTH)), int(capture.get(CAP_PROP_FRAME_HEIGHT))
    src = (h, w) if int(params.get("hip_rotate") or 0) in (90, 270) else (w, h)   # the map is in upright terms
    S = int(view.get("supersample", 1))
    kw = {k: view[k] for k in ("yaw", "pitch", "roll", "src_hfov", "src_vfov") if view.get(k) is not None}
    m = frontend.view_map(src, (ctx.width, ctx.height), view["projection"], view["fov"], supersample=S,
                          rect=frontend.eye_rect(src, view.get("stereo"), view.get("eye", "left")), **kw)
    return {"remap": ctx.remap_create(m, src, S)}


def drop_remap(ctx, view):
    """frees the map view_remap created (`view`: what it returned); safe straight after the last upload that used it"""
    if view.get("remap") is not None:
        ctx.remap_destroy(view["remap"])


def ring_depth(deep):
    """the depth keyword of PrefetchRing out of yuv_params' keywords: only when the frames are not uint8"""
    return {"depth": deep["depth"]} if deep.get("depth", 8) != 8 else {}


def video_to_actions(ctx, capture, params, engine=None, ring_frames=None):
    """process_video's body from frame sampling to the action list (FF:1119-1385) on the HIP path, decoding
    included: sequential reads into the pinned ring, device front-end, two-pass pair engine, host post-chain."""
    from . import frontend, pipeline
    total, fps = int(capture.get(CAP_PROP_FRAME_COUNT)), float(capture.get(CAP_PROP_FPS))
    _, _, indices = postchain.sampling(fps, total)
    bracket = int(params.get("batch_size", 3000.0))
    # params["hip_yuv"] = "i420" | "nv12": the capture yields 4:2:0 frames; a caller's engine must
    # then have been built with frontend.DecodedUploader(ctx, yuv=...).  params["hip_yuv_depth"] = 9..16 and the optional
    # params["hip_yuv_msb"]: those frames are uint16 (rule Y5)
    # params["hip_view"]: a pinhole view through a source map instead of resize + crop (view_remap); a caller's engine is
    # left as it is
    yuv, deep = yuv_params(params)
    view = view_remap(ctx, capture, params) if engine is None else {}   # this call's own map: freed below
    engine = engine or pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, bool(params.get("vr_mode")), False, yuv=yuv, **deep,
                                                                         **view))
    # params["hip_flow"] / ["hip_dis"] pick the flow algorithm for this call (a caller's engine is left as it is)
    algo = _capi.flow_choice(params) if ("hip_flow" in params or "hip_dis" in params) else None
    fbk = pipeline.farneback_kwargs(params, ctx.width, ctx.height)   # params["hip_farneback"], ["hip_farneback_window"]: this call's
    dots, cuts, frame_idx = [], [], []
    ring = None
    try:
        ring = PrefetchRing(ctx, capture, indices, bracket, ring_frames or 4 * ctx.max_batch + 2, yuv=yuv, **ring_depth(deep))
        for chunk, fidx in ring.chunks():
            # params["hip_pass2"] = "device": the chunk's window, cut test and pass 2 on the device, one read per chunk
            d, recs = pipeline._chunk_scalars(engine, chunk, params, **({"algo": algo} if algo is not None else {}), **fbk)
            dots += [float(v) for v in d]
            cuts += [bool(r[4]) for r in recs]
            frame_idx += fidx
    finally:
        if ring is not None:
            ring.close()
        drop_remap(ctx, view)
    return postchain.actions_from_scalars(dots, cuts, frame_idx, fps, params)


def process_video(video_path, params, log_func, open_capture, make_context, progress_callback=None, cancel_flag=None):
    """The call shape and outcomes of the reference's process_video (FF:1094-1404) on the HIP path: returns
    `error_occurred`, writes `<video>.funscript` next to the video, never lets an exception escape (errors are logged as
    "ERROR: ..." and reported through the return value, FF:1115-1117, FF:1396-1398), skips existing outputs unless
    params["overwrite"] (FF:1107-1109).  The two things the reference hard-wires are arguments here:
        open_capture(video_path) -> a cv2.VideoCapture-like object (FF:1114 opens one through VideoReaderCV)
        make_context(capture)    -> the device Context for the operand size (256x256 in the reference, FF:1057)
    cancel_flag() is polled per chunk like FF:1146."""
    import os
    import time
    start = time.time()
    base, _ = os.path.splitext(video_path)
    output_path = base + ".funscript"
    if os.path.exists(output_path) and not params.get("overwrite", False):
        log_func(f"Skipping: output file exists ({output_path})")
        return False
    try:
        log_func(f"Processing video: {video_path}")
        cap = open_capture(video_path)
        if hasattr(cap, "isOpened") and not cap.isOpened():
            raise DecodeError("capture did not open")
    except Exception as e:  # noqa: BLE001
        log_func(f"ERROR: Unable to open video at {video_path}: {e}")
        return True
    try:
        total, fps = int(cap.get(CAP_PROP_FRAME_COUNT)), float(cap.get(CAP_PROP_FPS))
        if total < 1 or fps <= 0:
            raise DecodeError(f"{total} frames at {fps} fps")
    except Exception as e:  # noqa: BLE001
        log_func(f"ERROR: Unable to read video properties: {e}")
        return True
    from . import frontend, pipeline
    step, effective_fps, indices = postchain.sampling(fps, total)
    log_func(f"FPS: {fps:.2f}; downsampled to ~{effective_fps:.2f} fps; {len(indices)} frames selected.")
    log_func("Using backend: HIP")
    error_occurred = False
    ctx = ring = None
    own = {}   # the map this call creates in the caller's context (view_remap)
    try:
        ctx = make_context(cap)
        flow, dis = _capi.flow_choice(params)
        yuv, deep = yuv_params(params)   # "i420" | "nv12": open_capture's read() yields (3h/2, w) 4:2:0 frames
        own = view_remap(ctx, cap, params)   # this video's map: freed below
        engine = pipeline.PairEngine(ctx, frontend.DecodedUploader(ctx, bool(params.get("vr_mode")), False, yuv=yuv, **deep, **own),
                                     flow=flow, dis=dis, farneback=_capi.farneback_choice(params),
                                     window=_capi.farneback_mode(params))
        ring = PrefetchRing(ctx, cap, indices, int(params.get("batch_size", 3000.0)), 4 * ctx.max_batch + 2, yuv=yuv,
                            **ring_depth(deep))
        dots, cuts, frame_idx, done = [], [], [], 0
        for view, fidx in ring.chunks():
            if cancel_flag and cancel_flag():
                log_func("User bailed.")
                return error_occurred
            d, recs = engine.process_chunk(view, bool(params.get("pov_mode", False)), float(params.get("cut_threshold", 7)))
            dots += [float(v) for v in d]
            cuts += [bool(r[4]) for r in recs]
            frame_idx += fidx
            done += len(view)
            if progress_callback:
                progress_callback(min(100, int(100 * done / max(len(indices), 1))))
        actions = postchain.actions_from_scalars(dots, cuts, frame_idx, fps, params)
        log_func(f"Keyframe reduction: {len(actions)} actions computed.")
        postchain.write_funscript(output_path, actions)
        log_func(f"Funscript saved: {output_path}")
    except Exception as e:  # noqa: BLE001
        log_func(f"ERROR: {e}")
        error_occurred = True
    finally:
        if ring is not None:
            ring.close()
        try:
            drop_remap(ctx, own)
        except Exception as e:  # noqa: BLE001
            log_func(f"ERROR: {e}")
            error_occurred = True
        if hasattr(cap, "release"):
            cap.release()
    log_func(f"Processing time: {time.time() - start:.2f} seconds")
    return error_occurred
