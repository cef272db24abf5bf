"""GPU tests of general Farneback's two modes (ffl_flow_pairs_farneback_ex): the Gaussian
window (k_fbg_gauss_solve) and the initial flow (k_fbg_flow_area).  Every flow is bit-identical to the restatement
(tests/fb_flags_ref: the stages of tests/fb_general_ref composed with the two new ones); the pass-1 argmax is exact in
position and bits, the mean magnitude and both radial scalars within the derived bounds of tests/post_ref.py.  The lists are
iterated as they stand.  Parity with cv2 itself is unpinned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import torch   # before the first context: the float16 seeds reach the device through it

import fb_flags_ref as ffr
import fb_general_ref as fbr
import param_domain as pd
import post_ref as pr
from funscript_flow_amd import _capi

GAUSS_SIZES = [(16, 16), (17, 19), (65, 17), (64, 33), (130, 66), (20, 300), (300, 20), (63, 65), (257, 255)]
GAUSS_PARAMS = [
    ("winsize3", {"winsize": 3}), ("winsize5", {"winsize": 5}), ("winsize15", {"winsize": 15}),
    ("winsize33", {"winsize": 33}), ("winsize63", {"winsize": 63}),
    ("winsize63_polyn7", {"winsize": 63, "poly_n": 7}),
    ("iters1", {"iterations": 1}), ("iters10", {"iterations": 10}),
    ("pyr08_levels12_win33_iters2", {"pyr_scale": 0.8, "levels": 12, "winsize": 33, "iterations": 2}),
]
HOSTILE_SIZES = [(130, 66), (257, 255)]
HOSTILE_PARAMS = [("winsize3", {"winsize": 3}), ("winsize63", {"winsize": 63})]

# (name, width, height, overrides, F.8 path, coarsest level size)
SEEDED = [
    ("a_16x16", 16, 16, {}, "a", (16, 16)),
    ("a_300x20", 300, 20, {}, "a", (300, 20)),
    ("a_40x40_pyr099_levels1", 40, 40, {"pyr_scale": 0.99, "levels": 1}, "a", (40, 40)),   # two scales of one size
    ("b_130x66", 130, 66, {}, "b", (65, 33)),
    ("b_64x64", 64, 64, {}, "b", (32, 32)),
    ("b_256x256", 256, 256, {}, "b", (32, 32)),
    ("c_127x129_levels1", 127, 129, {"levels": 1}, "c", (64, 64)),
    ("c_128x127_levels1", 128, 127, {"levels": 1}, "c", (64, 64)),
    ("c_257x255_levels2_iters1", 257, 255, {"levels": 2, "iterations": 1}, "c", (64, 64)),
    ("c_257x255_levels2_iters3", 257, 255, {"levels": 2, "iterations": 3}, "c", (64, 64)),
    ("c_257x255_pyr08", 257, 255, {"pyr_scale": 0.8, "levels": 12, "winsize": 33, "iterations": 2}, "c", (34, 34)),
]
SEED_KINDS = ["previous_batch", "upload_flow", "import_f16"]
WINDOWS = ["box", "gaussian"]
SLOTS = 8

_frames, _rcache = {}, {}


def frames_of(w, h):
    if (w, h) not in _frames:
        _frames[(w, h)] = pd.fb_frames(w, h)
    return _frames[(w, h)]


def ref(f0, f1, over, window, seed=None, info=None):
    return ffr.flow(f0, f1, over, window, seed, info, _rcache)


@pytest.fixture(scope="module")
def ctx_of():
    """one context per frame size for the whole module"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = _capi.Context(w, h, frame_slots=SLOTS, flow_slots=4, max_batch=4)
        return made[(w, h)]
    yield get
    for c in made.values():
        c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, want, tag):
    assert np.isfinite(want).all(), tag
    assert np.array_equal(bits(got), bits(want)), \
        f"{tag}: {np.count_nonzero(bits(got) != bits(want))} values differ, max |diff| {np.abs(got - want).max()}"


def check_post(ctx, slots, refs, pov_mode, tag):
    """records and radial scalars of the slots against the exact references of the flows `refs`"""
    n = len(slots)
    c = (0.37 * ctx.width + 0.25, 0.41 * ctx.height + 0.5)
    recs = ctx.pass1_results(slots)
    rad = ctx.radial(slots, [c] * n, [False] * n, False)
    pov = ctx.radial(slots, [c] * n, [False] * n, True)
    for k, want in enumerate(refs):
        x, y, v, mm, cut = recs[k]
        if not pov_mode:
            rx, ry, rv = pr.argmax_ref(want)
            assert (x, y) == (rx, ry) and np.float32(v).tobytes() == np.float32(rv).tobytes(), (tag, k, (x, y, v), (rx, ry, rv))
        pr.check_mean_mag(mm, want)
        pr.check_radial(rad[k], want, c, False)
        pr.check_radial(pov[k], want, c, True)


def run_gaussian(ctx, frames, pairs, over, tag):
    """one Gaussian-window batch of `pairs` (indices into frames), then the same batch with pov_mode on"""
    n = len(pairs)
    ctx.upload_frames(0, frames)
    a, b, slots = [p[0] for p in pairs], [p[1] for p in pairs], list(range(n))
    refs = [ref(frames[i], frames[j], over, "gaussian") for i, j in pairs]
    for pov_mode in (False, True):
        ctx.flow_pairs_farneback(a, b, slots, pov_mode, _capi.FarnebackParams(**over), window="gaussian")
        for k, want in enumerate(refs):
            same_bits(ctx.download_flow(k), want, f"{tag} {ctx.width}x{ctx.height} pair {pairs[k]} pov_mode {pov_mode}")
        check_post(ctx, slots, refs, pov_mode, tag)
    st = ctx.graph_stats()
    assert st["capture_failures"] == 0 and st["captured"] == 0          # general batches are launched eagerly


@pytest.mark.parametrize("name,over", GAUSS_PARAMS, ids=[n for n, _ in GAUSS_PARAMS])
@pytest.mark.parametrize("w,h", GAUSS_SIZES, ids=[f"{w}x{h}" for w, h in GAUSS_SIZES])
def test_gaussian_window_every_size_under_every_parameter_set(ctx_of, w, h, name, over):
    run_gaussian(ctx_of(w, h), frames_of(w, h), pd.FB_BATCH, over, name)


def test_gaussian_window_batch_of_33():
    w, h, B = 130, 66, 33
    frames = pd.fb_frames(w, h, n=B + 1)
    refs = [ref(frames[i], frames[i + 1], {}, "gaussian") for i in range(B)]
    with _capi.Context(w, h, frame_slots=B + 1, flow_slots=B, max_batch=B) as ctx:
        ctx.upload_frames(0, frames)
        ctx.flow_pairs_farneback(list(range(B)), list(range(1, B + 1)), list(range(B)), False, None, window="gaussian")
        for k in range(B):
            same_bits(ctx.download_flow(k), refs[k], f"B33 pair {k}")
        check_post(ctx, list(range(B)), refs, False, "B33")


@pytest.mark.parametrize("name,over", HOSTILE_PARAMS, ids=[n for n, _ in HOSTILE_PARAMS])
@pytest.mark.parametrize("w,h", HOSTILE_SIZES, ids=[f"{w}x{h}" for w, h in HOSTILE_SIZES])
def test_gaussian_window_hostile_content(ctx_of, w, h, name, over):
    """constants 77 / 79, uniform noise, a 1-px checkerboard against its roll, a 40-px jump: bit-exact and finite"""
    kinds = pd.hostile(w, h)
    frames = [f for _, a, b in kinds for f in (a, b)]
    run_gaussian(ctx_of(w, h), frames, [(2 * i, 2 * i + 1) for i in range(len(kinds))], over, name)


def seed_fields(ctx, kind, frames, pairs, over, window):
    """puts a seed into flow slot k of every pair and returns the float32 fields the slots then hold"""
    w, h, n = ctx.width, ctx.height, len(pairs)
    slots = list(range(n))
    if kind == "previous_batch":   # the slots' own flows: an unseeded batch of the same pairs under the same parameters
        ctx.flow_pairs_farneback([p[0] for p in pairs], [p[1] for p in pairs], slots, False, _capi.FarnebackParams(**over),
                                 window=window)
        return [ctx.download_flow(k) for k in slots]
    rng = np.random.default_rng(w * 31 + h + len(kind))
    fields = [(np.float32(ffr.TEXTURE_FLOW) + 0.25 * rng.standard_normal((h, w, 2))).astype(np.float32)   # true flow + noise
              for k in slots]
    if kind == "upload_flow":
        for k in slots:
            ctx.upload_flow(k, fields[k])
        return fields
    t = torch.from_numpy(np.stack(fields)).to("cuda:0").half()
    ctx.import_flows(t, slots)
    return [f for f in t.float().cpu().numpy()]


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("kind", SEED_KINDS)
@pytest.mark.parametrize("name,w,h,over,path,coarsest", SEEDED, ids=[s[0] for s in SEEDED])
def test_initial_flow(ctx_of, name, w, h, over, path, coarsest, kind, window):
    """the content is the translated texture whose estimate keeps its starting field (tests/test_fb_flags_host.py)"""
    ctx, frames, pairs = ctx_of(w, h), ffr.textured_frames(w, h, 3), [(0, 1), (1, 2)]
    ns = fbr.geometry(w, h, over)
    assert fbr.level_params(w, h, over, ns - 1)[:2] == coarsest
    ctx.upload_frames(0, frames)
    seeds = seed_fields(ctx, kind, frames, pairs, over, window)
    refs = []
    for (i, j), s in zip(pairs, seeds):
        info = {}
        refs.append(ref(frames[i], frames[j], over, window, s, info))
        assert info["path"] == path
    ctx.flow_pairs_farneback([0, 1], [1, 2], [0, 1], False, _capi.FarnebackParams(**over), window=window, initial_flow=True)
    for k, want in enumerate(refs):
        same_bits(ctx.download_flow(k), want, f"{name} {kind} {window} pair {pairs[k]}")
    check_post(ctx, [0, 1], refs, False, name)     # the records are this batch's, not the seed's


def test_seeding_an_unwritten_slot_is_refused_and_leaves_it_alone():
    w, h = 64, 64
    frames = frames_of(w, h)
    with _capi.Context(w, h, frame_slots=4, flow_slots=3, max_batch=2) as ctx:
        ctx.upload_frames(0, frames[:3])
        field = np.full((h, w, 2), 0.5, np.float32)
        ctx.upload_flow(0, field)
        before = ctx.pass1_results([0])
        with pytest.raises(_capi.FFLError) as e:    # slot 1 holds nothing: the whole batch is refused
            ctx.flow_pairs_farneback([0, 1], [1, 2], [0, 1], False, None, initial_flow=True)
        assert e.value.code == _capi.FFL_ERR_STATE and "flow slot 1 holds no flow" in str(e.value)
        with pytest.raises(_capi.FFLError) as e:    # and stays unwritten
            ctx.download_flow(1)
        assert e.value.code == _capi.FFL_ERR_STATE
        assert np.array_equal(ctx.download_flow(0), field) and ctx.pass1_results([0]) == before


def test_a_seed_still_queued_gives_the_bits_of_a_synced_one():
    """the seeded batch runs on the other lane than the batch that writes its seed: the read waits for that writer"""
    w, h = 256, 256
    frames, over = frames_of(w, h), {"winsize": 33}
    p = _capi.FarnebackParams(**over)
    pairs = pd.FB_BATCH
    a, b, slots = [q[0] for q in pairs], [q[1] for q in pairs], list(range(4))
    got = {}
    with _capi.Context(w, h, frame_slots=SLOTS, flow_slots=4, max_batch=4) as ctx:
        ctx.upload_frames(0, frames)
        for synced in (True, False):
            ctx.flow_pairs_farneback(a, b, slots, False, p)
            if synced:
                ctx.sync()
            ctx.flow_pairs_farneback(a, b, slots, False, p, window="gaussian", initial_flow=True)
            got[synced] = [ctx.download_flow(k) for k in slots]
    for k in slots:
        assert np.array_equal(bits(got[True][k]), bits(got[False][k])), k
    seed = ref(frames[0], frames[1], over, "box")
    same_bits(got[False][0], ref(frames[0], frames[1], over, "gaussian", seed), "queued seed")


def test_the_window_at_the_default_numbers_runs_the_general_kernels():
    """a result the tuned path (the box window) cannot give; nothing is captured for it"""
    w, h = 256, 256
    frames = frames_of(w, h)
    with _capi.Context(w, h, frame_slots=2, flow_slots=2, max_batch=1) as ctx:
        ctx.upload_frames(0, frames[:2])
        ctx.flow_pairs_farneback([0], [1], [0], False, None)
        ctx.flow_pairs_farneback([0], [1], [1], False, _capi.FarnebackParams(), window="gaussian")
        box, gauss = ctx.download_flow(0), ctx.download_flow(1)
        captured = ctx.graph_stats()["captured"]
    same_bits(box, fbr.flow(frames[0], frames[1]), "tuned path")
    same_bits(gauss, ref(frames[0], frames[1], {}, "gaussian"), "default numbers, Gaussian window")
    assert np.abs(gauss - box).max() > 0.1
    assert captured <= 1     # the tuned batch's graph at most


def test_mode_0_through_ex_is_ffl_flow_pairs_farneback():
    w, h = 130, 66
    frames = frames_of(w, h)
    import ctypes as C
    with _capi.Context(w, h, frame_slots=2, flow_slots=2, max_batch=1) as ctx:
        ctx.upload_frames(0, frames[:2])
        i0, i1, s1 = (C.c_int * 1)(0), (C.c_int * 1)(1), (C.c_int * 1)(1)
        for p in (None, _capi.FarnebackParams(winsize=33)):
            ctx.flow_pairs_farneback([0], [1], [0], False, p)
            ctx._chk(ctx.L.ffl_flow_pairs_farneback_ex(ctx._h, 1, i0, i1, s1, 0, None if p is None else C.byref(p), 0))
            assert np.array_equal(bits(ctx.download_flow(0)), bits(ctx.download_flow(1)))
            assert ctx.pass1_results([0]) == ctx.pass1_results([1])
        with pytest.raises(_capi.FFLError) as e:
            ctx._chk(ctx.L.ffl_flow_pairs_farneback_ex(ctx._h, 1, i0, i1, s1, 0, None, 2))
        assert e.value.code == _capi.FFL_ERR_INVALID and "unknown mode bit" in str(e.value)


def test_the_window_key_reaches_the_device_through_backend_and_pipeline():
    """params["hip_farneback_window"] alone: the default numbers under the Gaussian window, from the drop-in call and from a
    PairEngine chunk"""
    from funscript_flow_amd import backend, pipeline
    w, h = 130, 66
    frames = frames_of(w, h)
    want = [ref(frames[i], frames[i + 1], {}, "gaussian") for i in range(3)]
    info = backend.precompute_flow_info(frames[0], frames[1], {"backend": "HIP", "hip_farneback_window": "gaussian"})
    same_bits(np.asarray(info["flow"]), want[0], "precompute_flow_info")
    B = 2
    with _capi.Context(w, h, frame_slots=pipeline.min_frame_slots(B, 2), flow_slots=pipeline.min_flow_slots(B, 2),
                       max_batch=B) as ctx:
        out = torch.empty((3, h, w, 2), device="cuda:0")
        pipeline.PairEngine(ctx, window="gaussian").process_chunk(frames[:4], flows_out=out)
        got = out.cpu().numpy()
    for k in range(3):
        same_bits(got[k], want[k], f"process_chunk pair {k}")
