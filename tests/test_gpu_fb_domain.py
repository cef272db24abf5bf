"""GPU sweep of Farneback with caller-chosen parameters (ffl_flow_pairs_farneback, kernels_farneback_general.hip) over its
declared domain (tests/param_domain.py): every FB_SIZES size -- levels smaller than one 64 x 16 tile, one 256-wide blur
segment, one 64 x 32 blur tile and, at winsize 63, than the box window itself -- under every FB_PARAMS set, hostile content
under the widest and narrowest windows, the two widest level Gaussians and winsize 63 at 1920x1080.  Each flow is
bit-identical to the plain-C restatement (tests/fb_general_ref) and, at the reference's values, to the
oracle; the pass-1 argmax is exact in position and bits, the mean magnitude and both radial scalars within the derived
bounds of tests/post_ref.py.  The lists are iterated as they stand.  Parity with cv2 itself is unpinned."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import fb_general_ref as fbr
import oracle as orc
import param_domain as pd
import post_ref as pr
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

SIZES, PARAMS, WIDE = pd.FB_SIZES, pd.FB_PARAMS, pd.FB_WIDE_GAUSSIAN
HOSTILE_SIZES, HOSTILE_PARAMS = pd.FB_HOSTILE_SIZES, pd.FB_HOSTILE_PARAMS
SLOTS = 8   # frames of the largest batch here (four hostile pairs)

_frames = {}


def frames_of(w, h):
    if (w, h) not in _frames:
        _frames[(w, h)] = pd.fb_frames(w, h)
    return _frames[(w, h)]


@pytest.fixture(scope="module")
def ctx_of():
    """one context per frame size for the whole module (a sweep entry costs a batch, not a context)"""
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


def run_and_check(ctx, frames, pairs, params, want_of, tag, force=0):
    """one batch of `pairs` (indices into frames) under params: flows against want_of(f0, f1), records and radial scalars
    against the exact references; then the same batch with pov_mode on: the same flows"""
    w, h, n = ctx.width, ctx.height, len(pairs)
    ctx.upload_frames(0, frames)
    a, b, slots = [p[0] for p in pairs], [p[1] for p in pairs], list(range(n))
    c = (0.37 * w + 0.25, 0.41 * h + 0.5)
    ctx.set_option("fb_general", force)
    refs = [want_of(frames[i], frames[j]) for i, j in pairs]
    for pov_mode in (False, True):
        ctx.flow_pairs_farneback(a, b, slots, pov_mode, params)
        recs = ctx.pass1_results(slots)
        rad = ctx.radial(slots, [c] * n, [False] * n, False)
        pov = ctx.radial(slots, [c] * n, [False] * n, True)
        for k, ref in enumerate(refs):
            got = ctx.download_flow(k)
            assert np.isfinite(ref).all(), (tag, pairs[k])
            assert np.array_equal(got, ref) and np.array_equal(bits(got), bits(ref)), \
                f"{tag} {w}x{h} pair {pairs[k]} pov_mode {pov_mode}: {np.count_nonzero(bits(got) != bits(ref))} values " \
                f"differ, max |diff| {np.abs(got - ref).max()}"
            x, y, v, mm, cut = recs[k]
            if not pov_mode:
                rx, ry, rv = pr.argmax_ref(ref)
                assert (x, y) == (rx, ry) and np.float32(v).tobytes() == np.float32(rv).tobytes(), \
                    (tag, pairs[k], (x, y, v), (rx, ry, rv))
            pr.check_mean_mag(mm, ref)
            pr.check_radial(rad[k], ref, c, False)
            pr.check_radial(pov[k], ref, c, True)
    ctx.set_option("fb_general", 0)
    st = ctx.graph_stats()
    assert st["capture_failures"] == 0 and st["captured"] == 0          # general batches are launched eagerly


@pytest.mark.parametrize("name,over", PARAMS, ids=[n for n, _ in PARAMS])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_size_under_every_parameter_set(ctx_of, w, h, name, over):
    assert _capi.farneback_geometry(w, h, _capi.FarnebackParams(**over))[0] == fbr.geometry(w, h, over)
    run_and_check(ctx_of(w, h), frames_of(w, h), pd.FB_BATCH, _capi.FarnebackParams(**over),
                  lambda a, b: fbr.flow(a, b, over), name)


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_size_at_the_reference_values_equals_the_oracle(ctx_of, w, h):
    """fb_general = 1 sends the reference's own parameters through the general kernels: the sweep is tied to the oracle, not
    only to the restatement"""
    run_and_check(ctx_of(w, h), frames_of(w, h), pd.FB_BATCH, _capi.FarnebackParams(), orc.farneback, "oracle", force=1)


@pytest.mark.parametrize("name,over", HOSTILE_PARAMS, ids=[n for n, _ in HOSTILE_PARAMS])
@pytest.mark.parametrize("w,h", HOSTILE_SIZES, ids=[f"{w}x{h}" for w, h in HOSTILE_SIZES])
def test_hostile_content(ctx_of, w, h, name, over):
    """constants 77 / 79, uniform noise, a 1-px checkerboard against its roll, a 40-px jump: bit-exact and finite"""
    kinds = pd.hostile(w, h)
    frames = [f for _, a, b in kinds for f in (a, b)]
    pairs = [(2 * i, 2 * i + 1) for i in range(len(kinds))]
    run_and_check(ctx_of(w, h), frames, pairs, _capi.FarnebackParams(**over), lambda a, b: fbr.flow(a, b, over), name)


@pytest.mark.parametrize("w,h,over", WIDE, ids=[f"{w}x{h}" for w, h, _ in WIDE])
def test_the_widest_level_gaussians(w, h, over):
    """one pair each: level Gaussians of 3 ... 159 taps over seven scales, and a 187-tap level (the cap is 191)"""
    taps = [fbr.level_params(w, h, over, k)[3] for k in range(fbr.geometry(w, h, over))]
    assert max(taps) == {3840: 159, 2432: 187}[w], taps
    fr = list(pd.wide_frames(w, h))     # motion the coarsest level must carry: a flat top level would hide its Gaussian
    with _capi.Context(w, h, frame_slots=2, flow_slots=1, max_batch=1) as ctx:
        run_and_check(ctx, fr, [(0, 1)], _capi.FarnebackParams(**over), lambda a, b: fbr.flow(a, b, over), "wide")


def test_winsize63_at_1080p_in_the_general_work_area():
    """the largest box-and-solve LDS request at full grid size, thirteen levels, R regions beyond the lane buffers"""
    w, h = 1920, 1080
    over = {"pyr_scale": 0.9, "levels": 12, "winsize": 63, "iterations": 1}
    p = _capi.FarnebackParams(**over)
    assert _capi.farneback_geometry(w, h, p)[0] == 13 and _capi.farneback_extra_bytes(w, h, 2, p) > 0
    fr = [np.ascontiguousarray(f) for f in sine_translate_frames(3, w, h, seed=17, amp=(2.5, 1.5), period=7, zoom=0.02)]
    with _capi.Context(w, h, frame_slots=3, flow_slots=2, max_batch=2) as ctx:
        run_and_check(ctx, fr, [(0, 1), (1, 2)], p, lambda a, b: fbr.flow(a, b, over), "winsize63 1080p")
