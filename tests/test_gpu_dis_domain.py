"""GPU sweep of the DIS path (ffl_flow_pairs_dis, kernels_dis.hip) over its declared domain (tests/param_domain.py): every
DIS_SIZES size at PRESET_FAST and every DIS_PARAMS set at three non-square sizes, six contents per batch.  Each flow is
bit-identical to the plain-C restatement (tests/dis_ref), the pass-1 argmax exact in position and bits,
the mean magnitude and both radial scalars within the derived bounds of tests/post_ref.py; every debug stage at every scale
equals the restatement's dump.  The lists are iterated as they stand: an entry the product refuses fails here and moves to
REFUSED by hand.  Parity with cv2.DISOpticalFlow itself is unpinned (no cv2 here)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dis_ref
import gen_dis_golden
import oracle as orc
import param_domain as pd
import post_ref as pr
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

SIZES, PARAM_PAIRS, REFUSED = pd.DIS_SIZES, pd.DIS_PARAM_PAIRS, pd.REFUSED
DIS_REFUSED = [r for r in REFUSED if r[0] == "dis"]
B = 6   # gen_dis_golden.contents: translate, zoom, blocks, noise, constant, identical

_contents, _refs = {}, {}


def contents(w, h):
    if (w, h) not in _contents:
        _contents[(w, h)] = gen_dis_golden.contents(w, h)
    return _contents[(w, h)]


def reference(w, h, over, name, f0, f1):
    """the restatement's field, computed once per distinct (size, parameters, pair)"""
    key = (w, h, tuple(sorted(over.items())), name)
    if key not in _refs:
        _refs[key] = dis_ref.flow(f0, f1, dis_ref.fast_params(**over))
    return _refs[key]


@pytest.fixture(scope="module")
def ctx_of():
    """one context per frame size for the whole module (a sweep entry costs a batch, not a context)"""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = _capi.Context(w, h, frame_slots=2 * B, flow_slots=B, max_batch=B)
        return made[(w, h)]
    yield get
    for c in made.values():
        c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_pairs(ctx, named_pairs, over, tag):
    """one DIS batch of the pairs under `over`: flows, pass-1 records and both radial scalars against the references"""
    w, h, n = ctx.width, ctx.height, len(named_pairs)
    p = _capi.DisParams(**over)
    ctx.upload_frames(0, [f for _, a, b in named_pairs for f in (a, b)])
    ctx.flow_pairs_dis(list(range(0, 2 * n, 2)), list(range(1, 2 * n, 2)), list(range(n)), False, p)
    recs = ctx.pass1_results(list(range(n)))
    c = (0.37 * w + 0.25, 0.41 * h + 0.5)
    rad = ctx.radial(list(range(n)), [c] * n, [False] * n, False)
    pov = ctx.radial(list(range(n)), [c] * n, [False] * n, True)
    for i, (name, f0, f1) in enumerate(named_pairs):
        ref = reference(w, h, over, name, f0, f1)
        got = ctx.download_flow(i)
        assert np.isfinite(ref).all(), (tag, name)
        assert np.array_equal(got, ref) and np.array_equal(bits(got), bits(ref)), \
            f"{tag} {w}x{h} {name}: {np.count_nonzero(bits(got) != bits(ref))} values differ, max |diff| {np.abs(got - ref).max()}"
        x, y, v, mm, cut = recs[i]
        rx, ry, rv = pr.argmax_ref(ref)
        assert (x, y) == (rx, ry) and np.float32(v).tobytes() == np.float32(rv).tobytes(), (tag, name, (x, y, v), (rx, ry, rv))
        pr.check_mean_mag(mm, ref)
        pr.check_radial(rad[i], ref, c, False)
        pr.check_radial(pov[i], ref, c, True)
        if name.split("/")[0] in ("constant", "identical"):
            assert not got.any(), (tag, name)
    assert ctx.graph_stats()["capture_failures"] == 0


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_every_size_at_the_defaults(ctx_of, w, h):
    assert _capi.dis_geometry(w, h) == dis_ref.geometry(w, h)
    check_pairs(ctx_of(w, h), contents(w, h), {}, "defaults")


@pytest.mark.parametrize("wh,name,over", PARAM_PAIRS, ids=[f"{w}x{h}-{n}" for (w, h), n, _ in PARAM_PAIRS])
def test_every_parameter_set_at_three_sizes(ctx_of, wh, name, over):
    check_pairs(ctx_of(*wh), contents(*wh), over, name)


STAGE_SIZES = [(192, 320, None), (768, 256, None), (64, 96, None), (1024, 1024, 2)]   # (w, h, the one scale run or all)


@pytest.mark.parametrize("w,h,only", STAGE_SIZES, ids=[f"{w}x{h}" for w, h, _ in STAGE_SIZES])
def test_every_debug_stage_at_every_scale(ctx_of, w, h, only):
    """pass-1 and pass-2 patch flows, the dense field, the refined field and the scale's images, coarsest to finest"""
    coarsest, finest = _capi.dis_geometry(w, h)
    scales = [only] if only is not None else list(range(coarsest, finest - 1, -1))
    assert len(scales) == {(192, 320): 2, (768, 256): 4, (64, 96): 1, (1024, 1024): 1}[(w, h)]
    _, f0, f1 = contents(w, h)[1]
    ctx = ctx_of(w, h)
    ctx.upload_frames(0, [f0, f1])
    for s in scales:
        for name, st in _capi.DIS_STAGES.items():
            got = ctx.debug_dis_pair(0, 1, s, name)
            _, want = dis_ref.flow(f0, f1, dis_ref.fast_params(), dbg=(s, st))
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), \
                f"{w}x{h} scale {s} stage {name}: {np.count_nonzero(bits(got) != bits(want))} values differ"
    assert np.array_equal(ctx.download_flow(0), reference(w, h, {}, "zoom", f0, f1))


@pytest.mark.parametrize("over", [{"patch_stride": 2}, {"patch_stride": 8, "finest_scale": 3}, {"stripes": 3}],
                         ids=["stride2", "stride8_finest3", "stripes3"])
def test_debug_stages_under_other_strides(ctx_of, over):
    """the patch-grid shape of the dumps follows patch_stride; 192x320 at every scale"""
    w, h = 192, 320
    p = _capi.DisParams(**over)
    coarsest, finest = _capi.dis_geometry(w, h, p)
    _, f0, f1 = contents(w, h)[2]
    ctx = ctx_of(w, h)
    ctx.upload_frames(0, [f0, f1])
    for s in range(coarsest, finest - 1, -1):
        for name, st in _capi.DIS_STAGES.items():
            got = ctx.debug_dis_pair(0, 1, s, name, p)
            _, want = dis_ref.flow(f0, f1, dis_ref.fast_params(**over), dbg=(s, st))
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), (over, s, name)


def test_b33_mixed_with_default_farneback_on_two_lanes_non_square():
    """192x320, B = 33: DIS and default-Farneback batches alternate over shared frame slots on a two-lane context; each
    result equals the pair computed alone, every flow slot recycled across the algorithms"""
    w, h, n = 192, 320, 33
    fr = [np.ascontiguousarray(f) for f in sine_translate_frames(2 * n + 1, w, h, seed=11, amp=(3.0, 2.0), zoom=0.02)]
    with _capi.Context(w, h, frame_slots=2 * n + 1, flow_slots=2 * n, max_batch=n) as ctx:
        assert ctx.get_option("lanes") == 2
        ctx.upload_frames(0, fr)
        lo_slots, hi_slots = list(range(n)), list(range(n, 2 * n))
        for rnd in range(2):
            lo = n * rnd
            f0, f1 = list(range(lo, lo + n)), list(range(lo + 1, lo + n + 1))
            first, second = (ctx.flow_pairs_dis, ctx.flow_pairs) if rnd == 0 else (ctx.flow_pairs, ctx.flow_pairs_dis)
            first(f0, f1, lo_slots)
            second(f0, f1, hi_slots)
            recs = ctx.pass1_results(lo_slots + hi_slots)
            for s in range(2 * n):
                a = lo + s % n
                dis = (s < n) == (rnd == 0)
                want = dis_ref.flow(fr[a], fr[a + 1]) if dis else orc.farneback(fr[a], fr[a + 1])
                got = ctx.download_flow(s)
                assert np.array_equal(bits(got), bits(want)), (rnd, s, "dis" if dis else "farneback")
                rx, ry, rv = pr.argmax_ref(want)
                assert recs[s][:2] == (rx, ry) and np.float32(recs[s][2]).tobytes() == np.float32(rv).tobytes(), (rnd, s)
                pr.check_mean_mag(recs[s][3], want)
        assert ctx.graph_stats()["capture_failures"] == 0


def test_b4_at_2048x512():
    """four workgroups with the patch table near its cap; the pairs in the other direction than the size sweep runs them"""
    w, h = 2048, 512
    pairs = [(n + "/reversed", b, a) for n, a, b in contents(w, h)[:4]]
    with _capi.Context(w, h, frame_slots=8, flow_slots=4, max_batch=4) as ctx:
        check_pairs(ctx, pairs, {}, "B=4")


@pytest.mark.parametrize("algo,w,h,over,word", DIS_REFUSED,
                         ids=[f"{w}x{h}-" + ",".join(f"{k}={v}" for k, v in o.items()) for _, w, h, o, _ in DIS_REFUSED])
def test_refused_entries_name_their_rule_and_leave_the_context_working(ctx_of, algo, w, h, over, word):
    ctx = ctx_of(w, h)
    f = sine_translate_frames(2, w, h, seed=5, amp=(2.0, 1.0))
    ctx.upload_frames(0, [f[0], f[1]])
    with pytest.raises(_capi.FFLError, match=word):
        ctx.flow_pairs_dis([0], [1], [0], False, _capi.DisParams(**over))
    if dis_ref.geometry(w, h) is not None:      # the size itself is served: a PRESET_FAST pair
        ctx.flow_pairs_dis([0], [1], [0])
        want = dis_ref.flow(f[0], f[1])
    else:                                        # DIS serves no parameters at this size: a Farneback pair
        ctx.flow_pairs([0], [1], [0])
        want = orc.farneback(f[0], f[1])
    ctx.pass1_results([0])
    assert np.array_equal(bits(ctx.download_flow(0)), bits(want))
