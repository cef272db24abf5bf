"""The numpy restatement of the four motion components (tests/axes_ref.py) against the reference's radial term, its closed
forms, and the multi-axis script plumbing (pipeline.frames_to_scripts, postchain.write_funscripts) against a fake engine.
No GPU."""
import json

import numpy as np
import pytest

import axes_ref as ar
import post_ref as pr
from funscript_flow_amd import _capi, pipeline, postchain

SIZES = [(16, 16), (130, 17), (257, 40)]


def noisy(w, h, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    f = (rng.standard_normal((h, w, 2)) * 0.7).astype(np.float32)
    f[..., 0] += 2.0 * np.sin(x * np.float32(0.05)) * np.cos(y * np.float32(0.11))
    f[..., 1] += 1.5 * np.cos(x * np.float32(0.07) + 1) * np.sin(y * np.float32(0.03))
    return f


def centres(w, h):
    return [(0.37 * w + 0.25, 0.41 * h + 0.5), (float(w // 3), float(h // 4)), (0.0, 0.0), (w - 1.0, h - 1.0), (-7.5, -3.25),
            (w + 4.5, h + 9.0)]


def test_binding_constants():
    assert _capi.AXES == ar.AXES == ("radial", "tangential", "shift_x", "shift_y")
    dt = _capi.PASS2_AXES_DTYPE
    assert dt.itemsize == 80 and dt.names[:9] == _capi.PASS2_DTYPE.names
    assert [dt.fields[k][1] for k in _capi.PASS2_DTYPE.names] == [_capi.PASS2_DTYPE.fields[k][1] for k in _capi.PASS2_DTYPE.names]
    assert [dt.fields[k][1] for k in ("tangential", "shift_x", "shift_y", "reserved")] == [48, 56, 64, 72]
    for name in ("ffl_radial_axes", "ffl_radial_window_axes", "ffl_axes_extra_bytes"):
        assert name in _capi.EXPORTS and hasattr(_capi.load(), name)


def test_extra_bytes_is_four_partials_per_workgroup():
    for w, h in SIZES + [(1920, 1080), (3840, 2160)]:
        nblk = -(-(-(-w // pr.P2_STRIP) * -(-h // pr.ROW_GROUP)) // 4)
        assert _capi.axes_extra_bytes(w, h) == 4 * nblk * 8 * _capi.FFL_MAX_BATCH
    with pytest.raises(_capi.FFLError, match="unsupported frame size 8x8"):
        _capi.axes_extra_bytes(8, 8)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_component_0_is_the_reference_term(size):
    """the kernel's order against the reference's: 4 roundings after `dot` on either side, 8 u |term| in all; none in POV
    mode, where both are `dot` itself"""
    w, h = size
    f = noisy(w, h, w)
    for c in centres(w, h):
        ours, ref = ar.axes_terms(f, c, False)[0], pr.radial_terms(f.astype(np.float32), c, False)
        assert (np.abs(ours - ref) <= 8 * pr.U * np.abs(ref)).all()
        assert np.array_equal(ar.axes_terms(f, c, True)[0], pr.radial_terms(f, c, True))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_closed_forms_hold_exactly(size):
    w, h = size
    for centre in ((w // 3, h // 4), (0, 0), (w - 1, h - 1)):
        for name, (f, want) in ar.known_fields(w, h, centre).items():
            got = [m for m, _ in ar.axes_exact(f, centre, True)]
            assert got == want, (name, centre, got, want)
            terms = ar.axes_terms(f, centre, True)
            assert all(np.array_equal(t, np.rint(t)) and np.abs(t).sum() < 2.0 ** 53 for t in terms)
    # rotation is clockwise-positive on screen (x right, y down): right of the centre the field points down
    f, want = ar.known_fields(w, h, (w // 2, h // 2))["rotation"]
    assert want[1] > 0 and f[h // 2, w - 1, 1] > 0 and f[h - 1, w // 2, 0] < 0


def test_weighted_uniform_field_at_16x16():
    for centre in ((5, 9), (0, 0), (15, 15), (8, 8)):
        f, sx, sy = ar.weighted_uniform_16(centre)
        got = ar.axes_exact(f, centre, False)
        assert (got[2][0], got[3][0]) == (sx, sy)
        t = ar.axes_terms(f, centre, False)
        assert np.array_equal(t[2] * 256, np.rint(t[2] * 256))


def test_non_finite_terms_stay_in_their_components():
    w, h = 130, 17
    f = noisy(w, h, 5)
    f[h // 2, w // 2, 0] = np.nan
    got = [m for m, _ in ar.axes_exact(f, (40.5, 8.25), False)]
    assert np.isnan(got[:3]).all() and np.isfinite(got[3])


# ---- scripts ------------------------------------------------------------------------------------------------------------
class FakeEngine:
    """process_chunk / process_flows of a PairEngine: four deterministic components per pair, a cut now and then"""

    def __init__(self):
        self.calls = []

    def _scalars(self, n, axes, key):
        rng = np.random.default_rng(1000 + n + key)
        comps = rng.standard_normal((n, 4)) * [40.0, 25.0, 3.0, 2.0]
        recs = [(int(rng.integers(0, 64)), int(rng.integers(0, 48)), np.float32(0.1), np.float32(1.0), bool(j % 9 == 4))
                for j in range(n)]
        comps[[r[4] for r in recs]] = 0.0
        self.calls.append((n, axes))
        return (comps if axes else comps[:, 0].copy()), recs

    def process_chunk(self, frames, pov_mode=False, cut_threshold=7.0, axes=False, **kw):
        return self._scalars(len(frames) - 1, axes, int(frames[0][0, 0]))

    def process_flows(self, flows, pov_mode=False, cut_threshold=7.0, axes=False, **kw):
        return self._scalars(len(flows), axes, 7)


PARAMS = {"detrend_window": 1.0, "norm_window": 1.0, "batch_size": 20, "keyframe_reduction": False, "pov_mode": False,
          "cut_threshold": 2.5}


def test_frames_to_scripts_against_a_fake_engine():
    total, fps = 50, 30.0
    frames = [np.full((48, 64), i, np.uint8) for i in range(total)]
    plan = pipeline.pair_plan(fps, total, PARAMS)
    assert len(plan) >= 2
    main = pipeline.frames_to_actions(FakeEngine(), frames, fps, PARAMS)
    eng = FakeEngine()
    scripts = pipeline.frames_to_scripts(eng, frames, fps, {**PARAMS, "hip_axes": {"roll": "tangential", "sway": "shift_x"}})
    assert list(scripts) == ["", "roll", "sway"] and all(a for _, a in eng.calls)
    assert scripts[""] == main and main
    # every script is actions_from_scalars of its own column with the chunks' cuts
    comps, cuts, idx = [], [], []
    for chunk in plan:
        c, recs = FakeEngine().process_chunk([frames[i] for i in chunk], axes=True)
        comps.append(c); cuts += [r[4] for r in recs]; idx += chunk[:-1]
    comps = np.concatenate(comps)
    assert any(cuts)
    for suffix, col in (("", 0), ("roll", 1), ("sway", 2)):
        assert scripts[suffix] == postchain.actions_from_scalars([float(v) for v in comps[:, col]], cuts, idx, fps, PARAMS)
    assert scripts["roll"] != scripts[""]
    # without hip_axes: the main script alone
    assert list(pipeline.frames_to_scripts(FakeEngine(), frames, fps, PARAMS)) == [""]
    # flows_to_scripts: the same plumbing over process_flows
    chunk_flows = [list(range(len(c) - 1)) for c in plan]
    fs = pipeline.flows_to_scripts(FakeEngine(), chunk_flows, fps, total, {**PARAMS, "hip_axes": {"heave": "shift_y"}})
    assert list(fs) == ["", "heave"] and fs[""] == pipeline.flows_to_actions(FakeEngine(), chunk_flows, fps, total, PARAMS)
    with pytest.raises(ValueError, match="flows_to_scripts: 1 chunks of flows"):
        pipeline.flows_to_scripts(FakeEngine(), chunk_flows[:1], fps, total, PARAMS)


@pytest.mark.parametrize("frames", [[], [np.zeros((16, 16), np.uint8)]], ids=["no frame", "one frame"])
def test_a_chunk_without_pairs_on_the_device_schedule(frames, monkeypatch):
    """post_out=True, or weights=, which implies it: a buffer for no records (never a negative size), whatever the keyword;
    without either, empty scalars and no records"""
    asked = []
    monkeypatch.setattr(pipeline, "post_buffer", lambda ctx, n, axes=False: asked.append((n, axes)) or ("buffer", n, axes))
    eng = pipeline.PairEngine.__new__(pipeline.PairEngine)
    eng.ctx, eng.B = type("Ctx", (), {"width": 16, "height": 16, "device": 0, "flow_slots": 8})(), 4
    assert eng.process_chunk(frames, post_out=True) == ("buffer", 0, False)
    assert eng.process_chunk(frames, post_out=True, axes=True) == ("buffer", 0, True)
    assert eng.process_chunk(frames, weights=object()) == ("buffer", 0, True)      # the maps of no pairs are not looked at
    assert eng.process_chunk(frames, post_out="mine", weights=object()) == "mine"
    assert asked == [(0, False), (0, True), (0, True)]
    for axes, shape in ((False, (0,)), (True, (0, 4))):
        d, recs = eng.process_chunk(frames, axes=axes)
        assert d.shape == shape and recs == []


def test_script_axes_refusals():
    frames = [np.zeros((48, 64), np.uint8)] * 10
    eng = FakeEngine()
    with pytest.raises(ValueError, match="unknown component 'yaw'"):
        pipeline.frames_to_scripts(eng, frames, 30.0, {**PARAMS, "hip_axes": {"twist": "yaw"}})
    with pytest.raises(ValueError, match="not a file suffix"):
        pipeline.frames_to_scripts(eng, frames, 30.0, {**PARAMS, "hip_axes": {"": "tangential"}})
    with pytest.raises(ValueError, match="not a file suffix"):
        pipeline.flows_to_scripts(eng, [], 30.0, 10, {**PARAMS, "hip_axes": {None: "tangential"}})
    assert not eng.calls                                    # refused before any chunk is processed
    assert pipeline.script_axes({"hip_axes": {"roll": "tangential", "main2": "radial"}}) == [("roll", 1), ("main2", 0)]


def test_sharded_schedules_refuse_axes():
    for call in (lambda: pipeline.process_chunk_sharded(None, [0, 1], 0, 1, None, axes=True),
                 lambda: pipeline.process_chunk_sharded_halo(None, [0, 1], 0, 1, None, axes=True),
                 lambda: pipeline.process_chunk_local_ranks([], [0, 1], axes=True)):
        with pytest.raises(ValueError, match="radial component alone"):
            call()


def test_write_funscripts(tmp_path):
    scripts = {"": [{"at": 0, "pos": 50}], "roll": [{"at": 0, "pos": 10}, {"at": 33, "pos": 90}], "sway": []}
    paths = postchain.write_funscripts(tmp_path / "video", scripts)
    assert [p[len(str(tmp_path)) + 1:] for p in paths] == ["video.funscript", "video.roll.funscript", "video.sway.funscript"]
    assert sorted(p.name for p in tmp_path.iterdir()) == ["video.funscript", "video.roll.funscript", "video.sway.funscript"]
    for p, (suffix, actions) in zip(paths, scripts.items()):
        single = tmp_path / "single.funscript"
        postchain.write_funscript(single, actions)
        assert open(p).read() == single.read_text() and json.load(open(p)) == {"version": "1.0", "actions": actions}
    # a path that already names the main script is its base
    assert postchain.write_funscripts(str(tmp_path / "v2.funscript"), {"": [], "roll": []}) == \
        [str(tmp_path / "v2.funscript"), str(tmp_path / "v2.roll.funscript")]
    with pytest.raises(ValueError, match="not a file suffix"):
        postchain.write_funscripts(tmp_path / "v3", {"../x": []})
