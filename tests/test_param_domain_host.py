"""Host tests of the declared domain of DIS and general Farneback (tests/param_domain.py): every accepted (size, parameters)
pair is accepted by the product and by the restatement with the same scale counts and gives a finite field, every REFUSED
entry is refused by both, the device sweeps iterate the lists as they stand, and the restatements reproduce the committed
corner fixtures (tests/golden/param_sweep_golden.npz).  No GPU needed."""
import json
import os

import numpy as np
import pytest

import dis_ref
import fb_general_ref as fbr
import gen_param_sweep_golden as gen
import param_domain as pd
from funscript_flow_amd import _capi

HERE = os.path.dirname(os.path.abspath(__file__))


def _dis_product(w, h, over):
    """(coarsest, finest) of the product (ffl_dis_geometry); a refusal raises, and fails the test that did not expect it"""
    return _capi.dis_geometry(w, h, _capi.DisParams(**over))


def _fb_product(w, h, over):
    """scale count of the product (ffl_farneback_geometry); a refusal raises, and fails the test that did not expect it"""
    return _capi.farneback_geometry(w, h, _capi.FarnebackParams(**over))[0]


# ---- no silent skipping ---------------------------------------------------------------------------------------------

def test_the_geometry_the_sizes_were_chosen_for():
    """scale counts and patch grids named in param_domain's comments are the restatement's own output"""
    def grid(w, h, s, st=4):
        return 1 + ((w >> s) - 8) // st, 1 + ((h >> s) - 8) // st
    assert dis_ref.geometry(64, 96) == (2, 2) and dis_ref.geometry(96, 64) == (2, 2)
    assert dis_ref.geometry(64, 2048) == (3, 2) and 64 >> 2 == 16
    assert dis_ref.geometry(768, 256) == (5, 2) and grid(768, 256, 5) == (5, 1) and grid(256, 768, 5) == (1, 5)
    assert dis_ref.geometry(1024, 1024) == (5, 2) and np.prod(grid(1024, 1024, 2)) == 3969
    assert dis_ref.geometry(2048, 512) == (6, 2) and grid(2048, 512, 6) == (7, 1) and np.prod(grid(2048, 512, 2)) == 3937
    assert dis_ref.geometry(512, 2048) == (6, 2) and grid(512, 2048, 6) == (1, 7)
    assert np.prod(grid(768, 256, 2, 1)) == 10545                      # the one refused pair of the parameter sweep
    w, h, over = pd.FB_WIDE_GAUSSIAN[0]
    assert fbr.geometry(w, h, over) == 7 and [fbr.level_params(w, h, over, k)[3] for k in range(7)] == [3, 3, 9, 19, 39, 79, 159]
    w, h, over = pd.FB_WIDE_GAUSSIAN[1]
    assert fbr.geometry(w, h, over) == 3 and fbr.level_params(w, h, over, 2)[::3] == (32, 187)


def test_every_accepted_dis_pair_is_accepted_by_product_and_restatement():
    pairs = [(wh, "defaults", {}) for wh in pd.DIS_SIZES] + pd.DIS_PARAM_PAIRS
    assert len(pairs) == len(pd.DIS_SIZES) + len(pd.DIS_PARAM_SIZES) * len(pd.DIS_PARAMS) - 1
    for (w, h), name, over in pairs:
        want = dis_ref.geometry(w, h, dis_ref.fast_params(**over))
        assert want is not None, (w, h, name)
        assert _dis_product(w, h, over) == want, (w, h, name)
    # every (size, entry) of the sweep's grid is either run or listed as refused: nothing is dropped
    refused = {(w, h, json.dumps(o, sort_keys=True)) for a, w, h, o, _ in pd.REFUSED if a == "dis"}
    run = {(wh, n) for wh, n, _ in pd.DIS_PARAM_PAIRS}
    for wh in pd.DIS_PARAM_SIZES:
        for name, over in pd.DIS_PARAMS:
            assert ((wh, name) in run) != ((*wh, json.dumps(over, sort_keys=True)) in refused), (wh, name)


@pytest.mark.parametrize("w,h", pd.DIS_PARAM_SIZES)
def test_every_dis_parameter_set_gives_a_finite_field(w, h):
    f0, f1 = gen.dis_frames(w, h)
    for wh, name, over in pd.DIS_PARAM_PAIRS:
        if wh == (w, h):
            assert np.isfinite(dis_ref.flow(f0, f1, dis_ref.fast_params(**over))).all(), name


def test_every_accepted_farneback_pair_is_accepted_by_product_and_restatement():
    for w, h in pd.FB_SIZES:
        f = pd.fb_frames(w, h, 2)
        for name, over in pd.FB_PARAMS:
            want = fbr.geometry(w, h, over)
            assert want is not None and _fb_product(w, h, over) == want, (w, h, name)
            assert np.isfinite(fbr.flow(f[0], f[1], over)).all(), (w, h, name)
    for w, h, over in pd.FB_WIDE_GAUSSIAN:
        assert fbr.geometry(w, h, over) is not None and _fb_product(w, h, over) == fbr.geometry(w, h, over)
    for w, h in pd.FB_HOSTILE_SIZES:
        for name, over in pd.FB_HOSTILE_PARAMS:
            assert _fb_product(w, h, over) == fbr.geometry(w, h, over) is not None


@pytest.mark.parametrize("algo,w,h,over,word", pd.REFUSED,
                         ids=[f"{a}-{w}x{h}-" + ",".join(f"{k}={v}" for k, v in o.items()) for a, w, h, o, _ in pd.REFUSED])
def test_every_refused_entry_is_refused_by_both(algo, w, h, over, word):
    if algo == "dis":
        assert dis_ref.geometry(w, h, dis_ref.fast_params(**over)) is None
        with pytest.raises(ValueError, match=word):       # the rule's own words, as on the device
            _dis_product(w, h, over)
    else:
        assert fbr.geometry(w, h, over) is None
        with pytest.raises(ValueError, match=word):
            _fb_product(w, h, over)


def test_the_device_sweeps_iterate_the_declared_lists_without_a_skip_path():
    """the lists the device tests are parametrised with are the domain's own objects, and none of the three new test
    files holds a skip, an expected-failure mark or a try block"""
    import test_gpu_dis_domain as gd
    import test_gpu_fb_domain as gf
    assert gd.SIZES is pd.DIS_SIZES and gd.PARAM_PAIRS is pd.DIS_PARAM_PAIRS and gd.REFUSED is pd.REFUSED
    assert gf.SIZES is pd.FB_SIZES and gf.PARAMS is pd.FB_PARAMS and gf.WIDE is pd.FB_WIDE_GAUSSIAN
    assert gf.HOSTILE_SIZES is pd.FB_HOSTILE_SIZES and gf.HOSTILE_PARAMS is pd.FB_HOSTILE_PARAMS
    # the words are assembled here so that this file does not match itself; it speaks of them in prose, so only the marks
    # and calls are looked for here
    words = {"test_gpu_dis_domain.py": ("sk" + "ip", "xf" + "ail", "tr" + "y:"),
             "test_gpu_fb_domain.py": ("sk" + "ip", "xf" + "ail", "tr" + "y:"),
             "test_param_domain_host.py": ("pytest.sk" + "ip", "mark.sk" + "ip", "xf" + "ail", "importorsk" + "ip", "tr" + "y:")}
    for name, ws in words.items():
        with open(os.path.join(HERE, name)) as f:
            src = f.read()
        for word in ws:
            assert word not in src, (name, word)


# ---- fixtures -------------------------------------------------------------------------------------------------------

def test_restatements_reproduce_the_committed_corner_fixtures(golden_dir):
    """tests/golden/param_sweep_golden.npz pins appendix D / F arithmetic at the new corners: one DIS entry per DIS_SIZES
    size, one general-Farneback entry per FB_PARAMS set"""
    g = np.load(os.path.join(golden_dir, "param_sweep_golden.npz"))
    e = gen.entries()
    assert list(g["names"]) == [c[0] for c in gen.cases()]
    assert len(g["names"]) == len(pd.DIS_SIZES) + len(pd.FB_PARAMS)
    for key in ("names", "params", "frames_sha256", "flow_sha256", "pass1_xy", "pass1_div", "pass1_mean_mag", "radial"):
        for i, name in enumerate(g["names"]):
            assert np.array_equal(np.asarray(e[key][i]), np.asarray(g[key][i])), (name, key)
    for i, (name, algo, w, h, over) in enumerate(gen.cases()):
        assert json.loads(str(g["params"][i])) == over, name
