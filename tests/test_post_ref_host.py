"""The exact post references (tests/post_ref.py) against the reference project's recorded outputs, before they judge a
kernel: every entry of post_goldens.npz (made by the real max_divergence and radial_motion_weighted, oracle/gen_golden.py),
and np.argmax's rule on fields with NaN and infinities."""
import math
import os

import numpy as np
import pytest

import post_ref as pr

GOLDENS = ["noise_36x64", "smooth_90x160", "noise_256x256", "ties_40x72", "negfirst_24x40", "farneback_180x320", "edge_32x48"]


@pytest.fixture(scope="module")
def post(golden_dir):
    return np.load(os.path.join(golden_dir, "post_goldens.npz"))


def reference_argmax(flow):
    """max_divergence as the reference writes it (FF:748-758)"""
    with np.errstate(all="ignore"):
        div = np.gradient(flow[..., 0], axis=0) + np.gradient(flow[..., 1], axis=1)
        y, x = np.unravel_index(np.argmax(np.abs(div)), div.shape)
    return int(x), int(y), div[y, x]


@pytest.mark.parametrize("name", GOLDENS)
def test_argmax_ref_reproduces_fixture(post, name):
    flow = post[f"{name}.flow"]
    x, y, v = pr.argmax_ref(flow)
    assert (x, y) == tuple(post[f"{name}.maxdiv"])
    assert np.float32(v).tobytes() == np.float32(post[f"{name}.maxdiv_val"]).tobytes()


@pytest.mark.parametrize("name", GOLDENS)
def test_radial_exact_reproduces_fixture(post, name):
    """the fixture values are np.mean of the same terms: pairwise summation of n terms is within (log2(n / 8) + 8) roundings
    of the exact sum, well inside 8 * u * S at these sizes"""
    flow = post[f"{name}.flow"]
    for c, (gw, gp, gc) in zip(post[f"{name}.centers"], post[f"{name}.radial"]):
        for pov, g in ((False, gw), (True, gp)):
            want, S = pr.radial_exact(flow, c, pov)
            assert abs(want - g) <= 8 * pr.U * S, (name, c, pov, abs(want - g) / (pr.U * S))
            # the terms themselves are the reference's: their np.mean is the fixture value to the last bit
            assert np.mean(pr.radial_terms(flow, c, pov)) == g


def nonfinite_fields():
    rng = np.random.default_rng(5)
    base = rng.standard_normal((40, 300, 2)).astype(np.float32)
    out = {}
    f = base.copy(); f[7, 10, 0] = np.nan; out["one_nan"] = f
    f = base.copy(); f[30, 200, 1] = np.float32(np.inf); out["plus_inf"] = f
    f = base.copy(); f[30, 200, 1] = np.float32(-np.inf); out["minus_inf"] = f
    f = base.copy(); f[3, 5, 0] = np.inf; f[5, 5, 0] = np.inf; f[35, 280, 1] = np.nan; out["inf_minus_inf_then_nan"] = f
    f = base.copy(); f.view(np.uint32)[20, 100, 0] = 0x7FC00001; f.view(np.uint32)[33, 250, 1] = 0xFFFFFFFF; out["payloads"] = f
    out["all_nan"] = np.full((40, 300, 2), np.nan, np.float32)
    out["all_zero"] = np.zeros((40, 300, 2), np.float32)
    out["neg_zero"] = np.full((40, 300, 2), -0.0, np.float32)
    return out


@pytest.mark.parametrize("name", list(nonfinite_fields()))
def test_argmax_ref_is_np_argmax_on_nonfinite(name):
    flow = nonfinite_fields()[name]
    x, y, v = pr.argmax_ref(flow)
    rx, ry, rv = reference_argmax(flow)
    assert (x, y) == (rx, ry)
    assert (math.isnan(v) and math.isnan(rv)) or np.float32(v).tobytes() == np.float32(rv).tobytes()


def test_first_nan_wins_whatever_its_payload():
    """the case DESIGN section 3 names: inf - inf early (default NaN), an input NaN with a larger payload late"""
    x, y, v = pr.argmax_ref(nonfinite_fields()["inf_minus_inf_then_nan"])
    assert (x, y) == (5, 4) and math.isnan(v)
    assert pr.argmax_ref(nonfinite_fields()["payloads"])[:2] == (100, 19)   # the row above the first NaN: its du is NaN
    assert pr.argmax_ref(nonfinite_fields()["all_zero"])[:2] == (0, 0)


def test_fsum_and_bounds():
    a = np.array([1e100, 1.0, -1e100, 1e-30], np.float64)
    assert pr.fsum(a) == 1.0 and float(np.sum(a)) != 1.0          # exact where a float64 running sum is not
    assert math.isnan(pr.fsum(np.array([1.0, np.inf, -np.inf]))) and pr.fsum(np.array([1.0, np.inf])) == math.inf
    assert pr.sum_bound(8, 56) == 64 * 2.0 ** -53
    # depth is derived from the kernel's constants: 32 + 6 + 3 + trips + 6 + 3 + 2
    assert pr.radial_depth(3840, 2160) == 56 and pr.pass1_blocks(3840, 2160) == 1047
    assert pr.pass1_depth(5760, 2880) == 61 and pr.pass1_blocks(5760, 2880) == 2070
    assert pr.pass1_blocks(1920, 1080) == 272 and pr.pass1_blocks(2880, 2880) == 1035
    assert pr.pass1_block_of(1920, 0, 0) == 0 and pr.pass1_block_of(1920, 1919, 1079) == 271


def test_mag_exact_and_acceptance_window():
    rng = np.random.default_rng(2)
    f = (rng.standard_normal((64, 200, 2)) * 2.5).astype(np.float32)
    mean, total = pr.mag_exact(f)
    assert abs(mean - float(np.mean(np.hypot(f[..., 0].astype(np.float64), f[..., 1].astype(np.float64))))) < 1e-6 * mean
    m, ok = pr.mean_mag_accepted(f)
    assert m == mean and 1 <= len(ok) <= 2 and np.float32(mean) in ok
    # a mean that sits on a float32 rounding boundary admits both neighbours, any other exactly one
    one = np.zeros((16, 16, 2), np.float32); one[..., 0] = 1.0
    assert pr.mean_mag_accepted(one)[1] == (np.float32(1.0),)
    tie = one.copy(); tie[0, 0, 0] = np.float32(1.0 + 256 * 2.0 ** -24)   # mean = 1 + 2^-24: halfway between 1 and 1 + 2^-23
    assert set(pr.mean_mag_accepted(tie)[1]) == {np.float32(1.0), np.float32(1.0 + 2.0 ** -23)}
