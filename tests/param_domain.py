"""The declared domain of the two parameterised flow paths (DIS, general Farneback): the sizes and parameter sets that the
device sweeps (tests/test_gpu_dis_domain.py, tests/test_gpu_fb_domain.py) run and that tests/test_param_domain_host.py
checks on the CPU first.  "Accepted" is stated here once: every (size, parameters) pair of the accepted lists is accepted
by the product and by the restatement, every REFUSED entry is refused by both, and the device tests iterate these lists as
they stand.  A combination found to be refused moves to REFUSED by hand; none is dropped.

Sizes are (width, height).  Parameter sets are (name, overrides) with the product's field names."""
import numpy as np

from funscript_flow_amd.synth import sine_translate_frames

# ---- DIS ------------------------------------------------------------------------------------------------------------
# chosen for their geometry (coarsest scale, patch grid at the coarsest scale, patches at the finest scale = 2):
DIS_SIZES = [
    (64, 96), (96, 64),          # one scale (coarsest == finest == 2): the start field is never upsampled
    (64, 2048), (2048, 64),      # a 16-pixel-wide finest scale
    (320, 192), (192, 320),      # two scales, non-square
    (768, 256), (256, 768),      # four scales; the coarsest is a one-row (one-column) patch grid
    (384, 640), (1280, 768),
    (1024, 1024),                # 3969 patches at the finest scale (the LDS table holds 4096)
    (2048, 512), (512, 2048),    # coarsest scale 6 with a 7 x 1 patch grid; 3937 patches at the finest scale
]
# the sizes every DIS_PARAMS entry runs at on the device (DIS_PARAM_PAIRS leaves out the one refused pair)
DIS_PARAM_SIZES = [(320, 192), (192, 320), (768, 256)]

DIS_PARAMS = [
    ("finest3", {"finest_scale": 3}),
    ("stride1", {"patch_stride": 1}), ("stride2", {"patch_stride": 2}), ("stride8", {"patch_stride": 8}),
    ("gd1", {"grad_descent_iters": 1}), ("gd15", {"grad_descent_iters": 15}), ("gd40", {"grad_descent_iters": 40}),
    ("vr0", {"var_refine_iters": 0}), ("vr1", {"var_refine_iters": 1}), ("vr12", {"var_refine_iters": 12}),
    ("alpha1_gamma0_delta0", {"vr_alpha": 1.0, "vr_gamma": 0.0, "vr_delta": 0.0}),
    ("stripes3", {"stripes": 3}), ("stripes5", {"stripes": 5}), ("stripes1000", {"stripes": 1000}),
    ("nomean_noprop", {"use_mean_norm": 0, "use_spatial_prop": 0}),
    # combinations
    ("stride8_finest3", {"patch_stride": 8, "finest_scale": 3}),
    ("stride2_stripes3", {"patch_stride": 2, "stripes": 3}),
    ("gd1_noprop", {"grad_descent_iters": 1, "use_spatial_prop": 0}),
    ("gd15_stride2_vr1", {"grad_descent_iters": 15, "patch_stride": 2, "var_refine_iters": 1}),
    ("finest3_stripes5_gamma0", {"finest_scale": 3, "stripes": 5, "vr_gamma": 0.0}),
]

_DIS_REFUSED_PAIRS = {((768, 256), "stride1")}   # 192 x 64 at scale 2: 185 x 57 = 10545 patches
DIS_PARAM_PAIRS = [(wh, name, over) for wh in DIS_PARAM_SIZES for name, over in DIS_PARAMS
                   if (wh, name) not in _DIS_REFUSED_PAIRS]

# ---- general Farneback ----------------------------------------------------------------------------------------------
FB_SIZES = [(16, 16), (17, 19), (31, 64), (64, 33), (65, 17), (127, 129), (130, 66), (20, 300), (300, 20),
            (63, 65), (64, 64), (257, 255)]

FB_PARAMS = [
    ("winsize3", {"winsize": 3}), ("winsize5", {"winsize": 5}), ("winsize7", {"winsize": 7}),
    ("winsize33", {"winsize": 33}), ("winsize61", {"winsize": 61}), ("winsize63", {"winsize": 63}),
    ("polyn7_sigma05", {"poly_n": 7, "poly_sigma": 0.5}), ("polyn7_sigma3", {"poly_n": 7, "poly_sigma": 3.0}),
    ("iters10", {"iterations": 10}),
    ("levels0", {"levels": 0}),
    ("pyr03_levels4", {"pyr_scale": 0.3, "levels": 4}),
    ("pyr08_levels12_win33_iters2", {"pyr_scale": 0.8, "levels": 12, "winsize": 33, "iterations": 2}),
    ("pyr09_levels12_win63_iters1", {"pyr_scale": 0.9, "levels": 12, "winsize": 63, "iterations": 1}),
    # combinations that stack the extremes
    ("winsize63_polyn7", {"winsize": 63, "poly_n": 7}),
    ("winsize3_iters10", {"winsize": 3, "iterations": 10}),
    ("polyn5_sigma3_levels0", {"poly_sigma": 3.0, "levels": 0}),
    ("polyn5_sigma05_winsize5", {"poly_sigma": 0.5, "winsize": 5}),
]

# (width, height, overrides): level Gaussians of 3 ... 159 taps over 7 scales; a 187-tap level on a 32 x 32 level
FB_WIDE_GAUSSIAN = [
    (3840, 2160, {"levels": 6}),
    (2432, 2432, {"pyr_scale": 0.115, "levels": 2}),
]

# ---- refused by product and restatement alike -----------------------------------------------------------------------
# (algorithm, width, height, overrides, words of the product's rule)
_WORKING_SET, _PATCHES = "working set exceeds", "too many patches"
_STRIDES, _SMALL, _DIVISIBLE = "whole number of patch strides", "too small for finest_scale", "divisible by 2\\^coarsest"


def _finest_word(w, h, finest):
    """finest_scale 0 / 1: the patch cap is checked before the working set, so it speaks first wherever a scale has more
    than 4096 patches at stride 4"""
    lw, lh = w >> finest, h >> finest
    return _PATCHES if (1 + (lw - 8) // 4) * (1 + (lh - 8) // 4) > 4096 else _WORKING_SET


REFUSED = [("dis", w, h, {"finest_scale": f}, _finest_word(w, h, f)) for (w, h) in DIS_SIZES for f in (0, 1)] + [
    ("dis", 320, 192, {"patch_stride": 3}, _STRIDES),
    ("dis", 1024, 1024, {"patch_stride": 2}, _PATCHES),
    ("dis", 512, 256, {"patch_stride": 1}, _PATCHES),
    ("dis", 768, 256, {"patch_stride": 1}, _PATCHES),
    ("dis", 320, 192, {"grad_descent_iters": 0}, "grad_descent_iters >= 1"),
    ("dis", 64, 64, {}, _SMALL),
    ("dis", 640, 360, {}, _DIVISIBLE),
    ("farneback", 5760, 2880, {"pyr_scale": 0.11, "levels": 2}, "5760x2880"),
]


# ---- content --------------------------------------------------------------------------------------------------------
def fb_frames(w, h, n=5):
    """n textured frames of a translating, slightly zooming pattern, seeded from the size"""
    fr = sine_translate_frames(n, w, h, seed=w * 31 + h, amp=(2.5, 1.5), period=7, zoom=0.02)
    return [np.ascontiguousarray(f) for f in fr]


def wide_frames(w, h, jump=48):
    """a pair whose motion the coarsest levels must carry: texture over a low-frequency pattern, the second frame the first
    moved by `jump` pixels along x (under one pixel at 1/64 size, out of reach of the fine levels alone)"""
    tex = sine_translate_frames(1, w + jump, h, seed=w * 31 + h, amp=(0.0, 0.0))[0].astype(np.float64)
    y, x = np.mgrid[0:h, 0:w + jump].astype(np.float64)
    low = 70.0 * np.sin(2 * np.pi * x / (w / 2.5)) * np.cos(2 * np.pi * y / (h / 1.5))
    img = np.clip(np.rint(128.0 + 0.45 * (tex - 128.0) + low), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(img[:, jump:]), np.ascontiguousarray(img[:, :w])


FB_BATCH = [(0, 1), (1, 2), (2, 0), (3, 4)]   # three pairs over three frames and one pair of two further frames: 5 < 2 * 4


def hostile(w, h):
    """(name, f0, f1) pairs of content a window sum or a solve may trip on: constants two grey levels apart, uniform noise,
    a 1-px checkerboard against its roll, a 40-px jump"""
    rng = np.random.default_rng(w * 31 + h)
    y, x = np.mgrid[0:h, 0:w]
    checker = (((x + y) & 1) * 255).astype(np.uint8)
    wide = sine_translate_frames(1, w + 40, h, seed=6)[0]
    return [("constant", np.full((h, w), 77, np.uint8), np.full((h, w), 79, np.uint8)),
            ("noise", rng.integers(0, 256, (h, w), dtype=np.uint8), rng.integers(0, 256, (h, w), dtype=np.uint8)),
            ("checker", checker, np.roll(checker, 1, axis=1)),
            ("jump40", np.ascontiguousarray(wide[:, :w]), np.ascontiguousarray(wide[:, 40:40 + w]))]


FB_HOSTILE_SIZES = [(130, 66), (257, 255)]
FB_HOSTILE_PARAMS = [("winsize63", {"winsize": 63}), ("winsize3", {"winsize": 3}),
                     ("pyr08_levels12", {"pyr_scale": 0.8, "levels": 12})]
