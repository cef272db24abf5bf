"""The post kernels (k_pass1 / k_pass1_final, k_strip_sums / k_radial_final, ffl_div_at, the importing loader) against the exact
references of tests/post_ref.py, at the sizes the library ships for and at sizes chosen against the kernels' constants, on
fields built to go wrong: winners planted on every kind of edge, exact ties across lanes / strips / row groups / workgroups /
final-loop trips, NaN and infinities, sums that cancel, magnitudes from float32 denormals to 1e4, and every bit pattern of
float16 and bfloat16.  Nothing here is compared with a tolerance that was not derived (post_ref's docstring)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import oracle as orc
import post_ref as pr
from funscript_flow_amd import _capi
from funscript_flow_amd.synth import sine_translate_frames

DEV = "cuda:0"
LARGE = [(1920, 1080), (3840, 2160), (2880, 2880), (5760, 2880)]
# widths on the edges of pass 1's 126-pixel strips and pass 2's 128-pixel strips, heights around the 16-row groups, a
# tall-thin and a wide-flat field, the smallest size ffl_create accepts
AWKWARD = [(126, 16), (127, 17), (252, 31), (253, 33), (128, 33), (129, 31), (24, 515), (1021, 18), (16, 16)]
GEOMS = LARGE + AWKWARD
A = np.float32(2.75)     # the planted bump: A / 2 + A / 2 is exact


def gid(g):
    return f"{g[0]}x{g[1]}"


def context(w, h, mb=None):
    mb = mb or (8 if w * h <= 1920 * 1080 else 5)
    return _capi.Context(w, h, max_batch=mb, frame_slots=2, flow_slots=2 * mb)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def batches(ctx, n, make):
    """import the fields make(0) .. make(n - 1) (host float32 (H, W, 2) arrays) max_batch at a time through import_flows;
    yields (index, field, slot, record) while the slot still holds the field"""
    mb = ctx.max_batch
    for i0 in range(0, n, mb):
        chunk = [make(i) for i in range(i0, min(i0 + mb, n))]
        slots = list(range(len(chunk)))
        ctx.import_flows(dev(np.stack(chunk)), slots)
        for j, rec in enumerate(ctx.pass1_results(slots)):
            yield i0 + j, chunk[j], slots[j], rec


def check_argmax(rec, flow, where=None):
    x, y, v = rec[:3]
    rx, ry, rv = pr.argmax_ref(flow)
    if where is not None:
        assert (rx, ry) == where, f"generator: reference winner {(rx, ry)} is not the planted {where}"
    assert (x, y) == (rx, ry), f"argmax {(x, y)} != reference {(rx, ry)} ({flow.shape[1]}x{flow.shape[0]})"
    if math.isnan(rv):
        assert math.isnan(float(v))     # not the bits: x86 and the device differ in the default NaN's sign
    else:
        assert np.float32(v).tobytes() == np.float32(rv).tobytes(), (float(v), float(rv))


def check_cut(ctx, slot, mm):
    """cut = float32 mean > threshold, for thresholds just below, at and just above the float32 mean"""
    mm = np.float32(mm)
    if math.isnan(float(mm)):
        for thr in (-1.0, 0.0, 7.0, float("inf")):
            assert ctx.pass1_result(slot, thr)[4] is False
        return
    lo, hi = np.nextafter(mm, np.float32(-np.inf)), np.nextafter(mm, np.float32(np.inf))
    assert ctx.pass1_result(slot, float(lo))[4] is (bool(mm > lo))
    assert ctx.pass1_result(slot, float(mm))[4] is False
    assert ctx.pass1_result(slot, float(hi))[4] is False


def same_by_upload(ctx, flow, rec, pov=False):
    """upload_flow of the same field gives the same record (the two share ffl_pass1_body)"""
    s = ctx.flow_slots - 1
    ctx.upload_flow(s, flow, pov)
    up = ctx.pass1_result(s)
    assert repr(up) == repr(rec), (up, rec)     # repr: NaN records compare equal


# ---- generators ---------------------------------------------------------------------------------------------------------
def background(w, h, seed, amp=0.01):
    """smooth, low amplitude: |div| stays below 1e-3"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float32)
    ph = rng.uniform(0, 6.28, 4).astype(np.float32)
    f = np.empty((h, w, 2), np.float32)
    f[..., 0] = amp * np.sin(x * np.float32(0.011) + ph[0]) * np.cos(y * np.float32(0.017) + ph[1])
    f[..., 1] = amp * np.cos(x * np.float32(0.013) + ph[2]) * np.sin(y * np.float32(0.007) + ph[3])
    return f


def plant(f, x, y, a=A):
    """make div(x, y) = du/dy + dv/dx jump by at least `a` by moving one vertical neighbour's u and one horizontal neighbour's
    v (the neighbour towards the middle of the image, so that the other pixel each of them touches is an interior one and
    moves by a / 2 only).  The two moved values share no other pixel's stencil."""
    h, w, _ = f.shape
    if y < h // 2:
        f[y + 1, x, 0] += a
    else:
        f[y - 1, x, 0] -= a
    if x < w // 2:
        f[y, x + 1, 1] += a
    else:
        f[y, x - 1, 1] -= a


def first_pixel_of_block(w, h, b):
    """a pixel owned by wave 4 * b of k_pass1, i.e. whose partial lands in slot b of k_pass1_final's loop"""
    nstrips = -(-w // pr.P1_STRIP)
    grp, strip = divmod(4 * b, nstrips)
    x, y = min(strip * pr.P1_STRIP + 5, w - 1), min(grp * pr.ROW_GROUP + 3, h - 1)
    assert pr.pass1_block_of(w, x, y) == b
    return x, y


def winner_pixels(w, h):
    px = {"tl": (0, 0), "tr": (w - 1, 0), "bl": (0, h - 1), "last": (w - 1, h - 1),
          "top": (w // 2, 0), "bottom": (w // 2, h - 1), "left": (0, h // 2), "right": (w - 1, h // 2),
          "rg_last_row": (min(7, w - 1), 15), "interior": (w // 3, h // 3)}
    if h > 16:
        px["rg_first_row"] = (min(9, w - 1), 16)
    for x in (125, 126, 127, 251, 252):
        if x < w:
            px[f"x{x}"] = (x, h // 2 + 1)
    nblk = pr.pass1_blocks(w, h)
    for b in (255, 256, nblk - 1):
        if 0 < b < nblk:
            px[f"slot{b}"] = first_pixel_of_block(w, h, b)
    return px


def tie_sets(w, h):
    """lists of (x, y, sign): interior pixels at least 3 apart in x or y whose |div| is exactly A"""
    a, b, c, d, m = (2, 2), (w - 3, 2), (2, h - 3), (w - 3, h - 3), (w // 2, h // 2)
    sets = [[a, b, c, d, m], [b, c], [c, b], [m, c], [d, m], [(b[0], 3), (2, 6)]]   # later row with the smaller x loses
    signed = [[(*b, 1), (*c, -1)], [(*b, -1), (*c, 1)], [(*m, -1), (*d, 1)]]
    if w > 270 and h > 50:
        sets += [[(10, 5), (50, 5)],                       # two lanes of one wave
                 [(120, 20), (130, 20), (260, 20)],        # three strips of one row
                 [(260, 20), (130, 21), (120, 22)],        # ... and against the strip order
                 [(125, 40), (126, 44)], [(126, 40), (125, 44)]]
    nblk = pr.pass1_blocks(w, h)
    if nblk > 257:   # one tying pixel per trip of the final loop, listed against their order
        p = [first_pixel_of_block(w, h, k) for k in (nblk - 1, 256, 255, 3)]
        sets += [p, p[:2], p[1:3], [p[0], p[2]]]
        signed += [[(*p[0], 1), (*p[3], -1)], [(*p[1], -1), (*p[2], 1)]]
    return [[(x, y, 1) for x, y in s] for s in sets] + signed


def tie_field(w, h, pixels, seed):
    """constant background with low-amplitude noise that keeps clear of the planted stencils, so every planted |div| is A"""
    rng = np.random.default_rng(seed)
    f = (rng.standard_normal((h, w, 2)) * 0.01).astype(np.float32)
    for x, y, _ in pixels:
        f[max(y - 4, 0):y + 5, max(x - 4, 0):x + 5] = 0
    f += np.float32(0.5)
    for x, y, s in pixels:
        plant(f, x, y, A * np.float32(s))
    return f


# ---- argmax -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_planted_winner(geom):
    w, h = geom
    px = winner_pixels(w, h)
    base = background(w, h, seed=w + h)
    names = list(px)

    def make(i):
        f = base.copy()
        plant(f, *px[names[i]])
        return f

    with context(w, h) as ctx:
        for i, f, slot, rec in batches(ctx, len(names), make):
            check_argmax(rec, f, px[names[i]])
            if i % ctx.max_batch == 0:
                pr.check_mean_mag(rec[3], f)
                same_by_upload(ctx, f, rec)


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_ties_first_in_c_order_wins(geom):
    w, h = geom
    sets = tie_sets(w, h)
    zero = np.zeros((h, w, 2), np.float32)
    mixed = zero.copy()
    mixed[::2, 1::3] = -0.0
    zeros = [zero, -zero, mixed]            # +-0 everywhere: every |div| ties at 0 and index 0 wins

    def make(i):
        return tie_field(w, h, sets[i], seed=i) if i < len(sets) else zeros[i - len(sets)]

    with context(w, h) as ctx:
        for i, f, slot, rec in batches(ctx, len(sets) + 3, make):
            if i < len(sets):
                first = min(sets[i], key=lambda p: p[1] * w + p[0])
                check_argmax(rec, f, first[:2])
                assert abs(float(rec[2])) == float(A)
            else:
                check_argmax(rec, f, (0, 0))
                assert float(rec[2]) == 0.0 and float(rec[3]) == 0.0
                check_cut(ctx, slot, rec[3])
            if i % ctx.max_batch == 1:
                same_by_upload(ctx, f, rec)


def nonfinite_fields(w, h):
    rng = np.random.default_rng(w * 7 + h)
    base = (rng.standard_normal((h, w, 2)) * 2.5).astype(np.float32)
    ye, xe, yl, xl = 3, min(5, w - 3), h - 4, w - 3          # an early and a late pixel
    out = {}
    f = base.copy(); f[h // 2, w // 2, 0] = np.nan; out["one_nan"] = f
    f = base.copy(); bits(f)[ye, xe, 0] = 0x7FC00001; bits(f)[yl, xl, 1] = 0xFFFFFFFF; out["later_payload_larger"] = f
    f = base.copy(); f[ye - 1, xe, 0] = np.inf; f[ye + 1, xe, 0] = np.inf; bits(f)[yl, xl, 1] = 0x7FFF0000
    out["inf_minus_inf_then_input_nan"] = f
    f = base.copy(); f[h // 2, w // 2, 1] = np.inf; out["plus_inf"] = f
    f = base.copy(); f[h // 2, w // 2, 0] = -np.inf; out["minus_inf"] = f
    f = base.copy(); f[h - 1, w - 1, 0] = np.nan; out["nan_last_pixel"] = f
    out["all_nan"] = np.full((h, w, 2), np.nan, np.float32)
    return out


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_non_finite_fields(geom):
    """np.argmax's rule: the first NaN of |div| in C order whatever its payload, else the first maximum (+inf included).  A
    NaN field has a NaN mean magnitude, is never a cut, and its radial value is NaN -- or exactly 0.0 when called as a cut."""
    w, h = geom
    named = nonfinite_fields(w, h)
    fields = list(named.values())
    centre = (0.37 * w + 0.25, 0.41 * h + 0.5)
    with context(w, h) as ctx:
        for i, f, slot, rec in batches(ctx, len(fields), fields.__getitem__):
            name = list(named)[i]
            check_argmax(rec, f)
            mean = pr.check_mean_mag(rec[3], f)
            has_nan = bool(np.isnan(f).any())
            assert math.isnan(float(rec[2])) == (name not in ("plus_inf", "minus_inf")), name
            assert math.isnan(mean) == has_nan and (has_nan or mean == math.inf)
            if has_nan:
                check_cut(ctx, slot, rec[3])
            assert rec[4] is (not has_nan)          # inf > 7.0; NaN > 7.0 is false
            for pov in (False, True):
                got = ctx.radial([slot, slot], [centre, centre], [False, True], pov)
                pr.check_radial(got[0], f, centre, pov)
                assert math.isnan(got[0]) == has_nan, (name, got)
                assert got[1] == 0.0
            same_by_upload(ctx, f, rec)
        # the same payload case through a bfloat16 import: an early NaN 0x7FC1, a late one 0x7FFF
        finite = named["one_nan"].copy()
        finite[h // 2, w // 2, 0] = 1.0
        t = dev(finite).bfloat16()
        raw = t.view(torch.int16)
        raw[3, min(5, w - 3), 0] = 0x7FC1
        raw[h - 4, w - 3, 1] = 0x7FFF
        wide = t.float().cpu().numpy()
        assert np.isnan(wide).sum() == 2
        ctx.import_flows(t, [0])
        rec = ctx.pass1_result(0)
        check_argmax(rec, wide)
        assert (rec[0], rec[1]) == (min(5, w - 3), 2) and math.isnan(float(rec[3])) and rec[4] is False
        same_by_upload(ctx, wide, rec)


# ---- sums ---------------------------------------------------------------------------------------------------------------
def centres(w, h):
    return {"fractional": (0.37 * w + 0.25, 0.41 * h + 0.5), "integer": (float(w // 3), float(h // 4)), "origin": (0.0, 0.0),
            "last": (w - 1.0, h - 1.0), "outside_neg": (-7.5, -3.25), "outside_pos": (w + 4.5, h + 9.0),
            "bottom_row": (float(w // 2), h - 1.0), "strip_edge": (float(min(128, w - 1)), float(min(16, h - 1))),
            "strip_last": (float(min(127, w - 2)), 15.0)}


def cancelling_field(w, h, centre, seed):
    """terms t(x, y) = -t(w - 1 - x, y) to float32 precision: u = t / (dx * wx * wy), v = 0, plus a residue far below the
    terms.  The generator is checked by the test: |sum| <= 1e-5 * sum |term|."""
    rng = np.random.default_rng(seed)
    t = rng.standard_normal((h, w))
    t = t - t[:, ::-1]
    t[:, 0] = t[:, -1] = t[0, :] = 0.0          # where a weight is 0 no u can carry the term: drop it on both sides
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    wx = np.where(x > centre[0], (w - x) / w, x / w)
    wy = np.where(y > centre[1], (h - y) / h, y / h)
    den = (x - centre[0]) * wx * wy
    f = np.zeros((h, w, 2), np.float32)
    with np.errstate(all="ignore"):
        f[..., 0] = np.where(den != 0, t / den, 0.0)
    f[..., 1] = np.float32(1e-9)
    return f


def spanning_field(w, h, seed):
    """magnitudes from 1e-30 to 1e4 with random directions; a sprinkling of float32 denormals and of -0"""
    rng = np.random.default_rng(seed)
    mag = 10.0 ** rng.uniform(-30, 4, (h, w))
    ang = rng.uniform(0, 2 * np.pi, (h, w))
    f = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(np.float32)
    f[::3, ::5, 0] = np.float32(1e-40)
    f[1::3, 2::5, 1] = np.float32(-1.4e-45)
    f[2::7, ::11] = -0.0
    return f


def sum_cases(w, h):
    """(name, field, [(centre, pov)]): everything at 1920x1080 and at the small sizes; at the three larger sizes (where one
    exact sum costs seconds of host time) every centre on the noise field and the centres that differ in kind elsewhere"""
    cs = centres(w, h)
    full = [(c, p) for p in (False, True) for c in cs.values()]
    big = w * h > 1920 * 1080
    some = [(cs[k], False) for k in ("fractional", "strip_edge", "last")] + [(cs["integer"], True)]
    cc = cs["fractional"]
    cases = [("randn2.5", (np.random.default_rng(w).standard_normal((h, w, 2)) * 2.5).astype(np.float32),
              [(c, False) for c in cs.values()] + [(cs[k], True) for k in ("fractional", "origin", "outside_pos")] if big else full),
             ("cancelling", cancelling_field(w, h, cc, seed=h), [(cc, False)] + (some[1:] if big else full)),
             ("spanning", spanning_field(w, h, seed=w + 1), some if big else full)]
    if (w, h) == (1920, 1080):
        fr = sine_translate_frames(2, w, h, seed=3)
        cases.append(("farneback", orc.farneback(fr[0], fr[1]), full))
    return cases


@pytest.mark.parametrize("geom", GEOMS, ids=gid)
def test_sums_within_derived_bound(geom, capsys):
    w, h = geom
    cases = sum_cases(w, h)
    worst = {}
    with context(w, h) as ctx:
        for i, f, slot, rec in batches(ctx, len(cases), lambda i: cases[i][1]):
            name, _, todo = cases[i]
            check_argmax(rec, f)
            pr.check_mean_mag(rec[3], f)
            check_cut(ctx, slot, rec[3])
            for pov in (False, True):
                cen = [c for c, p in todo if p == pov]
                if not cen:
                    continue
                got = ctx.radial([slot] * len(cen), cen, [False] * len(cen), pov)
                for c, g in zip(cen, got):
                    e, b = pr.check_radial(g, f, c, pov)
                    worst[name] = max(worst.get(name, 0.0), e)
            if name == "cancelling":
                want, S = pr.radial_exact(f, todo[0][0], False)
                assert abs(want) <= 1e-5 * S, f"generator: the field does not cancel ({want} against S = {S})"
            if name == "spanning":
                sq = f[..., 0] * f[..., 0]
                assert ((sq > 0) & (sq < 1.17e-38)).any() and pr.mag_terms(f).min() == 0.0   # denormal and flushed squares
                assert pr.mag_terms(f).max() > 1.0
            same_by_upload(ctx, f, rec)
    with capsys.disabled():
        print(f"\n  {w}x{h}: worst radial error in u*S {({k: round(v, 2) for k, v in worst.items()})}, "
              f"bound {8 + pr.radial_depth(w, h)}")


@pytest.mark.parametrize("geom", [(1920, 1080), (253, 33), (3840, 2160)], ids=gid)
def test_results_do_not_depend_on_batch_position(geom):
    """n = 1, 5, 32 fields per import_flows / radial call (5 at most above 1920x1080, the context's max_batch there): a field's
    record, radial value and slot bits are those of the same field alone"""
    w, h = geom
    rng = np.random.default_rng(11)
    kinds = [(rng.standard_normal((h, w, 2)) * 2.5).astype(np.float32), spanning_field(w, h, 5),
             tie_field(w, h, tie_sets(w, h)[0], 3), background(w, h, 2), nonfinite_fields(w, h)["one_nan"]]
    c = centres(w, h)["fractional"]
    with context(w, h, 32 if w * h <= 1920 * 1080 else 5) as ctx:
        alone = []
        for f in kinds:
            ctx.import_flows(dev(f), [0])
            alone.append((repr(ctx.pass1_result(0)), repr(ctx.radial([0], [c], [False])[0])))
            assert np.array_equal(bits(ctx.download_flow(0)), bits(f))
        for n in sorted({1, 5, ctx.max_batch}):
            order = [(3 * j + n) % len(kinds) for j in range(n)]
            slots = [(7 * j + 2) % (2 * ctx.max_batch) for j in range(n)]
            assert len(set(slots)) == n
            ctx.import_flows(dev(np.stack([kinds[k] for k in order])), slots)
            recs = ctx.pass1_results(slots)
            rad = ctx.radial(slots, [c] * n, [False] * n)
            for j, k in enumerate(order):
                assert (repr(recs[j]), repr(rad[j])) == alone[k], (n, j, k)
            assert np.array_equal(bits(ctx.download_flow(slots[-1])), bits(kinds[order[-1]]))


# ---- half precision, exhaustively ---------------------------------------------------------------------------------------
def all_patterns():
    """(128, 256, 2) int16: every 16-bit pattern once, scattered so that neighbours are unrelated values"""
    p = np.arange(65536, dtype=np.uint32)
    p = ((p * 40503) & 0xFFFF).astype(np.uint16)          # an odd multiplier: a permutation of 0..65535
    assert len(np.unique(p)) == 65536
    return p.reshape(128, 256, 2)


def widen(pat, dtype):
    """the exact float32 of each pattern: bfloat16 is the upper half of a float32; float16 through numpy"""
    if dtype == torch.bfloat16:
        return (pat.astype(np.uint32) << 16).view(np.float32)
    return pat.view(np.float16).astype(np.float32)


def layouts(t):
    """NHWC, NCHW planes, a padded row pitch, and a view with a pixel stride of four elements (element by element)"""
    n, h, w, _ = t.shape
    pad = torch.zeros((n, h + 3, w + 5, 2), dtype=t.dtype, device=t.device)
    pad[:, 2:2 + h, 1:1 + w] = t
    wide = torch.zeros((n, h, w, 4), dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    return {"nhwc": t, "nchw": t.permute(0, 3, 1, 2).contiguous(), "padded": pad[:, 2:2 + h, 1:1 + w], "strided": wide[..., ::2]}


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
def test_every_half_precision_pattern_widens_exactly(dtype):
    w, h = 256, 128
    pat = all_patterns()
    want = widen(pat, dtype)
    finite = np.isfinite(want)
    assert (~np.isnan(want)).sum() == 65536 - (2046 if dtype == torch.float16 else 254)
    # the second field: the non-finite patterns replaced by the pattern of 1.0
    pat2 = np.where(finite, pat, np.uint16(0x3C00 if dtype == torch.float16 else 0x3F80)).astype(np.uint16)
    want2 = widen(pat2, dtype)
    # both zeros and every denormal of the type are there (bfloat16's are float32 denormals, float16's widen to normals)
    tiny = (want2 != 0) & (np.abs(want2) < (2.0 ** -14 if dtype == torch.float16 else 2.0 ** -126))
    assert np.isfinite(want2).all() and (want2 == 0).sum() == 2 and tiny.sum() == (2046 if dtype == torch.float16 else 254)
    t = torch.from_numpy(np.stack([pat, pat2]).view(np.int16)).to(DEV).view(dtype)
    cs = centres(w, h)
    with _capi.Context(w, h, max_batch=2, frame_slots=2, flow_slots=8) as ctx:
        for name, view in layouts(t).items():
            ctx.import_flows(view, [0, 1])
            recs = ctx.pass1_results([0, 1])
            got, got2 = ctx.download_flow(0), ctx.download_flow(1)
            nan = np.isnan(want)
            assert np.array_equal(bits(got)[~nan], bits(want)[~nan]), name      # -0, denormals, the largest values, +-inf
            assert np.isnan(got[nan]).all(), name
            assert np.array_equal(bits(got2), bits(want2)), name
            # records: the field with NaN follows the non-finite rule, the finite one equals upload_flow's bit for bit
            check_argmax(recs[0], want)
            assert math.isnan(float(recs[0][3])) and recs[0][4] is False
            check_argmax(recs[1], want2)
            mean = pr.check_mean_mag(recs[1][3], want2)
            assert mean > 100          # float16's 65504 and bfloat16's 3.4e38 dominate: the sum spans the whole range
            ctx.upload_flow(4, want2)
            assert repr(ctx.pass1_result(4)) == repr(recs[1]), name
            for pov in (False, True):
                cen = list(cs.values())
                for c, g in zip(cen, ctx.radial([1] * len(cen), cen, [False] * len(cen), pov)):
                    pr.check_radial(g, want2, c, pov)
