"""numpy restatement of the per-cell statistics grid and the variance centre: rules G1-G6
in the stated orders, which ffl_cell_stats and ffl_radial_window_axes_centres are held to bit for bit, and the closed-form
fields the fixtures of tests/golden/grid_golden.npz were computed on.

Loops run over rows, columns and blocks -- the axes whose order the rules fix -- and are vectorised over the others.  Every
sum starts at +0.0.  Nothing here reads the reference; tests/gen_grid_golden.py compares this file with the real
center_of_mass_variance (FF:721-746) where the reference exists."""
import numpy as np

MAX_CELLS = 64    # FFL_MAX_CELLS
BLOCK = 256       # the column block of rule G3
CELL_FIELDS = ("mean_u", "mean_v", "mean_mag", "var_mag")


# ---- G1 ---------------------------------------------------------------------------------------------------------------
def geometry(w, h, G):
    """(gw, gh) of a G x G grid on a w x h field (FF:728); ValueError outside rule G1"""
    if not 1 <= G <= MAX_CELLS:
        raise ValueError(f"rule G1: cells = {G} outside 1..{MAX_CELLS}")
    if G > min(w, h):
        raise ValueError(f"rule G1: cells = {G} exceeds min(width, height) of {w}x{h}")
    return w // G, h // G


# ---- G2, G3 -----------------------------------------------------------------------------------------------------------
def magnitude(flow):
    """m = sqrtf(u*u + v*v), float32 throughout"""
    f = np.asarray(flow, np.float32)
    u, v = f[..., 0], f[..., 1]
    with np.errstate(all="ignore"):
        return np.sqrt(u * u + v * v)


def cell_sums(flow, G):
    """K float32[G, G] and the four float64[G, G] sums S_u, S_v, S_d, S_dd in rule G3's order"""
    f = np.asarray(flow, np.float32)
    h, w = f.shape[:2]
    gw, gh = geometry(w, h, G)
    wc, hc = G * gw, G * gh
    with np.errstate(all="ignore"):
        m = magnitude(f)[:hc, :wc]
        K = m[::gh, ::gw].copy()                                                  # [i, j]: the cell's top-left pixel
        d = m.astype(np.float64) - np.repeat(np.repeat(K, gh, axis=0), gw, axis=1).astype(np.float64)
        terms = [f[:hc, :wc, 0].astype(np.float64), f[:hc, :wc, 1].astype(np.float64), d, d * d]
        sums = []
        for t in terms:
            t = t.reshape(G, gh, wc)
            col = np.zeros((G, wc))
            for r in range(gh):                                                   # a column: top to bottom
                col = col + t[:, r, :]
            S = np.zeros((G, G))
            for j in range(G):
                cell = np.zeros(G)
                for blk in range(j * gw // BLOCK, ((j + 1) * gw - 1) // BLOCK + 1):   # ascending block order
                    part = np.zeros(G)
                    for x in range(max(j * gw, blk * BLOCK), min((j + 1) * gw, (blk + 1) * BLOCK)):   # left to right
                        part = part + col[:, x]
                    cell = cell + part
                S[:, j] = cell
            sums.append(S)
    return K, sums[0], sums[1], sums[2], sums[3]


# ---- G4 ---------------------------------------------------------------------------------------------------------------
def cell_records(flow, G):
    """float64[G, G, 4]: mean_u, mean_v, mean_mag, var_mag of every cell"""
    f = np.asarray(flow, np.float32)
    gw, gh = geometry(f.shape[1], f.shape[0], G)
    K, Su, Sv, Sd, Sdd = cell_sums(f, G)
    n = np.float64(gh * gw)
    with np.errstate(all="ignore"):
        var = (Sdd - Sd * Sd / n) / n
        var = np.where(var < 0.0, 0.0, var)                                       # a NaN stays a NaN
        return np.stack([Su / n, Sv / n, K.astype(np.float64) + Sd / n, var], axis=2)


# ---- G5 ---------------------------------------------------------------------------------------------------------------
def centre_of(var, w, h):
    """(cx, cy, T, empty) of a float64[G, G] variance grid on a w x h field"""
    var = np.asarray(var, np.float64)
    G = var.shape[0]
    gw, gh = geometry(w, h, G)
    with np.errstate(all="ignore"):
        t, xs = np.zeros(G), np.zeros(G)
        for j in range(G):                                                        # per cell row, over j in order
            t = t + var[:, j]
            xs = xs + np.float64(j) * var[:, j]
        T = X = Y = np.float64(0.0)
        for i in range(G):
            T = T + t[i]
            X = X + xs[i]
            Y = Y + np.float64(i) * t[i]
        if T == 0:
            return np.float64(w // 2), np.float64(h // 2), T, 1
        return X * gw / T + gw / 2.0, Y * gh / T + gh / 2.0, T, 0


def centre(flow, G):
    f = np.asarray(flow, np.float32)
    return centre_of(cell_records(f, G)[..., 3], f.shape[1], f.shape[0])


# ---- G6 ---------------------------------------------------------------------------------------------------------------
def window(centres, radius=6):
    """float64[n, 2]: the window means of rule G6 over n caller centres"""
    c = np.asarray(centres, np.float64).reshape(-1, 2)
    n = len(c)
    out = np.empty((n, 2))
    with np.errstate(all="ignore"):
        for j in range(n):
            acc, count = c[j].copy(), 1
            for i in range(1, radius + 1):
                if j - i >= 0:
                    acc = acc + c[j - i]
                    count += 1
                if j + i < n:
                    acc = acc + c[j + i]
                    count += 1
            out[j] = acc / np.float64(count)
    return out


# ---- the fixture fields: an integer hash -> float32, the same bytes under every numpy ---------------------------------------
def _unit(w, h, seed, salt):
    """float32[h, w] in [0, 1): 24 hashed bits per pixel, every value exact in float32"""
    y, x = np.mgrid[0:h, 0:w].astype(np.uint64)
    M = np.uint64(0xFFFFFFFF)
    v = (x * np.uint64(0x9E3779B1) + y * np.uint64(0x85EBCA77) + np.uint64(seed) * np.uint64(0xC2B2AE3D)
         + np.uint64(salt) * np.uint64(0x27D4EB2F) + np.uint64(0x165667B1)) & M
    v ^= v >> np.uint64(15)
    v = (v * np.uint64(0x2C1B3C6D)) & M
    v ^= v >> np.uint64(12)
    v = (v * np.uint64(0x297A2D39)) & M
    v ^= v >> np.uint64(15)
    return ((v >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def field(w, h, seed=0):
    """(h, w, 2) float32: a background of +-0.01 px, a patch of +-3 px noise in the lower left and a divergent blob (flow
    0.3 px per pixel away from its centre) in the upper right.  float32 products and sums only: closed form."""
    y, x = np.mgrid[0:h, 0:w]
    f = np.empty((h, w, 2), np.float32)
    half = np.float32(0.5)
    for c in range(2):
        f[..., c] = (_unit(w, h, seed, c) - half) * np.float32(0.02)
    patch = (x >= w // 8) & (x < w // 8 + max(1, w // 4)) & (y >= h // 2) & (y < h // 2 + max(1, h // 3))
    for c in range(2):
        f[..., c] += np.where(patch, (_unit(w, h, seed, 2 + c) - half) * np.float32(6.0), np.float32(0.0)).astype(np.float32)
    bx, by, r = (2 * w) // 3, h // 3, max(2, min(w, h) // 5)
    blob = (x - bx) ** 2 + (y - by) ** 2 < r * r
    f[..., 0] += np.where(blob, (x - bx).astype(np.float32) * np.float32(0.3), np.float32(0.0)).astype(np.float32)
    f[..., 1] += np.where(blob, (y - by).astype(np.float32) * np.float32(0.3), np.float32(0.0)).astype(np.float32)
    return f


# (w, h, G) of the fixtures: the six of the reference's operating range, then three whose cells cross a 256-column block
GOLDEN_CASES = [(64, 64, 32), (80, 48, 8), (53, 37, 5), (256, 256, 32), (192, 136, 32), (130, 33, 3),
                (300, 20, 3), (600, 16, 1), (520, 16, 2)]
CENTRE_BOUND = 1e-5   # px, against the real function's float32 np.var
