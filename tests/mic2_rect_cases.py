"""Inputs of the rectilinear 2-D marker tests, shared by tests/test_mic2_rect_model.py (CPU: oracle against the plain model)
and tests/test_hip_mic_resident_rect.py (GPU: the resident stage kernels against the oracle).  Plain helper module.

Grids: cell widths linspace(1, 4, n-1) * uniform(0.8, 1.25), cumulated, scaled to L, last node = L exactly; one seed per axis.
Shapes: the smallest that reach every path of the tile division of k_scatter_binned (8 x 32 sort cells per workgroup):
    19x39   18 x 38 cells: row tiles of 8, 8, 2, column tiles of 32, 6
    11x69   10 x 68 cells: column tiles of 32, 32, 4 -- a middle tile whose window ring overlaps both neighbours
    5x5     the smallest grid: one partial tile, every cell against a wall
"""
import functools

import numpy as np

TR_RHO, TR_ETA, TR_MRK, TR_TMP, TR_HCD, TR_HCP, TR_RH0, TR_ALP, TR_MAT, TR_ACE, TR_ET0, TR_IHT, TR__ID = range(13)

SHAPES = {"19x39": ([19, 39], [540e3, 1140e3], (1901, 3901)),
          "11x69": ([11, 69], [300e3, 2040e3], (1101, 6901)),
          "5x5": ([5, 5], [400e3, 500e3], (501, 502))}

# [19, 39]: cells with a given number of tracers -- runs that are cut at 8 lanes, runs that end on a cut, a cell that spans two
# 256-lane trips of its tile row (the row of column tile 1 then holds 5 x 16 + 300 tracers: the last trip has invalid lanes)
NAMED = {(3, 5): 0, (5, 12): 1, (8, 31): 7, (7, 32): 8, (12, 20): 9, (16, 33): 17, (10, 34): 300,
         (0, 0): 0, (17, 37): 0}                        # the two corner cells: NaN at a corner node
HOLE = (slice(13, 16), slice(24, 27))                   # 3 x 3 empty cells: NaN nodes in all four target sets


def axis(n, L, seed):
    rng = np.random.default_rng(seed)
    c = np.concatenate([[0.0], np.cumsum(np.linspace(1, 4, n - 1) * rng.uniform(0.8, 1.25, n - 1))])
    c *= L / c[-1]
    c[-1] = L
    return c


def shape(name):
    """(nx, L, [gz, gx])"""
    nx, L, seeds = SHAPES[name]
    return nx, L, [axis(nx[d], L[d], seeds[d]) for d in range(2)]


def search_cells(grid, X):
    """Linear sort cell of every tracer: per axis the largest i with c[i] <= x, clamped into the grid."""
    ci = np.clip(np.searchsorted(grid[0], X[:, 0], "right") - 1, 0, grid[0].size - 2)
    cj = np.clip(np.searchsorted(grid[1], X[:, 1], "right") - 1, 0, grid[1].size - 2)
    return ci * (grid[1].size - 1) + cj


def regular_cells(grid, X):
    """The cell the regular-grid formula floor((n - 1) x / L) gives."""
    n = [grid[0].size, grid[1].size]
    ci = np.clip(np.floor((n[0] - 1) * X[:, 0] / grid[0][-1]), 0, n[0] - 2).astype(np.int64)
    cj = np.clip(np.floor((n[1] - 1) * X[:, 1] / grid[1][-1]), 0, n[1] - 2).astype(np.int64)
    return ci * (n[1] - 1) + cj


def share_off_regular(grid, X):
    return float(np.mean(search_cells(grid, X) != regular_cells(grid, X)))


def census_of(grid, X):
    ncz, ncx = grid[0].size - 1, grid[1].size - 1
    return np.bincount(search_cells(grid, X), minlength=ncz * ncx).reshape(ncz, ncx)


def counts(name, rng, empties=True):
    """Tracers per cell: 16, on 19x39 the named cells and -- empties -- about 5 % empty cells and the 3 x 3 hole."""
    nx = SHAPES[name][0]
    cnt = np.full((nx[0] - 1, nx[1] - 1), 16, dtype=np.int64)
    if name != "19x39":
        return cnt
    if empties:
        cnt[rng.random(cnt.shape) < 0.05] = 0
        cnt[HOLE] = 0
    for cell, m in NAMED.items():
        if m > 0 or empties:
            cnt[cell] = m
    return cnt


def populate(grid, cnt, rng):
    """cnt[i, j] tracers strictly inside the GRADED cell (i, j), in shuffled order."""
    ci, cj = np.nonzero(cnt)
    rep = cnt[ci, cj]
    i = np.repeat(ci, rep); j = np.repeat(cj, rep)
    hz = np.diff(grid[0]); hx = np.diff(grid[1])
    X = np.stack([grid[0][i] + rng.uniform(0.01, 0.99, i.size) * hz[i], grid[1][j] + rng.uniform(0.01, 0.99, j.size) * hx[j]], axis=1)
    return X[rng.permutation(X.shape[0])]


def columns(X, L, rng):
    n = X.shape[0]
    return {TR_RH0: rng.uniform(3200, 3400, n), TR_ET0: 10 ** rng.uniform(19, 22, n), TR_HCP: rng.uniform(1000, 1300, n),
            TR_HCD: rng.uniform(2, 5, n), TR_TMP: 273 + 1350 * X[:, 0] / L[0] + rng.uniform(-30, 30, n),
            TR_IHT: 1e-11 * rng.uniform(0.5, 2, n), TR_MAT: np.round(rng.uniform(0, 3, n))}


def tracer_fields(X, cols):
    F = np.zeros((X.shape[0], 13))
    F[:, TR__ID] = np.arange(X.shape[0])
    for k, v in cols.items():
        F[:, k] = v
    return F


def base(name, seed, empties=True):
    """(nx, L, grid, X, F) of a shape's base population."""
    nx, L, grid = shape(name)
    rng = np.random.default_rng(seed)
    X = populate(grid, counts(name, rng, empties), rng)
    return nx, L, grid, X, tracer_fields(X, columns(X, L, rng))


def targets(grid):
    """The four target node sets of a step: midpoints with the one extrapolated entry of pylamp2.py:92-95."""
    gmp = []
    for g in grid:
        m = (g[1:] + g[:-1]) / 2
        gmp.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return {"nodes": grid, "centres": gmp, "zmid": [gmp[0], grid[1]], "xmid": [grid[0], gmp[1]]}


def padded_centres(grid):
    """The (n + 1)-entry centre grids of the advection velocities (pylamp2.py:491-545)."""
    gmp = targets(grid)["centres"]
    return [np.insert(m, 0, m[0] - (m[1] - m[0])) for m in gmp]


def line_tracers(grid, rng, last=True):
    """19x39: tracers EXACTLY on node lines (tile rims: cell row 8, cell column 32, and others), on centre lines (the node lines
    of the staggered sets), on the walls z = 0, x = 0 and -- last -- on z = L, x = L (last cell, a = 1)."""
    gz, gx = grid
    mz, mx = targets(grid)["centres"]
    Lz, Lx = gz[-1], gx[-1]

    def fz(): return gz[rng.integers(0, gz.size - 1)] + rng.uniform(0.05, 0.95) * 1e3
    def fx(): return gx[rng.integers(0, gx.size - 1)] + rng.uniform(0.05, 0.95) * 1e3
    pts = []
    for i in (3, 8, 16, 17):
        pts += [(gz[i], fx()), (gz[i], fx())]
    for j in (5, 31, 32, 33):
        pts += [(fz(), gx[j]), (fz(), gx[j])]
    pts += [(gz[8], gx[32]), (gz[16], gx[32]), (gz[8], gx[5]), (gz[1], gx[37])]
    for i in (0, 7, 8, 15, 17):
        pts += [(mz[i], fx())]
    for j in (0, 31, 32, 37):
        pts += [(fz(), mx[j])]
    pts += [(mz[7], mx[31]), (mz[8], mx[32]), (gz[8], mx[32]), (mz[8], gx[32])]
    pts += [(0.0, fx()), (0.0, fx()), (fz(), 0.0), (fz(), 0.0), (0.0, 0.0), (0.0, gx[32]), (gz[8], 0.0), (0.0, mx[5]), (mz[3], 0.0)]
    if last:
        pts += [(Lz, fx()), (Lz, fx()), (fz(), Lx), (fz(), Lx), (Lz, Lx), (Lz, 0.0), (0.0, Lx), (Lz, gx[32]), (gz[8], Lx), (Lz, mx[33]), (mz[16], Lx)]
    return np.array(pts)


def outside_tracers(grid, rng, n=300):
    """About n tracers up to 2.5 end-cell widths beyond the walls: every side, and the corners."""
    gz, gx = grid
    h = [(gz[1] - gz[0], gz[-1] - gz[-2]), (gx[1] - gx[0], gx[-1] - gx[-2])]
    L = [gz[-1], gx[-1]]

    def beyond(d, side, m):
        return -2.5 * h[d][0] * rng.random(m) if side == 0 else L[d] + 2.5 * h[d][1] * rng.random(m)
    m = n // 6                      # 4 sides of m and 4 corners of m / 2
    parts = []
    for side in (0, 1):
        parts.append(np.stack([beyond(0, side, m), L[1] * rng.random(m)], 1))
        parts.append(np.stack([L[0] * rng.random(m), beyond(1, side, m)], 1))
        for side2 in (0, 1):
            parts.append(np.stack([beyond(0, side, m // 2), beyond(1, side2, m // 2)], 1))
    return np.concatenate(parts)


def with_extra(X, L, extra, rng):
    """(X, F) of the base positions plus `extra`, shuffled together."""
    X = np.concatenate([X, extra])
    X = X[rng.permutation(X.shape[0])]
    return X, tracer_fields(X, columns(X, L, rng))


@functools.lru_cache(maxsize=None)
def case(name):
    """(nx, L, grid, X, F), built once and read-only:
         19x39 | 11x69 | 5x5   base populations                19x39-full   no empty cells (every node has a tracer in reach)
         lines                 19x39 + the tracers on lines    lines-inside the same without the tracers on z = L / x = L
         outside               19x39 + the tracers beyond the walls"""
    if name in SHAPES:
        out = base(name, 7)
    elif name == "19x39-full":
        out = base("19x39", 8, empties=False)
    else:
        nx, L, grid, X, _ = base("19x39", 7)
        rng = np.random.default_rng(9)
        extra = outside_tracers(grid, rng) if name == "outside" else line_tracers(grid, rng, last=(name == "lines"))
        out = (nx, L, grid) + with_extra(X, L, extra, rng)
    for a in list(out[2]) + [out[3], out[4]]:
        a.setflags(write=False)
    return out


def velocities(grid, rng, cells=1.5):
    """(Vz, Vx, dt): smooth + 10 % noise on the padded centre grid; the largest displacement dt max|V| is `cells` of the SMALLEST
    cell, so that stages of tracers near the walls leave the grid."""
    gzp, gxp = padded_centres(grid)
    Lz, Lx = grid[0][-1], grid[1][-1]
    Z, X = np.meshgrid(gzp, gxp, indexing="ij")
    Vz = 1e-9 * (np.cos(np.pi * Z / Lz) * np.sin(2 * np.pi * X / Lx) + 0.1 * rng.standard_normal(Z.shape))
    Vx = 1e-9 * (np.sin(2 * np.pi * Z / Lz) * np.cos(np.pi * X / Lx) + 0.1 * rng.standard_normal(Z.shape))
    hmin = min(np.diff(grid[0]).min(), np.diff(grid[1]).min())
    dt = cells * hmin / max(np.abs(Vz).max(), np.abs(Vx).max())
    return Vz, Vx, dt
