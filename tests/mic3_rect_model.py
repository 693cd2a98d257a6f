"""Float64 NumPy model of the 3-D marker-in-cell operations in SEARCH mode (rectilinear grids); plain helper module, no fixtures,
no project code.

The cell rule, per axis, for strictly increasing coordinates c[0..n-1] with end spacings h0 = c[1] - c[0], h1 = c[n-1] - c[n-2]:

  * c[0] <= p < c[n-1]:  the i with c[i] <= p < c[i+1], by exact comparisons (np.searchsorted(c, p, side='right') - 1);
  * p < c[0]:            floor((p - c[0]) / h0), negative: the auto-extended node set of mic3_model.ext_coord;
  * p >= c[n-1]:         n - 1 + floor((p - c[n-1]) / h1);
  * NaN:                 far below the set (outside for a gather, dropped by a scatter, cell 0 for the sort).

Everything downstream of the cell is the regular-grid model's: the functions below are the bodies of tests/mic3_model.py and
tests/mic3_refill_model.py evaluated with this cell function in place of floor((n-1)(x-x0)/L).  In particular the subgrid time
scale of temp_to_tracers keeps the mean spacing L / (n - 1).
"""
import contextlib

import numpy as np

import mic3_model as _U
import mic3_refill_model as _R

NAN_CELL = -(1 << 40)


def cell(c, x):
    c = np.asarray(c, dtype=np.float64); x = np.asarray(x, dtype=np.float64)
    n = c.size
    out = (np.searchsorted(c, x, side="right") - 1).astype(np.int64)
    nan = np.isnan(x)
    lo = x < c[0]
    hi = x >= c[-1]
    with np.errstate(invalid="ignore"):
        out[lo] = np.floor((x[lo] - c[0]) / (c[1] - c[0])).astype(np.int64)
        big = np.clip(np.floor((x[hi] - c[-1]) / (c[-1] - c[-2])), 0, 2.0 ** 40)
    out[hi] = n - 1 + big.astype(np.int64)
    out[nan] = NAN_CELL
    return out


def cells_of(tr_x, grid):
    """(linear sort cell, [i, j, k]): the rule's cell clamped into 0..n-2 per axis."""
    idx = [np.clip(cell(grid[d], tr_x[:, d]), 0, len(grid[d]) - 2) for d in range(3)]
    ncx, ncy = len(grid[1]) - 1, len(grid[2]) - 1
    return (idx[0] * ncx + idx[1]) * ncy + idx[2], idx


@contextlib.contextmanager
def _search():
    old = _U.cell, _R.cells_of
    _U.cell, _R.cells_of = cell, cells_of
    try:
        yield
    finally:
        _U.cell, _R.cells_of = old


def _searching(fn):
    def run(*a, **kw):
        with _search():
            return fn(*a, **kw)
    run.__doc__ = fn.__doc__
    return run


trac2grid = _searching(_U.trac2grid)
grid2trac = _searching(_U.grid2trac)
veldiv = _searching(_U.veldiv)
rk4 = _searching(_U.rk4)
temp_to_tracers = _searching(_U.temp_to_tracers)
refill = _searching(_R.refill)
locate = _searching(_U._locate)


def graded(n, L, ratio, origin=0.0):
    """n coordinates from origin to origin + L whose spacings grow smoothly (geometrically) by `ratio` from first to last."""
    h = float(ratio) ** np.linspace(0.0, 1.0, n - 1)
    c = np.concatenate([[0.0], np.cumsum(h)])
    c = origin + c * (L / c[-1])
    c[-1] = origin + L
    return c


def refined(n, L, ratio):
    """Fine at both ends, coarse in the middle (spacing ratio `ratio`), smoothly."""
    s = np.linspace(-1.0, 1.0, n - 1)
    h = float(ratio) ** (1.0 - s * s)
    c = np.concatenate([[0.0], np.cumsum(h)])
    c = c * (L / c[-1])
    c[-1] = L
    return c
