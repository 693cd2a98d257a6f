"""The 2-D Stokes stencil one launch at a time, exactly as pl_stokes_solve issues it (pl_stokes_apply_probe, pl_stokes_scale_rows):
the unscaled and the row-scaled operator at every row-block height, the add / coef operand of the lazy deflation correction and the
three reduction epilogues, against the oracle's explicit matrix and the row scales of tests/stokes2_scaled_model.py.

Grids are rectilinear in both axes (cell widths uniform random in 0.7 .. 1.3), viscosities random over three decades: on such a grid
every reciprocal-width table entry of the stencil differs from its neighbours, so a swapped table index changes the result.  The
shapes are the smallest at which each code path exists: a wave of the kernel covers 128 columns of a row, and the branch-free interior
path runs only for a wave whose 128 columns are all interior (at least 258 columns).

Bounds are the suite's existing ones: row-wise 1e-13 |A||x| for an operator application (tests/test_hip_parity.py), rtol 1e-14 for a
vector that is one product per entry (the rhs checks), 8 eps and SUM_TOL for the epilogues (tests/test_hip_krylov_fused.py), 1e-6 on
the velocities of a solve (tests/test_hip_solve.py).  Every test prints the margin it saw; the largest per check is printed when the
module is done."""
import ctypes as C

import numpy as np
import pytest

import stokes2_scaled_model as M
from test_hip_krylov_fused import EPS, SUM_TOL, _close          # noqa: F401  (SUM_TOL: the rule _close applies)
from test_hip_solve import VEL_TOL, _vel_err

pytestmark = pytest.mark.gpu

ROW_TOL = 1e-13
TSTEP, THETA = 3.0e11, 0.5                                       # oracle/gen_golden.py, the surface-stabilisation fixtures
COEF = -0.37
BCS = {"ffff": [1, 1, 1, 1], "nfnf": [0, 1, 0, 1], "nfff": [0, 1, 1, 1], "ffnf": [1, 1, 0, 1]}
PAIR_A, PAIR_B, ALL4 = ("ffff", "nfnf"), ("nfff", "ffnf"), ("ffff", "nfnf", "nfff", "ffnf")
SHAPES = [([5, 6], PAIR_A), ([7, 9], PAIR_B),                    # all rows wall or near-wall, the anchor (3, 2) included
          ([18, 127], PAIR_A), ([18, 128], PAIR_B), ([23, 129], PAIR_A), ([23, 130], PAIR_B),     # the edge of one wave
          ([23, 257], ALL4),                                     # control: no wave qualifies for the interior path
          ([23, 258], ALL4),                                     # exactly one interior wave
          ([35, 259], ALL4), ([5, 259], ALL4),                   # ... plus a one-column tail lane in the third block
          ([35, 386], ALL4)]                                     # two interior waves; 35 rows leave a remainder at every height
CASES = [(tuple(s), b) for s, bs in SHAPES for b in bs]
EPI_CASES = [(tuple(s), b) for s, bs in SHAPES if s in ([23, 130], [35, 259], [35, 386]) for b in bs]
_id = lambda c: "%dx%d-%s" % (c[0][0], c[0][1], c[1])

_cases = {}
_margins = {}


def _note(check, what, value):
    print("launch %-14s %-22s %.3e" % (check, what, value))
    _margins[check] = max(_margins.get(check, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for check in sorted(_margins):
        print("\nlargest margin %-14s %.3e" % (check, _margins[check]), end="")
    print()
    _cases.clear(); _margins.clear()
    from pylamp_amd import _context
    _context.clear_contexts()


def _nonuni(n, Ld, rng):
    w = rng.uniform(0.7, 1.3, n - 1); g = np.concatenate([[0.0], np.cumsum(w)]); return g * (Ld / g[-1])


def _build(shape, bcname, surfstab=False, nan_ghost=False):
    """One operator on the device and its reference, built once per (shape, walls, variant) and shared read-only by every test:
    the oracle's matrix A, the model's scales d, x, A x, |A||x|, and the vectors the operands and epilogues take."""
    key = (shape, bcname, surfstab, nan_ghost)
    if key in _cases:
        return _cases[key]
    from pylamp_amd import pylamp_stokes as S
    nx = list(shape); bc = BCS[bcname]
    grng = np.random.default_rng([nx[0], nx[1]])                 # one grid (one device context) per shape
    grid = [_nonuni(nx[d], 5e3 * (nx[d] - 1), grng) for d in range(2)]
    rng = np.random.default_rng([nx[0], nx[1], ALL4.index(bcname) + 1, int(surfstab), int(nan_ghost)])
    etas = 1e19 * 10 ** rng.uniform(0, 3, nx); etan = 1e19 * 10 ** rng.uniform(0, 3, nx)
    if nan_ghost:
        etan[:, -1] = np.nan                                     # empty ghost column (tests/test_hip_parity.py, the 513 x 257 case)
    rho = 3300 + rng.uniform(-50, 50, nx)
    kw = dict(surfstab=True, tstep=TSTEP, theta=THETA) if surfstab else {}
    A, d = M.scaled_system(nx, grid, etas, etan, rho, bc, **kw)
    op, _ = S.makeStokesMatrix(nx, grid, etas, etan, rho, bc, surfstab=surfstab, tstep=TSTEP if surfstab else None,
                               surfstab_theta=THETA)
    n = A.shape[0]
    x, v, add, s, rt, g = (rng.standard_normal(n) for _ in range(6))
    Ax = A @ x; absAx = abs(A) @ np.abs(x)
    assert np.isfinite(Ax).all() and np.isfinite(d).all() and np.all(absAx > 0)
    hz, hx = np.diff(grid[0]), np.diff(grid[1])
    wgt = np.zeros(nx); wgt[:-1, :-1] = hz[:, None] + hx[None, :]   # the deflation's left vector: (hz + hx) on the continuity rows,
    wgt[3, 2] = 0.0                                                  # i.e. every cell but the anchor and the four corner cells
    for i in (0, nx[0] - 2):
        for j in (0, nx[1] - 2):
            wgt[i, j] = 0.0
    c = dict(nx=nx, grid=grid, bc=bc, etas=etas, etan=etan, rho=rho, op=op, A=A, d=d, x=x, v=v, add=add, s=s, rt=rt, g=g, Ax=Ax,
             absAx=absAx, wgt=wgt,
             tag="%dx%d-%s" % (nx[0], nx[1], bcname))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _cases[key] = c
    return c


def _probe(c, scaled, mode, rows, x, a1=None, a2=None, add=None, coef=0.0, want_out2=False):
    from pylamp_amd import _lib
    op = c["op"]; op._activate()
    null = C.POINTER(C.c_double)()
    p = lambda a: _lib.dptr(a) if a is not None else null
    out = np.full(x.size, np.nan); out2 = np.full(x.size, np.nan) if want_out2 else None
    sums = np.full(8, np.nan)
    op._ctx.check(op._ctx.lib.pl_stokes_apply_probe(op._ctx.handle(), scaled, mode, rows, p(x), p(a1), p(a2), p(add), float(coef),
                                                    p(out), p(out2), p(sums)))
    return out, out2, sums


def _scale_rows(c, v):
    from pylamp_amd import _lib
    op = c["op"]; op._activate()
    out = np.full(v.size, np.nan)
    op._ctx.check(op._ctx.lib.pl_stokes_scale_rows(op._ctx.handle(), _lib.dptr(v), _lib.dptr(out)))
    return out


def _ratio(got, want, scale):
    """largest row-wise |got - want| / scale (NaN if anything is not finite, which no bound admits)"""
    if not np.isfinite(got).all():
        return float("nan")
    return float(np.max(np.abs(got - want) / np.maximum(scale, 1e-300)))


def _scaled_t(c):
    """the mode-0 launch of the scaled operator at the default height: what the epilogue launches must reproduce"""
    key = ("t", c["tag"])
    if key not in _cases:
        t = _probe(c, 1, 0, 0, c["x"])[0]; t.setflags(write=False)
        _cases[key] = t
    return _cases[key]


@pytest.mark.parametrize("rows", [2, 4, 8, 16])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_unscaled_launch_vs_matrix(case, rows):
    c = _build(*case)
    got = _probe(c, 0, 0, rows, c["x"])[0]
    r = _ratio(got, c["Ax"], c["absAx"])
    _note("unscaled", "%s rows %d" % (c["tag"], rows), r)
    assert r <= ROW_TOL


@pytest.mark.parametrize("rows", [2, 4, 8, 16])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_scaled_launch_vs_model(case, rows):
    """D_r A x: the stencil's inline reciprocals, the interior path's scales and the row classification in one go."""
    c = _build(*case)
    got = _probe(c, 1, 0, rows, c["x"])[0]
    r = _ratio(got, c["d"] * c["Ax"], c["d"] * c["absAx"])
    _note("scaled", "%s rows %d" % (c["tag"], rows), r)
    assert r <= ROW_TOL


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_scale_rows_vs_model(case):
    """The scaling the right-hand side gets (k_stokes_scale_rows): one product per entry."""
    c = _build(*case)
    got = _scale_rows(c, c["v"])
    want = c["d"] * c["v"]
    _note("scale_rows", c["tag"], _ratio(got, want, np.abs(want)))
    assert np.allclose(got, want, rtol=1e-14, atol=0)


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_scaled_launch_is_scale_rows_of_unscaled(case):
    """The solver scales b with one kernel and applies D_r A with another: both must mean the same D_r."""
    c = _build(*case)
    u = _probe(c, 0, 0, 0, c["x"])[0]
    t = _probe(c, 1, 0, 0, c["x"])[0]
    r = _ratio(t, _scale_rows(c, u), c["d"] * c["absAx"])
    _note("cross", c["tag"], r)
    assert r <= ROW_TOL


@pytest.mark.parametrize("mode", [0, 3])
@pytest.mark.parametrize("scaled", [0, 1], ids=["unscaled", "scaled"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_add_coef_operand(case, scaled, mode):
    """out = op(x) + coef add (the lazy deflation correction), added after the row scaling; under the residual epilogue
    out = b - (that) and out2 = that, and the sums see the corrected vector.  (The odd widths read add as scalars in the last lane.)
    The residual's own bound adds one rounding of the subtraction on the device and one in NumPy: eps |b - t|."""
    c = _build(*case)
    nx = c["nx"]
    dd = c["d"] if scaled else 1.0
    cadd = COEF * c["add"]
    want = dd * c["Ax"] + cadd
    scale = dd * c["absAx"] + np.abs(cadd)
    what = "%s %s mode %d" % (c["tag"], "scaled" if scaled else "unscaled", mode)
    if mode == 0:
        got = _probe(c, scaled, 0, 0, c["x"], add=c["add"], coef=COEF)[0]
        r = _ratio(got, want, scale)
        _note("add", what, r)
        assert r <= ROW_TOL
        return
    b = 0.5 * c["g"] * (dd * c["absAx"])                      # of each row's own magnitude, so that b - t cancels digits in every row
    res, t, sums = _probe(c, scaled, 3, 0, c["x"], a1=b, add=c["add"], coef=COEF, want_out2=True)
    r = _ratio(t, want, scale)
    _note("add", what, r)
    assert r <= ROW_TOL
    assert np.isfinite(res).all() and np.all(np.abs(res - (b - want)) <= ROW_TOL * scale + EPS * np.abs(b - want))
    r3 = res.reshape(nx[0], nx[1], 3)
    uv = c["x"].reshape(nx[0], nx[1], 3)[:, :, :2]
    for q, terms in enumerate([res * res, r3[:, :, 2] ** 2, b * b, uv * uv, c["wgt"] * r3[:, :, 2]]):
        assert _close(sums[q], np.sum(terms), terms), (q, sums[q], np.sum(terms))


@pytest.mark.parametrize("rows", [4, 16])
@pytest.mark.parametrize("mode", [1, 2, 3])
@pytest.mark.parametrize("case", EPI_CASES, ids=_id)
def test_epilogues_on_scaled_operator(case, mode, rows):
    """The reductions of the Krylov loop on the operator the loop runs on: the vectors are the mode-0 launch's (8 eps), every sum
    is NumPy's on those vectors (SUM_TOL) and the same bits on a second launch.  The weights of the deflation's sum (mode 3,
    sum 4) are the grid's own cell widths: on these grids no two are alike."""
    c = _build(*case)
    nx, x, s, rt = c["nx"], c["x"], c["s"], c["rt"]
    t = _scaled_t(c)
    what = "%s mode %d rows %d" % (c["tag"], mode, rows)
    if mode == 1:
        y, _, sums = _probe(c, 1, 1, rows, x, a1=rt)
        want = [rt * t]
        again = _probe(c, 1, 1, rows, x, a1=rt)[2]
    elif mode == 2:
        y, _, sums = _probe(c, 1, 2, rows, x, a1=s, a2=rt)
        cont = np.zeros(t.size, dtype=bool); cont[2::3] = True          # the continuity plane
        want = [t * s, t * t, rt * s, rt * t, s * s, (t * s)[cont], (t * t)[cont], (s * s)[cont]]
        again = _probe(c, 1, 2, rows, x, a1=s, a2=rt)[2]
    else:
        b = c["g"] * np.abs(t).mean()                                    # of the operator's magnitude, so that b - t cancels digits
        r, y, sums = _probe(c, 1, 3, rows, x, a1=b, a2=s, want_out2=True)
        assert np.all(np.abs(r - (b - t)) <= 8 * EPS * (np.abs(b) + np.abs(t)))
        r3 = r.reshape(nx[0], nx[1], 3)
        uv = (x + s).reshape(nx[0], nx[1], 3)[:, :, :2]
        want = [r * r, r3[:, :, 2] ** 2, b * b, uv * uv, c["wgt"] * r3[:, :, 2]]
        again = _probe(c, 1, 3, rows, x, a1=b, a2=s, want_out2=True)[2]
    _note("epi_vector", what, _ratio(y, t, np.abs(t)) / EPS)             # in units of eps
    assert np.all(np.abs(y - t) <= 8 * EPS * np.abs(t))
    for q, terms in enumerate(want):
        _note("epi_sum", "%s sum %d" % (what, q), abs(sums[q] - np.sum(terms)) / np.sum(np.abs(terms)))
        assert _close(sums[q], np.sum(terms), terms), (q, sums[q], np.sum(terms))
    assert np.isfinite(sums).all() and np.array_equal(sums, again)


@pytest.mark.parametrize("rows", [4, 16])
@pytest.mark.parametrize("scaled", [0, 1], ids=["unscaled", "scaled"])
def test_surface_stabilisation_at_interior_path_width(scaled, rows):
    """With the stabilisation on the interior path is off: the classified path at a width where the interior path would run.
    D_r leaves the stabilisation term out (tests/stokes2_scaled_model.py)."""
    c = _build((23, 258), "ffff", surfstab=True)
    dd = c["d"] if scaled else 1.0
    got = _probe(c, scaled, 0, rows, c["x"])[0]
    r = _ratio(got, dd * c["Ax"], dd * c["absAx"])
    _note("surfstab", "%s %s rows %d" % (c["tag"], "scaled" if scaled else "unscaled", rows), r)
    assert r <= ROW_TOL
    A0 = M.scaled_system(c["nx"], c["grid"], c["etas"], c["etan"], c["rho"], c["bc"])[0]
    assert abs(c["A"] - A0).max() > 0                               # the stabilisation terms are in the matrix that was compared


def test_empty_ghost_column_does_not_leak():
    """etan[:, -1] = NaN: the last column belongs to no cell.  Neither the scaled launch nor the sums of the epilogue may see it."""
    c = _build((23, 258), "nfff", nan_ghost=True)
    x, s, rt = c["x"], c["s"], c["rt"]
    want = c["d"] * c["Ax"]
    t = _probe(c, 1, 0, 0, x)[0]
    assert not np.isnan(t).any()
    r = _ratio(t, want, c["d"] * c["absAx"])
    _note("nan_ghost", c["tag"], r)
    assert r <= ROW_TOL
    y, _, sums = _probe(c, 1, 2, 0, x, a1=s, a2=rt)
    assert not np.isnan(y).any() and not np.isnan(sums).any()
    assert np.all(np.abs(y - t) <= 8 * EPS * np.abs(t))
    cont = np.zeros(t.size, dtype=bool); cont[2::3] = True
    for q, terms in enumerate([t * s, t * t, rt * s, rt * t, s * s, (t * s)[cont], (t * t)[cont], (s * s)[cont]]):
        assert _close(sums[q], np.sum(terms), terms), (q, sums[q], np.sum(terms))
    v = _scale_rows(c, c["v"])
    assert not np.isnan(v).any() and np.allclose(v, c["d"] * c["v"], rtol=1e-14, atol=0)


def test_entry_points_reject_bad_arguments_by_name():
    from pylamp_amd import _lib
    c = _build((7, 9), "nfff")
    op = c["op"]; op._activate()
    lib, h = op._ctx.lib, op._ctx.handle()
    x = c["x"]; out = np.empty_like(x); sums = np.zeros(8)
    null = C.POINTER(C.c_double)()
    X, O, SM = _lib.dptr(x), _lib.dptr(out), _lib.dptr(sums)
    for args, msg in [((2, 0, 0, X, null, null, null, 0.0, O, null, null), "scaled must be 0 or 1"),
                      ((1, 4, 0, X, null, null, null, 0.0, O, null, null), "mode must be 0, 1, 2 or 3"),
                      ((1, 0, 3, X, null, null, null, 0.0, O, null, null), "rows must be 0, 2, 4, 8 or 16 in mode 0"),
                      ((1, 2, 8, X, X, X, null, 0.0, O, null, SM), "rows must be 0, 4 or 16 in modes 1, 2 and 3"),
                      ((1, 0, 0, null, null, null, null, 0.0, O, null, null), "x is NULL"),
                      ((1, 0, 0, X, null, null, null, 0.0, null, null, null), "out is NULL"),
                      ((1, 1, 0, X, null, null, null, 0.0, O, null, SM), "aux1 is NULL"),
                      ((1, 2, 0, X, X, null, null, 0.0, O, null, SM), "aux2 is NULL"),
                      ((1, 3, 0, X, X, null, null, 0.0, O, null, null), "sums is NULL"),
                      ((1, 0, 0, X, null, null, X, float("nan"), O, null, null), "coef is NaN")]:
        with pytest.raises(Exception, match="pl_stokes_apply_probe: " + msg):
            op._ctx.check(lib.pl_stokes_apply_probe(h, *args))
    for args, msg in [((null, O), "v is NULL"), ((X, null), "out is NULL")]:
        with pytest.raises(Exception, match="pl_stokes_scale_rows: " + msg):
            op._ctx.check(lib.pl_stokes_scale_rows(h, *args))
    assert np.array_equal(_probe(c, 1, 0, 0, x)[0], _probe(c, 1, 0, 4, x)[0])      # and the context still works; 0 is height 4 here


def test_solve_rectilinear_wide_enough_for_interior_path(oracle):
    """66 x 259, rectilinear in both axes, no-slip top: the first solve whose operator takes the interior path on a non-uniform grid."""
    from pylamp_amd import pylamp_stokes as S
    nx = [66, 259]; bc = [0, 1, 1, 1]
    L = [660e3, 660e3 * (nx[1] - 1) / (nx[0] - 1)]
    rng = np.random.default_rng(4)
    grid = [_nonuni(nx[d], L[d], rng) for d in range(2)]
    Z, X = np.meshgrid(*grid, indexing='ij')
    Zc, Xc = np.meshgrid(*oracle.gridmp_of(grid), indexing='ij')
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / L[1]) * np.cos(np.pi * z / L[0]))
    es, en = f(Z, X), f(Zc, Xc)
    rho = 3300 + 40 * np.sin(2 * np.pi * X / L[1]) * np.sin(np.pi * Z / L[0])
    A, rhs = S.makeStokesMatrix(nx, grid, es, en, rho, bc)
    x = S.solve(A, rhs)
    ev, ep = _vel_err(S, x, oracle.stokes_solve(nx, grid, es, en, rho, bc), nx)
    print("solve 66x259 rectilinear: velocity error %.3e, pressure %.3e, %s" % (ev, ep, A.last_stats))
    assert A.last_stats["converged"] == 1 and ev < VEL_TOL, (ev, A.last_stats)
