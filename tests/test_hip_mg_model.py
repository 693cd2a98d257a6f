"""pl_stokes_precond_apply against tests/stokes2_mg_model.py, the NumPy model of the 2-D Stokes preconditioner on rectilinear grids:
z = M^-1 r of the device, component by component, against the model evaluated in longdouble with the lmax the device used.

The cases (tests/test_stokes2_mg_model.py, CASES) name the smallest shape at which each path of pl_solver.hip exists: the tile
kernels with 16- and 32-node tiles and partial last tiles, the LDS and the global-memory tail, the staged kernels down to the coarsest
level, the NS = 1 / 2 / 3 instances of k_mg_pre / k_mg_post, grids that coarsen once or not at all, k_vv_line<0> / <1> up to the
4097-point line, the anisotropy rule, the wall stencil of the pressure block with its gates, and the stabilisation-aware velocity
block.  Knobs are read when a context's solver is created: one fresh context per case.  Every case is below 200 000 nodes: no level
is FP32.

Bar per component: |z - z_ld|_inf <= max(1e-11, 50 x floor) |z_ld|_inf -- 1e-11 is the bar of test_preconditioner_matches_prototype,
floor the model's own rounding (float64 against longdouble, measured per case by tests/test_stokes2_mg_model.py), 50 the allowance
for the kernels' summation order and FMA contraction.  The pressure component is closed-form and is held row by row to
1e-13 x sum |terms|.  lmax / safety of every level lies within 15 % of the converged eigenvalue of the model's iteration matrix.
Every test prints the ratios it saw; the largest per check is printed when the module is done (DESIGN.md section 2 quotes them)."""
import os

import numpy as np
import pytest

import stokes2_mg_model as M
from test_stokes2_mg_model import CASES, LMAX_BAND, TSTEP, build_case, converged_lambdas, model_knobs, rounding_floor

pytestmark = pytest.mark.gpu

Z_TOL = 1e-11
FLOOR_FACTOR = 50.0
P_ROW_TOL = 1e-13
LMAX_SAFETY = 1.1

_margins = {}


def _note(check, what, value):
    print("mg-model %-10s %-30s %.3e" % (check, what, value))
    _margins[check] = max(_margins.get(check, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for check in sorted(_margins):
        print("\nlargest ratio %-10s %.3e" % (check, _margins[check]), end="")
    print()
    _margins.clear()
    from pylamp_amd import _context
    _context.clear_contexts()


def _device_apply(c, extra=None):
    """z = M^-1 r on a fresh context under the case's environment, and what that application used."""
    from pylamp_amd import pylamp_stokes as S, _context
    env = dict(c["env"])
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        _context.clear_contexts()
        kw = dict(surfstab=True, tstep=TSTEP, surfstab_theta=abs(c["stab"]), strict_reference=c["stab"] > 0) if c["stab"] is not None else {}
        A, rhs = S.makeStokesMatrix(c["nx"], c["grid"], c["etas"], c["etan"], c["rho"], c["bc"], **kw)
        z = A.precond(c["r"])
        nl, lm = A.mg_info()
        out = dict(z=z, nlevels=nl, lmax=lm, plan=A.mg_plan(), fp32=A.mg_precision()[1])
        if extra:
            extra(S, A, rhs, out)
        del A
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        _context.clear_contexts()


def _check_plan(c, kw, dev):
    """The device chose what the model's rules choose from the grid and the knobs."""
    plan = dev["plan"]
    assert dev["fp32"] == 0
    assert dev["nlevels"] == len(kw["smoothers"]), (dev["nlevels"], kw["smoothers"])
    assert plan["smoother"] == list(kw["smoothers"]), (plan, kw["smoothers"])
    assert plan["nu"] == tuple(kw["nu"]) and plan["nu0"] == tuple(kw["nu0"] or kw["nu"]), (plan, kw)
    assert plan["ratio"] == kw["ratio"], (plan, kw)
    assert plan["wall"] == kw["wall"], (plan, kw)


def _check_lmax(c, dev):
    conv = converged_lambdas(c)
    for l, (lm, cv) in enumerate(zip(dev["lmax"], conv)):
        ratio = lm / LMAX_SAFETY / cv
        _note("lmax", "%s level %d" % (c["id"], l), abs(ratio - 1.0))
        assert 1 - LMAX_BAND <= ratio <= 1 + LMAX_BAND, (l, lm, cv)


def _model(c, kw, lmax):
    return M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=lmax, ld=True, **kw)


def _check_pressure(c, P, z):
    """z_p row by row: closed form, no lmax."""
    nz, nx = c["nx"]
    zp, mag = P.pressure(c["r"], terms=True)
    got = z.reshape(nz, nx, 3)[:, :, 2]
    err = np.abs(got - zp).astype(np.float64); bar = (P_ROW_TOL * mag).astype(np.float64)
    assert np.all(mag[:nz - 1, :nx - 1] > 0)
    worst = float(np.max(err[bar > 0] / bar[bar > 0]))
    _note("pressure", c["id"], worst * P_ROW_TOL)
    assert np.all(err <= bar), (worst, np.argwhere(err > bar)[:5])


def _check_z(c, P, z):
    fl = rounding_floor(c["id"])
    zl = P.apply(c["r"], rounded=False).reshape(-1, 3)
    Z = z.reshape(-1, 3)
    for q in range(3):
        ratio = float(np.max(np.abs(Z[:, q] - zl[:, q])) / np.max(np.abs(zl[:, q])))
        bar = max(Z_TOL, FLOOR_FACTOR * fl[q])
        _note("z", "%s component %d (floor %.1e)" % (c["id"], q, fl[q]), ratio)
        assert ratio <= bar, (q, ratio, bar)


@pytest.mark.parametrize("cid", sorted(CASES))
def test_preconditioner_matches_the_rectilinear_model(cid):
    c = build_case(cid)
    assert c["nx"][0] * c["nx"][1] < 200000
    kw = model_knobs(c)
    dev = _device_apply(c)
    _check_plan(c, kw, dev)
    _check_lmax(c, dev)
    P = _model(c, kw, dev["lmax"])
    _check_pressure(c, P, dev["z"])
    _check_z(c, P, dev["z"])


def test_wall_stencil_does_not_depend_on_the_call_order():
    """257 x 33 on a square, isoviscous (test_wall_stencil_of_the_pressure_block's grid): pl_stokes_precond_apply on a fresh context
    before any solve, after a solve, and after a second makeStokesMatrix on the same context applies the same pressure block -- the
    wall-stencil one -- bit for bit.  (Every application re-estimates lmax from the previous eigenvector, so the velocity components
    of two applications differ by design: each is held to the model with the lmax that application used.)"""
    nx = [257, 33]
    grid = [np.linspace(0, 1, nx[0]), np.linspace(0, 1, nx[1])]
    Z, X = np.meshgrid(grid[0], grid[1], indexing="ij")
    eta = np.ones(nx)
    rho = 1.0 + 0.1 * np.exp(-((Z - 0.4) ** 2 + (X - 0.55) ** 2) / 0.02)
    bc = [1, 1, 1, 1]
    r = np.random.default_rng(3).standard_normal((nx[0], nx[1], 3))
    L0 = M.Level(grid[0], grid[1], eta, eta, bc, True)
    r[:, :, 0][~L0.iz] = 0.0; r[:, :, 1][~L0.ix] = 0.0
    c = dict(id="order-257x33", nx=nx, grid=grid, etas=eta, etan=eta, rho=rho, bc=bc, env={}, stab=None, r=r.reshape(-1))
    kw = model_knobs(c)
    assert kw["wall"] and set(kw["smoothers"]) == {M.ZLINES}
    later = []

    def more(S, A, rhs, out):
        x = S.solve(A, rhs)
        assert A.last_stats["converged"] == 1
        later.append((A.precond(c["r"]), A.mg_info()[1], A.mg_plan()))
        A2, _ = S.makeStokesMatrix(nx, grid, eta, eta, rho, bc)
        assert A2._ctx is A._ctx
        later.append((A2.precond(c["r"]), A2.mg_info()[1], A2.mg_plan()))
    dev = _device_apply(c, more)
    _check_plan(c, kw, dev)
    first = dev["z"].reshape(nx[0], nx[1], 3)
    P = _model(c, kw, dev["lmax"])
    _check_pressure(c, P, dev["z"])
    diag = M.Precond(nx, grid, eta, eta, bc, lmax=dev["lmax"], **dict(kw, wall=False)).pressure(c["r"])
    assert np.max(np.abs(first[:, :, 2] - diag)) > 0.1 * np.max(np.abs(diag))          # not the diagonal block
    for z, lm, plan in later:
        assert plan["wall"]
        assert np.array_equal(z.reshape(nx[0], nx[1], 3)[:, :, 2], first[:, :, 2])
        zl = _model(c, kw, lm).apply(c["r"], rounded=False).reshape(-1, 3)
        for q in range(2):
            ratio = float(np.max(np.abs(z.reshape(-1, 3)[:, q] - zl[:, q])) / np.max(np.abs(zl[:, q])))
            _note("z", "order-257x33 later component %d" % q, ratio)
            assert ratio <= Z_TOL, (q, ratio)
