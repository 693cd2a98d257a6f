"""The Krylov solver's reductions in the epilogue of the Stokes operator kernel (PYLAMP_KRYLOV_FUSED, pl_stokes.hip / pl_solver.hip):
the epilogue modes one launch at a time against NumPy (pl_stokes_apply_reduce), and whole solves and a short time loop with the
switch on against off.  Smooth viscosity (log-sinusoidal over three decades) and free-slip walls throughout."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
SUM_TOL = 1e-11          # n eps with n <= 2e4 terms per partial chain is ~2e-12: five times that bound


def _model(oracle, nx):
    L = [660e3, 660e3 * (nx[1] - 1) / (nx[0] - 1)]
    grid = [np.linspace(0, L[d], nx[d]) for d in range(2)]
    Z, X = np.meshgrid(*grid, indexing='ij')
    Zc, Xc = np.meshgrid(*oracle.gridmp_of(grid), indexing='ij')
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / L[1]) * np.cos(np.pi * z / L[0]))
    rho = 3300 + 40 * np.sin(2 * np.pi * X / L[1]) * np.sin(np.pi * Z / L[0])
    return grid, f(Z, X), f(Zc, Xc), rho


def _reduce(A, mode, rows, x, a1, a2, want_out2=False):
    from pylamp_amd import _lib
    A._activate()
    out = np.empty_like(x); out2 = np.empty_like(x) if want_out2 else None
    sums = np.zeros(8)
    null = C.POINTER(C.c_double)()
    A._ctx.check(A._ctx.lib.pl_stokes_apply_reduce(A._ctx.handle(), mode, rows, _lib.dptr(x), _lib.dptr(a1),
                                                   _lib.dptr(a2) if a2 is not None else null, _lib.dptr(out),
                                                   _lib.dptr(out2) if want_out2 else null, _lib.dptr(sums)))
    return out, out2, sums


def _close(got, want, terms):
    """|got - want| <= SUM_TOL * sum |a_i b_i|"""
    return abs(got - want) <= SUM_TOL * np.sum(np.abs(terms))


# (515 x 517 on top of the three grids of the issue: 645 workgroups at row-block height 4, 165 at 16 -- the second stage folds the
#  partial sums of more than 256 workgroups in an extra kernel, so both of its paths run)
@pytest.fixture(scope="module", params=[[33, 41], [66, 259], [130, 128], [515, 517]], ids=lambda n: "%dx%d" % tuple(n))
def case(request, oracle):
    """One operator per grid, random x, b, s, r~, and A x from pl_stokes_apply: computed once, shared by both row-block heights."""
    from pylamp_amd import pylamp_stokes as S
    nx = request.param
    grid, es, en, rho = _model(oracle, nx)
    A, _ = S.makeStokesMatrix(nx, grid, es, en, rho, [1, 1, 1, 1])
    rng = np.random.default_rng(nx[0] * 1000 + nx[1])
    n = 3 * nx[0] * nx[1]
    x, s, rt = (rng.standard_normal(n) for _ in range(3))
    Ax = A @ x
    b = rng.standard_normal(n) * np.abs(Ax).mean()           # of the operator's magnitude, so that b - A x cancels digits
    return dict(nx=nx, grid=grid, A=A, x=x, b=b, s=s, rt=rt, Ax=Ax)


@pytest.mark.parametrize("rows", [4, 16])
def test_dot1_epilogue(case, rows):
    A, x, rt, Ax = case["A"], case["x"], case["rt"], case["Ax"]
    y, _, sums = _reduce(A, 1, rows, x, rt, None)
    assert np.all(np.abs(y - Ax) <= 8 * EPS * np.abs(Ax))
    print("dot1 %s rows %d: %.17g vs %.17g" % (case["nx"], rows, sums[0], np.sum(rt * Ax)))
    assert _close(sums[0], np.sum(rt * Ax), rt * Ax)
    _, _, again = _reduce(A, 1, rows, x, rt, None)
    assert np.array_equal(sums, again)


@pytest.mark.parametrize("rows", [4, 16])
def test_dot5_epilogue(case, rows):
    A, x, s, rt, t = case["A"], case["x"], case["s"], case["rt"], case["Ax"]
    y, _, sums = _reduce(A, 2, rows, x, s, rt)
    assert np.all(np.abs(y - t) <= 8 * EPS * np.abs(t))
    c = np.zeros(t.size, dtype=bool); c[2::3] = True          # the continuity plane
    want = [t * s, t * t, rt * s, rt * t, s * s, (t * s)[c], (t * t)[c], (s * s)[c]]
    for q, terms in enumerate(want):
        print("dot5 %s rows %d sum %d: %.17g vs %.17g" % (case["nx"], rows, q, sums[q], np.sum(terms)))
        assert _close(sums[q], np.sum(terms), terms), (q, sums[q], np.sum(terms))
    _, _, again = _reduce(A, 2, rows, x, s, rt)
    assert np.array_equal(sums, again)


@pytest.mark.parametrize("rows", [4, 16])
@pytest.mark.parametrize("with_x2", [False, True], ids=["x", "x+x2"])
def test_resid_epilogue(case, rows, with_x2):
    A, x, b, Ax, nx, grid = case["A"], case["x"], case["b"], case["Ax"], case["nx"], case["grid"]
    x2 = case["s"] if with_x2 else None
    r, ax, sums = _reduce(A, 3, rows, x, b, x2, want_out2=True)
    assert np.all(np.abs(ax - Ax) <= 8 * EPS * np.abs(Ax))
    assert np.all(np.abs(r - (b - Ax)) <= 8 * EPS * (np.abs(b) + np.abs(Ax)))
    r3 = r.reshape(nx[0], nx[1], 3)
    # the deflation's left vector: (hz + hx) on the continuity rows -- every cell but the anchor (3, 2) and the four corner cells
    hz, hx = np.diff(grid[0]), np.diff(grid[1])
    wgt = np.zeros(nx); wgt[:-1, :-1] = hz[:, None] + hx[None, :]
    wgt[3, 2] = 0.0
    for i in (0, nx[0] - 2):
        for j in (0, nx[1] - 2):
            wgt[i, j] = 0.0
    u = x + x2 if with_x2 else x
    uv = u.reshape(nx[0], nx[1], 3)[:, :, :2]
    want = [r * r, r3[:, :, 2] ** 2, b * b, uv * uv, wgt * r3[:, :, 2]]
    for q, terms in enumerate(want):
        print("resid %s rows %d sum %d: %.17g vs %.17g" % (nx, rows, q, sums[q], np.sum(terms)))
        assert _close(sums[q], np.sum(terms), terms), (q, sums[q], np.sum(terms))
    _, _, again = _reduce(A, 3, rows, x, b, x2, want_out2=True)
    assert np.array_equal(sums, again)
    r_only, none, _ = _reduce(A, 3, rows, x, b, x2)           # without the second destination
    assert none is None and np.array_equal(r_only, r)


def _solve_pair(oracle, monkeypatch, nx, bc):
    from pylamp_amd import pylamp_stokes as S, _context
    grid, es, en, rho = _model(oracle, nx)
    out = {}
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("PYLAMP_KRYLOV_FUSED", mode)
        _context.clear_contexts()
        A, rhs = S.makeStokesMatrix(nx, grid, es, en, rho, bc)
        x = S.solve(A, rhs)
        s1 = dict(A.last_stats)
        x2 = S.solve(A, 1.02 * rhs, x0=x)         # warm start on the same context: fused set-up, kept deflation vector, confirmation
        out[mode] = (x.copy(), s1, x2.copy(), dict(A.last_stats))
        del A
    _context.clear_contexts()
    return out


@pytest.mark.parametrize("nx,bc", [([257, 193], [1, 1, 1, 1]), ([97, 131], [0, 1, 1, 1])], ids=["257x193", "97x131-noslip-top"])
def test_same_solve_switch_on_and_off(oracle, monkeypatch, nx, bc):
    """The epilogue reductions change the order of the sums, nothing else: cold and warm-started solves converge with iteration
    counts within one and the same velocities, and as many operator and preconditioner applications when the counts agree.  Both
    the default (1) and every epilogue (2: r~.v of the first reduction point too) against none (0)."""
    out = _solve_pair(oracle, monkeypatch, nx, bc)
    xs, ss, xs2, ss2 = out["0"]
    v = lambda x: x.reshape(nx[0], nx[1], 3)[:, :, :2]
    for level in ("1", "2"):
        xf, sf, xf2, sf2 = out[level]
        for a, b_, xa, xb in ((sf, ss, xf, xs), (sf2, ss2, xf2, xs2)):
            print("fused(%s) %s\nsplit %s" % (level, a, b_))
            assert a["converged"] == 1 and b_["converged"] == 1, (a, b_)
            assert abs(a["iterations"] - b_["iterations"]) <= 1, (a, b_)
            assert np.linalg.norm(v(xa) - v(xb)) / np.linalg.norm(v(xb)) < 1e-6
            if a["iterations"] == b_["iterations"]:
                assert a["operator_applies"] == b_["operator_applies"] and a["precond_applies"] == b_["precond_applies"], (a, b_)


def test_time_loop_switch_on_and_off(monkeypatch):
    """Four steps of the mantle model at 65 x 81 (every solve after the first is warm-started: the first update of each reads r0 for
    r and p and writes the correction without reading it): both runs converge in every step with iteration counts within one, and the
    velocities after the last step agree.  (Four steps of this model stay well-conditioned: in the oracle's own run the velocities
    grow by 7-8 % per step, the time step stays at the heat-diffusion limit and the viscosity within 1e20 .. 1e23, so a difference
    between the two runs is amplified by about 1.3 over the four steps.)"""
    from pylamp_amd import driver
    nx = [65, 81]; L = [660e3, 825e3]
    res = {}
    for mode in ("2", "1", "0"):
        monkeypatch.setenv("PYLAMP_KRYLOV_FUSED", mode)
        tr_x, tr_f = driver.mantle_tracers(nx, L, 16, np.random.default_rng(7))
        sim = driver.Simulation(nx, L, tr_x, tr_f, driver.Options())
        reps = [sim.step()["stokes"] for _ in range(4)]
        res[mode] = (reps, sim.field("velz"), sim.field("velx"))
        sim.close()
    rs, vzs, vxs = res["0"]
    for level in ("1", "2"):
        rf, vzf, vxf = res[level]
        for a, b_ in zip(rf, rs):
            print("fused(%s) %s\nsplit %s" % (level, a, b_))
            assert a["converged"] == 1 and b_["converged"] == 1, (a, b_)
            assert abs(a["iterations"] - b_["iterations"]) <= 1, (a, b_)
        err = np.sqrt((np.sum((vzf - vzs) ** 2) + np.sum((vxf - vxs) ** 2)) / (np.sum(vzs ** 2) + np.sum(vxs ** 2)))
        assert err < 1e-6, (level, err)
