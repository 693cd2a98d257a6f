"""The 3-D Stokes and heat kernels (pl_3d.hip) against the independent NumPy model tests/stokes3_model.py, which
tests/test_stokes3_model.py ties to the 2-D oracle: operator, right-hand side and scaling on genuinely 3-D non-uniform grids and
viscosities (per-node kernels, the marching LDS kernels, the block decomposition), and solutions against a refined direct solve
of the model's assembled matrix.  Nothing here certifies a GPU result with another GPU result."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import relerr
import stokes3_model as M

pytestmark = pytest.mark.gpu

LDS_THRESHOLD = 200000            # nodes per block from which k3_apply_m / k3_sweep_m take over (pl_3d.hip, k3_use_lds)
GRAVS = [None, (0.0, 9.81, 0.0), (0.0, 0.0, 9.81), (3.0, -4.0, 5.0)]
COMP = ["vz", "vx", "vy", "P"]


def _nonuniform(n, L, rng):
    w = rng.uniform(0.7, 1.3, n - 1)
    g = np.concatenate([[0.0], np.cumsum(w)])
    return g * (L / g[-1])


def _mid(grid):
    out = []
    for c in grid:
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


@functools.lru_cache(maxsize=None)
def _problem(n):
    """Non-uniform grid in all three axes (cell widths U(0.7, 1.3)), one smooth viscosity function with 3 decades and a different
    wavenumber along every axis sampled at the nodes and at the centres, density smooth + noise, and a test vector that is
    standard normal on ALL entries (ghosts and walls included).  Cached: nobody writes to these arrays."""
    n = list(n)
    rng = np.random.default_rng(1000 + n[0] * 10007 + n[1] * 101 + n[2])
    L = [660e3, 660e3 * (n[1] - 1) / (n[0] - 1), 660e3 * (n[2] - 1) / (n[0] - 1)]
    grid = [_nonuniform(n[a], L[a], rng) for a in range(3)]
    mid = _mid(grid)
    f = lambda z, x, y: 1e20 * 10 ** (1.5 * np.cos(np.pi * z / L[0]) * np.sin(2 * np.pi * x / L[1] + 0.3) * np.cos(3 * np.pi * y / L[2] + 0.7))
    Z, X, Y = np.meshgrid(*grid, indexing="ij", sparse=True)
    Zc, Xc, Yc = np.meshgrid(*mid, indexing="ij", sparse=True)
    rho = 3300 + 40 * np.sin(np.pi * Z / L[0]) * np.sin(2 * np.pi * X / L[1]) * np.cos(np.pi * Y / L[2]) + rng.uniform(-1, 1, n)
    x = rng.standard_normal(4 * int(np.prod(n)))
    return dict(n=n, L=L, grid=grid, mid=mid, etas=f(Z, X, Y), etan=f(Zc, Xc, Yc), rho=rho, x=x)


@functools.lru_cache(maxsize=None)
def _model_apply(n, strict):
    p = _problem(n)
    return M.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], p["x"], strict=strict)


@functools.lru_cache(maxsize=None)
def _model_rhs(n, strict, grav):
    p = _problem(n)
    return M.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, strict=strict)


def _check_apply(y, yr, n, what):
    """Per component max |y - y_ref| <= 1e-12 max |y_ref|; the message names the component and the node of the largest error."""
    Y, R = np.asarray(y).reshape(list(n) + [-1]), np.asarray(yr).reshape(list(n) + [-1])
    for q in range(Y.shape[-1]):
        d = np.abs(Y[..., q] - R[..., q])
        s = np.abs(R[..., q]).max()
        node = np.unravel_index(int(np.argmax(d)), d.shape)
        print("%s %s: max err %.3e of max %.3e at node %s" % (what, COMP[q] if Y.shape[-1] == 4 else "T", d.max(), s, node))
        assert d.max() <= 1e-12 * s, "%s: component %s, node (i, j, k) = %s: gpu %r model %r (error %.3e of the maximum %.3e)" % (
            what, COMP[q] if Y.shape[-1] == 4 else "T", tuple(int(v) for v in node), Y[node + (q,)], R[node + (q,)], d.max() / s, s)


def _check_rhs(r, rr, what):
    assert np.array_equal(r == 0, rr == 0), what + ": zero pattern differs at %d entries" % int(np.sum((r == 0) != (rr == 0)))
    bad = ~np.isclose(r, rr, rtol=1e-14, atol=0)
    assert not bad.any(), what + ": %d entries off, first at flat index %d: gpu %r model %r" % (
        int(bad.sum()), int(np.argmax(bad)), r[np.argmax(bad)], rr[np.argmax(bad)])


def _stokes_against_model(n, lds):
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    p = _problem(n)
    assert (int(np.prod(n)) >= LDS_THRESHOLD) == lds, "the shape is on the wrong side of the LDS threshold"
    kc, kb = M.scaling(p["grid"], p["etas"], p["etan"])
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        for strict in (True, False):
            A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], ctx=ctx, strict_reference=strict)
            assert A.Kcont == pytest.approx(kc, rel=1e-13) and A.Kbond == pytest.approx(kb, rel=1e-13)
            what = "apply %s strict=%s" % (list(n), strict)
            y = A @ p["x"]
            _check_apply(y, _model_apply(n, strict), n, what)
            ident = M.identity_rows(p["n"], strict).reshape(-1)
            assert np.array_equal(y[ident], A.Kcont * p["x"][ident]), what + ": identity rows are not exactly Kcont * x"
            for grav in GRAVS:
                if grav is not None:
                    A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, ctx=ctx, strict_reference=strict)
                _check_rhs(rhs, _model_rhs(n, strict, grav), "rhs %s strict=%s grav=%s" % (list(n), strict, grav))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [[5, 5, 5], [6, 7, 9], [13, 10, 70]])
def test_operator_per_node_kernel_matches_model(n):
    """[5, 5, 5]: the smallest grid the library accepts -- the anchor on the last cell layer in z, every node on the rim;
    [13, 10, 70]: a y-line crossing the 64-lane tile.  Both wall-row modes, all four gravity vectors."""
    _stokes_against_model(n, lds=False)


@pytest.mark.parametrize("n", [[37, 45, 131], [57, 53, 67]])
def test_operator_marching_lds_kernel_matches_model(n):
    """Over the 200 000-node threshold: k3_apply_m with its spacing tables, ring and rim.  [37, 45, 131]: partial tiles on all three
    tile axes, zc = 8 with a 5-plane last chunk; [57, 53, 67]: the last y-tile holds exactly one interior column."""
    assert int(np.prod(n)) >= LDS_THRESHOLD
    _stokes_against_model(n, lds=True)


# ---- heat ------------------------------------------------------------------------------------------------------------
WALLS = {"fixtemp": ([0, 0, 0, 0, 0, 0], [273.0, 500.0, 700.0, 1623.0, 900.0, 1100.0]),
         "flow": ([0, 1, 1, 1, 1, 1], [273.0, 0.011, -0.007, 0.02, -0.013, 0.005]),
         "mixed": ([0, 1, 0, 0, 1, 1], [273.0, 0.004, 800.0, 1623.0, -0.006, 0.009])}


@functools.lru_cache(maxsize=None)
def _heat_problem(n):
    p = _problem(n)
    n = list(n)
    rng = np.random.default_rng(2000 + n[0] * 10007 + n[1] * 101 + n[2])
    k = [rng.uniform(2, 5, n) for _ in range(3)]
    Cp, rho = rng.uniform(1000, 1250, n), rng.uniform(3200, 3400, n)
    H, T0 = rng.uniform(0, 1e-9, n) * 3300, rng.uniform(273, 1623, n)
    hmin = min(np.diff(g).min() for g in p["grid"])
    dt = 0.67 * hmin ** 2 / np.max(2 * k[0] / (rho * Cp)) * 4
    return dict(n=n, grid=p["grid"], mid=p["mid"], k=k, Cp=Cp, rho=rho, H=H, T0=T0, dt=dt, x=rng.standard_normal(int(np.prod(n))))


@functools.lru_cache(maxsize=None)
def _heat_model(n, walls):
    h = _heat_problem(n)
    bc, bv = WALLS[walls]
    return (M.heat_apply(h["n"], h["grid"], h["mid"], h["k"], h["Cp"], h["rho"], bc, h["dt"], h["x"]),
            M.heat_rhs(h["n"], h["T0"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"]))


def _check_heat(y, r, n, walls, what):
    """Apply to 1e-12 of the maximum -- of each row class separately (fixed-temperature rows exactly): the flux rows k / delta are
    orders of magnitude below the others and a bound on the overall maximum would not see them.  Right-hand side to rtol 1e-14."""
    h = _heat_problem(n)
    yr, rr = _heat_model(n, walls)
    own = M._owner(h["n"]).reshape(-1)
    bc = np.array(WALLS[walls][0])
    fixed = (own >= 0) & (bc[np.maximum(own, 0)] == M.FIXTEMP)
    flux = (own >= 0) & ~fixed
    assert np.array_equal(y[fixed], h["x"][fixed]), what + ": fixed-temperature rows"
    for name, m in (("flux", flux), ("interior", own < 0)):
        if m.any():
            d = np.abs(y - yr) * m
            s = np.abs(yr[m]).max()
            node = np.unravel_index(int(np.argmax(d)), h["n"])
            print("%s %s rows: max err %.3e of max %.3e" % (what, name, d.max(), s))
            assert d.max() <= 1e-12 * s, "%s: %s row at node %s off by %.3e of the maximum" % (what, name, node, d.max() / s)
    assert np.abs(y - yr).max() <= 1e-12 * np.abs(yr).max()
    _check_rhs(r, rr, what + " rhs")


def _make_heat(P3, n, walls, ctx):
    h = _heat_problem(n)
    bc, bv = WALLS[walls]
    return P3.makeDiffusionMatrix(h["n"], h["grid"], h["mid"], h["T0"], h["k"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"], ctx=ctx)


@pytest.mark.parametrize("n", [[5, 5, 5], [9, 6, 70], [37, 45, 131]])
def test_heat_operator_matches_model(n):
    """Non-uniform grid and midpoints in all axes, independent random kz, kx, ky, Cp, rho, H; all six walls fixed with distinct values,
    all flux walls but z0, and the mixed set [0, 1, 0, 0, 1, 1]."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    h = _heat_problem(n)
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        for walls in WALLS:
            A, rhs = _make_heat(P3, n, walls, ctx)
            _check_heat(A @ h["x"], rhs, n, walls, "heat %s %s" % (list(n), walls))
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [[9, 6, 70], [17, 13, 21]])
def test_heat_solution_matches_direct_solve_of_the_model(n):
    """relerr < 1e-6 (the project's bound for the heat solve) against the refined direct solve of the model's assembled matrix.
    Measured on MI355X: [9, 6, 70] 5.0e-13 (fixed) 6.8e-13 (flux) 3.2e-13 (mixed); [17, 13, 21] 4.0e-13, 1.3e-13, 2.2e-13."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    h = _heat_problem(n)
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        for walls in WALLS:
            bc, bv = WALLS[walls]
            ap = lambda x, rounded=True: M.heat_apply(h["n"], h["grid"], h["mid"], h["k"], h["Cp"], h["rho"], bc, h["dt"], x, rounded=rounded)
            Tref = M.direct_solve(M.assemble(ap, h["n"], ncomp=1), ap, _heat_model(n, walls)[1])
            A, rhs = _make_heat(P3, n, walls, ctx)
            T = P3.solve_heat(A)
            assert A.last_stats["converged"] == 1, A.last_stats
            e = relerr(T, Tref)
            print("heat solve %s %s: relerr %.3e" % (list(n), walls, e))
            assert e < 1e-6, (walls, e)
    finally:
        ctx.close()


# ---- blocks ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,layout,lds", [([25, 33, 41], (2, 2, 2), False), ([25, 33, 41], (3, 1, 4), False), ([73, 45, 131], (2, 1, 1), True)])
def test_blocks_match_model_on_every_rank(n, layout, lds):
    """The block decomposition on a grid that is non-uniform in all axes: a local / global mix-up in the indices of the spacing
    tables (invisible on the uniform grids of test_hip_3d.py) shows on every rank but the first.  Stokes operator (both wall-row
    modes), right-hand side (gravity with three components), heat operator and right-hand side, all against the model.
    [73, 45, 131] on 2 x 1 x 1: blocks over the LDS threshold."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    p, h = _problem(n), _heat_problem(n)
    grav = GRAVS[3]
    vc = P3.VirtualCluster3(p["n"], p["grid"], *layout)

    def run(ctx, rank):
        first, count = (C.c_int * 3)(), (C.c_int * 3)()
        ctx.check(ctx.lib.pl3_local_block(ctx.handle(), first, count))
        out = dict(count=list(count))
        for strict in (True, False):
            A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, ctx=ctx, strict_reference=strict)
            out[strict] = (A @ p["x"], rhs, A.Kcont, A.Kbond)
        Hm, hr = _make_heat(P3, n, "mixed", ctx)
        out["heat"] = (Hm @ h["x"], hr)
        return out
    try:
        res = vc.all(run)
    finally:
        vc.close()
    kc, kb = M.scaling(p["grid"], p["etas"], p["etan"])
    for rank, out in enumerate(res):
        assert (int(np.prod(out["count"])) >= LDS_THRESHOLD) == lds, (rank, out["count"])
        for strict in (True, False):
            y, rhs, kcg, kbg = out[strict]
            assert kcg == pytest.approx(kc, rel=1e-13) and kbg == pytest.approx(kb, rel=1e-13)
            what = "blocks %s %s rank %d strict=%s" % (list(n), layout, rank, strict)
            _check_apply(y, _model_apply(n, strict), n, what)
            ident = M.identity_rows(p["n"], strict).reshape(-1)
            assert np.array_equal(y[ident], kcg * p["x"][ident]), what
            _check_rhs(rhs, _model_rhs(n, strict, grav), what + " rhs")
        _check_heat(out["heat"][0], out["heat"][1], n, "mixed", "blocks %s %s rank %d heat" % (list(n), layout, rank))


# ---- solutions -------------------------------------------------------------------------------------------------------
SOLVE_N = (17, 13, 21)


@functools.lru_cache(maxsize=None)
def _direct(strict):
    p = _problem(SOLVE_N)
    ap = lambda x, rounded=True: M.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, strict=strict, rounded=rounded)
    return M.DirectSolver(M.assemble(ap, p["n"]), ap)


@functools.lru_cache(maxsize=None)
def _direct_solution(strict, grav):
    return _direct(strict).solve(_model_rhs(SOLVE_N, strict, grav))


def _solution_errors(x, xr, n):
    X, R = x.reshape(list(n) + [4]), xr.reshape(list(n) + [4])
    ev = np.sqrt(np.sum((X[..., :3] - R[..., :3]) ** 2) / np.sum(R[..., :3] ** 2))
    return ev, relerr(X[:-1, :-1, :-1, 3], R[:-1, :-1, :-1, 3])


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("grav", [None, (3.0, -4.0, 5.0)])
def test_solution_matches_direct_solve_of_the_model(strict, grav):
    """[17, 13, 21] non-uniform, 3 decades of viscosity: P3.solve against the refined direct solution of the model's assembled matrix
    (a solve that touches none of the project's kernels): velocity relative L2 < 1e-6, pressure on the non-ghost cells < 1e-5,
    converged == 1 -- the bounds of test_extrusion_solution_matches_2d_direct_solve.  The strict / lateral-gravity case is solved
    device-resident as well.  Measured on MI355X (velocity, pressure): strict, default gravity 2.4e-9, 4.8e-11 (46 iterations);
    natural 4.2e-9, 1.3e-11 (40); strict, grav (3, -4, 5) 3.7e-9, 2.8e-11 (58), device-resident 5.7e-9, 1.2e-10; natural, grav
    (3, -4, 5) 4.1e-9, 6.8e-12 (49)."""
    from pylamp_amd import pylamp3d as P3
    p = _problem(SOLVE_N)
    xr = _direct_solution(strict, grav)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, ctx=ctx, strict_reference=strict)
        x = P3.solve(A)
        assert A.last_stats["converged"] == 1, A.last_stats
        ev, ep = _solution_errors(x, xr, SOLVE_N)
        print("solve strict=%s grav=%s: velocity %.3e pressure %.3e (%d iterations)" % (strict, grav, ev, ep, A.last_stats["iterations"]))
        assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        if strict and grav is not None:
            assert P3.solve(A, resident=True) is None and A.last_stats["converged"] == 1, A.last_stats
            ev, ep = _solution_errors(P3.solution(A), xr, SOLVE_N)
            print("solve resident: velocity %.3e pressure %.3e" % (ev, ep))
            assert ev < 1e-6 and ep < 1e-5, (ev, ep)
    finally:
        ctx.close()


def test_lds_solve_residual_by_the_model():
    """[37, 45, 131]: the LDS smoother and residual inside the V-cycle (a direct solve is too large here).  The residual is the
    MODEL's, not A @ x: ||rhs_ref - A_ref x_gpu|| / ||rhs_ref|| < 1e-6; discrete divergence with the model's own spacings, as
    test_config5_solve_129_cubed (RMS over the cells away from the walls, times the largest cell width, against the RMS velocity).
    Measured on MI355X: model residual 2.0e-11, divergence 2.8e-10, 55 iterations."""
    from pylamp_amd import pylamp3d as P3
    n = (37, 45, 131)
    assert int(np.prod(n)) >= LDS_THRESHOLD
    p = _problem(n)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], ctx=ctx)
        x = P3.solve(A)
        st = A.last_stats
    finally:
        ctx.close()
    assert st["converged"] == 1 and st["rel_residual"] <= P3.DEFAULT_RTOL, st
    rr = _model_rhs(n, True, None)
    res = rr.astype(np.longdouble) - M.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, strict=True, rounded=False)
    rel = float(np.sqrt(np.sum(res * res)) / np.linalg.norm(rr))
    (vz, vx, vy), _ = P3.x2vp(x, p["n"])
    d = [np.diff(g) for g in p["grid"]]
    div = ((vz[1:, :-1, :-1] - vz[:-1, :-1, :-1]) / d[0][:, None, None] + (vx[:-1, 1:, :-1] - vx[:-1, :-1, :-1]) / d[1][None, :, None]
           + (vy[:-1, :-1, 1:] - vy[:-1, :-1, :-1]) / d[2][None, None, :])[1:-1, 1:-1, 1:-1]
    hmax = max(w.max() for w in d)
    dv = hmax * np.sqrt(np.mean(div ** 2)) / np.sqrt(np.mean(vz ** 2 + vx ** 2 + vy ** 2))
    print("lds solve: model residual %.3e, divergence %.3e, %d iterations" % (rel, dv, st["iterations"]))
    assert rel < 1e-6, rel
    assert dv < 1e-6, dv
    vmax = max(np.abs(vz).max(), np.abs(vx).max(), np.abs(vy).max())
    assert np.abs(vy).max() > 1e-3 * vmax and np.abs(vx).max() > 1e-3 * vmax            # genuinely 3-D flow
