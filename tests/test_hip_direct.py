"""The blocked banded LU of the Stokes solve (pl_direct.hip): the reference's stock model (viscosity contrast 1e10) on grids the
one-workgroup LU could not take, the node order across the narrow axis, the kernels alone under PYLAMP_FORCE_DIRECT, the
compensated residual, and the device-memory budget.

"Accurate" = SuperLU on A.tocsc() (the GPU operator's own FP64 entries) + 6 refinement steps, the recipe of
oracle.stokes_solve_refined with the residual in double-double instead of np.longdouble (which stalls ~1e-9 from the solution on
this system).  At a contrast of 1e10 the solution moves by ~1e-6 when every entry moves by one ulp, so bars below that are set
against the same entries; against the reference's own entries the bar is that sensitivity floor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from conftest import golden

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def _dd_residual(A, x, b):
    """b - A x for a CSR A: error-free products (Dekker) summed with TwoSum per row, rounded once."""
    k = np.diff(A.indptr)
    rows = np.repeat(np.arange(A.shape[0]), k)
    pos = np.arange(A.data.size) - np.repeat(A.indptr[:-1], k)
    a, xv = A.data, x[A.indices]
    p = a * xv
    ah, al = _split(a); xh, xl = _split(xv)
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    P = np.zeros((A.shape[0], k.max())); E = np.zeros_like(P)
    P[rows, pos] = -p; E[rows, pos] = -e
    hi = np.array(b, dtype=np.float64); lo = np.zeros_like(hi)
    for j in range(P.shape[1]):
        s = hi + P[:, j]; bb = s - hi
        lo = lo + ((hi - (s - bb)) + (P[:, j] - bb)) + E[:, j]
        hi = s
    return hi + lo


def _accurate(Acsc, rhs, refinements=6):
    """SuperLU of the equilibrated matrix + refinement, the recipe of oracle.stokes_solve_refined, with the residual in
    double-double: an np.longdouble residual stalls ~1e-9 from the solution on the stock model (|A| |x| is 1e9 |b| in the stiff
    sphere's rows; its steps wander by 1e-10 .. 2e-9)."""
    A = sp.csr_matrix(Acsc)
    dr = 1.0 / np.abs(A).max(axis=1).toarray().ravel()
    As = sp.diags(dr) @ A
    dc = 1.0 / np.abs(As).max(axis=0).toarray().ravel()
    lu = spla.splu((As @ sp.diags(dc)).tocsc())
    x = dc * lu.solve(dr * rhs)
    for _ in range(refinements):
        x = x + dc * lu.solve(dr * _dd_residual(A, x, rhs))
    return x


def _vel_err(x, xr, nx):
    v = lambda y: y.reshape(nx[0], nx[1], 3)[:, :, :2]
    return float(np.linalg.norm(v(x) - v(xr)) / np.linalg.norm(v(xr)))


def _stock_fields(oracle, nz, nx):
    """The reference's stock model 5 on an nz x nx grid of its 1 x 0.2 box, fields made from its own tracer draw the way the
    step makes them (45 tracers per node)."""
    from pylamp_amd import driver
    g = golden("traj_model5")
    L = [1.0, 0.2]
    grid = [np.linspace(0, L[0], nz), np.linspace(0, L[1], nx)]
    tr_x, tr_f = driver.sphere_tracers([nz, nx], L, int(g["tracdens"]), int(g["seed"]))
    oracle.property_update(tr_f, False, False)
    rho, etas = oracle.trac2grid(tr_x, tr_f[:, [0, 1]], grid, [nz, nx], [5, 6])
    etan, = oracle.trac2grid(tr_x, tr_f[:, [1]], oracle.gridmp_of(grid), [nz, nx], [6])
    assert etas.max() / etas.min() > 1e9
    return grid, etas, etan, rho


def _check_stock(oracle, nx, grid, etas, etan, rho):
    from pylamp_amd import pylamp_stokes as S
    bc = [1, 1, 1, 1]
    A, rhs = S.makeStokesMatrix(nx, grid, etas, etan, rho, bc)
    x = S.solve(A, rhs)
    st = A.last_stats
    err = _vel_err(x, _accurate(A.tocsc(), rhs), nx)
    xo = oracle.stokes_solve_refined(nx, grid, etas, etan, rho, bc, refinements=4)
    err_ref = _vel_err(x, xo, nx)
    print("%s: error %.2e (vs the reference's entries %.2e), stats %s, LU %s" % (nx, err, err_ref, st, A.direct_info()))
    assert st["converged"] == 1 and st["used_direct"] == 1, st
    assert err <= 1e-7, (err, st)
    assert err / 4 <= st["error_estimate"] <= 1e-6, (err, st)
    assert err_ref <= 5e-5, (err_ref, st)


def test_stock_model_401x81(oracle):
    """The stock model refined to 401 x 81 nodes: beyond the one-workgroup LU's 60 M band doubles, now solved by the blocked LU."""
    grid, etas, etan, rho = _stock_fields(oracle, 401, 81)
    _check_stock(oracle, [401, 81], grid, etas, etan, rho)


def test_stock_model_transposed_81x401(oracle):
    """The same fields transposed (81 x 401 nodes, gravity now across the long axis): the LU numbers the nodes along z, across
    the narrow axis, so the band is as narrow as for 401 x 81."""
    grid, etas, etan, rho = _stock_fields(oracle, 401, 81)
    _check_stock(oracle, [81, 401], [grid[1], grid[0]], etas.T.copy(), etan.T.copy(), rho.T.copy())


def test_stock_model_two_resident_steps_401x81(oracle):
    """Two steps of driver.Simulation on the stock model at 401 x 81: every Stokes solve by the LU, and within 1e-6 of the
    accurate solution of the step's own nodal fields."""
    from pylamp_amd import driver, pylamp_stokes as S
    g = golden("traj_model5")
    nx = [401, 81]; L = [1.0, 0.2]
    tr_x, tr_f = driver.sphere_tracers(nx, L, int(g["tracdens"]), int(g["seed"]))
    opt = driver.Options(do_heatdiff=False, tdep_rho=False, tdep_eta=False, tracdens=int(g["tracdens"]), tracdens_min=int(g["tracdens_min"]))
    sim = driver.Simulation(nx, L, tr_x, tr_f, opt)
    grid = [np.linspace(0, L[0], nx[0]), np.linspace(0, L[1], nx[1])]
    try:
        for it in range(2):
            rep = sim.step()
            st = rep["stokes"]
            assert st["converged"] == 1 and st["used_direct"] == 1, (it, st)
            A, rhs = S.makeStokesMatrix(nx, grid, sim.field("etas"), sim.field("etan"), sim.field("rho"), [1, 1, 1, 1])
            xa = _accurate(A.tocsc(), rhs)
            (rz, rx), _ = S.x2vp(xa, nx)
            vz, vx = sim.field("velz"), sim.field("velx")
            ev = np.sqrt((np.sum((vz - rz) ** 2) + np.sum((vx - rx) ** 2)) / (np.sum(rz ** 2) + np.sum(rx ** 2)))
            print("step %d: error %.2e, %s" % (it + 1, ev, st))
            assert ev <= 1e-6, (it, ev, st)
            del A
    finally:
        sim.close()


def _random_system(nx, seed):
    """Two decades of random viscosity on a graded grid."""
    rng = np.random.default_rng(seed)
    gz = np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, nx[0] - 1)]); gx = np.cumsum(np.r_[0.0, rng.uniform(0.5, 1.5, nx[1] - 1)])
    etas = 10 ** rng.uniform(0, 2, nx); etan = 10 ** rng.uniform(0, 2, nx)
    rho = 1.0 + 0.1 * rng.standard_normal(nx)
    return [gz, gx], etas, etan, rho


@pytest.mark.parametrize("nx", [[33, 41], [57, 23], [23, 57], [5, 97]])
def test_lu_kernels_forced(monkeypatch, nx):
    """PYLAMP_FORCE_DIRECT=1: the LU alone (n = 3 nz nx is not a multiple of the panel width; both node orders; a band narrower
    than two panels) against the accurate solution."""
    from pylamp_amd import pylamp_stokes as S
    monkeypatch.setenv("PYLAMP_FORCE_DIRECT", "1")
    grid, etas, etan, rho = _random_system(nx, 7 + nx[0])
    A, rhs = S.makeStokesMatrix(nx, grid, etas, etan, rho, [1, 1, 1, 1])
    x = S.solve(A, rhs)
    st = A.last_stats
    err = _vel_err(x, _accurate(A.tocsc(), rhs), nx)
    assert st["used_direct"] == 1 and st["converged"] == 1, st
    assert err <= 1e-10, (err, st)


def test_lu_kernels_reference_sign_surfstab(monkeypatch, oracle):
    """The reference-sign free-surface stabilisation at the Courant step: an indefinite velocity block, which the LU takes only
    with its row interchanges."""
    from pylamp_amd import pylamp_stokes as S
    g = golden("traj_surfstab41")
    gz, gx = g["gz"], g["gx"]
    nx = [gz.size, gx.size]; grid = [gz, gx]
    tr_x = g["init_tr_x"]; tr_f = g["init_tr_f"].copy()
    oracle.property_update(tr_f, False, False)
    rho, etas = oracle.trac2grid(tr_x, tr_f[:, [0, 1]], grid, nx, [5, 6])
    etan, = oracle.trac2grid(tr_x, tr_f[:, [1]], oracle.gridmp_of(grid), nx, [2])
    (vz, vx), _ = oracle.x2vp(oracle.stokes_solve(nx, grid, etas, etan, rho, [1, 1, 1, 1]), nx)
    courant = 0.67 * (gz[1] - gz[0]) / max(vz.max(), vx.max())
    monkeypatch.setenv("PYLAMP_FORCE_DIRECT", "1")
    A, rhs = S.makeStokesMatrix(nx, grid, etas, etan, rho, [1, 1, 1, 1], surfstab=True, tstep=courant, surfstab_theta=0.5,
                                strict_reference=True)
    x = S.solve(A, rhs)
    st = A.last_stats
    err = _vel_err(x, _accurate(A.tocsc(), rhs), nx)
    assert st["used_direct"] == 1 and st["converged"] == 1, st
    assert err <= 1e-10, (err, st)


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18, reason="np.longdouble is not an extended type here")
def test_compensated_residual_vs_extended_precision():
    """b - A x in double-double on the device against an np.longdouble CSR residual of A.tocsc(), for a random x and a right-hand
    side next to A x (where an FP64 residual is all rounding): within 1e-18 of |A| |x| in every row."""
    from pylamp_amd import pylamp_stokes as S
    nx = [41, 33]
    grid, etas, etan, rho = _random_system(nx, 3)
    etas[10:20, 10:20] *= 1e8
    A, _ = S.makeStokesMatrix(nx, grid, etas, etan, rho, [1, 1, 1, 1])
    C = sp.csr_matrix(A.tocsc())
    rng = np.random.default_rng(5)
    x = rng.standard_normal(C.shape[0])
    b = C @ x
    b = b + 1e-15 * np.abs(b) * rng.standard_normal(b.size)
    r = A.residual_dd(b, x)
    data = C.data.astype(np.longdouble)
    rl = b.astype(np.longdouble) - np.add.reduceat(data * x.astype(np.longdouble)[C.indices], C.indptr[:-1])
    scale = np.abs(C) @ np.abs(x)
    dev = np.abs(r.astype(np.longdouble) - rl).astype(np.float64) / np.maximum(scale, 1e-300)
    r64 = b - C @ x
    dev64 = np.abs(r64.astype(np.longdouble) - rl).astype(np.float64) / np.maximum(scale, 1e-300)
    print("compensated: max %.2e of |A||x|; FP64: max %.2e" % (dev.max(), dev64.max()))
    assert dev.max() <= 1e-18, dev.max()
    assert dev64.max() > 1e-17                      # the comparison can tell the two apart


def test_budget_knob_keeps_the_old_behaviour(oracle):
    """PYLAMP_DIRECT_MAX_GB=0.1: the 401 x 81 band (0.6 GB) does not fit, the iteration's answer stands, honestly unconverged."""
    code = (
        "import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "from oracle import pylamp_oracle as oracle\n"
        "import test_hip_direct as T\n"
        "from pylamp_amd import pylamp_stokes as S\n"
        "grid, etas, etan, rho = T._stock_fields(oracle, 401, 81)\n"
        "A, rhs = S.makeStokesMatrix([401, 81], grid, etas, etan, rho, [1, 1, 1, 1])\n"
        "S.solve(A, rhs)\n"
        "print('STATS', A.last_stats['used_direct'], A.last_stats['converged'])\n" % (ROOT, os.path.join(ROOT, "tests")))
    env = dict(os.environ, PYLAMP_DIRECT_MAX_GB="0.1")
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("STATS")][-1]
    assert line.split()[1:] == ["0", "0"], line
