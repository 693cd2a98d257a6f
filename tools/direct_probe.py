"""Blocked banded LU of the Stokes solve on the reference's stock model (sphere of viscosity 1e12 in 1e2, contrast 1e10):
factorisation and triangular-solve times, refinement, and the velocity error against
  * the accurate solution of the GPU's own operator (SuperLU on A.tocsc() + 4 refinement steps with an np.longdouble residual),
  * oracle.stokes_solve_refined (the same, on the reference's own matrix entries).

    python tools/direct_probe.py [NZxNX ...]        (default: 201x41 401x81 81x401 801x161)

NZxNX with NZ < NX is the transposed model (the fields of the NXxNZ model, transposed): the LU numbers its nodes across the
narrow axis, so both orientations cost the same.  Run on the GPU box with PYLAMP_SOLVER_TRACE=1 to see the solver's own line.
"""
import os
import sys
import time

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
os.environ.setdefault("PYLAMP_SOLVER_TRACE", "1")


def stock_fields(nz, nx, tracdens=45, seed=17):
    """etas, etan, rho of the stock model on an nz x nx grid of the 1 x 0.2 box, the way the step builds them."""
    from pylamp_amd import driver
    from oracle import pylamp_oracle as O
    L = [1.0, 0.2]
    grid = [np.linspace(0, L[0], nz), np.linspace(0, L[1], nx)]
    tr_x, tr_f = driver.sphere_tracers([nz, nx], L, tracdens, seed)
    O.property_update(tr_f, False, False)
    rho, etas = O.trac2grid(tr_x, tr_f[:, [0, 1]], grid, [nz, nx], [5, 6])
    etan, = O.trac2grid(tr_x, tr_f[:, [1]], O.gridmp_of(grid), [nz, nx], [6])
    return grid, etas, etan, rho


def split(a):
    c = 134217729.0 * a
    hi = c - (c - a)
    return hi, a - hi


def dd_residual(A, x, b):
    """b - A x for a CSR A: error-free products (Dekker) summed with TwoSum per row, rounded once."""
    k = np.diff(A.indptr)
    rows = np.repeat(np.arange(A.shape[0]), k)
    pos = np.arange(A.data.size) - np.repeat(A.indptr[:-1], k)
    a, xv = A.data, x[A.indices]
    p = a * xv
    ah, al = split(a); xh, xl = split(xv)
    e = ((ah * xh - p) + ah * xl + al * xh) + al * xl
    P = np.zeros((A.shape[0], k.max())); E = np.zeros_like(P)
    P[rows, pos] = -p; E[rows, pos] = -e
    hi = np.array(b, dtype=np.float64); lo = np.zeros_like(hi)
    for j in range(P.shape[1]):
        s = hi + P[:, j]; bb = s - hi
        lo = lo + ((hi - (s - bb)) + (P[:, j] - bb)) + E[:, j]
        hi = s
    return hi + lo


def accurate(Acsc, rhs, refinements=6):
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
        x = x + dc * lu.solve(dr * dd_residual(A, x, rhs))
    return x


def vel_err(x, xr, nx):
    v = lambda y: y.reshape(nx[0], nx[1], 3)[:, :, :2]
    return float(np.linalg.norm(v(x) - v(xr)) / np.linalg.norm(v(xr)))


def probe(nz, nx):
    from pylamp_amd import pylamp_stokes as S, _context
    from oracle import pylamp_oracle as O
    tz, tx = (nz, nx) if nz >= nx else (nx, nz)
    grid, etas, etan, rho = stock_fields(tz, tx, 45 if tz * tx <= 40000 else 12)
    if nz < nx:
        grid, etas, etan, rho = [grid[1], grid[0]], etas.T.copy(), etan.T.copy(), rho.T.copy()
    bc = [1, 1, 1, 1]
    A, rhs = S.makeStokesMatrix([nz, nx], grid, etas, etan, rho, bc)
    t0 = time.time()
    x = S.solve(A, rhs)
    wall = time.time() - t0
    st, info = A.last_stats, A.direct_info()
    xa = accurate(A.tocsc(), rhs)
    xo = O.stokes_solve_refined([nz, nx], grid, etas, etan, rho, bc, refinements=4)
    print("%dx%d: band %d, factorisation %.1f ms, triangular solves %.2f ms each (%d), solve %.0f ms wall | converged %d direct %d "
          "iterations %d estimate %.2e | error vs accurate(A.tocsc()) %.2e, vs oracle refined %.2e"
          % (nz, nx, info["band"], info["factor_ms"], info["solve_ms"] / max(info["nsolve"], 1), info["nsolve"], 1e3 * wall,
             st["converged"], st["used_direct"], st["iterations"], st["error_estimate"], vel_err(x, xa, [nz, nx]),
             vel_err(x, xo, [nz, nx])), flush=True)
    del A
    _context.clear_contexts()


if __name__ == "__main__":
    shapes = sys.argv[1:] or ["201x41", "401x81", "81x401", "801x161"]
    for s in shapes:
        nz, nx = (int(v) for v in s.split("x"))
        probe(nz, nx)
