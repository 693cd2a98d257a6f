"""CPU checks that earn tests/stokes2_scaled_model.py (the row scales D_r of the 2-D Stokes system, stated from the oracle's matrix)
its authority: on a uniform free-slip grid it IS the scaling of the solver prototype (oracle/proto_stokes_solver.Scaled, written
from the uniform spacings and the matrix diagonal of every row), on a rectilinear grid the diagonal it inverts has the structure the
stencil relies on (an interior momentum row's diagonal is minus the sum of its four same-component neighbours), the no-slip wall
rows keep 1 / Kc although their diagonal is not Kc, and the surface stabilisation changes A but not D_r."""
import numpy as np
import pytest

import stokes2_scaled_model as M

EPS = np.finfo(np.float64).eps


def _nonuni(n, Ld, rng):
    w = rng.uniform(0.7, 1.3, n - 1); g = np.concatenate([[0.0], np.cumsum(w)]); return g * (Ld / g[-1])


def _fields(nx, rng):
    etas = 1e19 * 10 ** rng.uniform(0, 3, nx); etan = 1e19 * 10 ** rng.uniform(0, 3, nx)
    return etas, etan, 3300 + rng.uniform(-50, 50, nx)


@pytest.mark.parametrize("nx,h", [([9, 11], [4096.0, 2048.0]), ([12, 10], [5000.0, 3000.0])], ids=["9x11", "12x10"])
def test_uniform_freeslip_is_the_prototype_scaling(oracle, nx, h):
    """Spacings that are exact in binary (and integers times them): np.linspace and np.diff then give every cell the same width
    bit for bit, and the two statements coincide exactly, not merely to rounding."""
    from oracle import proto_stokes_solver as PS
    rng = np.random.default_rng(21)
    grid = [np.arange(nx[d]) * h[d] for d in range(2)]
    etas, etan, rho = _fields(nx, rng)
    bc = [1, 1, 1, 1]
    A, d = M.scaled_system(nx, grid, etas, etan, rho, bc)
    P = PS.Precond(nx, grid, etas, etan, rho, bc)
    s = PS.Scaled(P, nx, grid).s
    assert np.array_equal(d, s)
    assert (abs(A - P.A)).max() == 0.0
    assert np.all(d > 0) and np.all(np.isfinite(d))


@pytest.mark.parametrize("nx", [[7, 9], [23, 261]], ids=["7x9", "23x261"])
def test_rectilinear_momentum_diagonal_is_the_sum_of_its_neighbours(oracle, nx):
    """The stencil never forms the diagonal: it scales by 1 / (cN + cS + cE + cW) of the coefficients it has.  In the matrix, the
    diagonal of an interior momentum row is minus the sum of the row's four off-diagonal entries of the same velocity component
    (four positive numbers: 4 eps covers their sum in either order)."""
    rng = np.random.default_rng(22)
    grid = [_nonuni(nx[d], 5e3 * (nx[d] - 1), rng) for d in range(2)]
    etas, etan, rho = _fields(nx, rng)
    for bc in ([1, 1, 1, 1], [0, 1, 0, 1]):
        A, d = M.scaled_system(nx, grid, etas, etan, rho, bc)
        cls = oracle.stokes_row_class(nx, bc)
        C = A.tocoo()
        same = (C.row % 3 == C.col % 3) & (C.row != C.col)
        off = np.bincount(C.row[same], weights=C.data[same], minlength=A.shape[0]).reshape(nx[0], nx[1], 3)
        cnt = np.bincount(C.row[same], minlength=A.shape[0]).reshape(nx[0], nx[1], 3)
        diag = A.diagonal().reshape(nx[0], nx[1], 3)
        D = d.reshape(nx[0], nx[1], 3)
        for q in (0, 1):
            m = cls[q] == 1
            assert m.sum() > 0 and np.all(cnt[:, :, q][m] == 4) and np.all(diag[:, :, q][m] < 0)
            assert np.all(np.abs(-diag[:, :, q][m] - off[:, :, q][m]) <= 4 * EPS * off[:, :, q][m])
            assert np.all(np.abs(D[:, :, q][m] * off[:, :, q][m] - 1.0) <= 6 * EPS)
        # continuity rows: the row's own four entries are +-Kc / hx_j and +-Kc / hz_i, so D_r is 2 / (sum of their magnitudes)
        absrow = np.asarray(abs(A).sum(axis=1)).ravel().reshape(nx[0], nx[1], 3)
        m = cls[2] == 1
        assert np.all(np.abs(D[:, :, 2][m] * absrow[:, :, 2][m] - 2.0) <= 8 * EPS)
        # everything else: 1 / Kc, but 1 / Kb at the corner pressures
        Kc, Kb = oracle.stokes_scaling(grid, etas, etan)
        for q in range(3):
            assert np.all(D[:, :, q][(cls[q] == 0) | (cls[q] == 2) | (cls[q] == 3)] == 1.0 / Kc)
        assert np.all(D[:, :, 2][cls[2] >= 4] == 1.0 / Kb) and (cls[2] >= 4).sum() == 4
        if bc[0] == 0:                                      # the no-slip wall rows: the diagonal is not Kc, the scale is 1 / Kc
            assert np.all(np.abs(diag[0, 1:-1, 1]) != Kc) and np.all(D[0, 1:-1, 1] == 1.0 / Kc)


def test_surface_stabilisation_changes_the_matrix_not_the_scales(oracle):
    nx = [9, 12]
    rng = np.random.default_rng(23)
    grid = [_nonuni(nx[d], 5e3 * (nx[d] - 1), rng) for d in range(2)]
    etas, etan, rho = _fields(nx, rng)
    A0, d0 = M.scaled_system(nx, grid, etas, etan, rho, [1, 1, 1, 1])
    A1, d1 = M.scaled_system(nx, grid, etas, etan, rho, [1, 1, 1, 1], surfstab=True, tstep=3.0e11, theta=0.5)
    assert np.array_equal(d0, d1)
    cls = oracle.stokes_row_class(nx)
    moved = (A1.diagonal() != A0.diagonal()).reshape(nx[0], nx[1], 3)
    assert moved[:, :, 0][cls[0] == 1].all() and not moved[:, :, 0][cls[0] != 1].any() and not moved[:, :, 2].any()
