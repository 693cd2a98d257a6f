"""NumPy reference of the row-scaled 2-D Stokes system D_r A the Krylov solver iterates on (tests/test_hip_stokes_launch.py).

A is the oracle's explicit matrix; D_r is stated from that matrix and the oracle's row classes, one rule per class:

  interior momentum rows (class 1 of vz, vx)   1 / |a_rr| of the matrix built WITHOUT surface stabilisation (the stabilisation term
                                               sits on the diagonal too, and the solver's scale leaves it out)
  continuity rows (class 1 of P)               1 / (Kc (1/hx_j + 1/hz_i)) with the widths of the row's own cell (the row has no diagonal)
  corner pressure rows (classes 4, 5)          1 / Kb
  every other row                              1 / Kc: identity rows and the tangential wall rows of classes 2 and 3, free-slip or
                                               no-slip (a no-slip row's diagonal is NOT Kc; its scale is)

tests/test_stokes2_scaled_model.py holds this against the solver prototype's own statement (oracle/proto_stokes_solver.Scaled) and
against the structure of the matrix rows."""
import numpy as np

from oracle import pylamp_oracle as O


def row_scales(nx, grid, etas, etan, rho, bc):
    """D_r per DOF in the reference's order (node-major, vz | vx | P per node)."""
    nz, nxx = int(nx[0]), int(nx[1])
    A0, _ = O.stokes_csr(nx, grid, etas, etan, rho, bc)
    Kc, Kb = O.stokes_scaling(grid, etas, etan)
    cls = O.stokes_row_class(nx, bc)
    d = np.full((nz, nxx, 3), 1.0 / Kc)
    diag = np.abs(A0.diagonal()).reshape(nz, nxx, 3)
    for q in (0, 1):
        m = cls[q] == 1
        d[:, :, q][m] = 1.0 / diag[:, :, q][m]
    hz = np.diff(np.asarray(grid[0], dtype=np.float64))
    hx = np.diff(np.asarray(grid[1], dtype=np.float64))
    cont = np.zeros((nz, nxx))
    cont[:-1, :-1] = 1.0 / (Kc * (1.0 / hx[None, :] + 1.0 / hz[:, None]))
    m = cls[2] == 1
    d[:, :, 2][m] = cont[m]
    d[:, :, 2][(cls[2] == 4) | (cls[2] == 5)] = 1.0 / Kb
    return d.reshape(-1)


def scaled_system(nx, grid, etas, etan, rho, bc, **surfstab):
    """(A, d): the oracle's CSR matrix (surfstab=True, tstep=, theta= as oracle.stokes_csr takes them) and D_r per DOF; the system
    the solver iterates on is diag(d) A."""
    A, _ = O.stokes_csr(nx, grid, etas, etan, rho, bc, **surfstab)
    return A, row_scales(nx, grid, etas, etan, rho, bc)
