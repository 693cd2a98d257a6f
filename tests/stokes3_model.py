"""A plain NumPy model of the 3-D staggered Stokes and heat discretisation, the reference the HIP
kernels of pl_3d.hip are compared with (tests/test_hip_3d_model.py).  No GPU, no project code: the rows are composed from
difference operators on the staggered grid by array slicing -- strain rates, stresses, the divergence of the stress --
and evaluated in np.longdouble; results are rounded to float64 unless rounded=False.  tests/test_stokes3_model.py ties it
to the 2-D oracle by extrusion along each of the three axes.

Arrays are (nz, nx, ny); vz lives at (z_i, x_j+1/2, y_k+1/2), vx at (z_i+1/2, x_j, y_k+1/2), vy at (z_i+1/2, x_j+1/2, y_k),
P and etan at the cell centres, etas and rho at the nodes; the last index of an axis along which a quantity sits at
midpoints is a ghost.  Vectors are C-order (nz, nx, ny, 4) with the components vz, vx, vy, P (pylamp3d.gidx).
"""
import contextlib

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

LD = np.longdouble
ANCHOR = (3, 2, 2)                 # the pressure cell whose row is Kcont * P
GRAV = (9.81, 0.0, 0.0)            # default gravity: along z
FIXTEMP, FIXFLOW = 0, 1


def _ld(a):
    return np.asarray(a, dtype=LD)


@contextlib.contextmanager
def working_precision(dtype):
    """Inside the block every function of this module (and of stokes3_walls_model) works in `dtype` instead of np.longdouble: the
    same expressions evaluated in float64 (tests/stokes3_mg_model.py: its float64 evaluation and its eigenvalue estimates)."""
    global LD
    old, LD = LD, dtype
    try:
        yield
    finally:
        LD = old


def _out(y, rounded):
    return y.astype(np.float64) if rounded else y


def _along(v, axis):
    """A 1-D array shaped to broadcast along `axis` of a 3-D array."""
    s = [1, 1, 1]; s[axis] = -1
    return np.asarray(v).reshape(s)


def _index(n):
    return [_along(np.arange(n[a]), a) for a in range(3)]


def _shift(a, axis, step):
    """b[i] = a[i + step] along axis (the wrapped entries are never used by a row that reads them)."""
    return np.roll(a, -step, axis=axis)


def scaling(grid, etas, etan):
    """Kcont = 3 min(eta) / sum_a (L_a / n_a), Kbond = 9 min(eta) / (sum_a L_a / n_a)^2: the 2-D rule with one more axis."""
    mineta = min(np.min(etas), np.min(etan))
    s = sum((float(g[-1]) - float(g[0])) / len(g) for g in grid)
    return 3 * mineta / s, 9 * mineta / s ** 2


# ---------------------------------------------------------------------------------------------------------------------
# Stokes
# ---------------------------------------------------------------------------------------------------------------------
def _momentum(D, grid, etas, etan, V, P, Kc):
    """Natural row of velocity component D: div(stress)_D - Kcont dP/dx_D, where idx[D] in 1 .. n_D - 2 and the two other indices
    are not ghosts; zero elsewhere.  Worked in the frame (D, E, F) = cyclic permutation of (z, x, y).  On a wall edge the
    dv_D/dx_E half of the shear strain rate is dropped and the dv_E/dx_D half kept."""
    E, F = (D + 1) % 3, (D + 2) % 3
    fr = (D, E, F)
    T = lambda a: np.transpose(a, fr)
    U, WE, WF, p, es, en = T(V[D]), T(V[E]), T(V[F]), T(P), T(etas), T(etan)
    cD, cE, cF = _ld(grid[D]), _ld(grid[E]), _ld(grid[F])
    nD, nE, nF = U.shape
    dD, dE, dF = np.diff(cD), np.diff(cE), np.diff(cF)                    # cell widths
    hD, hE, hF = [(c[2:] - c[:-2]) / 2 for c in (cD, cE, cF)]            # distance of the centres of the cells i-1 and i, i = 1 .. n-2
    # normal stress at the cell centres
    eDD = (U[1:, :-1, :-1] - U[:-1, :-1, :-1]) / dD[:, None, None]
    sDD = 2 * en[:-1, :-1, :-1] * eDD
    # shear stress on the D-E edges (D node 1 .. nD-2, E node 0 .. nE-1, F midpoint): viscosity = mean of the two nodes spanning the edge
    dUdE = np.zeros((nD - 2, nE, nF - 1), dtype=LD)
    dUdE[:, 1:-1, :] = (U[1:-1, 1:nE - 1, :-1] - U[1:-1, 0:nE - 2, :-1]) / hE[None, :, None]
    dWdD = (WE[1:-1, :, :-1] - WE[:-2, :, :-1]) / hD[:, None, None]
    sDE = 2 * (0.5 * (es[1:-1, :, :-1] + es[1:-1, :, 1:])) * (0.5 * (dUdE + dWdD))
    # shear stress on the D-F edges (D node, E midpoint, F node)
    dUdF = np.zeros((nD - 2, nE - 1, nF), dtype=LD)
    dUdF[:, :, 1:-1] = (U[1:-1, :-1, 1:nF - 1] - U[1:-1, :-1, 0:nF - 2]) / hF[None, None, :]
    dWdD = (WF[1:-1, :-1, :] - WF[:-2, :-1, :]) / hD[:, None, None]
    sDF = 2 * (0.5 * (es[1:-1, :-1, :] + es[1:-1, 1:, :])) * (0.5 * (dUdF + dWdD))
    row = np.zeros((nD, nE, nF), dtype=LD)
    row[1:-1, :-1, :-1] = ((sDD[1:] - sDD[:-1]) / hD[:, None, None]
                           + (sDE[:, 1:, :] - sDE[:, :-1, :]) / dE[None, :, None]
                           + (sDF[:, :, 1:] - sDF[:, :, :-1]) / dF[None, None, :]
                           - Kc * (p[1:-1, :-1, :-1] - p[:-2, :-1, :-1]) / hD[:, None, None])
    return np.transpose(row, np.argsort(fr))


def velocity_classes(D, n, strict):
    """(interior, slaved, nb_axis_E) boolean maps of component D's rows; everything else is an identity row."""
    E, F = (D + 1) % 3, (D + 2) % 3
    ix = _index(n)
    dom = (ix[D] >= 1) & (ix[D] <= n[D] - 2) & (ix[E] <= n[E] - 2) & (ix[F] <= n[F] - 2)
    if not strict:
        return dom, np.zeros_like(dom), np.zeros_like(dom)
    bE = (ix[E] == 0) | (ix[E] == n[E] - 2)
    bF = (ix[F] == 0) | (ix[F] == n[F] - 2)
    slaved = dom & (bE | bF)
    return dom & ~slaved, slaved, slaved & bE


def pressure_classes(n, strict):
    """(continuity, symmetry along x, symmetry along y) maps; everything else (ghosts, the anchor) is an identity row."""
    ix = _index(n)
    cell = (ix[0] <= n[0] - 2) & (ix[1] <= n[1] - 2) & (ix[2] <= n[2] - 2)
    cell = cell & ~((ix[0] == ANCHOR[0]) & (ix[1] == ANCHOR[1]) & (ix[2] == ANCHOR[2]))
    if not strict:
        return cell, np.zeros_like(cell), np.zeros_like(cell)
    b = [(ix[a] == 0) | (ix[a] == n[a] - 2) for a in range(3)]
    sx = cell & b[0] & b[1]                              # z-x cube edges: the 2-D corner rule, inward along x
    sy = cell & b[2] & (b[0] | b[1]) & ~sx               # the remaining cube edges: inward along y
    return cell & ~sx & ~sy, sx, sy


def _inward(a, axis, n):
    """Value of the inward neighbour along axis for the indices 0 and n - 2 (undefined elsewhere)."""
    i = _index(n)[axis]
    return np.where(i == 0, _shift(a, axis, 1), _shift(a, axis, -1))


def stokes_apply(nx, grid, etas, etan, x, strict=True, rounded=True):
    """The unscaled operator, as pl3_stokes_apply."""
    n = [int(v) for v in nx]
    Kc, Kb = scaling(grid, etas, etan)
    Kc, Kb = LD(Kc), LD(Kb)
    X = _ld(x).reshape(n + [4])
    V, P = [X[..., 0], X[..., 1], X[..., 2]], X[..., 3]
    es, en = _ld(etas), _ld(etan)
    Y = np.empty(n + [4], dtype=LD)
    for D in range(3):
        E, F = (D + 1) % 3, (D + 2) % 3
        interior, slaved, viaE = velocity_classes(D, n, strict)
        y = Kc * V[D]                                                     # wall-normal and ghost velocities
        y = np.where(interior, _momentum(D, grid, es, en, V, P, Kc), y)
        if strict:                                                        # slaved to the neighbour along the first boundary axis, E before F
            nb = np.where(viaE, _inward(V[D], E, n), _inward(V[D], F, n))
            y = np.where(slaved, Kc * (V[D] - nb), y)
        Y[..., D] = y
    cont, sx, sy = pressure_classes(n, strict)
    div = np.zeros(n, dtype=LD)
    for a in range(3):
        div = div + (_shift(V[a], a, 1) - V[a]) / _along(np.append(np.diff(_ld(grid[a])), LD(1)), a)
    y = Kc * P                                                            # ghost pressures and the anchor
    y = np.where(cont, Kc * div, y)
    if strict:
        y = np.where(sx, Kb * (_inward(P, 1, n) - P), y)
        y = np.where(sy, Kb * (_inward(P, 2, n) - P), y)
    Y[..., 3] = y
    return _out(Y.reshape(-1), rounded)


def stokes_rhs(nx, grid, etas, etan, rho, grav=None, strict=True, rounded=True):
    """The unscaled right-hand side, as pl3_stokes_rhs: -g_D times the density averaged onto the face normal to D, on the interior
    momentum rows; zero everywhere else."""
    n = [int(v) for v in nx]
    g = GRAV if grav is None else grav
    r = _ld(rho)
    R = np.zeros(n + [4], dtype=LD)
    for D in range(3):
        E, F = (D + 1) % 3, (D + 2) % 3
        if float(g[D]) == 0.0:
            continue
        interior = velocity_classes(D, n, strict)[0]
        face = (r + _shift(r, E, 1) + _shift(r, F, 1) + _shift(_shift(r, E, 1), F, 1)) / 4
        R[..., D] = np.where(interior, -face * LD(float(g[D])), 0)
    return _out(R.reshape(-1), rounded)


def identity_rows(nx, strict):
    """Boolean (nz, nx, ny, 4): the rows that are Kcont times the unknown."""
    n = [int(v) for v in nx]
    m = np.zeros(n + [4], dtype=bool)
    for D in range(3):
        interior, slaved, _ = velocity_classes(D, n, strict)
        m[..., D] = ~(interior | slaved)
    cont, sx, sy = pressure_classes(n, strict)
    m[..., 3] = ~(cont | sx | sy)
    return m


# ---------------------------------------------------------------------------------------------------------------------
# heat
# ---------------------------------------------------------------------------------------------------------------------
def _owner(n):
    """Wall number 0 .. 5 = [z0, x0, y0, zL, xL, yL] that owns a node, -1 inside: z-walls own their edges, then x-walls, then y."""
    ix = _index(n)
    w = np.full(n, -1)
    for a in (2, 1, 0):
        w = np.where(ix[a] == 0, a, np.where(ix[a] == n[a] - 1, a + 3, w))
    return w


def heat_apply(nx, grid, gridmp, k, Cp, rho, bc, tstep, T, rounded=True):
    """pylamp_diff's rows with one more axis.  k = [kz, kx, ky] on the faces normal to z, x, y (k_a[i] between the nodes i and i + 1)."""
    n = [int(v) for v in nx]
    T = _ld(T).reshape(n)
    c = LD(tstep) / (_ld(rho) * _ld(Cp))
    own = _owner(n)
    flux_div = np.zeros(n, dtype=LD)
    y = np.empty(n, dtype=LD)
    y[...] = T                                                              # fixed-temperature walls
    for a in range(3):
        d = np.diff(_ld(grid[a]))
        mp = _ld(gridmp[a])
        Tm, km = np.moveaxis(T, a, 0), np.moveaxis(_ld(k[a]), a, 0)
        q = km[:-1] * (Tm[1:] - Tm[:-1]) / d[:, None, None]                 # k dT/dx on the faces 0 .. n-2
        f = np.zeros_like(Tm)
        f[1:-1] = (q[1:] - q[:-1]) / (mp[1:n[a] - 1] - mp[0:n[a] - 2])[:, None, None]
        flux_div = flux_div + np.moveaxis(f, 0, a)
        w = np.zeros_like(Tm)
        w[0] = q[0]; w[-1] = q[-1]                                          # flux rows: k / delta times the difference across the wall cell
        w = np.moveaxis(w, 0, a)
        for wall in (a, a + 3):
            if int(bc[wall]) == FIXFLOW:
                y = np.where(own == wall, w, y)
            elif int(bc[wall]) != FIXTEMP:
                raise Exception("heat: boundary condition must be FIXTEMP or FIXFLOW")
    y = np.where(own < 0, c * flux_div - T, y)
    return _out(y.reshape(-1), rounded)


def heat_rhs(nx, T, Cp, rho, H, bc, bcvalue, tstep, rounded=True):
    n = [int(v) for v in nx]
    r = -_ld(T) - LD(tstep) * _ld(H) / (_ld(rho) * _ld(Cp))
    own = _owner(n)
    for wall in range(6):
        r = np.where(own == wall, LD(float(bcvalue[wall])), r)
    return _out(r.reshape(-1), rounded)


# ---------------------------------------------------------------------------------------------------------------------
# assembled matrix and direct solve
# ---------------------------------------------------------------------------------------------------------------------
def assemble(apply_fn, n, ncomp=4):
    """CSR matrix of the linear map apply_fn (flat vector -> flat vector, C-order (nz, nx, ny, ncomp)) by probing with coloured unit
    vectors: a row reaches at most +-1 node per axis, so 3 x 3 x 3 colours x components suffice."""
    n = [int(v) for v in n]
    ix = np.indices(n)
    node = np.arange(int(np.prod(n))).reshape(n)
    rows, cols, vals = [], [], []
    for cz in range(3):
        for cx in range(3):
            for cy in range(3):
                col = (cz, cx, cy)
                hit = (ix[0] % 3 == cz) & (ix[1] % 3 == cx) & (ix[2] % 3 == cy)
                # the only node of this colour within reach of a row's node
                tgt = [ix[a] + ((col[a] - ix[a] + 1) % 3) - 1 for a in range(3)]
                ok = np.ones(n, dtype=bool)
                for a in range(3):
                    ok &= (tgt[a] >= 0) & (tgt[a] < n[a])
                tnode = np.where(ok, node[tuple(np.clip(tgt[a], 0, n[a] - 1) for a in range(3))], -1)
                for q in range(ncomp):
                    e = np.zeros(n + [ncomp])
                    e[..., q] = hit
                    y = np.asarray(apply_fn(e.reshape(-1)), dtype=np.float64).reshape(n + [ncomp])
                    if np.any(y[~ok] != 0):
                        raise Exception("assemble: a row reaches further than one node")
                    r = np.nonzero(y)
                    rows.append(node[r[0], r[1], r[2]] * ncomp + r[3])
                    cols.append(tnode[r[0], r[1], r[2]] * ncomp + q)
                    vals.append(y[r])
    N = int(np.prod(n)) * ncomp
    return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, N)).tocsr()


class DirectSolver:
    """Sparse LU of the equilibrated assembled matrix + iterative refinement with the model's longdouble residual
    (apply_fn(x, rounded=False)): refined until ||rhs - A x|| <= tol ||rhs||, raises otherwise."""

    def __init__(self, A, apply_fn):
        A = sp.csr_matrix(A)
        self.apply = apply_fn
        self.dr = 1.0 / np.abs(A).max(axis=1).toarray().ravel()
        As = sp.diags(self.dr) @ A
        self.dc = 1.0 / np.abs(As).max(axis=0).toarray().ravel()
        self.lu = spla.splu((As @ sp.diags(self.dc)).tocsc())

    def solve(self, rhs, tol=1e-12, maxref=8):
        rl = _ld(rhs)
        bn = np.sqrt(np.sum(rl * rl))
        x = self.dc * self.lu.solve(self.dr * np.asarray(rhs, dtype=np.float64))
        for _ in range(maxref + 1):
            r = rl - self.apply(x, rounded=False)
            self.residual = float(np.sqrt(np.sum(r * r)) / bn)
            if self.residual <= tol:
                return x
            x = x + self.dc * self.lu.solve(self.dr * r.astype(np.float64))
        raise Exception("direct solve: residual %.3e after %d refinements" % (self.residual, maxref))


def direct_solve(A, apply_fn, rhs, tol=1e-12):
    return DirectSolver(A, apply_fn).solve(rhs, tol)
