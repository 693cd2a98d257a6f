"""A plain NumPy model of the 3-D Stokes preconditioner z = M^-1 r, the reference that
pl3_stokes_precond_apply is compared with (tests/test_hip_3d_mg_model.py).  No GPU, no project code.  It is written from the rules
of the multigrid cycle, not from the kernels, and carries no stencil of its own: the velocity block of every level is the velocity
part of the operator model (tests/stokes3_walls_model.py, which tests/test_stokes3_model.py and test_stokes3_walls_model.py tie to
the 2-D oracle) on that level's grid with zero pressure, and its diagonal is read off that operator by probing.
tests/test_stokes3_mg_model.py says why the model can be trusted.

    M = [[A_vv, A_vp], [0, S^]]:   z_p = S^-1 r_p  (the diagonal approximation sum(1/d) eta_n / Kcont of the SCALED continuity rows),
                                    z_v = one V-cycle for A_vv z_v = f,  f = r_v * diag - A_vp z_p.

r is the ROW-SCALED residual, as the Krylov iteration hands it over: every row divided by the coefficient of its own unknown, the
interior momentum rows by minus that coefficient (diag > 0 above is minus the diagonal of A_vv, which is negative definite).

Evaluated in float64 or -- ld=True -- in np.longdouble; the operator model switches with it (stokes3_model.working_precision).
Arrays are (nz, nx, ny), vectors C-order (nz, nx, ny, 4) = vz, vx, vy, P; (D, E, F) is a cyclic permutation of (z, x, y).
Row classes of component D: ZERO (wall-normal rows idx[D] = 0, n_D - 1 and the ghosts idx[E] = n_E - 1, idx[F] = n_F - 1), SLAVE
(slaved wall rows of level 0: idx[E] or idx[F] in {0, n - 2}), INT (carries an equation).

The closure of a velocity field (done inside every sweep, after the prolongation and in the power iteration): ZERO rows are 0; a
SLAVE row takes the value of its master -- the row moved one layer inward along every axis on whose outermost layer it lies, so
two layers on a cube edge -- times v_slave / v_master = w0 / (2 w0 + w1) for every NOSLIP wall crossed on the way (w0, w1: the
widths of the wall cell and the next one; the line through the two values vanishes on the wall), 1 on a FREESLIP wall.  On a cube
edge the device's matrix row couples along the first boundary axis only; the closure uses the product over both, which is the
same thing once the neighbour's own row holds.
"""
import numpy as np
import scipy.sparse.linalg as spla

import stokes3_model as M
import stokes3_walls_model as W

LD = np.longdouble
NOSLIP, FREESLIP = W.NOSLIP, W.FREESLIP
LDS_NODES = 200000                 # nodes of a level (of a block) from which the marching LDS kernels take it
BIG_NODES = 1000000                # nodes of the finest grid from which the default plan is V(1,1) on level 0, V(3,3) below
W3 = (0.25, 0.5, 0.25)
W4 = (0.125, 0.375, 0.375, 0.125)


# ---------------------------------------------------------------------------------------------------------------------
# selection rules: functions of the grid and the knobs alone
# ---------------------------------------------------------------------------------------------------------------------
def level_grids(grid, P=(1, 1, 1)):
    """Node coordinates of every level: every second node while all three axes have an even cell count and at least 4 cells after
    halving; with P = (Pz, Px, Py) blocks every block must also keep an even cell count and at least 2 cells after halving."""
    g = [np.asarray(c) for c in grid]
    out = [g]
    while True:
        cells = [c.size - 1 for c in g]
        stop = any(c % 2 or c // 2 < 4 for c in cells)
        stop = stop or any(p > 1 and ((c // p) % 2 or c // p // 2 < 2) for c, p in zip(cells, P))
        if stop:
            return out
        g = [c[::2] for c in g]
        out.append(g)


def sweeps(n, env=None):
    """(sweeps on the finest level, sweeps on the others): 2 and 2; from 10^6 nodes up 1 and 3; PYLAMP_MG_NU3 (1 .. 6) sets both and
    switches the size rule off, PYLAMP_MG_NU3_FINE (1 .. 6) sets the finest level's."""
    env = env or {}
    nu, nu_set, fine = 2, False, 0
    if "PYLAMP_MG_NU3" in env and 1 <= int(env["PYLAMP_MG_NU3"]) <= 6:
        nu, nu_set = int(env["PYLAMP_MG_NU3"]), True
    if "PYLAMP_MG_NU3_FINE" in env and 1 <= int(env["PYLAMP_MG_NU3_FINE"]) <= 6:
        fine = int(env["PYLAMP_MG_NU3_FINE"])
    big = int(np.prod([int(v) for v in n])) >= BIG_NODES and not nu_set
    return (fine if fine > 0 else (1 if big else nu)), (3 if big else nu)


def coarsest_sweeps(n, coarse_sweeps=12):
    """(sweeps, Chebyshev ratio) of the level that is not coarsened further: ratio = max(30, 0.4 N^(2/3)), N its node count."""
    ratio = max(30.0, 0.4 * float(np.prod([float(v) for v in n])) ** (2.0 / 3.0))
    return min(150, max(int(np.sqrt(ratio)), coarse_sweeps)), ratio


def lds_levels(grid, P=(1, 1, 1)):
    """Per level: whether the marching LDS kernels take it (the nodes of one block reach LDS_NODES)."""
    out = []
    for g in level_grids(grid, P):
        blk = [(c.size - 1) // p + 1 for c, p in zip(g, P)]
        out.append(int(np.prod(blk)) >= LDS_NODES)
    return out


def cheb_coeffs(lmax, ratio, n):
    """c1, c2 of n three-term Chebyshev sweeps on [lmax / ratio, lmax]: theta = (lmax + lmin) / 2, delta = (lmax - lmin) / 2,
    sigma = theta / delta; first sweep c1 = 0, c2 = 1 / theta; then rho' = 1 / (2 sigma - rho), c1 = rho' rho, c2 = 2 rho' / delta."""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma = theta / delta
    rho_old = 1.0 / sigma
    c1, c2 = [], []
    for k in range(n):
        if k == 0:
            c1.append(0.0); c2.append(1.0 / theta)
        else:
            rho = 1.0 / (2.0 * sigma - rho_old)
            c1.append(rho * rho_old); c2.append(2.0 * rho / delta); rho_old = rho
    return c1, c2


# ---------------------------------------------------------------------------------------------------------------------
# hierarchy
# ---------------------------------------------------------------------------------------------------------------------
def coarsen_nodes(a):
    """[1 2 1]^3 / 64 at every second node, edge values repeated beyond the walls."""
    for ax in range(3):
        p = np.pad(a, [(1, 1) if q == ax else (0, 0) for q in range(3)], mode="edge")
        lo, mid, hi = [np.take(p, np.arange(k, k + a.shape[ax], 2), axis=ax) for k in range(3)]
        a = ((lo + hi) + 2 * mid) / 4                       # (this order reproduces a constant exactly)
    return a


def coarsen_centres(a):
    """Mean of the 2 x 2 x 2 fine cells a coarse cell covers; ghost entries copy their neighbour."""
    n = a.shape
    c = a[:n[0] - 1, :n[1] - 1, :n[2] - 1]
    for ax in range(3):                                   # pairwise, axis by axis: a constant is reproduced exactly
        lo, hi = [np.take(c, np.arange(k, c.shape[ax], 2), axis=ax) for k in range(2)]
        c = (lo + hi) / 2
    m = c
    return np.pad(m, [(0, 1)] * 3, mode="edge")


class Level:
    """The velocity block of one level: apply() is the operator model with zero pressure on the INT rows, diag its diagonal (by
    probing with unit vectors of seven colours: the rows of one component reach one node along each axis within that component)."""

    def __init__(self, grid, etas, etan, bc, strict, dt):
        self.dt = dt
        self.grid = [np.asarray(c, dtype=dt) for c in grid]
        self.n = [c.size for c in self.grid]
        self.etas, self.etan = np.asarray(etas, dtype=dt), np.asarray(etan, dtype=dt)
        self.bc = W.walls(bc)
        self.strict = bool(strict)
        cls = [M.velocity_classes(D, self.n, self.strict) for D in range(3)]
        self.int_ = [c[0] for c in cls]
        self.slave = [c[1] for c in cls]
        self._diag = None
        # master of every slaved row (the row itself elsewhere) and v_slave / v_master
        ix = M._index(self.n)
        self.master, self.fac = [], []
        for D in range(3):
            idx = [np.broadcast_to(ix[a], self.n).copy() for a in range(3)]
            f = np.ones(self.n, dtype=dt)
            if self.strict:
                for a in ((D + 1) % 3, (D + 2) % 3):
                    c, N = self.grid[a], self.n[a]
                    g0 = (c[1] - c[0]) / (2 * (c[1] - c[0]) + (c[2] - c[1])) if self.bc[a] == NOSLIP else dt(1)
                    gL = (c[N - 1] - c[N - 2]) / (2 * (c[N - 1] - c[N - 2]) + (c[N - 2] - c[N - 3])) if self.bc[a + 3] == NOSLIP else dt(1)
                    lo, hi = self.slave[D] & (ix[a] == 0), self.slave[D] & (ix[a] == N - 2)
                    idx[a] = np.where(lo, 1, np.where(hi, N - 3, idx[a]))
                    f = f * np.where(lo, g0, np.where(hi, gL, dt(1)))
            self.master.append(tuple(idx)); self.fac.append(f)

    def _apply4(self, X):
        with M.working_precision(self.dt):
            return W.stokes_apply(self.n, self.grid, self.etas, self.etan, X.reshape(-1), bc=self.bc, strict=self.strict,
                                  rounded=False).reshape(self.n + [4])

    def apply(self, V):
        """A_vv V on the INT rows, zero elsewhere."""
        X = np.zeros(self.n + [4], dtype=self.dt)
        for D in range(3):
            X[..., D] = V[D]
        Y = self._apply4(X)
        return [np.where(self.int_[D], Y[..., D], 0) for D in range(3)]

    @property
    def diag(self):
        """The diagonal of A_vv on the INT rows (negative), 1 elsewhere."""
        if self._diag is None:
            ix = M._index(self.n)
            colour = (ix[0] + 2 * ix[1] + 4 * ix[2]) % 7          # the six neighbours of a node along the axes have six other colours
            self._diag = []
            for D in range(3):
                d = np.ones(self.n, dtype=self.dt)
                for col in range(7):
                    hit = self.int_[D] & (colour == col)
                    X = np.zeros(self.n + [4], dtype=self.dt)
                    X[..., D] = hit
                    d = np.where(hit, self._apply4(X)[..., D], d)
                self._diag.append(d)
        return self._diag

    def close(self, V):
        out = []
        for D in range(3):
            v = np.where(self.int_[D], V[D], 0)
            if self.strict:
                v = np.where(self.slave[D], self.fac[D] * v[self.master[D]], v)
            out.append(v)
        return out

    def sweep(self, v, vprev, f, c1, c2):
        """v + c1 (v - vprev) + c2 D^-1 (f - A v) on the INT rows, then closed.  v None: the zero guess."""
        d = self.diag
        if v is None:
            return self.close([c2 * f[D] / d[D] for D in range(3)])
        Av = self.apply(v)
        return self.close([v[D] + c1 * (v[D] - vprev[D]) + c2 * (f[D] - Av[D]) / d[D] for D in range(3)])

    def smooth(self, v, f, n, lmax, ratio):
        """n Chebyshev-Jacobi sweeps for A v = f from v (None: from the zero guess)."""
        c1, c2 = cheb_coeffs(lmax, ratio, n)
        dt = self.dt
        zero = [np.zeros(self.n, dtype=dt)] * 3
        prev = zero
        for k in range(n):
            new = self.sweep(v, prev, f, dt(c1[k]), dt(c2[k]))
            prev, v = (zero if v is None else v), new
        return v

    def residual(self, v, f):
        Av = self.apply(v)
        return [np.where(self.int_[D], f[D] - Av[D], 0) for D in range(3)]

    # ---- the iteration matrix T = close . D^-1 A of the smoother ----
    def jacobi(self, v):
        Av, d = self.apply(v), self.diag
        return self.close([Av[D] / d[D] for D in range(3)])

    def power_iteration(self, iters=12, seed=0):
        """|T v| / |v| after `iters` iterations from a closed random start: what a cold estimate of the solver gives."""
        rng = np.random.default_rng([seed, 3] + self.n)
        v = self.close([np.asarray(rng.uniform(-1, 1, self.n), dtype=self.dt) for _ in range(3)])
        lam = 0.0
        for _ in range(iters):
            y = self.jacobi(v)
            ny, nv = np.sqrt(sum(np.sum(a * a) for a in y)), np.sqrt(sum(np.sum(a * a) for a in v))
            lam = float(ny / nv)
            v = [a / ny for a in y]
        return lam

    def lambda_max(self, tol=1e-3):
        """The converged largest eigenvalue of D^-1 A_vv with closure (Arnoldi on the INT rows, the closure folded in; tol is
        ARPACK's stopping criterion, the eigenvalue itself is several times closer)."""
        idx = [np.flatnonzero(m.reshape(-1)) for m in self.int_]
        cut = np.cumsum([0] + [i.size for i in idx])
        N = int(np.prod(self.n))

        def mv(x):
            V = []
            for D in range(3):
                a = np.zeros(N, dtype=self.dt); a[idx[D]] = x[cut[D]:cut[D + 1]]
                V.append(a.reshape(self.n))
            y = self.jacobi(self.close(V))
            return np.concatenate([y[D].reshape(-1)[idx[D]] for D in range(3)]).astype(np.float64)
        v0 = np.random.default_rng(5).uniform(-1, 1, int(cut[-1]))
        lam = spla.eigs(spla.LinearOperator((int(cut[-1]),) * 2, matvec=mv, dtype=np.float64), k=1, which="LM", tol=tol, v0=v0,
                        return_eigenvectors=False)
        return float(np.abs(lam[0]))


def build_levels(grid, etas, etan, bc=None, strict=True, P=(1, 1, 1), dt=np.float64):
    """Level 0 with the wall-row mode given (strict: slaved rows), every coarse level with natural rows; the wall kinds on all."""
    es, en = np.asarray(etas, dtype=dt), np.asarray(etan, dtype=dt)
    out = []
    for l, g in enumerate(level_grids(grid, P)):
        if l > 0:
            es, en = coarsen_nodes(es), coarsen_centres(en)
        out.append(Level(g, es, en, bc, strict and l == 0, dt))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# transfers (the uniform-grid weights on every grid)
# ---------------------------------------------------------------------------------------------------------------------
def restrict(C, r):
    """Full weighting of the fine residual r onto the INT rows of the coarse level C: [1/4 1/2 1/4] around node 2I along the
    component's own axis, [1/8 3/8 3/8 1/8] from node 2J - 1 along the other two; zero on the other coarse rows."""
    out = []
    for D in range(3):
        a = np.pad(r[D], [(1, 2)] * 3)
        for ax in range(3):
            w = W3 if ax == D else W4
            a = sum(wk * np.take(a, 2 * np.arange(C.n[ax]) + k, axis=ax) for k, wk in enumerate(w))
        out.append(np.where(C.int_[D], a, 0))
    return out


def prolong(nf, C, e):
    """Interpolation of the coarse field e to every node of a fine grid of nf nodes: linear between the coarse nodes i // 2 and
    (i + 1) // 2 along the own axis; along the other two 3/4 of the nearest coarse midpoint i // 2 and 1/4 of the next one on the
    other side (+1 for odd i, -1 for even), both clamped to 0 .. n_coarse - 2."""
    out = []
    for D in range(3):
        a = e[D]
        for ax in range(3):
            i = np.arange(nf[ax])
            if ax == D:
                a = 0.5 * (np.take(a, i // 2, axis=ax) + np.take(a, (i + 1) // 2, axis=ax))
            else:
                near = i // 2
                other = np.where(i % 2 == 1, near + 1, near - 1)
                last = C.n[ax] - 2
                a = 0.75 * np.take(a, np.clip(near, 0, last), axis=ax) + 0.25 * np.take(a, np.clip(other, 0, last), axis=ax)
        out.append(a)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: the pressure block
# ---------------------------------------------------------------------------------------------------------------------
def pressure_block(grid, etan, Kc, rp, strict, dt=np.float64, terms=False):
    """z_p = S^-1 r_p from the scaled residual, class by class: ghost and anchor rows give r; continuity rows r sum(1/d) eta_n /
    Kcont; a symmetry row (P_nb - P = r) follows its chain -- inward along x on the z-x cube edges, inward along y on the others --
    to the first continuity or identity cell and gives that cell's value minus the residuals on the way.
    terms=True: also the sum of the absolute values of the terms of every entry."""
    g = [np.asarray(c, dtype=dt) for c in grid]
    n = [c.size for c in g]
    rp = np.asarray(rp, dtype=dt); en = np.asarray(etan, dtype=dt)
    cont, sx, sy = M.pressure_classes(n, strict)
    srd = sum(M._along(np.append(1 / np.diff(g[a]), dt(0)), a) for a in range(3))
    z = np.where(cont, rp * srd * en / Kc, rp)
    mag = np.abs(z)
    ix = M._index(n)
    # resolve the chains from their ends: first the y-symmetry cells (their neighbour is never a symmetry cell), then the x ones
    for m, ax in ((sy, 2), (sx, 1)):
        nb = [np.broadcast_to(ix[a], n) for a in range(3)]
        nb[ax] = np.where(nb[ax] == 0, 1, n[ax] - 3)
        z = np.where(m, z[tuple(nb)] - rp, z)
        mag = np.where(m, mag[tuple(nb)] + np.abs(rp), mag)
    return (z, mag) if terms else z


# ---------------------------------------------------------------------------------------------------------------------
# the preconditioner
# ---------------------------------------------------------------------------------------------------------------------
class Precond:
    """z = M^-1 r for a ROW-SCALED r, (nz, nx, ny, 4).

    bc: the six wall kinds (None: all FREESLIP); strict: the wall-row mode of level 0; P: the block layout (it only ends the
    hierarchy earlier); nu = (sweeps on the finest level, on the others), each run before and after the coarse correction; ratio:
    the Chebyshev window; coarse_sweeps: the least number of sweeps on the coarsest level; lmax: one bound per level from outside
    (None: 1.1 x the converged eigenvalue)."""

    def __init__(self, grid, etas, etan, bc=None, strict=True, P=(1, 1, 1), nu=(2, 2), ratio=6.0, coarse_sweeps=12, lmax=None,
                 ld=False):
        self.dt = dt = LD if ld else np.float64
        self.strict = bool(strict)
        self.nu, self.ratio, self.coarse_sweeps = tuple(nu), ratio, coarse_sweeps
        self.levels = build_levels(grid, etas, etan, bc, strict, P, dt)
        self.n = self.levels[0].n
        self.Kc = dt(M.scaling(grid, etas, etan)[0])
        self.lmax = list(lmax) if lmax is not None else [1.1 * L.lambda_max() for L in self.levels]
        assert len(self.lmax) == len(self.levels)

    def lambda_max(self, level):
        return self.levels[level].lambda_max()

    def power_iteration(self, level, iters=12, seed=0):
        return self.levels[level].power_iteration(iters, seed)

    def pressure(self, r, terms=False):
        R = np.asarray(r, dtype=self.dt).reshape(self.n + [4])
        L0 = self.levels[0]
        return pressure_block(L0.grid, L0.etan, self.Kc, R[..., 3], self.strict, self.dt, terms)

    def rhs(self, r, zp):
        """f = r_v * diag - A_vp z_p on the INT rows of level 0, zero elsewhere."""
        L0 = self.levels[0]
        R = np.asarray(r, dtype=self.dt).reshape(self.n + [4])
        X = np.zeros(self.n + [4], dtype=self.dt); X[..., 3] = zp
        G = L0._apply4(X)
        return [np.where(L0.int_[D], R[..., D] * -L0.diag[D] - G[..., D], 0) for D in range(3)]

    def vcycle(self, l, f):
        L, lmax = self.levels[l], self.dt(self.lmax[l])
        if l == len(self.levels) - 1:
            n, ratio = coarsest_sweeps(L.n, self.coarse_sweeps)
            return L.smooth(None, f, n, lmax, ratio)
        nu = self.nu[0] if l == 0 else self.nu[1]
        v = L.smooth(None, f, nu, lmax, self.ratio)
        C = self.levels[l + 1]
        e = self.vcycle(l + 1, restrict(C, L.residual(v, f)))
        p = prolong(L.n, C, e)
        v = L.close([v[D] + p[D] for D in range(3)])
        return L.smooth(v, f, nu, lmax, self.ratio)

    def apply(self, r, rounded=True, terms=False):
        """z; terms=True: (z, sum of |terms| of every pressure entry)."""
        zp, mag = self.pressure(r, terms=True)
        v = self.vcycle(0, self.rhs(r, zp))
        z = np.stack(v + [zp], axis=3).reshape(-1)
        z = z.astype(np.float64) if rounded else z
        return (z, mag.astype(np.float64)) if terms else z
