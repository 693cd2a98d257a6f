"""A plain NumPy model of the 2-D Stokes preconditioner z = M^-1 r on rectilinear grids, the reference the
HIP preconditioner of pl_solver.hip is compared with (tests/test_hip_mg_model.py).  No GPU, no project code beyond the oracle's
explicit matrix (for f = r_v - A_vp z_p): one rank, written for arrays of node coordinates, float64 or -- ld=True -- np.longdouble.
tests/test_stokes2_mg_model.py ties it to the oracle's matrix level by level and to oracle/proto_stokes_solver.py on uniform grids.

    M = [[A_vv, A_vp], [0, S^]]:   z_p = S^-1 r_p  (diagonal eta_n / Kc^2, or the wall stencil next to the walls of stretched cells),
                                    z_v = one V-cycle for A_vv z_v = r_v - A_vp z_p.

Everything that selects a path is an argument of Precond (sweeps, Chebyshev ratio, smoother per level, wall stencil, lmax per
level); the rules by which the solver chooses them from the grid alone are the functions line_levels, wall_stencil_on and
aniso_rule, so that a test can ask the device for what the model chose.

Arrays are (nz, nx): vz lives at (z_i, x_j+1/2), vx at (z_i+1/2, x_j), P and etan at the cell centres, etas and rho at the nodes; the
last row / column of a midpoint quantity is a ghost.  Vectors are C-order (nz, nx, 3) with the components vz, vx, P.
Row classes of a velocity component: ZERO (walls, ghosts), INT (carries an equation), SLAVE (s x its inner neighbour)."""
import numpy as np
from scipy.linalg import solve_banded

LD = np.longdouble
NOSLIP, FREESLIP = 0, 1
ANCHOR = (3, 2)                    # the pressure cell whose row is Kc * P
GRAV_Z = 9.81
ZERO, INT, SLAVE = 0, 1, 2
POINT, ZLINES, XLINES = -1, 0, 1   # smoother of a level (the line kinds are the device's line_ax)
LINE_MAX_PTS = 4097                # longest line the line smoother takes


# ---------------------------------------------------------------------------------------------------------------------
# selection rules: functions of the grid alone
# ---------------------------------------------------------------------------------------------------------------------
def level_grids(grid, min_cells=4):
    """Node coordinates of every level: every second node, until a cell count is odd or the next level would have fewer than
    min_cells cells per side."""
    z, x = np.asarray(grid[0]), np.asarray(grid[1])
    out = [(z, x)]
    while True:
        cz, cx = z.size - 1, x.size - 1
        if cz % 2 or cx % 2 or cz // 2 < min_cells or cx // 2 < min_cells:
            return out
        z, x = z[::2], x[::2]
        out.append((z, x))


def line_levels(grid, knob=-1, min_cells=4):
    """Smoother of every level.  A level takes z-lines where some cell is at least 6 x wider than high (widest dx over smallest dz)
    and that is its stronger anisotropy, x-lines where some cell is at least 6 x higher than wide; lines of 4 .. 4097 points only.
    knob: 0 never, 1 / 2 z- / x-lines on every level, -1 by the rule."""
    out = []
    for z, x in level_grids(grid, min_cells):
        dz, dx = np.diff(z), np.diff(x)
        wide, high = dx.max() / dz.min(), dz.max() / dx.min()
        kind, npts = POINT, 0
        if knob == 1 or (knob < 0 and wide >= 6.0 and wide >= high):
            kind, npts = ZLINES, z.size
        elif knob == 2 or (knob < 0 and high >= 6.0):
            kind, npts = XLINES, x.size
        out.append(kind if kind != POINT and 4 <= npts <= LINE_MAX_PTS else POINT)
    return out


def aniso_rule(grid, lines_allowed=True):
    """(Chebyshev ratio, sweeps or None) from the mean cell shape a: without line relaxation and a > 1.5 the window is widened to
    6 a^2 and ceil(2 a) <= 10 sweeps run before and after; otherwise ratio 6 and the default sweeps."""
    z, x = np.asarray(grid[0]), np.asarray(grid[1])
    hz, hx = (z[-1] - z[0]) / (z.size - 1), (x[-1] - x[0]) / (x.size - 1)
    a = hz / hx if hz > hx else hx / hz
    ok = lambda n: 4 <= n <= LINE_MAX_PTS
    lines = lines_allowed and ((hx >= 6.0 * hz and ok(z.size)) or (hz >= 6.0 * hx and ok(x.size)))
    if a > 1.5 and not lines:
        return 6.0 * a * a, min(10, int(np.ceil(2.0 * a)))
    return 6.0, None


def wall_stencil_on(grid, knob=-1):
    """Whether stage 1 applies the wall stencil at all: both axes >= 9 nodes, and a cell in the x-wall columns at least twice as wide
    as the lowest cell is high, or a cell in the z-wall rows twice as high as the narrowest is wide.  knob: 0 never, 1 always."""
    z, x = np.asarray(grid[0]), np.asarray(grid[1])
    if z.size < 9 or x.size < 9 or knob == 0:
        return False
    dz, dx = np.diff(z), np.diff(x)
    wx = max(dx[0], dx[-1]) / dz.min()
    wz = max(dz[0], dz[-1]) / dx.min()
    return knob == 1 or wx >= 2.0 or wz >= 2.0


def coarsest_sweeps(nz, nx, coarse_sweeps=12):
    """(sweeps, Chebyshev ratio) on the level that is not coarsened further."""
    ratio = max(30.0, 0.4 * nz * nx)
    return min(150, max(coarse_sweeps, int(np.sqrt(ratio)))), ratio


def cheb_coeffs(lmax, ratio, n):
    """c1, c2 of n three-term Chebyshev sweeps on [lmax / ratio, lmax]."""
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


def scaling(grid, etas, etan):
    """Kc, Kb of the reference (span / number of NODES, sic)."""
    mineta = min(np.min(etas), np.min(etan))
    s = sum((float(g[-1]) - float(g[0])) / len(g) for g in (grid[1], grid[0]))
    return 2 * mineta / s, 4 * mineta / s ** 2


# ---------------------------------------------------------------------------------------------------------------------
# hierarchy
# ---------------------------------------------------------------------------------------------------------------------
def coarsen_nodes(a):
    """[1 2 1] x [1 2 1] / 16 at every second node, edge values repeated beyond the walls."""
    p = np.pad(a, 1, mode="edge")
    w = (p[:-2, :-2] + p[:-2, 2:] + p[2:, :-2] + p[2:, 2:]) + 2 * (p[:-2, 1:-1] + p[2:, 1:-1] + p[1:-1, :-2] + p[1:-1, 2:]) + 4 * p[1:-1, 1:-1]
    return (w / 16)[::2, ::2]


def coarsen_centres(a):
    """Mean of the 2 x 2 fine cells a coarse cell covers; the ghost row and column copy their neighbours."""
    nz, nx = a.shape
    c = a[:nz - 1, :nx - 1]
    m = 0.25 * (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2])
    out = np.empty(((nz - 1) // 2 + 1, (nx - 1) // 2 + 1), dtype=a.dtype)
    out[:-1, :-1] = m
    out[-1, :-1] = m[-1, :]; out[:, -1] = out[:, -2]
    return out


def _tables(x):
    """rd[k] = 1 / (x[k+1] - x[k]), k = 0 .. n-2;  rD[k] = 1 / (x[k+1] - x[k-1]), k = 1 .. n-2; zero outside.  Stored at k + 2."""
    n = x.size
    rd = np.zeros(n + 4, dtype=x.dtype); rD = np.zeros(n + 4, dtype=x.dtype)
    rd[2:n + 1] = 1 / (x[1:] - x[:-1])
    rD[3:n + 1] = 1 / (x[2:] - x[:-2])
    return rd, rD


class Level:
    """The velocity block of one level from its reciprocal tables.  finest: the reference's slaved wall rows (vz columns 0 and
    nx-2 copy their inner neighbour, vx rows 0 and nz-2 copy theirs or, NOSLIP, take s x it); coarse levels: natural mirror rows,
    except the NOSLIP vx rows, which stay slaved with the factor of the level's own three coordinates.  Coefficients are stored
    with the sign of the device: A v = sum c (v_nb - v), diagonal -dg."""

    def __init__(self, z, x, etas, etan, bc, finest, rho=None, coef=0.0, dt=np.float64):
        self.dt = dt
        z = np.asarray(z, dtype=dt); x = np.asarray(x, dtype=dt)
        self.z, self.x = z, x
        nz, nx = self.nz, self.nx = z.size, x.size
        es = np.asarray(etas, dtype=dt); en = np.asarray(etan, dtype=dt)
        self.etas, self.etan = es, en
        rdz, rDz = _tables(z); rdx, rDx = _tables(x)
        i = np.arange(nz)[:, None]; j = np.arange(nx)[None, :]
        rdz_i, rdz_m, rDz_i, rDz_p = rdz[i + 2], rdz[i + 1], rDz[i + 2], rDz[i + 3]
        rdx_j, rdx_m, rDx_j, rDx_p = rdx[j + 2], rdx[j + 1], rDx[j + 2], rDx[j + 3]
        E, N = np.pad(es, 1), np.pad(en, 1)
        sh = self._sh
        # z rows: own couplings to (i+1, i-1, j+1, j-1), cross couplings to vx
        self.zN = 4 * en * rdz_i * rDz_i; self.zS = 4 * sh(N, -1, 0) * rdz_m * rDz_i
        self.zE = 2 * sh(E, 0, 1) * rDx_p * rdx_j; self.zW = 2 * es * rDx_j * rdx_j
        self.zxE = 2 * sh(E, 0, 1) * rDz_i * rdx_j; self.zxW = 2 * es * rDz_i * rdx_j
        # x rows: own couplings to (j+1, j-1, i+1, i-1), cross couplings to vz
        self.xE = 4 * en * rdx_j * rDx_j; self.xW = 4 * sh(N, 0, -1) * rdx_m * rDx_j
        self.xN = 2 * sh(E, 1, 0) * rDz_p * rdz_i; self.xS = 2 * es * rDz_i * rdz_i
        self.xzN = 2 * sh(E, 1, 0) * rDx_j * rdz_i; self.xzS = 2 * es * rDx_j * rdz_i
        # row classes
        ns0, nsL = bc[0] != FREESLIP, bc[2] != FREESLIP
        self.slave_x = bool(finest)
        self.slave_z0, self.slave_zL = bool(finest or ns0), bool(finest or nsL)
        self.s0 = (1 / (z[2] - z[0])) / (1 / (z[2] - z[0]) + 1 / (z[1] - z[0])) if ns0 else dt(1)
        self.sL = (1 / (z[-1] - z[-3])) / (1 / (z[-1] - z[-3]) + 1 / (z[-1] - z[-2])) if nsL else dt(1)
        cz = np.zeros((nz, nx), dtype=np.int8); cz[1:nz - 1, 0:nx - 1] = INT
        if self.slave_x:
            cz[1:nz - 1, 0] = SLAVE; cz[1:nz - 1, nx - 2] = SLAVE
        cx = np.zeros((nz, nx), dtype=np.int8); cx[0:nz - 1, 1:nx - 1] = INT
        if self.slave_z0:
            cx[0, 1:nx - 1] = SLAVE
        if self.slave_zL:
            cx[nz - 2, 1:nx - 1] = SLAVE
        self.cz, self.cx = cz, cx
        self.iz, self.ix = cz == INT, cx == INT
        # free-surface stabilisation of the z rows, rediscretised on this level: row_z += szz vz + szx vx
        self.szz = self.szx = None
        dgz = self.zN + self.zS + self.zE + self.zW
        if rho is not None and coef != 0.0:
            rho = np.asarray(rho, dtype=dt); self.rho = rho
            R = np.pad(rho, 1)
            jm = np.where(j > 0, -1, 0) + 0 * i; jp = np.where(j < nx - 1, 1, 0) + 0 * i
            I = i + 0 * j; J = j + 0 * i
            at = lambda di, dj: R[I + 1 + di, J + 1 + dj]
            hx = np.where((jm != 0) & (jp != 0), rDx_j + 0 * rdz_i, rdx_j + 0 * rdz_i)
            a = coef * 0.5 * (at(1, 0) + at(1, jp) - at(-1, 0) - at(-1, jp)) * rDz_i
            b = coef * 0.5 * (at(0, jp) + at(1, jp) - at(0, jm) - at(1, jm)) * hx
            self.szz = np.where(self.iz, a, 0); self.szx = np.where(self.iz, b, 0)
            d = dgz - self.szz                       # the smoother keeps the diagonal at least half the viscous one
            dgz = np.where(d > 0.5 * dgz, d, 0.5 * dgz)
        one = dt(1)
        self.dgz = np.where(self.iz, dgz, one)
        self.dgx = np.where(self.ix, self.xE + self.xW + self.xN + self.xS, one)

    def _sh(self, a, di, dj):
        """b[i, j] = a[i + di, j + dj] of an array padded by one."""
        return a[1 + di:self.nz + 1 + di, 1 + dj:self.nx + 1 + dj]

    def close(self, vz, vx):
        """Constraint rows: walls and ghosts 0, slaved rows s x their master."""
        nz, nx = self.nz, self.nx
        vz = np.where(self.iz, vz, 0); vx = np.where(self.ix, vx, 0)
        if self.slave_x:
            vz[1:nz - 1, 0] = vz[1:nz - 1, 1]; vz[1:nz - 1, nx - 2] = vz[1:nz - 1, nx - 3]
        if self.slave_z0:
            vx[0, 1:nx - 1] = self.s0 * vx[1, 1:nx - 1]
        if self.slave_zL:
            vx[nz - 2, 1:nx - 1] = self.sL * vx[nz - 3, 1:nx - 1]
        return vz, vx

    def apply(self, vz, vx):
        """A_vv v on the INT rows (zero elsewhere) of a closed v."""
        sh = self._sh
        Z, X = np.pad(vz, 1), np.pad(vx, 1)
        z0, x0 = vz, vx
        yz = (self.zN * (sh(Z, 1, 0) - z0) - self.zS * (z0 - sh(Z, -1, 0)) + self.zE * (sh(Z, 0, 1) - z0) - self.zW * (z0 - sh(Z, 0, -1))
              + self.zxE * (sh(X, 0, 1) - sh(X, -1, 1)) - self.zxW * (x0 - sh(X, -1, 0)))
        if self.szz is not None:
            yz = yz + self.szz * z0 + self.szx * x0
        yx = (self.xE * (sh(X, 0, 1) - x0) - self.xW * (x0 - sh(X, 0, -1)) + self.xN * (sh(X, 1, 0) - x0) - self.xS * (x0 - sh(X, -1, 0))
              + self.xzN * (sh(Z, 1, 0) - sh(Z, 1, -1)) - self.xzS * (z0 - sh(Z, 0, -1)))
        return np.where(self.iz, yz, 0), np.where(self.ix, yx, 0)

    # ---- the splitting: D (point), or the tridiagonal T of each component's own couplings along the line axis
    def line_matrix(self, comp, ax):
        """(lower, diagonal, upper) of T, each (nz, nx): T v = dg v - c_next v[next] - c_prev v[prev] on the INT rows, couplings to
        rows that are not INT dropped; every other row is an identity row."""
        m = self.iz if comp == 0 else self.ix
        dg = self.dgz if comp == 0 else self.dgx
        if comp == 0:
            nxt, prv = (self.zN, self.zS) if ax == 0 else (self.zE, self.zW)
        else:
            nxt, prv = (self.xN, self.xS) if ax == 0 else (self.xE, self.xW)
        mp = np.pad(m, 1)
        d = (1, 0) if ax == 0 else (0, 1)
        up = np.where(m & self._sh(mp, d[0], d[1]), -nxt, 0)
        lo = np.where(m & self._sh(mp, -d[0], -d[1]), -prv, 0)
        return lo, dg, up

    def line_solve(self, comp, ax, rhs):
        """T^-1 rhs (rhs zero outside the INT rows), line by line.  float64: LAPACK's banded solve of all lines at once (they do
        not couple); longdouble: the same solve refined three times with the residual in longdouble."""
        lo, dg, up = self.line_matrix(comp, ax)
        t = (lambda a: a.T) if ax == 0 else (lambda a: a)           # lines contiguous
        lo, dg, up, b = (np.ascontiguousarray(t(a)).reshape(-1) for a in (lo, dg, up, rhs))
        ab = np.zeros((3, b.size))
        ab[0, 1:] = up[:-1]; ab[1] = dg; ab[2, :-1] = lo[1:]
        x = solve_banded((1, 1), ab, b.astype(np.float64)).astype(self.dt)
        if self.dt is LD:
            for _ in range(3):
                r = b - dg * x
                r[:-1] -= up[:-1] * x[1:]; r[1:] -= lo[1:] * x[:-1]
                x = x + solve_banded((1, 1), ab, r.astype(np.float64))
        return t(x.reshape(t(rhs).shape))

    def precondition(self, kind, gz, gx):
        """D^-1 g or T^-1 g on the INT rows, for g = A v - f there (sign of the device: D = -diag A)."""
        gz = np.where(self.iz, gz, 0); gx = np.where(self.ix, gx, 0)
        if kind == POINT:
            return gz / self.dgz, gx / self.dgx
        return self.line_solve(0, kind, gz), self.line_solve(1, kind, gx)

    def iteration_matrix_apply(self, kind, vz, vx):
        """close(D^-1 A v) resp. close(T^-1 A v): the matrix whose largest eigenvalue is lambda_max."""
        vz, vx = self.close(vz, vx)
        yz, yx = self.apply(vz, vx)
        return self.close(*self.precondition(kind, yz, yx))

    def smooth(self, kind, vz, vx, fz, fx, n, lmax, ratio):
        """n Chebyshev sweeps  v <- v + c1 (v - v_prev) + c2 B^-1 (A v - f),  B = D or T, slaved rows copied after each."""
        c1, c2 = cheb_coeffs(lmax, ratio, n)
        pz, px = vz, vx
        for k in range(n):
            yz, yx = self.apply(vz, vx)
            dz, dx = self.precondition(kind, yz - fz, yx - fx)
            nz_ = vz + c1[k] * (vz - pz) + c2[k] * dz
            nx_ = vx + c1[k] * (vx - px) + c2[k] * dx
            pz, px = vz, vx
            vz, vx = self.close(nz_, nx_)
        return vz, vx

    def lambda_max(self, kind, tol=1e-6):
        """Largest eigenvalue of the iteration matrix, converged to tol (ARPACK on the float64 operator)."""
        from scipy.sparse.linalg import LinearOperator, eigs
        n = self.nz * self.nx
        sp_ = (self.nz, self.nx)

        def mv(v):
            v = np.asarray(v, dtype=self.dt).reshape(-1)
            yz, yx = self.iteration_matrix_apply(kind, v[:n].reshape(sp_), v[n:].reshape(sp_))
            return np.concatenate([yz.reshape(-1), yx.reshape(-1)]).astype(np.float64)
        v0 = np.random.default_rng(0).standard_normal(2 * n)
        w = eigs(LinearOperator((2 * n, 2 * n), matvec=mv, dtype=np.float64), k=1, which="LM", tol=tol, v0=v0, ncv=min(2 * n - 1, 40),
                 maxiter=200000, return_eigenvectors=False)
        return float(np.abs(w[0]))

    def lambda_power(self, kind, iters=12, seed=0):
        """The estimate of a cold solve: `iters` power iterations from a random start."""
        rng = np.random.default_rng(seed)
        vz, vx = self.close(rng.standard_normal((self.nz, self.nx)), rng.standard_normal((self.nz, self.nx)))
        lam = 0.0
        for _ in range(iters):
            n0 = np.sqrt(np.sum(vz ** 2) + np.sum(vx ** 2))
            yz, yx = self.iteration_matrix_apply(kind, vz, vx)
            lam = float(np.sqrt(np.sum(yz ** 2) + np.sum(yx ** 2)) / n0)
            vz, vx = yz / lam, yx / lam
        return lam


def build_levels(grid, etas, etan, bc, rho=None, coef=0.0, min_cells=4, dt=np.float64):
    """Every second node; viscosities (and the density of a stabilised operator) coarsened arithmetically."""
    es, en = np.asarray(etas, dtype=dt), np.asarray(etan, dtype=dt)
    rh = None if rho is None else np.asarray(rho, dtype=dt)
    out = []
    for l, (z, x) in enumerate(level_grids(grid, min_cells)):
        if l > 0:
            es, en = coarsen_nodes(es), coarsen_centres(en)
            if rh is not None:
                rh = coarsen_nodes(rh)
        out.append(Level(z, x, es, en, bc, l == 0, rh, coef, dt))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# transfers (the uniform-grid weights the kernels use on every grid)
# ---------------------------------------------------------------------------------------------------------------------
W3 = (0.25, 0.5, 0.25)
W4 = (0.125, 0.375, 0.375, 0.125)


def restrict(C, rz, rx):
    """Full weighting of the fine residual onto the INT rows of the coarse level C: vz is a vertex quantity in z (1/4 1/2 1/4 around
    row 2I) and a centre quantity in x (1/8 3/8 3/8 1/8 from column 2J - 1); vx the other way round."""
    nzc, nxc = C.nz, C.nx
    Z, X = np.pad(rz, 2), np.pad(rx, 2)
    I = 2 * np.arange(nzc)[:, None] + 2; J = 2 * np.arange(nxc)[None, :] + 2
    cz = sum(wi * wj * Z[I + di - 1, J + dj - 1] for di, wi in enumerate(W3) for dj, wj in enumerate(W4))
    cx = sum(wi * wj * X[I + di - 1, J + dj - 1] for di, wi in enumerate(W4) for dj, wj in enumerate(W3))
    return np.where(C.iz, cz, 0), np.where(C.ix, cx, 0)


def prolong(F, C, ez, ex):
    """Bilinear interpolation of the closed coarse correction to every node of the fine level F: linear between the two coarse
    vertices along a component's vertex axis, 3/4 - 1/4 between the two nearest coarse centres along its centre axis (the centre
    beyond a wall is the one inside it)."""
    def nearest_other(k, last):
        near = k // 2
        other = np.where(k % 2 == 1, near + 1, near - 1)
        return np.clip(near, 0, last), np.clip(other, 0, last)
    i = np.arange(F.nz); j = np.arange(F.nx)
    I0, I1 = (i // 2)[:, None], ((i + 1) // 2)[:, None]
    Jn, Jo = nearest_other(j, C.nx - 2)
    a = 0.5 * (ez[I0, Jn[None, :]] + ez[I1, Jn[None, :]]); b = 0.5 * (ez[I0, Jo[None, :]] + ez[I1, Jo[None, :]])
    pz = 0.75 * a + 0.25 * b
    J0, J1 = (j // 2)[None, :], ((j + 1) // 2)[None, :]
    In, Io = nearest_other(i, C.nz - 2)
    a = 0.5 * (ex[In[:, None], J0] + ex[In[:, None], J1]); b = 0.5 * (ex[Io[:, None], J0] + ex[Io[:, None], J1])
    px = 0.75 * a + 0.25 * b
    return pz, px


# ---------------------------------------------------------------------------------------------------------------------
# stage 1: the pressure block
# ---------------------------------------------------------------------------------------------------------------------
def continuity_mask(nz, nx):
    """Plain continuity rows: every cell but the anchor and the four corner cells."""
    m = np.zeros((nz, nx), dtype=bool); m[:nz - 1, :nx - 1] = True
    m[ANCHOR] = False
    for i in (0, nz - 2):
        for j in (0, nx - 2):
            m[i, j] = False
    return m


def _wall_pairs(A2, gate, EN, RH, CONT):
    """The wall stencil for walls along axis 0 of the arrays given: cell pairs (wall, neighbour) = columns (0, 1) and (n-2, n-3).
    A2: the squared aspect ratio (long over short edge) of every cell; gate: where a cell may take the stencil.
    Returns (took, value, sum of |terms|)."""
    n1 = RH.shape[1]
    took = np.zeros(RH.shape, dtype=bool); val = np.zeros_like(RH); mag = np.zeros_like(RH)
    for jw, ji in ((0, 1), (n1 - 2, n1 - 3)):
        pair = CONT[:, jw] & CONT[:, ji]
        r0, r1 = RH[:, jw], RH[:, ji]
        d = np.where(pair, r0 - r1, 0)
        pm, dm = np.pad(pair, 1), np.pad(d, 1)
        d2 = np.where(pm[:-2], dm[:-2] - d, 0) + np.where(pm[2:], dm[2:] - d, 0)
        ad2 = np.where(pm[:-2], np.abs(dm[:-2]) + np.abs(d), 0) + np.where(pm[2:], np.abs(dm[2:]) + np.abs(d), 0)
        took[:, ji] = pair & gate[:, ji]
        val[:, ji] = EN[:, ji] * (0.25 * r0 + 0.775 * r1)
        mag[:, ji] = EN[:, ji] * (0.25 * np.abs(r0) + 0.775 * np.abs(r1))
        took[:, jw] = pair & gate[:, jw]
        val[:, jw] = EN[:, jw] * (1.45 * r0 - 0.225 * r1 - 0.25 * A2[:, jw] * d2)
        mag[:, jw] = EN[:, jw] * (1.45 * np.abs(r0) + 0.225 * np.abs(r1) + 0.25 * A2[:, jw] * ad2)
    return took, val, mag


def pressure_block(grid, etan, Kc, Kb, rp, wall, dt=np.float64, terms=False):
    """z_p = S^-1 r_p.  Continuity rows eta_n r / Kc^2; ghost rows and the anchor r / Kc; a corner cell takes its neighbour's
    diagonal value minus r / Kb.  wall: in the two cell columns next to an x-wall, where the cell is at least twice as wide as high
    (a = dx / dz >= 2), with r^ = r / Kc^2, wall column 0 and its neighbour 1, d = r^0 - r^1,
        z_0(i) = eta_n [1.45 r^0 - 0.225 r^1 - a^2/4 (d(i-1) - 2 d(i) + d(i+1))],     z_1(i) = eta_n [0.25 r^0 + 0.775 r^1]
    (a row pair that holds the anchor or a corner cell takes no stencil and adds no term to its neighbours' second difference), and
    the same with rows and columns swapped, 1/a for a, next to the z-walls where 1/6 < a <= 1/2.  Both axes need 9 nodes.
    terms=True: also the sum of the absolute values of the terms of every entry (for a row-wise bar)."""
    z, x = np.asarray(grid[0], dtype=dt), np.asarray(grid[1], dtype=dt)
    nz, nx = z.size, x.size
    en = np.asarray(etan, dtype=dt); rp = np.asarray(rp, dtype=dt)
    cont = continuity_mask(nz, nx)
    rh = np.where(cont, rp / Kc ** 2, 0)
    zp = np.where(cont, en * rh, rp / Kc)
    mag = np.abs(zp)
    for i0 in (0, nz - 2):
        for jc, jn in ((0, 1), (nx - 2, nx - 3)):
            zp[i0, jc] = en[i0, jn] * rh[i0, jn] - rp[i0, jc] / Kb
            mag[i0, jc] = abs(en[i0, jn] * rh[i0, jn]) + abs(rp[i0, jc] / Kb)
    if wall and nz >= 9 and nx >= 9:
        # the gates are decided in float64 from the reciprocal widths, whatever dt is
        z64, x64 = np.asarray(grid[0], dtype=np.float64), np.asarray(grid[1], dtype=np.float64)
        a64 = np.zeros((nz, nx)); a64[:nz - 1, :nx - 1] = (1 / np.diff(z64))[:, None] / (1 / np.diff(x64))[None, :]
        a = np.ones((nz, nx), dtype=dt); a[:nz - 1, :nx - 1] = (1 / np.diff(z))[:, None] / (1 / np.diff(x))[None, :]
        tx, vx_, mx_ = _wall_pairs(a * a, a64 >= 2.0, en, rh, cont)
        tz, vz_, mz_ = _wall_pairs((1 / (a * a)).T, ((a64 <= 0.5) & (a64 > 1.0 / 6.0)).T, en.T, rh.T, cont.T)
        zp = np.where(tx, vx_, np.where(tz.T, vz_.T, zp))
        mag = np.where(tx, mx_, np.where(tz.T, mz_.T, mag))
    return (zp, mag) if terms else zp


# ---------------------------------------------------------------------------------------------------------------------
# the preconditioner
# ---------------------------------------------------------------------------------------------------------------------
def _matvec(A, x, dt):
    """Sparse A times x with the products and sums in dt."""
    A = A.tocoo()
    y = np.zeros(A.shape[0], dtype=dt)
    np.add.at(y, A.row, A.data.astype(dt) * np.asarray(x, dtype=dt)[A.col])
    return y


class Precond:
    """z = M^-1 r for an UNSCALED r in the reference's DOF order, one rank.

    nu = (pre, post) sweeps, nu0 those of level 0 (None: as nu); ratio the Chebyshev window; coarse_sweeps the least number of
    sweeps on the coarsest level; smoothers one of POINT / ZLINES / XLINES per level (None: line_levels' choice); wall the wall
    stencil of the pressure block (None: wall_stencil_on's choice); lmax one value per level (None: 1.1 x the converged
    eigenvalue); rho / tstep / theta: the free-surface stabilisation terms in the velocity block of every level."""

    def __init__(self, nx, grid, etas, etan, bc, nu=(2, 2), nu0=None, ratio=6.0, coarse_sweeps=12, smoothers=None, wall=None,
                 lmax=None, rho=None, tstep=None, theta=0.5, min_cells=4, ld=False):
        from oracle import pylamp_oracle as O
        self.dt = dt = LD if ld else np.float64
        self.nx = [int(nx[0]), int(nx[1])]
        self.grid = grid
        self.nu, self.nu0, self.ratio, self.coarse_sweeps = nu, nu0 or nu, ratio, coarse_sweeps
        stab = tstep is not None and rho is not None
        coef = theta * tstep * GRAV_Z if stab else 0.0
        self.levels = build_levels(grid, etas, etan, bc, rho if stab else None, coef, min_cells, dt)
        self.smoothers = list(smoothers) if smoothers is not None else line_levels(grid, -1, min_cells)
        assert len(self.smoothers) == len(self.levels)
        self.wall = wall_stencil_on(grid) if wall is None else bool(wall)
        self.Kc, self.Kb = scaling(grid, etas, etan)
        self.lmax = list(lmax) if lmax is not None else [1.1 * L.lambda_max(k) for L, k in zip(self.levels, self.smoothers)]
        assert len(self.lmax) == len(self.levels)
        # A_vp of the reference's matrix (the pressure columns of the momentum rows)
        A, _ = O.stokes_csr(self.nx, grid, np.asarray(etas, dtype=np.float64), np.asarray(etan, dtype=np.float64),
                            np.zeros(self.nx) if rho is None else np.asarray(rho, dtype=np.float64), bc)
        N = self.nx[0] * self.nx[1]
        iv = np.sort(np.concatenate([np.arange(N) * 3, np.arange(N) * 3 + 1])); ip = np.arange(N) * 3 + 2
        self.Avp = A[iv][:, ip].tocoo()

    def pressure(self, r, terms=False):
        R = np.asarray(r, dtype=self.dt).reshape(self.nx[0], self.nx[1], 3)
        return pressure_block(self.grid, self.levels[0].etan, self.Kc, self.Kb, R[:, :, 2], self.wall, self.dt, terms)

    def vcycle(self, l, fz, fx):
        L, kind, lmax = self.levels[l], self.smoothers[l], self.lmax[l]
        zero = np.zeros((L.nz, L.nx), dtype=self.dt)
        if l == len(self.levels) - 1:
            n, ratio = coarsest_sweeps(L.nz, L.nx, self.coarse_sweeps)
            return L.smooth(kind, zero, zero, fz, fx, n, lmax, ratio)
        pre, post = self.nu0 if l == 0 else self.nu
        vz, vx = L.smooth(kind, zero, zero, fz, fx, pre, lmax, self.ratio)
        yz, yx = L.apply(vz, vx)
        C = self.levels[l + 1]
        cz, cx = restrict(C, np.where(L.iz, fz - yz, 0), np.where(L.ix, fx - yx, 0))
        ez, ex = self.vcycle(l + 1, cz, cx)
        pz, px = prolong(L, C, ez, ex)
        vz, vx = L.close(vz + pz, vx + px)
        return L.smooth(kind, vz, vx, fz, fx, post, lmax, self.ratio)

    def apply(self, r, rounded=True):
        nz, nx = self.nx
        L0 = self.levels[0]
        R = np.asarray(r, dtype=self.dt).reshape(nz, nx, 3)
        zp = self.pressure(r)
        g = _matvec(self.Avp, zp.reshape(-1), self.dt).reshape(nz, nx, 2)
        fz = np.where(L0.iz, R[:, :, 0] - g[:, :, 0], 0); fx = np.where(L0.ix, R[:, :, 1] - g[:, :, 1], 0)
        vz, vx = self.vcycle(0, fz, fx)
        z = np.stack([vz, vx, zp], axis=2).reshape(-1)
        return z.astype(np.float64) if rounded else z
