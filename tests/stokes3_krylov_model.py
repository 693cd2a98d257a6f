"""A plain NumPy model of what lies between the 3-D Stokes preconditioner and the numbers a solve hands back:
the shadow residual, the hydrostatic start with its reference norm, the deflation of the pressure-anchor mode, the right-preconditioned
BiCGStab recurrence in correction form with its stopping rule, and the velocity-error estimate.  tests/test_hip_3d_krylov.py compares
the device with it; tests/test_stokes3_krylov_model.py says why it can be trusted.  No GPU, no project code.  It is written from the
equations and stands on the models below it: the operator and the right-hand side of tests/stokes3_walls_model.py /
stokes3_moving_model.py / stokes3_flow_model.py and the preconditioner of tests/stokes3_mg_model.py.

Everything is evaluated in float64 or -- ld=True -- in np.longdouble (stokes3_model.working_precision).  Vectors are flat C-order
(nz, nx, ny, 4) = vz, vx, vy, P.  The system is the ROW-SCALED one the solve iterates on: every row divided by the coefficient of its own
unknown (stokes3_moving_model.row_divisor).
"""
import numpy as np

import stokes3_flow_model as F
import stokes3_mg_model as G
import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W

LD = np.longdouble
RTOL, ETOL, MAXIT = 1e-7, 3e-8, 600
MAX_CHECKS = 6
SHADOW_SEED = 1234


def dot(a, b):
    return np.sum(a * b)


def norm(a):
    return np.sqrt(np.sum(a * a))


# ---------------------------------------------------------------------------------------------------------------------
# the shadow residual
# ---------------------------------------------------------------------------------------------------------------------
def shadow(nx, seed=SHADOW_SEED):
    """(nz, nx, ny, 4) float64: component c is an integer hash of the node index (i, j, k) with the seed `seed + c`, mapped to [-1, 1) as
    h 2 / 2^32 - 1, on the nodes with i < nz - 1, j < nx - 1, k < ny - 1 and zero elsewhere.  The hash, in uint32 arithmetic:
    h = (73856093 i) xor (19349663 j) xor (83492791 k) xor seed;  h ^= h >> 16;  h *= 0x7feb352d;  h ^= h >> 15;  h *= 0x846ca68b;
    h ^= h >> 16.  Every step is exact in uint32, and so is the map to float64."""
    n = [int(v) for v in nx]
    i, j, k = [a.astype(np.uint32) for a in np.meshgrid(*[np.arange(v) for v in n], indexing="ij")]
    inside = (i < n[0] - 1) & (j < n[1] - 1) & (k < n[2] - 1)
    out = np.zeros(n + [4])
    with np.errstate(over="ignore"):
        base = (i * np.uint32(73856093)) ^ (j * np.uint32(19349663)) ^ (k * np.uint32(83492791))
        for c in range(4):
            h = base ^ np.uint32((int(seed) + c) & 0xFFFFFFFF)
            h = h ^ (h >> np.uint32(16)); h = h * np.uint32(0x7feb352d)
            h = h ^ (h >> np.uint32(15)); h = h * np.uint32(0x846ca68b)
            h = h ^ (h >> np.uint32(16))
            out[..., c] = np.where(inside, h.astype(np.float64) * (2.0 / 4294967296.0) - 1.0, 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the system
# ---------------------------------------------------------------------------------------------------------------------
class System:
    """The row-scaled Stokes system of one problem: A(x), b, the hydrostatic start and the deflation vectors, in the precision chosen.

    bc: six wall kinds (None: free-slip); strict: slaved wall rows; grav: (gz, gx, gy) (None: stokes3_model.GRAV); wallflow: the flow
    through the walls (stokes3_flow_model).  divisor: row_divisor of the problem, if the caller has it already."""

    def __init__(self, grid, etas, etan, rho, bc=None, strict=True, grav=None, wallflow=None, ld=True, divisor=None):
        self.dt = dt = LD if ld else np.float64
        self.grid = [np.asarray(c, dtype=np.float64) for c in grid]
        self.n = [c.size for c in self.grid]
        self.etas, self.etan, self.rho = [np.asarray(a, dtype=np.float64) for a in (etas, etan, rho)]
        self.bc, self.strict, self.wallflow = bc, bool(strict), wallflow
        self.grav = tuple(M.GRAV if grav is None else grav)
        self.Kc = dt(M.scaling(self.grid, self.etas, self.etan)[0])
        self._b = None
        g = [np.asarray(c, dtype=dt) for c in self.grid]
        self.width = [M._along(np.append(np.diff(g[a]), dt(1)), a) for a in range(3)]           # cell widths (1 on the ghost layer)
        self.cont, sx, sy = M.pressure_classes(self.n, self.strict)
        if divisor is None:
            # velocity rows: the coefficient of the row's own unknown; pressure rows: a continuity row by Kc sum_a 1 / d_a (it becomes
            # div v / sum_a 1 / d_a), a symmetry row by Kbond (it becomes P_nb - P), an identity row by Kc
            divisor = V.row_divisor(self.n, self.grid, self.etas, self.etan, bc, strict)
            Kc, Kb = M.scaling(self.grid, self.etas, self.etan)
            srd = sum(M._along(np.append(1 / np.diff(self.grid[a]), 0.0), a) for a in range(3))
            divisor[..., 3] = np.where(self.cont, Kc * srd, np.where(sx | sy, Kb, Kc))
        self.divisor = divisor

    def other(self, ld):
        """The same system in the other precision (the divisor is shared)."""
        return System(self.grid, self.etas, self.etan, self.rho, self.bc, self.strict, self.grav, self.wallflow, ld, self.divisor)

    def A(self, x):
        """The row-scaled operator."""
        with M.working_precision(self.dt):
            y = W.stokes_apply(self.n, self.grid, self.etas, self.etan, np.asarray(x, dtype=self.dt), bc=self.bc, strict=self.strict,
                               rounded=False)
        return np.asarray(y, dtype=self.dt) / np.asarray(self.divisor, dtype=self.dt).reshape(-1)

    @property
    def b(self):
        """The row-scaled right-hand side (rounded to float64: it is data of the iteration)."""
        if self._b is None:
            self._b = np.asarray(F.stokes_rhs_scaled(self.n, self.grid, self.etas, self.etan, self.rho, grav=self.grav, bc=self.bc,
                                                     wallflow=self.wallflow, strict=self.strict, divisor=self.divisor), dtype=self.dt)
        return self._b

    # ---- hydrostatic start ----
    def column_load(self):
        """The gravity term of the z-momentum right-hand side on every row 1 .. nz - 2 of every column of cells, as the natural rows
        carry it: -g_z times the density averaged onto the face (nz, nx, ny; zero on the walls and the ghosts)."""
        with M.working_precision(self.dt):
            R = M.stokes_rhs(self.n, self.grid, self.etas, self.etan, self.rho, grav=self.grav, strict=False, rounded=False)
        return np.asarray(R, dtype=self.dt).reshape(self.n + [4])[..., 0]

    def hydrostatic(self, terms=False):
        """x_h: zero velocities; the pressure integrates -2 Kc rD_i (P_i - P_{i-1}) = b_z, rD_i = 1 / (z_{i+1} - z_{i-1}), down every
        column from P_0 = 0, then shifts so that the anchor cell is zero; ghost planes zero.  terms=True: also the sum of the absolute
        values of the terms of every column's pressure (nz, nx, ny)."""
        dt, n = self.dt, self.n
        z = np.asarray(self.grid[0], dtype=dt)
        bz = self.column_load()
        step = np.zeros(n, dtype=dt)
        step[1:-1] = -bz[1:-1] * (z[2:] - z[:-2])[:, None, None] / (2 * self.Kc)
        P = np.cumsum(step, axis=0)
        mag = np.cumsum(np.abs(step), axis=0)
        anchor = P[M.ANCHOR]
        P = P - anchor
        ix = M._index(n)
        ghost = (ix[0] >= n[0] - 1) | (ix[1] >= n[1] - 1) | (ix[2] >= n[2] - 1)
        P = np.where(ghost, 0, P)
        x = np.zeros(n + [4], dtype=dt)
        x[..., 3] = P
        x = x.reshape(-1)
        if terms:
            return x, np.where(ghost, 0, mag + np.abs(anchor))
        return x

    def reference_norm(self, xh=None):
        """|b - A x_h|, returned as 0 when it is <= 1e-9 |b|."""
        xh = self.hydrostatic() if xh is None else xh
        ref, bn = norm(self.b - self.A(xh)), norm(self.b)
        return ref if ref > 1e-9 * bn else self.dt(0)

    # ---- deflation of the pressure-anchor mode ----
    def deflation_vectors(self):
        """(u, yw), each (nz, nx, ny): u = 1 / (eta_n sum_a 1 / d_a) and yw = cell volume x sum_a 1 / d_a on the continuity cells, zero
        elsewhere.  u is the continuity residual that the pressure stage of the preconditioner turns into the constant 1 / Kc."""
        dt = self.dt
        srd = sum(1 / self.width[a] for a in range(3))
        vol = self.width[0] * self.width[1] * self.width[2]
        u = np.where(self.cont, 1 / (np.asarray(self.etan, dtype=dt) * srd), 0)
        yw = np.where(self.cont, vol * srd, 0)
        return u, yw

    def cont_rows(self, v):
        """The scaled continuity rows of the velocity part of the flat vector v, (nz, nx, ny): div v / sum_a 1 / d_a, zero elsewhere."""
        X = np.asarray(v, dtype=self.dt).reshape(self.n + [4])
        div = sum((M._shift(X[..., a], a, 1) - X[..., a]) / self.width[a] for a in range(3))
        return np.where(self.cont, div / sum(1 / self.width[a] for a in range(3)), 0)

    def u_vector(self):
        x = np.zeros(self.n + [4], dtype=self.dt)
        x[..., 3] = self.deflation_vectors()[0]
        return x.reshape(-1)

    def yAw(self, w):
        return dot(self.deflation_vectors()[1], self.cont_rows(w))

    def M_deflated(self, Mfn, w, terms=False):
        """r -> M r + w (yw . r_p - yw . cont_rows((M r)_vel)) / (yw . cont_rows(w_vel)): afterwards yw . (r - A z)_cont = 0.
        terms=True: the function returns (z, coef)."""
        yw = self.deflation_vectors()[1]
        w = np.asarray(w, dtype=self.dt)
        yAw = dot(yw, self.cont_rows(w))

        def apply(r):
            r = np.asarray(r, dtype=self.dt)
            z = Mfn(r)
            coef = (dot(yw, r.reshape(self.n + [4])[..., 3]) - dot(yw, self.cont_rows(z))) / yAw
            z = z + coef * w
            return (z, coef) if terms else z
        return apply

    def vel(self, x):
        return np.asarray(x, dtype=self.dt).reshape(-1, 4)[:, :3]

    def prs(self, x):
        return np.asarray(x, dtype=self.dt).reshape(-1, 4)[:, 3]

    # ---- the velocity-error estimate ----
    def estimate(self, s, Ms, x, yAw=None, wvel2=None):
        """(n_amp |s_cont| + |(M s)_vel|) / |x_vel|, n_amp = max(nz, nx, ny), for the residual s of the iterate x and its preconditioned
        image Ms; with a deflation (yAw, |w_vel|^2) plus the anchor term |yw . s_p / yAw| sqrt(|w_vel|^2 / |x_vel|^2)."""
        xx = dot(self.vel(x), self.vel(x))
        if not xx > 0:
            return self.dt(0)
        est = (max(self.n) * norm(self.prs(s)) + norm(self.vel(Ms))) / np.sqrt(xx)
        if yAw is not None:
            yw = self.deflation_vectors()[1].reshape(-1)
            est = est + abs(dot(yw, self.prs(s)) / yAw) * np.sqrt(wvel2 / xx)
        return est


def preconditioner(sys_, lmax, **knobs):
    """M r of tests/stokes3_mg_model.py for the system, in its precision, with the bounds lmax (one per level)."""
    P = G.Precond(sys_.grid, sys_.etas, sys_.etan, bc=sys_.bc, strict=sys_.strict, lmax=lmax, ld=sys_.dt is LD, **knobs)
    return lambda r: np.asarray(P.apply(np.asarray(r, dtype=sys_.dt), rounded=False), dtype=sys_.dt)


# ---------------------------------------------------------------------------------------------------------------------
# BiCGStab, right-preconditioned, correction form
# ---------------------------------------------------------------------------------------------------------------------
class _State:
    pass


def _start(A, b, x0, rt):
    st = _State()
    st.r0 = b - A(x0)
    st.r = st.r0.copy()
    st.dx = np.zeros_like(b)
    st.rt = np.asarray(rt, dtype=b.dtype).reshape(-1)
    return st


def _reset(st):
    st.p = np.zeros_like(st.r); st.v = np.zeros_like(st.r)
    st.rho = st.alpha = st.omega = st.r.dtype.type(1)


def _iterate(A, Mfn, st):
    """One BiCGStab iteration on the state: p = r + beta (p - omega v), v = A M p, alpha = rt.r / rt.v, s = r - alpha v, t = A M s,
    omega = t.s / t.t, dx += alpha M p + omega M s, r = s - omega t."""
    rho_new = dot(st.rt, st.r)
    if not abs(rho_new) > 0:
        raise Exception("BiCGStab breakdown: rt . r = 0")
    beta = (rho_new / st.rho) * (st.alpha / st.omega)
    st.p = st.r + beta * (st.p - st.omega * st.v)
    y = Mfn(st.p)
    st.v = A(y)
    st.alpha = rho_new / dot(st.rt, st.v)
    s = st.r - st.alpha * st.v
    z = Mfn(s)
    t = A(z)
    st.omega = dot(t, s) / dot(t, t)
    st.dx = st.dx + st.alpha * y + st.omega * z
    st.r = s - st.omega * t
    st.rho = rho_new


def bicgstab_steps(A, Mfn, b, x0, rt, m, trace=False):
    """Exactly m iterations from x0.  Returns (dx, r): the correction (the iterate is x0 + dx) and the recurrence residual;
    trace=True: the list of (dx, r) after each of the m iterations."""
    st = _start(A, np.asarray(b), np.asarray(x0, dtype=np.asarray(b).dtype), rt)
    _reset(st)
    out = []
    for _ in range(m):
        _iterate(A, Mfn, st)
        out.append((st.dx.copy(), st.r.copy()))
    return out if trace else (st.dx, st.r)


def bicgstab(sys_, Mfn, b, x0, rt, ref_norm=0.0, rtol=RTOL, etol=ETOL, maxit=MAXIT, defl=None):
    """The iteration run to the solve's stopping rule.  |r| <= tol |b| (ref_norm > 0 replaces |b|) ends the recurrence, where tol starts
    at rtol; once |r| <= 1000 tol |b| the estimate is also followed from the recurrence residual, with a_mom |r_mom| for |(M r)_vel|,
    and the recurrence goes on while that is above 0.7 etol.  Then the true residual s = r0 - A dx is formed; if it meets tol, a CHECK
    evaluates the estimate from s and M s itself (renewing a_mom = |(M s)_vel| / |s_mom|, clamped to [1, n_amp^2]); above etol the
    tolerance tightens, tol = min(tol, |s| / |b|) min(0.5, 0.7 etol / estimate), and the recurrence resumes as it stands; at most
    MAX_CHECKS checks.  A true residual that misses tol restarts the recurrence from it (at most 4 times, and only while it halves).
    defl = (yAw, |w_vel|^2) adds the anchor term to every estimate.

    Returns a dict: x, iterations, converged, rel_residual, error_estimate, checks, and history = [(|r| / |b|, estimate or 0)] per
    iteration."""
    dt = sys_.dt
    A = sys_.A
    b = np.asarray(b, dtype=dt); x0 = np.asarray(x0, dtype=dt)
    bnorm = norm(b)
    if ref_norm > 0 and bnorm > 0:
        bnorm = dt(ref_norm)
    n_amp = max(sys_.n)
    yw = sys_.deflation_vectors()[1].reshape(-1)

    def anchor(res, xx):
        if defl is None or not xx > 0:
            return dt(0)
        return abs(dot(yw, sys_.prs(res)) / defl[0]) * np.sqrt(defl[1] / xx)

    st = _start(A, b, x0, rt)
    tol, a_mom, rec, est = dt(rtol), dt(1), dt(0), dt(0)
    it = restarts = checks = 0
    resume = False
    true_norm = last_true = -1.0
    history = []
    while True:
        if not resume:
            _reset(st)
        rnorm = norm(st.r)
        resume = False
        while it < maxit and (rnorm > tol * bnorm or rec > 0.7 * etol):
            it += 1
            _iterate(A, Mfn, st)
            rnorm = norm(st.r)
            rec = dt(0)
            if rnorm <= 1e3 * tol * bnorm:
                x = x0 + st.dx
                xx = dot(sys_.vel(x), sys_.vel(x))
                rc = dot(sys_.prs(st.r), sys_.prs(st.r))
                rm = max(rnorm * rnorm - rc, 0)
                rec = (n_amp * np.sqrt(rc) + a_mom * np.sqrt(rm)) / np.sqrt(xx) + anchor(st.r, xx) if xx > 0 else dt(0)
            history.append((float(rnorm / bnorm), float(rec)))
        s = st.r0 - A(st.dx)
        last_true, true_norm = true_norm, norm(s)
        if true_norm <= tol * bnorm and it < maxit and checks < MAX_CHECKS:
            x = x0 + st.dx
            Ms = Mfn(s)
            est = sys_.estimate(s, Ms, x, *(defl or ()))
            checks += 1
            rc = dot(sys_.prs(s), sys_.prs(s)); zz = dot(sys_.vel(Ms), sys_.vel(Ms))
            rm = true_norm * true_norm - rc
            if rm > 0 and zz > 0:
                a_mom = min(max(np.sqrt(zz / rm), 1), n_amp * n_amp)
            resume = bool(est > etol and tol > 1e-15)
            if resume:
                tol = min(tol, true_norm / bnorm) * min(0.5, 0.7 * etol / est)
                rec = est
                continue
        if true_norm <= tol * bnorm or it >= maxit or restarts >= 4:
            break
        if last_true >= 0 and not true_norm < 0.5 * last_true:
            break
        restarts += 1
        st.r = s.copy()
    rel = true_norm / bnorm
    return dict(x=x0 + st.dx, iterations=it, rel_residual=float(rel), error_estimate=float(est), checks=checks,
                converged=bool(rel <= rtol and not est > 1.5 * etol), history=history)


def deflation_solve(sys_, Mfn, rtol=1e-3, maxit=80):
    """A deflation vector of the model's own: BiCGStab for A w = u from zero until |u - A w| <= rtol |u|.  Returns (w, |u - A w| / |u|)."""
    u = sys_.u_vector()
    st = _start(sys_.A, u, np.zeros_like(u), shadow(sys_.n).reshape(-1))
    _reset(st)
    un = norm(u)
    for _ in range(maxit):
        if norm(st.r) <= rtol * un:
            break
        _iterate(sys_.A, Mfn, st)
    return st.dx, float(norm(u - sys_.A(st.dx)) / un)
