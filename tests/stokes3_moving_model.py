"""The NumPy model of moving no-slip walls in the 3-D Stokes system, written from the statement of the rule in include/pylamp_hip.h
(pl3_stokes_set_wall_velocity) and DESIGN.md section 6c; the HIP kernels are compared with it in tests/test_hip_3d_moving.py.  No GPU,
no project code: it stands on tests/stokes3_walls_model.py (the rows of walls at rest, `slaved_rows`, `stokes_apply`) and adds what a
wall velocity adds -- terms of the right-hand side and the advection ghosts -- in np.longdouble.  tests/test_stokes3_moving_model.py
ties it to the 2-D oracle.

Every wall w of [z0, x0, y0, zL, xL, yL] carries U_w = (Uz, Ux, Uy), default 0; only the two components tangential to the wall may be
non-zero, and only on a NOSLIP wall.  The operator does not depend on U.
"""
import numpy as np

import stokes3_model as M
import stokes3_walls_model as W

LD = np.longdouble
NOSLIP, FREESLIP = W.NOSLIP, W.FREESLIP
WALLS = W.WALLS
COMP = ("Uz", "Ux", "Uy")
_ld = M._ld


def velocities(wallvel, bc=None):
    """(6, 3) float64 after the three checks of a velocity setting; bc None: all free-slip."""
    kinds = W.walls(bc)
    if wallvel is None:
        return np.zeros((6, 3))
    U = np.array(wallvel, dtype=np.float64)
    if U.shape != (6, 3):
        raise Exception("six walls [z0, x0, y0, zL, xL, yL] times (Uz, Ux, Uy)")
    for w in range(6):
        for q in range(3):
            if not np.isfinite(U[w, q]):
                raise Exception("wall %s: non-finite velocity component %s = %r" % (WALLS[w], COMP[q], float(U[w, q])))
        if U[w, w % 3] != 0:
            raise Exception("wall %s: normal velocity component %s = %r: through-flow needs the marker deletion path, which is not built "
                            "in 3-D" % (WALLS[w], COMP[w % 3], float(U[w, w % 3])))
        if U[w].any() and kinds[w] != NOSLIP:
            raise Exception("wall %s: FREESLIP walls cannot move (velocity %r)" % (WALLS[w], tuple(float(u) for u in U[w])))
    return U


class WallState:
    """The state a context keeps: kinds and velocities, each checked against the other when it is set."""

    def __init__(self):
        self.bc = [FREESLIP] * 6
        self.vel = np.zeros((6, 3))

    def set_walls(self, bc):
        kinds = W.walls(bc)
        for w in range(6):
            if self.vel[w].any() and kinds[w] != NOSLIP:
                raise Exception("wall %s: moves with velocity %r and cannot become FREESLIP" % (WALLS[w], tuple(float(u) for u in self.vel[w])))
        self.bc = kinds

    def set_wall_velocity(self, wallvel):
        self.vel = velocities(wallvel, self.bc)


def wall_rhs(nx, grid, etas, etan, bc, wallvel, strict=True):
    """The terms a wall velocity adds to the unscaled right-hand side, (nz, nx, ny, 4) longdouble; linear in wallvel."""
    n = [int(v) for v in nx]
    kinds = W.walls(bc)
    U = _ld(velocities(wallvel, bc))
    Kc = LD(M.scaling(grid, etas, etan)[0])
    es = _ld(etas)
    ix = M._index(n)
    R = np.zeros(n + [4], dtype=LD)
    for D in range(3):
        E, F = (D + 1) % 3, (D + 2) % 3
        if strict:
            # a row slaved along a at a NOSLIP wall: "v_D extrapolated linearly to the wall is U_D"
            for rows, a, hi, kind in W.slaved_rows(n, bc)[D]:
                if kind != NOSLIP:
                    continue
                c = _ld(grid[a])
                N = n[a]
                if hi:
                    val = Kc * (1 / (c[N - 1] - c[N - 2])) * U[a + 3, D]         # +Kcont rd_a[n-2] U_D
                else:
                    val = -Kc * (1 / (c[1] - c[0])) * U[a, D]                     # -Kcont rd_a[0] U_D
                R[..., D] = np.where(rows, val, R[..., D])
        else:
            # natural rows: the wall-edge stress is eta (v - U) / (w / 2) on the low side and eta (U - v) / (w / 2) on the high side; the row
            # is (upper stress - lower stress) / w, so each side leaves + 2 eta U / w^2 beside the operator: -2 eta U / w^2 on the right
            interior = M.velocity_classes(D, n, False)[0]
            for a, b in ((E, F), (F, E)):
                c = _ld(grid[a])
                N = n[a]
                for hi in (0, 1):
                    if kinds[a + 3 * hi] != NOSLIP:
                        continue
                    rows = interior & (ix[a] == (N - 2 if hi else 0))
                    eta = (es + M._shift(es, b, 1)) / 2                            # edge at the a-node of the row's own index ...
                    if hi:
                        eta = M._shift(eta, a, 1)                                  # ... the high wall's edge is one node up
                        w = c[N - 1] - c[N - 2]
                    else:
                        w = c[1] - c[0]
                    R[..., D] = R[..., D] + np.where(rows, -2 * eta * U[a + 3 * hi, D] / (w * w), 0)
    return R


def stokes_rhs(nx, grid, etas, etan, rho, grav=None, bc=None, wallvel=None, strict=True, rounded=True):
    """The unscaled right-hand side, as pl3_stokes_rhs after pl3_stokes_set_walls(bc) and pl3_stokes_set_wall_velocity(wallvel)."""
    n = [int(v) for v in nx]
    R = _ld(W.stokes_rhs(n, grid, etas, etan, rho, grav=grav, bc=bc, strict=strict, rounded=False)).reshape(n + [4])
    if wallvel is not None and np.any(np.asarray(wallvel, dtype=np.float64) != 0):
        R = R + wall_rhs(n, grid, etas, etan, bc, wallvel, strict)
    else:
        velocities(wallvel, bc)
    return M._out(R.reshape(-1), rounded)


def row_divisor(nx, grid, etas, etan, bc=None, strict=True):
    """What the row scaling divides a row by: the coefficient of the row's own unknown -- minus it on the interior momentum rows, where
    the scaling uses the (positive) sum of the own-component couplings.  Taken from the assembled model matrix."""
    n = [int(v) for v in nx]
    ap = lambda x: W.stokes_apply(n, grid, etas, etan, x, bc=bc, strict=strict)
    d = M.assemble(ap, n).diagonal().reshape(n + [4])
    for D in range(3):
        interior = M.velocity_classes(D, n, strict)[0]
        d[..., D] = np.where(interior, -d[..., D], d[..., D])
    return d


def stokes_rhs_scaled(nx, grid, etas, etan, rho, grav=None, bc=None, wallvel=None, strict=True, divisor=None):
    """The velocity rows of the right-hand side divided by row_divisor (the pressure rows are zero), as pl3_stokes_rhs_scaled."""
    n = [int(v) for v in nx]
    R = stokes_rhs(n, grid, etas, etan, rho, grav=grav, bc=bc, wallvel=wallvel, strict=strict, rounded=False).reshape(n + [4])
    d = row_divisor(n, grid, etas, etan, bc, strict) if divisor is None else divisor
    out = np.zeros(n + [4], dtype=LD)
    out[..., :3] = R[..., :3] / _ld(d[..., :3])
    return out.reshape(-1).astype(np.float64)


def extrapolation_defect(nx, grid, x, bc, wallvel):
    """Strict mode: the largest |v - gamma v_nb - (1 - gamma) U| over the slaved rows of the NOSLIP walls, gamma = rD / (rD + rd)."""
    n = [int(v) for v in nx]
    U = velocities(wallvel, bc)
    X = np.asarray(x).reshape(n + [4])
    worst, count = 0.0, 0
    for D, lst in enumerate(W.slaved_rows(n, bc)):
        v = X[..., D]
        for rows, a, hi, kind in lst:
            if kind != NOSLIP or not rows.any():
                continue
            c = grid[a]
            nb = M._shift(v, a, -1 if hi else 1)
            rD, rd = (1 / (c[-1] - c[-3]), 1 / (c[-1] - c[-2])) if hi else (1 / (c[2] - c[0]), 1 / (c[1] - c[0]))
            g = rD / (rD + rd)
            worst = max(worst, float(np.abs(v - g * nb - (1 - g) * U[a + 3 * hi, D])[rows].max()))
            count += int(rows.sum())
    assert count > 0
    return worst


def advection_velocity(newvel, gridmp, nx, bc=None, wallvel=None):
    """As W.advection_velocity, but the pass of a NOSLIP wall with a non-zero velocity runs in its slot z0 .. yL: from the neighbouring
    plane as it is at that moment, -V for the normal component and 2 U_c - V for each tangential component c.  The pass of a NOSLIP wall
    at rest is skipped (deliberately discontinuous at U = 0: the reference's behaviour for walls at rest)."""
    kinds = W.walls(bc)
    U = velocities(wallvel, bc)
    n = [int(v) for v in nx]
    shp = tuple(v + 1 for v in n)
    g, V = W.advection_velocity(newvel, gridmp, n, bc=[FREESLIP] * 6)      # the inner values; its ghost passes are redone below
    for q in range(3):
        inner = V[q][1:-1, 1:-1, 1:-1].copy()
        V[q][...] = 0.0
        V[q][1:-1, 1:-1, 1:-1] = inner
    for w in range(6):
        moving = kinds[w] == NOSLIP and U[w].any()
        if kinds[w] == NOSLIP and not moving:
            continue
        a = w % 3
        ghost, inner = (0, 1) if w < 3 else (shp[a] - 1, shp[a] - 2)
        for q in range(3):
            Vm = np.moveaxis(V[q], a, 0)                    # a view
            if q == a:
                Vm[ghost] = -Vm[inner]
            elif moving:
                Vm[ghost] = 2 * U[w, q] - Vm[inner]
            else:
                Vm[ghost] = Vm[inner]
    return g, V
