"""The NumPy model of flow through the walls of the 3-D Stokes system, written from the statement of the rule in include/pylamp_hip.h
(pl3_stokes_set_wall_flow) and DESIGN.md section 6c; the HIP kernels are compared with it in tests/test_hip_3d_flow.py.  No GPU, no
project code: it stands on tests/stokes3_moving_model.py (walls at rest or sliding, whose operator is the walls model's) and adds what a
flow adds -- terms on the identity rows of the wall-normal velocities and the advection ghosts -- in np.longdouble.

Walls are [z0, x0, y0, zL, xL, yL].  For wall w of axis a, p < q are the two other axes in z, x, y order, and the flow of the wall is an
array Un_w of shape (n_p - 1, n_q - 1): entry (i, j) is the wall-normal velocity along +a on the wall face between the nodes i, i + 1
along p and j, j + 1 along q.  A scalar is the constant profile, None no flow.  The operator does not depend on the flow.
"""
import numpy as np

import mic3_model
import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W

LD = np.longdouble
NOSLIP, FREESLIP = W.NOSLIP, W.FREESLIP
WALLS = W.WALLS
AXES = ((1, 2), (0, 2), (0, 1))                             # p < q of axis a
FLUX_BOUND = 1e-10                                          # |Phi| <= FLUX_BOUND sum |Un| dp dq
_ld = M._ld


def rk4_classic(tr_x, grids, vels, tstep):
    """The marker step a flow through the walls wants (pl3_mic_set_rk4_classic): the four VELDIV stages of mic3_model.rk4, out-of-grid
    velocity 0, with the classical weights (1, 2, 2, 1) / 6, which sum to 1 -- a uniform field U moves a tracer by U tstep (the
    reference's (1, 1, 1, 1) / 6 by 2/3 of that)."""
    k1 = mic3_model.veldiv(tr_x, grids, vels)
    k2 = mic3_model.veldiv(tr_x + 0.5 * tstep * k1, grids, vels)
    k3 = mic3_model.veldiv(tr_x + 0.5 * tstep * k2, grids, vels)
    k4 = mic3_model.veldiv(tr_x + tstep * k3, grids, vels)
    xnew = tr_x + (1 / 6) * tstep * (k1 + 2 * k2 + 2 * k3 + k4)
    return (xnew - tr_x) / tstep, xnew


def flows(wallflow, nx):
    """Six entries, None or a float64 (n_p - 1, n_q - 1) array; a non-finite entry is an error that names the wall and the index."""
    n = [int(v) for v in nx]
    if wallflow is None:
        return [None] * 6
    wallflow = list(wallflow)
    if len(wallflow) != 6:
        raise Exception("six walls [z0, x0, y0, zL, xL, yL]")
    out = []
    for w, f in enumerate(wallflow):
        if f is None:
            out.append(None)
            continue
        p, q = AXES[w % 3]
        a = np.array(f, dtype=np.float64)
        if a.ndim == 0:
            a = np.full((n[p] - 1, n[q] - 1), float(a))
        if a.shape != (n[p] - 1, n[q] - 1):
            raise Exception("wall %s: the flow has the shape %r, the wall has %r faces" % (WALLS[w], a.shape, (n[p] - 1, n[q] - 1)))
        bad = np.argwhere(~np.isfinite(a))
        if bad.size:
            raise Exception("wall %s: non-finite flow entry %r" % (WALLS[w], tuple(int(v) for v in bad[0])))
        out.append(a)
    return out


def net_flux(grid, wallflow):
    """(Phi, the six signed wall fluxes, sum |Un| dp dq) in longdouble: fluxes[w] = s_w sum_ij Un_w[i, j] dp_i dq_j with s = +1 on the
    low walls and -1 on the high walls, the volume per time that enters through wall w."""
    g = [_ld(c) for c in grid]
    fl = flows(wallflow, [c.size for c in g])
    flux, tot = np.zeros(6, dtype=LD), LD(0)
    for w, a in enumerate(fl):
        if a is None:
            continue
        p, q = AXES[w % 3]
        area = np.diff(g[p])[:, None] * np.diff(g[q])[None, :]
        flux[w] = (1 if w < 3 else -1) * np.sum(_ld(a) * area)
        tot += np.sum(np.abs(_ld(a)) * area)
    return flux.sum(), flux, tot


def balanced(grid, wallflow):
    phi, _, tot = net_flux(grid, wallflow)
    return bool(abs(phi) <= LD(FLUX_BOUND) * tot)


def check_flux(grid, wallflow):
    phi, flux, tot = net_flux(grid, wallflow)
    if abs(phi) > LD(FLUX_BOUND) * tot:
        raise Exception("net flux %r through the walls (wall fluxes %r)" % (float(phi), [float(f) for f in flux]))


def flow_rhs(nx, wallflow):
    """What a flow adds to the ROW-SCALED right-hand side, (nz, nx, ny, 4) longdouble: Un_w[i, j] on the identity row of v_a at the wall
    plane (index 0 or n_a - 1 along a, i <= n_p - 2, j <= n_q - 2); the ghost entries beyond stay 0.  Linear in the flow."""
    n = [int(v) for v in nx]
    R = np.zeros(n + [4], dtype=LD)
    for w, un in enumerate(flows(wallflow, n)):
        if un is None:
            continue
        a = w % 3
        plane = np.moveaxis(R[..., a], a, 0)[0 if w < 3 else n[a] - 1]          # a view, (n_p, n_q)
        plane[:-1, :-1] = _ld(un)
    return R


def stokes_rhs(nx, grid, etas, etan, rho, grav=None, bc=None, wallvel=None, wallflow=None, strict=True, rounded=True):
    """The unscaled right-hand side, as pl3_stokes_rhs after the three wall settings: the identity rows of the wall-normal velocities
    gain Kcont Un."""
    n = [int(v) for v in nx]
    check_flux(grid, wallflow)
    R = _ld(V.stokes_rhs(n, grid, etas, etan, rho, grav=grav, bc=bc, wallvel=wallvel, strict=strict, rounded=False)).reshape(n + [4])
    if wallflow is not None:
        R = R + LD(M.scaling(grid, etas, etan)[0]) * flow_rhs(n, wallflow)
    return M._out(R.reshape(-1), rounded)


def stokes_rhs_scaled(nx, grid, etas, etan, rho, grav=None, bc=None, wallvel=None, wallflow=None, strict=True, divisor=None):
    """The row-scaled right-hand side, as pl3_stokes_rhs_scaled: an identity row is divided by Kcont, so its entry is Un itself.
    divisor (V.row_divisor) is needed only where gravity or a sliding wall makes other rows non-zero."""
    n = [int(v) for v in nx]
    check_flux(grid, wallflow)
    plain = (grav is not None and not np.any(np.asarray(grav, dtype=np.float64) != 0)) and \
            (wallvel is None or not np.any(np.asarray(wallvel, dtype=np.float64) != 0))
    if plain:
        V.velocities(wallvel, bc)
        S = np.zeros(n + [4], dtype=LD)
    else:
        S = _ld(V.stokes_rhs_scaled(n, grid, etas, etan, rho, grav=grav, bc=bc, wallvel=wallvel, strict=strict, divisor=divisor)).reshape(n + [4])
    if wallflow is not None:
        S = S + flow_rhs(n, wallflow)
    return S.reshape(-1).astype(np.float64)


def advection_velocity(newvel, gridmp, nx, bc=None, wallvel=None, wallflow=None):
    """As V.advection_velocity, but the pass of a wall with a flow runs in its slot z0 .. yL, even for a NOSLIP wall at rest: from the
    neighbouring plane as it is at that moment, 2 Un[ci, cj] - V for the normal component (ci, cj: the padded tangential indices minus
    1, clamped to [0, n - 2]); tangential components are copied on a FREESLIP wall and become 2 U_c - V on a NOSLIP wall (U_c possibly
    0).  Walls without a flow keep the arithmetic of V.advection_velocity (-V, not 2 0 - V)."""
    kinds = W.walls(bc)
    U = V.velocities(wallvel, bc)
    n = [int(v) for v in nx]
    Un = flows(wallflow, n)
    shp = tuple(v + 1 for v in n)
    g, A = W.advection_velocity(newvel, gridmp, n, bc=[FREESLIP] * 6)      # the inner values; its ghost passes are redone below
    for q in range(3):
        inner = A[q][1:-1, 1:-1, 1:-1].copy()
        A[q][...] = 0.0
        A[q][1:-1, 1:-1, 1:-1] = inner
    for w in range(6):
        flow = Un[w] is not None
        shear = kinds[w] == NOSLIP and (U[w].any() or flow)
        if kinds[w] == NOSLIP and not shear:
            continue
        a = w % 3
        ghost, inner = (0, 1) if w < 3 else (shp[a] - 1, shp[a] - 2)
        p, q_ = AXES[a]
        for c in range(3):
            Vm = np.moveaxis(A[c], a, 0)                    # a view; the remaining axes keep their z, x, y order
            if c == a and flow:
                ci = np.clip(np.arange(shp[p]) - 1, 0, n[p] - 2)
                cj = np.clip(np.arange(shp[q_]) - 1, 0, n[q_] - 2)
                Vm[ghost] = 2 * Un[w][np.ix_(ci, cj)] - Vm[inner]
            elif c == a:
                Vm[ghost] = -Vm[inner]
            elif shear:
                Vm[ghost] = 2 * U[w, c] - Vm[inner]
            else:
                Vm[ghost] = Vm[inner]
    return g, A
