"""The NumPy model of the 3-D Stokes rows with per-wall no-slip boundaries, written from the statement of the rows in
include/pylamp_hip.h (pl3_stokes_set_walls) and DESIGN.md section 6c; the HIP kernels are compared with it in
tests/test_hip_3d_walls.py.  No GPU, no project code: it takes the free-slip rows of tests/stokes3_model.py and rewrites the
rows that a no-slip wall changes, in np.longdouble.  tests/test_stokes3_walls_model.py ties it to the 2-D oracle.

A wall is one of [z0, x0, y0, zL, xL, yL]; its kind is FREESLIP (1) or NOSLIP (0).  (D, E, F) is a cyclic permutation of
(z, x, y); v_D is tangential to the walls of E and F.  Identity rows, pressure rows and the right-hand side do not depend on the
kinds.
"""
import numpy as np

import stokes3_model as M

NOSLIP, FREESLIP = 0, 1
WALLS = ("z0", "x0", "y0", "zL", "xL", "yL")
_ld = M._ld


def walls(bc):
    if bc is None:
        return [FREESLIP] * 6
    bc = [int(b) for b in bc]
    if len(bc) != 6:
        raise Exception("six walls [z0, x0, y0, zL, xL, yL]")
    for w, b in enumerate(bc):
        if b not in (NOSLIP, FREESLIP):
            raise Exception("wall %s: kind %d is neither FREESLIP nor NOSLIP" % (WALLS[w], b))
    return bc


def stokes_apply(nx, grid, etas, etan, x, bc=None, strict=True, rounded=True):
    """The unscaled operator, as pl3_stokes_apply after pl3_stokes_set_walls(bc)."""
    n = [int(v) for v in nx]
    kinds = walls(bc)
    Y = np.array(M.stokes_apply(n, grid, etas, etan, x, strict=strict, rounded=False), dtype=M.LD).reshape(n + [4])
    Kc = M.LD(M.scaling(grid, etas, etan)[0])
    X = _ld(x).reshape(n + [4])
    es = _ld(etas)
    ix = M._index(n)
    for D in range(3):
        E, F = (D + 1) % 3, (D + 2) % 3
        interior, slaved, viaE = M.velocity_classes(D, n, strict)
        v = X[..., D]
        for a, b in ((E, F), (F, E)):                      # a: the axis whose walls v_D is tangential to, b: the other one
            c = _ld(grid[a])
            N = n[a]
            for hi in (0, 1):
                if kinds[a + 3 * hi] != NOSLIP:
                    continue
                layer = ix[a] == (N - 2 if hi else 0)      # the outermost in-domain layer of v_D at that wall
                if strict:
                    # slaved rows that couple along a (E before F): the extrapolation row -- the line through v (half a cell from the
                    # wall) and v_nb (one layer further in) vanishes on the wall
                    rows = slaved & layer & (viaE if a == E else ~viaE)
                    if hi:
                        rD, rd = 1 / (c[N - 1] - c[N - 3]), 1 / (c[N - 1] - c[N - 2])
                        val = Kc * ((rD + rd) * v - rD * M._shift(v, a, -1))
                    else:
                        rD, rd = 1 / (c[2] - c[0]), 1 / (c[1] - c[0])
                        val = Kc * (-(rD + rd) * v + rD * M._shift(v, a, 1))
                    Y[..., D] = np.where(rows, val, Y[..., D])
                else:
                    # natural rows: the shear stress on the wall edge keeps its dv_D/dx_a half, one-sided against v_D = 0 on the wall
                    # (the free-slip row dropped it); the edge's viscosity is the mean of the two nodes that span it along b
                    rows = interior & layer
                    eta = (es + M._shift(es, b, 1)) / 2       # edge at the a-node of the row's own index ...
                    if hi:
                        eta = M._shift(eta, a, 1)             # ... the high wall's edge is one node up
                        w = c[N - 1] - c[N - 2]
                        stress = eta * (-v / (w / 2))
                        extra = stress / w                    # + stress on the upper edge / cell width
                    else:
                        w = c[1] - c[0]
                        stress = eta * (v / (w / 2))
                        extra = -stress / w                   # - stress on the lower edge / cell width
                    Y[..., D] = Y[..., D] + np.where(rows, extra, 0)
    return M._out(Y.reshape(-1), rounded)


def stokes_rhs(nx, grid, etas, etan, rho, grav=None, bc=None, strict=True, rounded=True):
    """The right-hand side does not depend on the wall kinds."""
    walls(bc)
    return M.stokes_rhs(nx, grid, etas, etan, rho, grav=grav, strict=strict, rounded=rounded)


def identity_rows(nx, strict, bc=None):
    """The rows that are Kcont times the unknown: the same with every wall kind."""
    walls(bc)
    return M.identity_rows(nx, strict)


def slaved_rows(nx, bc=None):
    """Strict mode: for every component D the list of (rows, axis, hi, kind): the slaved rows that couple along `axis` at its low /
    high wall, and that wall's kind."""
    n = [int(v) for v in nx]
    kinds = walls(bc)
    ix = M._index(n)
    out = []
    for D in range(3):
        E, F = (D + 1) % 3, (D + 2) % 3
        _, slaved, viaE = M.velocity_classes(D, n, True)
        lst = []
        for a in (E, F):
            for hi in (0, 1):
                layer = ix[a] == (n[a] - 2 if hi else 0)
                lst.append((slaved & layer & (viaE if a == E else ~viaE), a, hi, kinds[a + 3 * hi]))
        out.append(lst)
    return out


def advection_velocity(newvel, gridmp, nx, bc=None):
    """Cell-centred velocities on the padded (nz+1, nx+1, ny+1) grid: each component averaged along its own axis, then one pass per
    wall in the order z0, x0, y0, zL, xL, yL.  The pass of a FREESLIP wall fills its ghost plane from the neighbouring plane as
    it is at that moment (normal component negated, tangential copied); the pass of a NOSLIP wall is skipped."""
    kinds = walls(bc)
    n = [int(v) for v in nx]
    shp = tuple(v + 1 for v in n)
    V = [np.zeros(shp) for _ in range(3)]
    for q in range(3):
        u = np.asarray(newvel[q], dtype=np.float64)
        up = np.moveaxis(u, q, 0)
        others = [a for a in range(3) if a != q]
        avg = 0.5 * (up[1:] + up[:-1])                      # own axis: nodes i, i - 1 -> centre i
        avg = np.moveaxis(avg, 0, q)
        sl = [slice(None)] * 3
        for a in others:
            sl[a] = slice(0, n[a] - 1)
        V[q][1:-1, 1:-1, 1:-1] = avg[tuple(sl)]
    for w in range(6):
        if kinds[w] == NOSLIP:
            continue
        a = w % 3
        ghost, inner = (0, 1) if w < 3 else (shp[a] - 1, shp[a] - 2)
        for q in range(3):
            Vm = np.moveaxis(V[q], a, 0)                    # a view
            Vm[ghost] = -Vm[inner] if q == a else Vm[inner]
    g = [np.insert(np.asarray(m, dtype=np.float64), 0, m[0] - (m[1] - m[0])) for m in gridmp]
    return g, V
