"""NumPy model of the 3-D heat walls with a profile and of the heat budget ("Heat walls and budget"), the
reference tests/test_hip_3d_heatwalls.py compares pl3_heat_set_wall_values and pl3_heat_budget with.  No GPU, no project code: written
from the definitions in include/pylamp_hip.h with array slicing on top of tests/stokes3_model.py, evaluated in np.longdouble.

A plane covers the NODES of its wall, C-order (n_p, n_q) with p < q the two other axes in z, x, y order.  z-walls own their edges,
then x-walls, then y-walls (stokes3_model._owner): an entry at a node another wall owns is never read.
"""
import numpy as np

import stokes3_model as M

LD = np.longdouble
PLANE_AXES = ((1, 2), (0, 2), (0, 1))          # the axes p < q of a plane of a wall of axis a


def plane_shape(n, wall):
    p, q = PLANE_AXES[wall % 3]
    return (int(n[p]), int(n[q]))


def read_mask(n, wall):
    """True where wall `wall` owns the node of its plane: the entries the right-hand side reads."""
    a = wall % 3
    own = np.take(M._owner([int(v) for v in n]), 0 if wall < 3 else int(n[a]) - 1, axis=a)
    return own == wall


def heat_rhs_planes(nx, T, Cp, rho, H, bc, bcvalue, tstep, planes, rounded=True):
    """stokes3_model.heat_rhs with planes[w] (None: the scalar bcvalue[w]) on the wall rows: the row of a wall node is its plane's entry,
    a temperature on a FIXTEMP wall and k dT/dx_a along +a on a FIXFLOW wall (the kind changes the meaning, not the number)."""
    n = [int(v) for v in nx]
    r = M._ld(M.heat_rhs(n, T, Cp, rho, H, bc, bcvalue, tstep, rounded=False)).reshape(n)
    own = M._owner(n)
    for wall in range(6):
        if planes is None or planes[wall] is None:
            continue
        a = wall % 3
        v = np.asarray(planes[wall], dtype=np.float64)
        assert v.shape == plane_shape(n, wall), (wall, v.shape)
        full = np.broadcast_to(np.expand_dims(M._ld(v), a), n)
        r = np.where(own == wall, full, r)
    return M._out(r.reshape(-1), rounded)


def _widths(gridmp, n):
    """w_a[i] = mp_a[i] - mp_a[i-1] for the interior nodes i = 1 .. n_a - 2 (entries 0 and n_a - 1 are not used: NaN)."""
    out = []
    for a in range(3):
        mp = M._ld(gridmp[a])
        w = np.full(n[a], np.nan, dtype=LD)
        w[1:n[a] - 1] = mp[1:n[a] - 1] - mp[0:n[a] - 2]
        out.append(w)
    return out


def heat_budget(nx, grid, gridmp, k, Cp, rho, H, Told, tstep, T):
    """(out, mag): out[0 .. 5] the heat flow into the box through z0, x0, y0, zL, xL, yL, out[6] the storage rate, out[7] the source,
    in np.longdouble; mag[q] the sum of the absolute values of the terms of out[q] (the scale of a summation error).

    Sums over the interior nodes with w_a[i] = mp_a[i] - mp_a[i-1], V = w_z w_x w_y:
      low wall of axis a   - k_a[0]   (T[1]   - T[0])   / (c_a[1]   - c_a[0])   w_p w_q
      high wall            + k_a[n-2] (T[n-1] - T[n-2]) / (c_a[n-1] - c_a[n-2]) w_p w_q
      storage  rho Cp (T - T_old) / tstep V,   source  H V."""
    n = [int(v) for v in nx]
    T, Told = M._ld(T).reshape(n), M._ld(Told).reshape(n)
    w = _widths(gridmp, n)
    inner = (slice(1, -1),) * 3
    V = (M._along(w[0], 0) * M._along(w[1], 1) * M._along(w[2], 2))[inner]
    out, mag = np.zeros(8, dtype=LD), np.zeros(8, dtype=LD)
    for a in range(3):
        p, q = PLANE_AXES[a]
        area = w[p][1:-1, None] * w[q][None, 1:-1]
        d = np.diff(M._ld(grid[a]))
        Tm, km = np.moveaxis(T, a, 0), np.moveaxis(M._ld(k[a]), a, 0)           # (n_a, n_p, n_q): p < q keep their order
        lo = -km[0] * (Tm[1] - Tm[0]) / d[0]
        hi = km[n[a] - 2] * (Tm[n[a] - 1] - Tm[n[a] - 2]) / d[n[a] - 2]
        for wall, f in ((a, lo), (a + 3, hi)):
            t = f[1:-1, 1:-1] * area
            out[wall], mag[wall] = t.sum(), np.abs(t).sum()
    st = (M._ld(rho) * M._ld(Cp) * (T - Told) / LD(tstep))[inner] * V
    so = M._ld(H).reshape(n)[inner] * V
    out[6], mag[6] = st.sum(), np.abs(st).sum()
    out[7], mag[7] = so.sum(), np.abs(so).sum()
    return out, mag


def imbalance(out):
    """(storage - source - sum of the wall flows, the same normalised by |storage| + |source| + sum |wall flow|)."""
    out = M._ld(out)
    im = out[6] - out[7] - out[:6].sum()
    return im, abs(im) / (abs(out[6]) + abs(out[7]) + np.abs(out[:6]).sum())


def fixflow_wall_flow(n, gridmp, wall, plane):
    """What wall_flow[wall] must be on a FIXFLOW wall with plane v: -sum v w_p w_q on a low wall, + on a high wall, over the nodes
    interior in p and q.  Returns (value, sum of |terms|)."""
    n = [int(v) for v in n]
    w = _widths(gridmp, n)
    p, q = PLANE_AXES[wall % 3]
    t = M._ld(plane)[1:-1, 1:-1] * (w[p][1:-1, None] * w[q][None, 1:-1])
    return (-1 if wall < 3 else 1) * t.sum(), np.abs(t).sum()
