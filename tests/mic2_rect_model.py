"""Plain per-tracer model of the 2-D marker-in-cell operations on a rectilinear grid; helper module: no fixtures, no NumPy
kernels, no project code (NumPy only carries the arrays in and out).

Written from the rule in include/pylamp_hip.h (pl_trac2grid_rect, pl_mic_set_search) and pylamp_amd/csrc/pl_mic.h
(mic_axis_locate), per axis, for strictly increasing coordinates c[0..n-1]:

  * c[0] <= z <= c[n-1]:  the largest ie with c[ie] <= z (bisect), in-cell coordinate a = (z - c[ie]) / (c[ie+1] - c[ie]);
                          a marker exactly on c[n-1] belongs to the last cell, ie = n - 2, with a = 1  (scatter),
                          and counts as outside                                                      (gather);
  * beyond an end the grid continues with the spacing h of the end cell: f = floor((z - c_end) / h) cells further, counted
    from that end, a = (z - (c_end + f h)) / h; the nodes out there do not exist, their contributions are dropped (scatter);
    the marker is outside (gather).

Scatter: node (ie + di, je + dj) receives the weight (a or 1 - a) * (b or 1 - b); a node's sums are taken with math.fsum --
exactly rounded once, whatever the order of the tracers -- which makes these values the yardstick for the rounding of any
summation order.  Scheme bits as in the reference: 1 arithmetic, 2 geometric, 4 weighted.  A node without a tracer in reach
(or whose weights sum to zero) is NaN.

Gather: LINEAR is the bilinear form of the four nodes of the cell; VELDIV adds the divergence-conserving correction of
pylamp_trac.py:98-154 and keeps the reference's quirk for a tracer outside the grid: cell (0, 0) with the tracer's own
coordinates, and only the LAST component (vx) is replaced by defval.  RK4: the reference's four stages with the weights
(1, 1, 1, 1) / 6 (pylamp_trac.py:385) and v = (x_new - x) / dt.
"""
import bisect
import math

import numpy as np

ARITH, GEOM, WEIGHTED = 1, 2, 4
NAN = float("nan")


def locate(c, z):
    """(ie, a) of the scatter rule; c a list of floats."""
    n = len(c)
    if z < c[0]:
        h = c[1] - c[0]
        f = math.floor((z - c[0]) / h)
        return int(f), (z - (c[0] + f * h)) / h
    if z > c[n - 1]:
        h = c[n - 1] - c[n - 2]
        f = math.floor((z - c[n - 1]) / h)
        return n - 1 + int(f), (z - (c[n - 1] + f * h)) / h
    ie = min(bisect.bisect_right(c, z) - 1, n - 2)
    return ie, (z - c[ie]) / (c[ie + 1] - c[ie])


def trac2grid(tr_x, tr_f, grid, schemes):
    """Fields (nz, nx) for the columns of tr_f, averaged onto the node set grid = [zc, xc]; also the number of contributions
    each node received (the length of its sums)."""
    zc = [float(v) for v in grid[0]]; xc = [float(v) for v in grid[1]]
    nz, nx = len(zc), len(xc)
    nf = len(schemes)
    wlist = {}
    vlist = [dict() for _ in range(nf)]
    for t in range(len(tr_x)):
        ie, a = locate(zc, float(tr_x[t][0]))
        je, b = locate(xc, float(tr_x[t][1]))
        vals = []
        for k in range(nf):
            v = float(tr_f[t][k])
            vals.append(math.log(v) if schemes[k] & GEOM else v)
        for di, wa in ((0, 1 - a), (1, a)):
            for dj, wb in ((0, 1 - b), (1, b)):
                i, j = ie + di, je + dj
                if i < 0 or i >= nz or j < 0 or j >= nx:
                    continue
                w = wb * wa
                wlist.setdefault((i, j), []).append(w)
                for k in range(nf):
                    vlist[k].setdefault((i, j), []).append(vals[k] * w if schemes[k] & WEIGHTED else vals[k])
    out = [np.full((nz, nx), NAN) for _ in range(nf)]
    count = np.zeros((nz, nx), dtype=np.int64)
    for (i, j), ws in wlist.items():
        count[i, j] = len(ws)
        wsum = math.fsum(ws)
        for k in range(nf):
            den = wsum if schemes[k] & WEIGHTED else float(len(ws))
            if den == 0.0:
                continue
            s = math.fsum(vlist[k][(i, j)]) / den
            out[k][i, j] = math.exp(s) if schemes[k] & GEOM else s
    return out, count


def _inside(c, z):
    return c[0] <= z < c[len(c) - 1]


def _gather_cell(zc, xc, z, x):
    """(outside, ie, je, a, b) of the gather rule: outside -> cell (0, 0) with the tracer's own coordinates."""
    if _inside(zc, z) and _inside(xc, x):
        ie = bisect.bisect_right(zc, z) - 1; je = bisect.bisect_right(xc, x) - 1
        return False, ie, je, (z - zc[ie]) / (zc[ie + 1] - zc[ie]), (x - xc[je]) / (xc[je + 1] - xc[je])
    return True, 0, 0, (z - zc[0]) / (zc[1] - zc[0]), (x - xc[0]) / (xc[1] - xc[0])


def _bilinear(F, ie, je, a, b):
    return math.fsum(((1 - b) * (1 - a) * float(F[ie][je]), b * (1 - a) * float(F[ie][je + 1]),
                      (1 - b) * a * float(F[ie + 1][je]), b * a * float(F[ie + 1][je + 1])))


def grid2trac_linear(tr_x, grid, fields, defval=NAN):
    """(n, nf) bilinear interpolation; returns also the number of tracers outside (stopOnError raises when it is not 0)."""
    zc = [float(v) for v in grid[0]]; xc = [float(v) for v in grid[1]]
    out = np.empty((len(tr_x), len(fields)))
    n_out = 0
    for t in range(len(tr_x)):
        bad, ie, je, a, b = _gather_cell(zc, xc, float(tr_x[t][0]), float(tr_x[t][1]))
        n_out += bad
        for k, F in enumerate(fields):
            out[t, k] = defval if bad else _bilinear(F, ie, je, a, b)
    return out, n_out


def _veldiv(zc, xc, Vz, Vx, z, x, defval):
    bad, ie, je, a, b = _gather_cell(zc, xc, z, x)
    hz = zc[ie + 1] - zc[ie]; hx = xc[je + 1] - xc[je]
    z00, z01, z10, z11 = float(Vz[ie][je]), float(Vz[ie][je + 1]), float(Vz[ie + 1][je]), float(Vz[ie + 1][je + 1])
    x00, x01, x10, x11 = float(Vx[ie][je]), float(Vx[ie][je + 1]), float(Vx[ie + 1][je]), float(Vx[ie + 1][je + 1])
    c10 = (0.5 * hx / hz) * math.fsum((z00, -z10, z11, -z01))
    c20 = (0.5 * hz / hx) * math.fsum((x00, -x01, x11, -x10))
    ux = math.fsum(((1 - b) * (1 - a) * x00, b * (1 - a) * x01, (1 - b) * a * x10, b * a * x11, b * (1 - b) * c10))
    uz = math.fsum(((1 - b) * (1 - a) * z00, b * (1 - a) * z01, (1 - b) * a * z10, b * a * z11, a * (1 - a) * c20))
    return uz, (defval if bad else ux)


def grid2trac_veldiv(tr_x, grid, vels, defval=NAN):
    """(n, 2) = (vz, vx) on the grid [gz, gx] of the two velocity fields."""
    zc = [float(v) for v in grid[0]]; xc = [float(v) for v in grid[1]]
    out = np.empty((len(tr_x), 2))
    for t in range(len(tr_x)):
        out[t] = _veldiv(zc, xc, vels[0], vels[1], float(tr_x[t][0]), float(tr_x[t][1]), defval)
    return out


def rk4(tr_x, grid, vels, dt):
    """(tracer velocities, new positions), both (n, 2)."""
    zc = [float(v) for v in grid[0]]; xc = [float(v) for v in grid[1]]
    v = np.empty((len(tr_x), 2)); xn = np.empty((len(tr_x), 2))
    for t in range(len(tr_x)):
        z, x = float(tr_x[t][0]), float(tr_x[t][1])
        k1 = _veldiv(zc, xc, vels[0], vels[1], z, x, 0.0)
        k2 = _veldiv(zc, xc, vels[0], vels[1], z + 0.5 * dt * k1[0], x + 0.5 * dt * k1[1], 0.0)
        k3 = _veldiv(zc, xc, vels[0], vels[1], z + 0.5 * dt * k2[0], x + 0.5 * dt * k2[1], 0.0)
        k4 = _veldiv(zc, xc, vels[0], vels[1], z + dt * k3[0], x + dt * k3[1], 0.0)
        zn = z + (1 / 6) * dt * (k1[0] + k2[0] + k3[0] + k4[0])
        xq = x + (1 / 6) * dt * (k1[1] + k2[1] + k3[1] + k4[1])
        xn[t] = (zn, xq); v[t] = ((zn - z) / dt, (xq - x) / dt)
    return v, xn
