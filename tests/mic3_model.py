"""Float64 NumPy model of the 3-D marker-in-cell operations (plain helper module, no fixtures).

The reference's marker code is 2-D only, so the 3-D kernels are checked against this model, and the model is tied to the
2-D oracle by extrusion (tests/test_mic3_model.py).  Conventions: positions (n, 3) in [z, x, y] order, grids as three
coordinate arrays, fields C-order (nz, nx, ny).  Cells come from the regular-grid formula floor((n-1)(x-x0)/L) per axis.
"""
import numpy as np

AVG_ARITH, AVG_GEOM, AVG_WEIGHTED = 1, 2, 4
M_NEAREST, M_LINEAR, M_VELDIV = 8, 16, 32
GASR = 8.31446
TR_RHO, TR_ETA, TR_TMP, TR_HCD, TR_HCP, TR_RH0, TR_ALP, TR_ACE, TR_ET0 = 0, 1, 3, 4, 5, 6, 7, 9, 10
CORNERS = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]        # corner index (di 2 + dj) 2 + dk


def cell(c, x):
    c = np.asarray(c, dtype=np.float64)
    return np.floor((c.size - 1) * (x - c[0]) / (c[-1] - c[0])).astype(np.int64)


def ext_coord(c, i):
    """Coordinate of node i of the auto-extended node set: beyond the ends it continues with the end spacing."""
    c = np.asarray(c, dtype=np.float64); n = c.size
    out = c[np.clip(i, 0, n - 1)].copy()
    lo, hi = i < 0, i > n - 1
    out[lo] = c[0] + i[lo] * (c[1] - c[0])
    out[hi] = c[-1] + (i[hi] - (n - 1)) * (c[-1] - c[-2])
    return out


def trac2grid(tr_x, tr_f, grid, avgscheme):
    """Tracer -> grid: trilinear weights on the eight corners, the four averaging schemes, auto-extension + crop (a
    contribution to a node outside the target set is dropped), NaN (0/0) where nothing arrives."""
    n = [len(c) for c in grid]
    idx, t = [], []
    for d in range(3):
        i = cell(grid[d], tr_x[:, d])
        c0, c1 = ext_coord(grid[d], i), ext_coord(grid[d], i + 1)
        idx.append(i); t.append((tr_x[:, d] - c0) / (c1 - c0))
    wsum = np.zeros(n); cnt = np.zeros(n)
    W, at = {}, {}
    for c in CORNERS:
        w = np.ones(tr_x.shape[0])
        for d in range(3):
            w = w * (t[d] if c[d] else 1 - t[d])
        node = [idx[d] + c[d] for d in range(3)]
        ok = np.ones(tr_x.shape[0], dtype=bool)
        for d in range(3):
            ok &= (node[d] >= 0) & (node[d] < n[d])
        W[c] = w[ok]; at[c] = (tuple(q[ok] for q in node), ok)
        np.add.at(wsum, at[c][0], W[c]); np.add.at(cnt, at[c][0], 1.0)
    out = []
    for f in range(tr_f.shape[1]):
        s = avgscheme[f]
        if not s & (AVG_ARITH | AVG_GEOM):
            raise Exception("invalid averaging scheme")
        with np.errstate(all="ignore"):
            val = tr_f[:, f] if s & AVG_ARITH else np.log(tr_f[:, f])
        acc = np.zeros(n)
        for c in CORNERS:
            node, ok = at[c]
            np.add.at(acc, node, val[ok] * W[c] if s & AVG_WEIGHTED else val[ok])
        den = wsum if s & AVG_WEIGHTED else cnt
        with np.errstate(all="ignore"):
            if s & AVG_ARITH:
                out.append(acc / den)
            else:
                acc[np.isinf(acc)] = 0
                out.append(np.exp(acc / den))
    return out


def _locate(p, g):
    n = [len(c) for c in g]
    idx = [cell(g[d], p[:, d]) for d in range(3)]
    bad = np.zeros(p.shape[0], dtype=bool)
    for d in range(3):
        bad |= (idx[d] < 0) | (idx[d] > n[d] - 2)
    idx = [np.where(bad, 0, i) for i in idx]
    d0 = [p[:, d] - np.asarray(g[d])[idx[d]] for d in range(3)]
    d1 = [-(p[:, d] - np.asarray(g[d])[idx[d] + 1]) for d in range(3)]
    t = [d0[d] / (d0[d] + d1[d]) for d in range(3)]
    h = [np.diff(np.asarray(g[d]))[idx[d]] for d in range(3)]
    return idx, bad, d0, d1, t, h


def _trilinear(F, idx, t):
    s = 0
    for c in CORNERS:
        w = (t[0] if c[0] else 1 - t[0]) * (t[1] if c[1] else 1 - t[1]) * (t[2] if c[2] else 1 - t[2])
        s = s + w * F[idx[0] + c[0], idx[1] + c[1], idx[2] + c[2]]
    return s


def veldiv(p, g, V, defval=0.0):
    """U_d = trilinear(V_d) + t_d (1 - t_d) (h_d / 2) [M_de(1/4 + t_f / 2) / h_e + M_df(1/4 + t_e / 2) / h_f] with
    M_de(s) = (1 - s) (delta_d delta_e V_e on the face f = 0) + s (the same on the face f = 1)."""
    idx, bad, _, _, t, h = _locate(p, g)

    def corner(F, c):
        return F[idx[0] + c[0], idx[1] + c[1], idx[2] + c[2]]

    def mixed(F, d, e, f, s):
        def face(kf):
            tot = 0
            for a in (0, 1):
                for b in (0, 1):
                    c = [0, 0, 0]; c[d] = a; c[e] = b; c[f] = kf
                    tot = tot + (1 if a == b else -1) * corner(F, c)
            return tot
        return (1 - s) * face(0) + s * face(1)
    out = np.empty((p.shape[0], 3))
    for d in range(3):
        e, f = [q for q in range(3) if q != d]
        G = 0.5 * h[d] * (mixed(V[e], d, e, f, 0.25 + 0.5 * t[f]) / h[e] + mixed(V[f], d, f, e, 0.25 + 0.5 * t[e]) / h[f])
        out[:, d] = _trilinear(V[d], idx, t) + t[d] * (1 - t[d]) * G
    out[bad, :] = defval
    return out


def grid2trac(tr_x, grid, fields, defval=np.nan, method=M_LINEAR):
    """Grid -> tracer, (n, nf).  Out-of-grid tracers (cell index < 0 or > n-2 on any axis) get defval in every column."""
    if method & M_VELDIV and not method & (M_NEAREST | M_LINEAR):
        return veldiv(tr_x, grid, fields, defval)
    idx, bad, d0, d1, t, _ = _locate(tr_x, grid)
    out = np.empty((tr_x.shape[0], len(fields)))
    if method & M_NEAREST:
        d2 = np.stack([(d1[0] if c[0] else d0[0]) ** 2 + (d1[1] if c[1] else d0[1]) ** 2 + (d1[2] if c[2] else d0[2]) ** 2 for c in CORNERS], axis=1)
        m = np.argmin(d2, axis=1)
        for k, F in enumerate(fields):
            out[:, k] = F[idx[0] + (m >> 2), idx[1] + ((m >> 1) & 1), idx[2] + (m & 1)]
    else:
        for k, F in enumerate(fields):
            out[:, k] = _trilinear(F, idx, t)
    out[bad, :] = defval
    return out


def rk4(tr_x, grids, vels, tstep):
    """Four VELDIV stages, out-of-grid velocity 0, the reference's weights (1,1,1,1)/6 (pylamp_trac.py:385)."""
    k1 = veldiv(tr_x, grids, vels)
    k2 = veldiv(tr_x + 0.5 * tstep * k1, grids, vels)
    k3 = veldiv(tr_x + 0.5 * tstep * k2, grids, vels)
    k4 = veldiv(tr_x + tstep * k3, grids, vels)
    xnew = tr_x + (1 / 6) * tstep * (k1 + k2 + k3 + k4)
    return (xnew - tr_x) / tstep, xnew


def fence(x, L, eps=2.0 ** -10):
    x = x.copy()
    for d in range(3):
        x[x[:, d] <= 0, d] = eps
        x[x[:, d] >= L[d], d] = L[d] - eps
    return x


def property_update(tr_f, tdep_rho, tdep_eta, Tref=1623.0, etamin=1e17, etamax=1e23):
    """pylamp2.py:291-303 (in place)."""
    if tdep_rho:
        tr_f[:, TR_RHO] = ((tr_f[:, TR_ALP] * (tr_f[:, TR_TMP] - Tref) + 1) / tr_f[:, TR_RH0]) ** (-1)
    else:
        tr_f[:, TR_RHO] = tr_f[:, TR_RH0]
    if tdep_eta:
        e = tr_f[:, TR_ET0] * np.exp(tr_f[:, TR_ACE] / (GASR * tr_f[:, TR_TMP]) - tr_f[:, TR_ACE] / (GASR * Tref))
        tr_f[:, TR_ETA] = np.clip(e, etamin, etamax)
    else:
        tr_f[:, TR_ETA] = tr_f[:, TR_ET0]


def temp_to_tracers(tr_x, tr_f, grid, field, absolute, subgrid, tstep):
    """pylamp2.py:445-480 with (2/dz)^2 + (2/dx)^2 + (2/dy)^2 in the subgrid time scale; returns the new tracer temperatures."""
    T = tr_f[:, TR_TMP]
    if absolute:
        return grid2trac(tr_x, grid, [field])[:, 0]
    Tn = T + grid2trac(tr_x, grid, [field])[:, 0]
    if not subgrid:
        return Tn
    inv2 = sum((2 / ((g[-1] - g[0]) / (len(g) - 1))) ** 2 for g in grid)
    dt0 = tr_f[:, TR_HCP] * tr_f[:, TR_RHO] / (tr_f[:, TR_HCD] * inv2)
    Tsub = T - (T - Tn) * np.exp(-0.5 * tstep / dt0)
    dTs = Tsub - Tn
    f_sgc, = trac2grid(tr_x, dTs[:, None], grid, [AVG_ARITH | AVG_WEIGHTED])
    return Tsub - grid2trac(tr_x, grid, [f_sgc])[:, 0]
