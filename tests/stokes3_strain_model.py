"""A plain NumPy model of the 3-D strain-rate, stress and dissipation fields, written from the statement of the definition in
include/pylamp_hip.h (pl3_stokes_strain_fields) and DESIGN.md section 6c; the HIP kernels are compared with it in
tests/test_hip_3d_strain.py.  No GPU, no project code: only NumPy, everything in np.longdouble.  tests/test_strain3_model.py ties it to
the operator model (tests/stokes3_model.py and its wall models): the divergence of these stresses is that operator's momentum row.

Arrays are (nz, nx, ny) as in stokes3_model: vz at (z_i, x_j+1/2, y_k+1/2), vx at (z_i+1/2, x_j, y_k+1/2), vy at (z_i+1/2, x_j+1/2, y_k),
etan at the cell centres, etas at the nodes.  A wall is one of [z0, x0, y0, zL, xL, yL], kind NOSLIP (0) or FREESLIP (1); wallvel is
(6, 3): (Uz, Ux, Uy) per wall.

Pair p of the shear components is (D, E) = (p, p + 1 mod 3) with F = p + 2 mod 3: (z, x), (x, y), (y, z).  Its edge array has n_D entries
along D, n_E along E (nodes) and n_F - 1 along F (cells), in (z, x, y) axis order.

Magnitudes.  Every quantity is a sum of products; its "magnitude" is the same expression with every velocity difference a - b replaced by
|a| + |b| (so a strain rate e has magnitude m >= |e|, and e^2 has m^2).  A computation in a floating-point format with unit eps errs by a
small multiple of eps x magnitude.  For the two square-root fields the error of the radicand Y, at most k eps M_Y, propagates to first
order as k eps M_Y / (4 sqrt(Y / 2)): that quotient is their magnitude (infinite where the field is exactly zero).
"""
import numpy as np

LD = np.longdouble
NOSLIP, FREESLIP = 0, 1
PAIRS = ((0, 1, 2), (1, 2, 0), (2, 0, 1))          # (D, E, F)


def _ld(a):
    return np.asarray(a, dtype=LD)


def _along(v, axis):
    s = [1, 1, 1]; s[axis] = -1
    return np.asarray(v).reshape(s)


def _take(a, axis, sl):
    idx = [slice(None)] * 3; idx[axis] = sl
    return a[tuple(idx)]


def widths(grid):
    """Per axis: cell widths d (n - 1) and the widths h of the node control volumes (n; half a cell on the walls)."""
    d = [np.diff(_ld(g)) for g in grid]
    h = []
    for a in range(3):
        w = np.empty(d[a].size + 1, dtype=LD)
        w[0] = d[a][0] / 2; w[-1] = d[a][-1] / 2; w[1:-1] = (d[a][:-1] + d[a][1:]) / 2
        h.append(w)
    return d, h


def _shear_half(vD, D, A, F, grid, noslip_lo, noslip_hi, U_lo, U_hi):
    """dv_D/dx_A on the edges of the pair {D, A}: (value, magnitude), n_A entries along A (nodes), n_F - 1 along F, n_D along D."""
    c = _ld(grid[A])
    n = c.size
    u = _take(vD, F, slice(0, -1))                    # the ghost along F goes
    shp = list(u.shape)
    g = np.zeros(shp, dtype=LD); m = np.zeros(shp, dtype=LD)
    hA = (c[2:] - c[:-2]) / 2                          # between the midpoints of the cells i - 1 and i, i = 1 .. n - 2
    a, b = _take(u, A, slice(1, n - 1)), _take(u, A, slice(0, n - 2))
    idx = [slice(None)] * 3; idx[A] = slice(1, n - 1)
    g[tuple(idx)] = (a - b) / _along(hA, A)
    m[tuple(idx)] = (np.abs(a) + np.abs(b)) / _along(hA, A)
    if noslip_lo:                                      # one-sided against the wall's velocity, half a cell away
        idx[A] = 0
        w = (c[1] - c[0]) / 2
        g[tuple(idx)] = (_take(u, A, 0) - U_lo) / w
        m[tuple(idx)] = (np.abs(_take(u, A, 0)) + abs(U_lo)) / w
    if noslip_hi:
        idx[A] = n - 1
        w = (c[n - 1] - c[n - 2]) / 2
        g[tuple(idx)] = (U_hi - _take(u, A, n - 2)) / w
        m[tuple(idx)] = (np.abs(_take(u, A, n - 2)) + abs(U_hi)) / w
    return g, m


def _to_nodes(q, axis, d, h):
    """Cells -> nodes along one axis: a cell gives each of its two end nodes half of its width."""
    n = d.size + 1
    shp = list(q.shape); shp[axis] = n
    out = np.zeros(shp, dtype=LD)
    lo = [slice(None)] * 3; hi = [slice(None)] * 3
    lo[axis] = slice(0, n - 1); hi[axis] = slice(1, n)
    half = q * _along(d, axis) / 2
    out[tuple(lo)] += half
    out[tuple(hi)] += half
    return out / _along(h, axis)


def strain_fields(nx, grid, etas, etan, v, bc=None, wallvel=None):
    """The centre and edge components, the three node fields, the integral of the dissipation and the magnitudes.  Returns a dict:
    eDD [3] (cells), mDD; eDE [3] (edges of the pairs), mDE; eta_edge [3]; strainrate, stress, dissipation (nodes, longdouble);
    total_centres, total_edges, total = their sum, total_nodes = sum dissipation x V_node; mag = {field: per-node magnitude} and
    mag_total = sum of the dissipation's magnitude x V_node."""
    n = [int(k) for k in nx]
    kinds = [FREESLIP] * 6 if bc is None else [int(b) for b in bc]
    U = np.zeros((6, 3), dtype=LD) if wallvel is None else _ld(wallvel).reshape(6, 3)
    V = [_ld(a) for a in v]
    es, en = _ld(etas), _ld(etan)
    d, h = widths(grid)
    cells = tuple(slice(0, k - 1) for k in n)
    enc = en[cells]
    # normal components at the cell centres
    eDD, mDD = [], []
    for D in range(3):
        a, b = _take(V[D], D, slice(1, None)), _take(V[D], D, slice(0, -1))
        o = list(cells); o[D] = slice(None)
        eDD.append(((a - b) / _along(d[D], D))[tuple(o)])
        mDD.append(((np.abs(a) + np.abs(b)) / _along(d[D], D))[tuple(o)])
    # shear components on the edges
    eDE, mDE, eta_e = [], [], []
    for D, E, F in PAIRS:
        g1, m1 = _shear_half(V[D], D, E, F, grid, kinds[E] == NOSLIP, kinds[E + 3] == NOSLIP, U[E, D], U[E + 3, D])
        g2, m2 = _shear_half(V[E], E, D, F, grid, kinds[D] == NOSLIP, kinds[D + 3] == NOSLIP, U[D, E], U[D + 3, E])
        eDE.append((g1 + g2) / 2); mDE.append((m1 + m2) / 2)
        eta_e.append((_take(es, F, slice(0, -1)) + _take(es, F, slice(1, None))) / 2)

    def nodes(centre, edge):
        """The control-volume weighted mean around the nodes of a centre quantity plus the three edge quantities."""
        q = centre
        for a in range(3):
            q = _to_nodes(q, a, d[a], h[a])
        for p, (D, E, F) in enumerate(PAIRS):
            q = q + _to_nodes(edge[p], F, d[F], h[F])
        return q

    s2, m2 = sum(e * e for e in eDD), sum(m * m for m in mDD)
    Y = nodes(s2, [2 * e * e for e in eDE]);                          MY = nodes(m2, [2 * m * m for m in mDE])
    T = nodes((2 * enc) ** 2 * s2, [2 * (2 * eta_e[p] * eDE[p]) ** 2 for p in range(3)])
    MT = nodes((2 * enc) ** 2 * m2, [2 * (2 * eta_e[p] * mDE[p]) ** 2 for p in range(3)])
    phi_c, phi_e = 2 * enc * s2, [4 * eta_e[p] * eDE[p] ** 2 for p in range(3)]
    P = nodes(phi_c, phi_e);                                          MP = nodes(2 * enc * m2, [4 * eta_e[p] * mDE[p] ** 2 for p in range(3)])
    e2, t2 = np.sqrt(Y / 2), np.sqrt(T / 2)
    vol_c = _along(d[0], 0) * _along(d[1], 1) * _along(d[2], 2)
    vol_n = _along(h[0], 0) * _along(h[1], 1) * _along(h[2], 2)
    tot_c = np.sum(phi_c * vol_c)
    tot_e = LD(0)
    for p, (D, E, F) in enumerate(PAIRS):
        tot_e = tot_e + np.sum(phi_e[p] * _along(h[D], D) * _along(h[E], E) * _along(d[F], F))
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = dict(dissipation=MP, strainrate=np.where(e2 > 0, MY / (4 * e2), np.inf), stress=np.where(t2 > 0, MT / (4 * t2), np.inf))
    return dict(eDD=eDD, mDD=mDD, eDE=eDE, mDE=mDE, eta_edge=eta_e, strainrate=e2, stress=t2, dissipation=P, total_centres=tot_c,
                total_edges=tot_e, total=tot_c + tot_e, total_nodes=np.sum(P * vol_n), mag=mag, mag_total=np.sum(MP * vol_n), vol_nodes=vol_n)


def stress_divergence(nx, grid, etan, res, P, Kc):
    """div(2 eta eps)_D - Kc dP/dx_D of the components `res` (strain_fields) on the rows of v_D with 1 <= i_D <= n_D - 2 and cell indices
    along the two other axes, and its magnitude: (rows, magnitudes), each (nz, nx, ny, 3), zero elsewhere."""
    n = [int(k) for k in nx]
    d, h = widths(grid)
    cells = tuple(slice(0, k - 1) for k in n)
    en, p = _ld(etan)[cells], _ld(P)[cells]
    rows = np.zeros(n + [3], dtype=LD); mags = np.zeros(n + [3], dtype=LD)
    for D, E, F in PAIRS:
        hD = _along(h[D][1:-1], D)
        inner = slice(1, n[D] - 1)
        acc, mag = [], []
        for q, absq in ((res["eDD"][D], res["mDD"][D]),):
            s, ms = 2 * en * q, 2 * en * absq
            acc.append((_take(s, D, slice(1, None)) - _take(s, D, slice(0, -1))) / hD)
            mag.append((_take(ms, D, slice(1, None)) + _take(ms, D, slice(0, -1))) / hD)
        acc.append(-LD(Kc) * (_take(p, D, slice(1, None)) - _take(p, D, slice(0, -1))) / hD)
        mag.append(LD(Kc) * (np.abs(_take(p, D, slice(1, None))) + np.abs(_take(p, D, slice(0, -1)))) / hD)
        # the pair {D, E} is pair D (edges: nodes along D and E, cells along F); the pair {D, F} is pair F (nodes along F and D, cells along E)
        for pair, A, B in ((D, E, F), (F, F, E)):
            s = 2 * res["eta_edge"][pair] * res["eDE"][pair]; ms = 2 * res["eta_edge"][pair] * res["mDE"][pair]
            s, ms = _take(s, D, inner), _take(ms, D, inner)            # (cells along B already)
            acc.append((_take(s, A, slice(1, None)) - _take(s, A, slice(0, -1))) / _along(d[A], A))
            mag.append((_take(ms, A, slice(1, None)) + _take(ms, A, slice(0, -1))) / _along(d[A], A))
        o = list(cells); o[D] = inner
        rows[tuple(o) + (D,)] = sum(acc)
        mags[tuple(o) + (D,)] = sum(mag)
    return rows, mags
