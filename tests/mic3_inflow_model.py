"""NumPy model of the inflow material of the 3-D refill (plain helper module, no fixtures, no project code): the rule that
include/pylamp_hip.h states at pl3_mic_set_inflow, laid over tests/mic3_refill_model.py.

  * walls w = 0 .. 5 = [z0, x0, y0, zL, xL, yL], axis a = w % 3, the two other axes p < q in z, x, y order;
  * material[w]: None or {column: plane (n_p - 1, n_q - 1)}; flow[w]: None or the plane Un_w of the wall-normal velocity along +a;
  * a refilled cell (i_z, i_x, i_y) is an inflow cell of w when w has a material, the cell's index along a is 0 (low wall) or
    n_a - 2 (high wall) and Un_w[i_p, i_q] > 0 (low) or < 0 (high); the first such w in the order 0 .. 5 decides alone;
  * s(x) = x_a - c_a[0] (low) or c_a[n_a - 1] - x_a (high); dmin = the smallest s among the cell's residents, NaN ignored, +inf without
    residents; new tracer q is an inflow tracer exactly when s(x_q) < dmin and then takes material[w][col][i_p, i_q] in the wall's
    columns; everything else is the refill's.

search = True takes the cell membership of the residents from np.searchsorted(c, x, 'right') - 1 (tests/mic3_rect_model.py), as the
header's search rule states; the overlay itself only uses the cell the refill reports for every row.
"""
import numpy as np

import mic3_refill_model as R
import mic3_rect_model as S

AXES = ((1, 2), (0, 2), (0, 1))


def inflow_wall(ic, nc, material, flow):
    """The wall whose material the cell ic = [i_z, i_x, i_y] takes (None: no inflow cell), and for every wall why it does not
    qualify: 'none' (no material), 'away' (the cell does not touch it), 'noflow', 'outward' (or zero), or 'in'."""
    why = []
    for w in range(6):
        a = w % 3
        p, q = AXES[a]
        if material is None or material[w] is None:
            why.append("none")
        elif ic[a] != (0 if w < 3 else nc[a] - 1):
            why.append("away")
        elif flow is None or flow[w] is None:
            why.append("noflow")
        else:
            un = float(np.asarray(flow[w])[ic[p], ic[q]])
            why.append("in" if (un > 0 if w < 3 else un < 0) else "outward")
    first = why.index("in") if "in" in why else None
    return first, why


def refill(tr_x, tr_f, grid, tracdens, tracdens_min, seed, it, unique_ids=False, tr_v=None, material=None, flow=None, search=False):
    """mic3_refill_model.refill (search: on the search rule's cells) with the inflow rule laid over it.  info gains: inflow (mask of
    the rows that took a wall's material), ninflow, wall (per deficient cell: the deciding wall or -1), why (per deficient cell: the
    six verdicts of inflow_wall), dmin (per deficient cell; inf where it has no wall or no resident)."""
    base = S.refill if search else R.refill
    x, f, v, info = base(tr_x, tr_f, grid, tracdens, tracdens_min, seed, it, unique_ids=unique_ids, tr_v=tr_v)
    grid = [np.asarray(g, dtype=np.float64) for g in grid]
    nc = [g.size - 1 for g in grid]
    new, cell = info["new"], info["cell"]
    inflow = np.zeros(x.shape[0], dtype=bool)
    walls, whys, dmins = [], [], []
    for c in info["cells"]:
        ic = [int(c) // (nc[2] * nc[1]), (int(c) // nc[2]) % nc[1], int(c) % nc[2]]
        w, why = inflow_wall(ic, nc, material, flow)
        walls.append(-1 if w is None else w); whys.append(why)
        if w is None:
            dmins.append(np.inf)
            continue
        a = w % 3
        p, q = AXES[a]
        dist = (lambda pos: pos - grid[a][0]) if w < 3 else (lambda pos: grid[a][-1] - pos)
        rows = np.where(cell == c)[0]
        res, fresh = rows[~new[rows]], rows[new[rows]]
        s = dist(x[res, a])
        s = s[~np.isnan(s)]
        dmin = float(s.min()) if s.size else np.inf
        dmins.append(dmin)
        take = fresh[dist(x[fresh, a]) < dmin]
        for col, plane in material[w].items():
            f[take, int(col)] = float(np.asarray(plane, dtype=np.float64)[ic[p], ic[q]])
        inflow[take] = True
    info = dict(info, inflow=inflow, ninflow=int(inflow.sum()), wall=np.array(walls, dtype=np.int64), why=whys, dmin=np.array(dmins))
    return x, f, v, info
