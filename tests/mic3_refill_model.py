"""NumPy model of the 3-D census + refill (plain helper module, no fixtures): the dimension-by-dimension extension of
pylamp2.py:588-633 that include/pylamp_hip.h describes for pl3_resident_refill.

  * cell of a tracer = floor((n-1)(x-c0)/L) per axis, clamped into the node set; linear index c = (i (nx-1) + j)(ny-1) + k;
  * the tracers are sorted by cell (stable); a cell with count < tracdens_min receives tracdens - count new tracers, which are
    placed directly behind its residents;
  * positions g_d[i_d] + u_d (g_d[i_d+1] - g_d[i_d]) with u_d = inj_uniform(seed, c, q, 3 it + d) for the q-th new tracer of the cell;
  * every field except TR__ID = the plain mean of the residents, summed one after the other in resident order (0/0 = NaN);
  * IDs: maxid + off[c] + q - rank[c] (the reference's rule) or maxid + 1 + off[c] + q (unique).

With ONE cell layer along y the cell number is the 2-D one and the rule is oracle.inject (tests/test_mic3_refill_model.py).
"""
import numpy as np

NF, TR_ID = 13, 12
MASK = (1 << 64) - 1


def inj_uniform(seed, a, b, c):
    """The counter-based generator of the injection kernels (inj_uniform in pylamp_amd/csrc/pl_internal.h) in Python integers:
    a, b, c are 32-bit unsigned (a + 1 wraps at 2^32), the mixing runs modulo 2^64."""
    h = (int(seed) & MASK) ^ ((0x9E3779B97F4A7C15 * ((int(a) + 1) & 0xFFFFFFFF)) & MASK) ^ ((0xC2B2AE3D27D4EB4F * ((int(b) + 1) & 0xFFFFFFFF)) & MASK) \
        ^ ((0x165667B19E3779F9 * ((int(c) + 1) & 0xFFFFFFFF)) & MASK)
    h ^= h >> 33; h = (h * 0xff51afd7ed558ccd) & MASK
    h ^= h >> 33; h = (h * 0xc4ceb9fe1a85ec53) & MASK
    h ^= h >> 33
    return float(h >> 11) * (1.0 / 9007199254740992.0)


def cells_of(tr_x, grid):
    """(linear cell, [i, j, k]) with the clamping of the sort (a tracer outside counts to the nearest cell)."""
    idx = []
    for d in range(3):
        g = np.asarray(grid[d], dtype=np.float64); n = g.size
        f = np.floor((n - 1) * (tr_x[:, d] - g[0]) / (g[-1] - g[0]))
        idx.append(np.clip(np.nan_to_num(f, nan=0.0), 0, n - 2).astype(np.int64))
    ncx, ncy = len(grid[1]) - 1, len(grid[2]) - 1
    return (idx[0] * ncx + idx[1]) * ncy + idx[2], idx


def refill(tr_x, tr_f, grid, tracdens, tracdens_min, seed, it, unique_ids=False, tr_v=None):
    """Returns (x, f, v, info) in the resident order the GPU leaves: cell by cell, residents in their stable order, the new
    tracers of the cell behind them.  info: ninjected, nrefilled, nempty, mincount, census (after), new (mask of the new rows),
    cell (of every row), ordinal (q of the new rows, -1 for residents), cells (the deficient ones), need."""
    tr_x = np.asarray(tr_x, dtype=np.float64); tr_f = np.asarray(tr_f, dtype=np.float64)
    n = tr_x.shape[0]
    tr_v = np.zeros((n, 3)) if tr_v is None else np.asarray(tr_v, dtype=np.float64)
    nc = [len(g) - 1 for g in grid]
    m = nc[0] * nc[1] * nc[2]
    cell, _ = cells_of(tr_x, grid)
    order = np.argsort(cell, kind="stable")
    cnt = np.bincount(cell, minlength=m)
    few = cnt < tracdens_min if tracdens_min > 0 else np.zeros(m, dtype=bool)
    need = np.where(few, tracdens - cnt, 0)
    off = np.cumsum(need) - need
    rank = np.cumsum(few) - few
    total = cnt + need
    start = np.cumsum(total) - total
    res0 = np.cumsum(cnt) - cnt                       # start of the residents in the plainly sorted arrays
    N = n + int(need.sum())
    x = np.empty((N, 3)); f = np.empty((N, NF)); v = np.zeros((N, 3))
    new = np.ones(N, dtype=bool); rcell = np.empty(N, dtype=np.int64); ordinal = np.full(N, -1, dtype=np.int64)
    sc = cell[order]
    dest = start[sc] + (np.arange(n) - res0[sc])
    x[dest] = tr_x[order]; f[dest] = tr_f[order]; v[dest] = tr_v[order]; new[dest] = False; rcell[dest] = sc
    maxid = float(np.max(tr_f[:, TR_ID])) if n > 0 else -1.0
    sx, sf = tr_x[order], tr_f[order]
    for c in np.where(few)[0]:
        k = int(cnt[c]); mnew = int(need[c])
        s = np.zeros(NF)
        for t in range(res0[c], res0[c] + k):         # one after the other, in resident order
            s = s + sf[t]
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = s / np.float64(k)
        ic = [c // (nc[2] * nc[1]), (c // nc[2]) % nc[1], c % nc[2]]
        for q in range(mnew):
            r = start[c] + k + q
            for d in range(3):
                g = np.asarray(grid[d], dtype=np.float64)
                u = inj_uniform(seed, c, q, 3 * it + d)
                x[r, d] = g[ic[d]] + u * (g[ic[d] + 1] - g[ic[d]])
            f[r] = mean
            f[r, TR_ID] = maxid + float(off[c] + q + 1) if unique_ids else maxid + float(off[c] + q - rank[c])
            rcell[r] = c; ordinal[r] = q
    info = dict(ninjected=int(need.sum()), nrefilled=int(few.sum()), nempty=int((cnt == 0).sum()), mincount=int(cnt.min()),
                census=total.reshape(nc), new=new, cell=rcell, ordinal=ordinal, cells=np.where(few)[0], need=need[few])
    return x, f, v, info
