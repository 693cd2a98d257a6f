"""CPU checks of the 3-D markers' search mode (rectilinear grids): the NumPy model tests/mic3_rect_model.py reduces to the 2-D
oracle under oracle.rect_search() by extrusion along each axis, equals the regular-grid model's cells on a uniform grid, has the
properties the regular formula loses on a graded grid, and the switch exists at every layer of the public surface."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, maxrel, pointrel
import mic3_model as U
import mic3_rect_model as M


def _positions(rng, g, n, outside=0.9, faces=200):
    """(n, len(g)) positions: random up to `outside` end spacings beyond the set, some exactly on interior faces and on the first
    coordinate -- none exactly on the last coordinate (there the 2-D oracle's answer depends on the other tracers)."""
    lo = np.array([c[0] - outside * (c[1] - c[0]) for c in g]); hi = np.array([c[-1] + outside * (c[-1] - c[-2]) for c in g])
    p = lo + rng.random((n, len(g))) * (hi - lo)
    k = 0
    for d, c in enumerate(g):
        p[k:k + faces, d] = c[rng.integers(0, len(c) - 1, faces)]; k += faces
    for d, c in enumerate(g):
        assert not (p[:, d] == c[-1]).any()
    return p


def _grids(ax):
    g2 = [M.graded(9, 660e3, 3.0), M.graded(11, 820e3, 1 / 3.0)]
    gax = M.graded(6, 300e3, 2.0)
    g3 = list(g2); g3.insert(ax, gax)
    return g2, gax, g3


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_model_grid2trac_reduces_to_the_2d_oracle_under_rect_search(oracle, ax):
    rng = np.random.default_rng(20 + ax)
    g2, gax, g3 = _grids(ax)
    keep = [d for d in range(3) if d != ax]
    n2 = [g2[0].size, g2[1].size]; n3 = [c.size for c in g3]
    V2 = [rng.standard_normal(n2) for _ in range(2)]
    V3 = [None] * 3
    for q, d in enumerate(keep):
        V3[d] = np.repeat(np.expand_dims(V2[q], ax), n3[ax], axis=ax)
    V3[ax] = np.zeros(n3)
    p2 = _positions(rng, g2, 3000)
    p3 = np.insert(p2, ax, rng.uniform(gax[0], gax[-1], 3000) * 0.999999, axis=1)
    with oracle.rect_search():
        for m3, m2 in ((U.M_LINEAR, oracle.M_LINEAR), (U.M_NEAREST, oracle.M_NEAREST)):
            a = M.grid2trac(p3, g3, [V3[keep[0]], V3[keep[1]]], defval=-7.0, method=m3)
            b = oracle.grid2trac(p2, g2, V2, n2, defval=-7.0, method=m2)
            assert (b[:, 0] == -7.0).sum() > 100 and maxrel(a, b) < 1e-14
        # VELDIV: in-domain tracers (the 2-D code leaves vz extrapolated for the others, which 3-D deliberately does not copy)
        ins = np.all([(p2[:, q] >= g2[q][0]) & (p2[:, q] < g2[q][-1]) for q in range(2)], axis=0)
        o3 = M.grid2trac(p3[ins], g3, V3, defval=0, method=U.M_VELDIV)
        o2 = oracle.grid2trac(p2[ins], g2, V2, n2, defval=0, method=oracle.M_VELDIV)
    assert np.abs(o3[:, keep] - o2).max() <= 4e-15 * np.abs(o2).max() and np.abs(o3[:, ax]).max() <= 1e-15


def _product(rng, g2, gax, ax, n2=3000, per_layer=2):
    p2 = _positions(rng, g2, n2)
    f2 = np.stack([rng.uniform(2900, 3300, n2), 10 ** rng.uniform(18, 23, n2)], 1)
    ys = np.concatenate([gax[i] + rng.uniform(0.1, 0.9, per_layer) * (gax[i + 1] - gax[i]) for i in range(gax.size - 1)])
    p3 = np.concatenate([np.insert(p2, ax, y, axis=1) for y in ys])
    return p2, f2, p3, np.tile(f2, (ys.size, 1))


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_model_trac2grid_reduces_to_the_2d_oracle_under_rect_search(oracle, ax):
    rng = np.random.default_rng(30 + ax)
    g2, gax, g3 = _grids(ax)
    nx2 = [g2[0].size, g2[1].size]; na = gax.size
    p2, f2, p3, f3 = _product(rng, g2, gax, ax)
    sch = [5, 6, 1, 2]
    with oracle.rect_search():
        r2 = oracle.trac2grid(p2, f2[:, [0, 1, 0, 1]], g2, nx2, sch)
    r3 = M.trac2grid(p3, f3[:, [0, 1, 0, 1]], g3, sch)
    for k in range(4):
        assert not np.isnan(r2[k]).any()
        for j in range(na):
            sl = np.take(r3[k], j, axis=ax)
            assert (maxrel(sl, r2[k]) < 1e-12) if sch[k] & 1 else (pointrel(sl, r2[k]) < 1e-11), (sch[k], j)
    # midpoint sets (with the appended point): tracers below the first and beyond the last coordinate of the target
    mp2 = oracle.gridmp_of(g2); mpa = oracle.gridmp_of([gax])[0]
    mp3 = list(mp2); mp3.insert(ax, mpa)
    with oracle.rect_search():
        r2 = oracle.trac2grid(p2, f2, mp2, nx2, [5, 6])
    r3 = M.trac2grid(p3, f3, mp3, [5, 6])
    for k in range(2):
        for j in range(na - 1):
            sl = np.take(r3[k], j, axis=ax)[:-1, :-1]
            assert (maxrel(sl, r2[k][:-1, :-1]) < 1e-12) if k == 0 else (pointrel(sl, r2[k][:-1, :-1]) < 1e-11), (k, j)


def test_model_cells_equal_the_regular_formula_on_a_uniform_grid():
    rng = np.random.default_rng(3)
    for n, lo, hi in ((7, -0.1, 1.3), (33, 0.0, 1.0e5), (18, 1.0e3, 0.9e5)):
        c = np.linspace(lo, hi, n)
        h = c[1] - c[0]
        x = rng.uniform(lo - 2.5 * h, hi + 2.5 * h, 20000)
        assert np.array_equal(M.cell(c, x), U.cell(c, x))


def test_properties_on_a_graded_grid():
    rng = np.random.default_rng(4)
    g = [M.graded(9, 1.0, 5.0, -0.1), M.graded(8, 2.0, 0.25), M.refined(10, 1.5, 3.0)]
    n = [c.size for c in g]
    p = np.stack([rng.uniform(c[0], c[-1], 5000) * (1 - 1e-12) for c in g], 1)
    p[:300, 1] = g[1][rng.integers(0, n[1] - 1, 300)]
    # weights in [0, 1] (the regular formula leaves the interval on this grid)
    _, bad, _, _, t, _ = M.locate(p, g)
    assert not bad.any() and all((t[d] >= 0).all() and (t[d] <= 1).all() for d in range(3))
    _, _, _, _, tu, _ = U._locate(p, g)
    assert any((tu[d] < 0).any() or (tu[d] > 1).any() for d in range(3))
    # trilinear interpolation reproduces a field that is linear in the coordinates
    Z, X, Y = np.meshgrid(*g, indexing="ij")
    F = 0.3 + 1.1 * Z - 0.7 * X + 0.45 * Y
    ref = 0.3 + 1.1 * p[:, 0] - 0.7 * p[:, 1] + 0.45 * p[:, 2]
    assert np.abs(M.grid2trac(p, g, [F])[:, 0] - ref).max() <= 1e-13 * np.abs(ref).max()
    # a constant tracer field scatters to the same constant, weighted or not, arithmetic or geometric
    dense = np.stack([rng.uniform(c[0], c[-1], 40000) for c in g], 1)
    out = M.trac2grid(dense, np.full((dense.shape[0], 4), 3.25), g, [5, 6, 1, 2])
    for k in range(4):
        assert not np.isnan(out[k]).any() and np.abs(out[k] - 3.25).max() <= 1e-13 * 3.25


def test_veldiv_divergence_is_constant_in_a_graded_cell():
    """Property (1) of tests/test_mic3_model.py with the spacings of the found cell.  The bound is the one derived there,
    3 terms * (1 + sum of spacing ratios / 4) * 16 rounded operations * eps max|V| / (delta h_d), with the spacings and the
    spacing ratios sum_{e != d} h_d / h_e (largest over d) of each cell instead of one number for the grid."""
    rng = np.random.default_rng(5)
    g = [M.graded(7, 1.4, 5.0, -0.1), M.graded(6, 2.2, 0.2, -0.2), M.graded(8, 0.95, 3.0, -0.05)]
    n = [c.size for c in g]
    V = [rng.standard_normal(n) for _ in range(3)]
    cells = rng.integers(0, [n[0] - 1, n[1] - 1, n[2] - 1], (200, 3))
    lo = np.stack([g[d][cells[:, d]] for d in range(3)], 1)
    hh = np.stack([np.diff(g[d])[cells[:, d]] for d in range(3)], 1)
    dl = 1e-3

    def div(p):
        s = 0
        for d in range(3):
            e = np.zeros((200, 3)); e[:, d] = dl * hh[:, d]
            s = s + (M.veldiv(p + e, g, V)[:, d] - M.veldiv(p - e, g, V)[:, d]) / (2 * dl * hh[:, d])
        return s
    d1 = div(lo + rng.uniform(0.1, 0.9, (200, 3)) * hh)
    d2 = div(lo + rng.uniform(0.1, 0.9, (200, 3)) * hh)
    md = np.zeros(200)
    for q, c in enumerate(cells):
        for d in range(3):
            blk = V[d][c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2]
            md[q] += (np.take(blk, 1, axis=d) - np.take(blk, 0, axis=d)).mean() / hh[q, d]
    ratios = np.max([sum(hh[:, d] / hh[:, e] for e in range(3) if e != d) for d in range(3)], axis=0)
    bound = 3 * (1 + ratios / 4) * 16 * 2.0 ** -52 * max(np.abs(v).max() for v in V) / (dl * hh.min(axis=1))
    assert (np.abs(d1 - d2) <= bound).all() and (np.abs(d1 - md) <= bound).all() and (np.abs(d2 - md) <= bound).all()


def test_the_switch_exists_at_every_layer():
    from pylamp_amd import _lib, pylamp3d as P3
    assert P3.Options3().marker_search is False
    nx, L = [5, 5, 5], [1.0, 1.0, 1.0]
    c = np.array([0, 0.1, 0.5, 0.8, 1.0])
    with pytest.raises(Exception, match="non-uniform"):
        P3.Simulation3(nx, L, grid=[c] * 3)
    opt = P3.Options3(marker_search=True)
    with pytest.raises(Exception, match=r"grid\[1\] does not span"):
        P3.Simulation3(nx, L, grid=[c, c * 0.9, c], options=opt)
    with pytest.raises(Exception, match=r"grid\[0\] does not span"):
        P3.Simulation3(nx, L, grid=[c + 0.0 + np.array([0.05, 0, 0, 0, 0]), c, c], options=opt)
    with pytest.raises(Exception, match=r"grid\[2\] is not strictly increasing"):
        P3.Simulation3(nx, L, grid=[c, c, np.array([0, 0.5, 0.5, 0.8, 1.0])], options=opt)
    for name in ("trac2grid", "grid2trac", "RK"):
        import inspect
        assert inspect.signature(getattr(P3, name)).parameters["search"].default is False
    assert callable(P3.Context3.set_marker_search)
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pylamp_hip.h")).read(), flags=re.S)
    for n in ("pl3_mic_set_search", "pl3_mic_get_search"):
        assert re.search(r"\b%s\s*\(" % n, txt), "not declared: " + n
        assert n in _lib.SIGNATURES, "not bound: " + n
    if os.path.exists(_lib.LIB_PATH):
        import subprocess
        syms = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        for n in ("pl3_mic_set_search", "pl3_mic_get_search"):
            assert re.search(r"\bT %s\b" % n, syms), "not exported: " + n
