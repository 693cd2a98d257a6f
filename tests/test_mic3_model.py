"""CPU checks of the 3-D marker-in-cell layer: the public names exist, and the NumPy model the GPU kernels are compared with
(tests/mic3_model.py) has the properties DESIGN.md section 4 derives and reduces to the 2-D oracle under extrusion along
each of the three axes."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, maxrel, pointrel
import mic3_model as M

NEW_C = ["pl3_trac2grid", "pl3_grid2trac", "pl3_rk4", "pl3_tracers_upload", "pl3_tracers_download", "pl3_tracers_count",
         "pl3_tracers_census", "pl3_resident_props", "pl3_resident_trac2grid", "pl3_resident_temp_to_tracers", "pl3_resident_rk4",
         "pl3_get_tracer_velocity", "pl3_resident_times"]
NEW_PY = ["trac2grid", "grid2trac", "RK", "advection_velocity", "Simulation3", "Options3", "gridmp_of", "INTERP_AVG_ARITHW",
          "INTERP_AVG_GEOMW", "INTERP_AVG_WEIGHTED", "INTERP_METHOD_LINEAR", "INTERP_METHOD_NEAREST", "INTERP_METHOD_VELDIV"]


def test_header_and_module_expose_the_marker_names():
    txt = open(os.path.join(ROOT, "include", "pylamp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from pylamp_amd import _lib, pylamp3d as P3
    for n in NEW_C:
        assert re.search(r"\b%s\s*\(" % n, txt), "not declared: " + n
        assert n in _lib.SIGNATURES, "not bound: " + n
    for n in NEW_PY:
        assert hasattr(P3, n), "pylamp3d." + n
    for n in ("step", "field", "tracers", "tracer_velocity", "census", "close"):
        assert callable(getattr(P3.Simulation3, n))


def test_unsupported_parts_are_rejected_by_name():
    from pylamp_amd import pylamp3d as P3
    nx, L = [5, 5, 5], [1.0, 1.0, 1.0]
    for kw, word in ((dict(tracdens_min=3), "injection"), (dict(tracs_fence_enabled=False), "fence-off"),
                     (dict(surface_stabilization=True), "surface stabilisation")):
        with pytest.raises(Exception, match=word):
            P3.Simulation3(nx, L, options=P3.Options3(**kw))
    with pytest.raises(Exception, match="non-uniform"):
        P3.Simulation3(nx, L, grid=[np.array([0, 0.1, 0.5, 0.8, 1.0])] * 3)


def test_advection_velocity_reduces_to_2d(oracle):
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(5)
    nx2 = [7, 9]; ny = 6
    grid = [np.linspace(0, 3.0, 7), np.linspace(0, 5.0, 9), np.linspace(0, 2.0, ny)]
    v2 = [rng.standard_normal(nx2), rng.standard_normal(nx2)]
    v3 = [np.repeat(v[:, :, None], ny, axis=2) for v in v2] + [np.zeros(nx2 + [ny])]
    g3, V3 = P3.advection_velocity(v3, P3.gridmp_of(grid), nx2 + [ny])
    g2, V2 = oracle.advection_velocity(v2, oracle.gridmp_of(grid[:2]), nx2, [1, 1, 1, 1])
    assert all(np.array_equal(a, b) for a, b in zip(g3[:2], g2)) and g3[2].size == ny + 1
    for k in range(ny + 1):
        assert np.array_equal(V3[0][:, :, k], V2[0]) and np.array_equal(V3[1][:, :, k], V2[1])
    assert not V3[2].any()
    # genuinely 3-D: the normal component changes sign across every wall, the tangential ones are copied
    v3 = [rng.standard_normal(nx2 + [ny]) for _ in range(3)]
    _, V = P3.advection_velocity(v3, P3.gridmp_of(grid), nx2 + [ny])
    inner = (slice(2, -2),) * 2
    assert np.array_equal(V[2][2:-2, 2:-2, 0], -V[2][2:-2, 2:-2, 1]) and np.array_equal(V[0][2:-2, 2:-2, -1], V[0][2:-2, 2:-2, -2])
    assert np.array_equal(V[1][2:-2, 0, 2:-2], -V[1][2:-2, 1, 2:-2]) and np.array_equal(V[2][0][inner], V[2][1][inner])


def _random_setup(seed=0):
    rng = np.random.default_rng(seed)
    n = [7, 6, 8]
    g = [np.linspace(-0.1, 1.3, n[0]), np.linspace(-0.2, 2.0, n[1]), np.linspace(-0.05, 0.9, n[2])]
    V = [rng.standard_normal(n) for _ in range(3)]
    return rng, n, g, V


def test_veldiv_divergence_is_constant_in_a_cell():
    """Property (1): the divergence of U is the same at every point of a cell and equals sum_d mean(delta_d V_d) / h_d.
    Central differences are exact for U_d as a function of x_d (quadratic), so what remains is rounding: each of the three
    terms is a difference of two values of size <= max|U| divided by 2 delta h_d, i.e. <= eps max|U| / (delta h_d) with
    eps = 2^-52; max|U| <= (1 + sum of spacing ratios / 4) max|V| <= 4 max|V| on this grid, and the evaluation of U itself
    carries ~16 rounded operations.  c = 3 * 4 * 16 = 192 covers that with every error at its worst."""
    rng, n, g, V = _random_setup()
    hh = np.array([c[1] - c[0] for c in g])
    cells = rng.integers(0, [n[0] - 1, n[1] - 1, n[2] - 1], (200, 3))
    lo = np.stack([g[d][cells[:, d]] for d in range(3)], 1)
    dl = 1e-3

    def div(p):
        s = 0
        for d in range(3):
            e = np.zeros(3); e[d] = dl * hh[d]
            s = s + (M.veldiv(p + e, g, V)[:, d] - M.veldiv(p - e, g, V)[:, d]) / (2 * dl * hh[d])
        return s
    p1 = lo + rng.uniform(0.1, 0.9, (200, 3)) * hh
    p2 = lo + rng.uniform(0.1, 0.9, (200, 3)) * hh
    d1, d2 = div(p1), div(p2)
    md = np.zeros(200)
    for q, c in enumerate(cells):
        for d in range(3):
            blk = V[d][c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2]
            md[q] += (np.take(blk, 1, axis=d) - np.take(blk, 0, axis=d)).mean() / hh[d]
    bound = 192 * 2.0 ** -52 * max(np.abs(v).max() for v in V) / (dl * hh.min())
    print("divergence: |d1-d2| %.3g  |d1-mean| %.3g  bound %.3g  scale %.3g" % (np.abs(d1 - d2).max(), np.abs(d1 - md).max(), bound, np.abs(md).max()))
    assert np.abs(d1 - d2).max() <= bound
    assert np.abs(d1 - md).max() <= bound and np.abs(d2 - md).max() <= bound
    # plain trilinear interpolation does not have the property (the test can fail)
    tri = lambda p: sum((M.grid2trac(p + np.eye(3)[d] * dl * hh[d], g, [V[d]])[:, 0] - M.grid2trac(p - np.eye(3)[d] * dl * hh[d], g, [V[d]])[:, 0])
                        / (2 * dl * hh[d]) for d in range(3))
    assert np.abs(tri(p1) - tri(p2)).max() > 1e3 * bound


def test_veldiv_normal_component_is_continuous_across_faces():
    """Property (3): the correction vanishes at t_d = 0 and 1, so on a cell face U_d is the plain trilinear value, from both sides."""
    rng, n, g, V = _random_setup(1)
    vmax = max(np.abs(v).max() for v in V)
    for d in range(3):
        p = np.stack([rng.uniform(g[a][0], g[a][-1], 300) for a in range(3)], 1)
        p[:, d] = g[d][rng.integers(1, n[d] - 1, 300)]                  # exactly on interior faces normal to d
        u = M.veldiv(p, g, V)[:, d]
        assert np.abs(u - M.grid2trac(p, g, [V[d]])[:, 0]).max() <= 1e-14 * vmax
        h = g[d][1] - g[d][0]
        for side in (-1, 1):        # a step of 1e-9 h changes U_d by at most ~ (2 |V| / h + correction slope) 1e-9 h < 1e-7 |V|
            q = p.copy(); q[:, d] += side * 1e-9 * h
            assert np.abs(M.veldiv(q, g, V)[:, d] - u).max() <= 1e-7 * vmax


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_model_grid2trac_and_rk4_reduce_to_the_2d_oracle(oracle, ax):
    """Property (2) and the other gather modes: a field that does not vary along `ax`, with zero velocity along it."""
    rng, n, g, _ = _random_setup(2 + ax)
    keep = [d for d in range(3) if d != ax]
    n2 = [n[keep[0]], n[keep[1]]]; g2 = [g[keep[0]], g[keep[1]]]
    V2 = [rng.standard_normal(n2) for _ in range(2)]
    V3 = [None] * 3
    for q, d in enumerate(keep):
        V3[d] = np.repeat(np.expand_dims(V2[q], ax), n[ax], axis=ax)
    V3[ax] = np.zeros(n)
    p = np.stack([rng.uniform(g[d][0], g[d][-1], 2000) for d in range(3)], 1)
    o3 = M.grid2trac(p, g, V3, defval=0, method=M.M_VELDIV)
    o2 = oracle.grid2trac(p[:, keep], g2, V2, n2, defval=0, method=oracle.M_VELDIV)
    assert np.abs(o3[:, keep] - o2).max() <= 4e-15 * np.abs(o2).max() and np.abs(o3[:, ax]).max() <= 1e-15
    for m3, m2 in ((M.M_LINEAR, oracle.M_LINEAR), (M.M_NEAREST, oracle.M_NEAREST)):
        a = M.grid2trac(p, g, [V3[keep[0]], V3[keep[1]]], method=m3)
        b = oracle.grid2trac(p[:, keep], g2, V2, n2, method=m2)
        assert maxrel(a, b) < 1e-14
    # RK4 on the padded centre grid of an nx-node grid: n - 1 nodes, so that n coordinates are the padded set
    # (the oracle indexes past its arrays for a stage position within one spacing beyond the last coordinate: start well inside)
    dt = 0.02
    p = np.stack([rng.uniform(g[d][0] + 0.15 * (g[d][-1] - g[d][0]), g[d][-1] - 0.15 * (g[d][-1] - g[d][0]), 2000) for d in range(3)], 1)
    v3, x3 = M.rk4(p, g, V3, dt)
    v2, x2 = oracle.rk4(p[:, keep], g2, V2, [n2[0] - 1, n2[1] - 1], dt)
    assert maxrel(x3[:, keep], x2) < 1e-14 and maxrel(v3[:, keep], v2) < 1e-9
    assert np.array_equal(x3[:, ax], p[:, ax]) and not v3[:, ax].any()


def product_tracers(rng, g2, L2, gax, ax, n2=3000, per_layer=2):
    """2-D positions replicated at the same coordinates along `ax` (per_layer in every cell layer): only then does the 3-D
    average reduce to the 2-D one exactly.  Fields depend on the 2-D index only."""
    p2 = rng.random((n2, 2)) * L2 * 0.999999 + 1e-3
    f2 = np.stack([rng.uniform(2900, 3300, n2), 10 ** rng.uniform(18, 23, n2)], 1)
    m = per_layer * (gax.size - 1)
    La = gax[-1] - gax[0]
    ys = gax[0] + (np.arange(m) + rng.uniform(0.1, 0.9, m)) * La / m
    p3 = np.concatenate([np.insert(p2, ax, y, axis=1) for y in ys])
    f3 = np.tile(f2, (m, 1))
    return p2, f2, p3, f3


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_model_trac2grid_reduces_to_the_2d_oracle(oracle, ax):
    rng = np.random.default_rng(10 + ax)
    nx2 = [9, 11]; L2 = np.array([660e3, 820e3]); na = 6
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    gax = np.linspace(0, 300e3, na)
    p2, f2, p3, f3 = product_tracers(rng, g2, L2, gax, ax)
    g3 = list(g2); g3.insert(ax, gax)
    for sch in ([5, 6], [1, 2]):
        r2 = oracle.trac2grid(p2, f2, g2, nx2, sch)
        r3 = M.trac2grid(p3, f3, g3, sch)
        for k in range(2):
            assert not np.isnan(r3[k]).any() and not np.isnan(r2[k]).any()
            for j in range(na):
                sl = np.take(r3[k], j, axis=ax)
                assert (maxrel(sl, r2[k]) < 1e-12) if sch[k] & 1 else (pointrel(sl, r2[k]) < 1e-11), (sch[k], j)
    # staggered target (cell centres with the appended point): tracers below the first and beyond the last coordinate
    mp2 = oracle.gridmp_of(g2); mpa = oracle.gridmp_of([gax])[0]
    mp3 = list(mp2); mp3.insert(ax, mpa)
    r2 = oracle.trac2grid(p2, f2[:, 1:], mp2, nx2, [6])[0]
    r3 = M.trac2grid(p3, f3[:, 1:], mp3, [6])[0]
    for j in range(na - 1):
        assert pointrel(np.take(r3, j, axis=ax)[:-1, :-1], r2[:-1, :-1]) < 1e-11
