"""3-D marker-in-cell on the GPU: the kernels against the NumPy model (tests/mic3_model.py) on genuinely 3-D inputs and
against the 2-D oracle under extrusion, run-to-run identity of the scatter, the resident stages against the module-level
functions, and Simulation3 against oracle.step on a y-invariant model.  Tolerances are the ones tests/test_hip_parity.py uses
for the same comparisons in 2-D."""
import numpy as np
import pytest

from conftest import maxrel, relerr
import mic3_model as M
from test_mic3_model import product_tracers, _random_setup

pytestmark = pytest.mark.gpu

NF = 13
TR_TMP, TR_HCD, TR_HCP, TR_RHO, TR_ID = 3, 4, 5, 0, 12


def _t2g(P3, tr_x, tr_f, grid, sch):
    shp = [len(c) for c in grid]
    out = [np.zeros(shp) for _ in sch]
    P3.trac2grid(tr_x, tr_f, None, grid, out, shp, avgscheme=list(sch))
    return out


def _g2t(P3, tr_x, grid, fields, defval=np.nan, method=16):
    out = np.zeros((tr_x.shape[0], len(fields)))
    P3.grid2trac(tr_x, out, grid, fields, [len(c) for c in grid], defval=defval, method=method)
    return out


def _cloud(rng, grid, n, margin=0.6):
    """Random positions reaching `margin` spacings beyond the node set on every side, plus tracers exactly on cell faces, on the
    first / last coordinate of every axis and well outside."""
    lo = np.array([c[0] - margin * (c[1] - c[0]) for c in grid]); hi = np.array([c[-1] + margin * (c[-1] - c[-2]) for c in grid])
    p = lo + rng.random((n, 3)) * (hi - lo)
    k = 0
    for d in range(3):
        m = 2000
        p[k:k + m, d] = grid[d][rng.integers(0, len(grid[d]), m)]; k += m          # exactly on faces, the walls included
        p[k:k + 50, d] = grid[d][0]; p[k + 50:k + 100, d] = grid[d][-1]; k += 100
    p[k:k + 100] = hi + (hi - lo)                                                     # far outside
    return p


def _sets(grid):
    mp = M_gridmp(grid)
    return {"nodes": grid, "centres": mp, "kz": [mp[0], grid[1], grid[2]], "kx": [grid[0], mp[1], grid[2]], "ky": [grid[0], grid[1], mp[2]]}


def M_gridmp(grid):
    out = []
    for c in grid:
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


def test_trac2grid_matches_model_all_staggerings_and_schemes():
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(0)
    grid = [np.linspace(0, 1.0e5, 41), np.linspace(0, 1.3e5, 33), np.linspace(0, 0.9e5, 49)]
    n = 1000000
    tr_x = _cloud(rng, grid, n, margin=0.9)
    vals = np.stack([rng.uniform(2900, 3300, n), 10 ** rng.uniform(18, 23, n)], 1)
    for name, tg in _sets(grid).items():
        sch = [5, 6, 1, 2] if name == "nodes" else [5, 6]
        f = vals[:, [0, 1, 0, 1][:len(sch)]]
        got = _t2g(P3, tr_x, f, tg, sch)
        ref = M.trac2grid(tr_x, f, tg, sch)
        for k, s in enumerate(sch):
            e = maxrel(got[k], ref[k])
            print("trac2grid %-8s scheme %d: %.3g  (NaN nodes %d)" % (name, s, e, np.isnan(ref[k]).sum()))
            assert e < (1e-12 if s & 1 else 1e-11), (name, s, e)


def test_grid2trac_and_rk4_match_model():
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(1)
    grid = [np.linspace(-2.0e3, 1.0e5, 24), np.linspace(1.0e3, 1.3e5, 32), np.linspace(0, 0.9e5, 18)]
    shp = [24, 32, 18]
    n = 1000000
    tr_x = _cloud(rng, grid, n, margin=0.3)
    F = [rng.standard_normal(shp) for _ in range(3)]
    for meth, name in ((16, "linear"), (8, "nearest"), (32, "veldiv")):
        got = _g2t(P3, tr_x, grid, F, defval=-7.0, method=meth)
        ref = M.grid2trac(tr_x, grid, F, defval=-7.0, method=meth)
        e = maxrel(got, ref)
        print("grid2trac %s: %.3g (outside: %d)" % (name, e, int((ref[:, 0] == -7.0).sum())))
        assert e < 1e-13, (name, e)
    # RK4: velocities that move a tracer by about a third of a cell per step
    h = min(c[1] - c[0] for c in grid)
    dt = 3.0e5
    V = [f * (h / 3 / dt) for f in F]
    v, x = P3.RK(tr_x, grid, V, [s - 1 for s in shp], dt)
    vr, xr = M.rk4(tr_x, grid, V, dt)
    print("rk4: x %.3g  v %.3g" % (maxrel(x, xr), maxrel(v, vr)))
    assert maxrel(x, xr) < 1e-14 and maxrel(v, vr) < 1e-9


@pytest.mark.parametrize("ax", [0, 1, 2])
def test_kernels_reduce_to_the_2d_oracle_under_extrusion(oracle, ax):
    """The cases of tests/test_mic3_model.py on the GPU: ties the kernels to the reference's own arithmetic."""
    from pylamp_amd import pylamp3d as P3
    rng, n, g, _ = _random_setup(2 + ax)
    keep = [d for d in range(3) if d != ax]
    n2 = [n[keep[0]], n[keep[1]]]; g2 = [g[keep[0]], g[keep[1]]]
    V2 = [rng.standard_normal(n2) for _ in range(2)]
    V3 = [None] * 3
    for q, d in enumerate(keep):
        V3[d] = np.repeat(np.expand_dims(V2[q], ax), n[ax], axis=ax)
    V3[ax] = np.zeros(n)
    p = np.stack([rng.uniform(g[d][0], g[d][-1], 2000) for d in range(3)], 1)
    o3 = _g2t(P3, p, g, V3, defval=0, method=32)
    o2 = oracle.grid2trac(p[:, keep], g2, V2, n2, defval=0, method=oracle.M_VELDIV)
    assert maxrel(o3[:, keep], o2) < 1e-13 and np.abs(o3[:, ax]).max() <= 1e-13 * np.abs(o2).max()
    for m3, m2 in ((16, oracle.M_LINEAR), (8, oracle.M_NEAREST)):
        assert maxrel(_g2t(P3, p, g, [V3[keep[0]], V3[keep[1]]], method=m3), oracle.grid2trac(p[:, keep], g2, V2, n2, method=m2)) < 1e-13
    dt = 0.02
    p = np.stack([rng.uniform(g[d][0] + 0.15 * (g[d][-1] - g[d][0]), g[d][-1] - 0.15 * (g[d][-1] - g[d][0]), 2000) for d in range(3)], 1)
    v3, x3 = P3.RK(p, g, V3, [s - 1 for s in n], dt)
    v2, x2 = oracle.rk4(p[:, keep], g2, V2, [n2[0] - 1, n2[1] - 1], dt)
    assert maxrel(x3[:, keep], x2) < 1e-14 and maxrel(v3[:, keep], v2) < 1e-9
    assert np.array_equal(x3[:, ax], p[:, ax]) and not v3[:, ax].any()
    # tracer -> grid on product tracer sets
    rng = np.random.default_rng(10 + ax)
    nx2 = [9, 11]; L2 = np.array([660e3, 820e3]); na = 6
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    gax = np.linspace(0, 300e3, na)
    p2, f2, p3, f3 = product_tracers(rng, g2, L2, gax, ax)
    g3 = list(g2); g3.insert(ax, gax)
    for sch in ([5, 6], [1, 2]):
        r2 = oracle.trac2grid(p2, f2, g2, nx2, sch)
        r3 = _t2g(P3, p3, f3, g3, sch)
        for k in range(2):
            for j in range(na):
                assert maxrel(np.take(r3[k], j, axis=ax), r2[k]) < (1e-12 if sch[k] & 1 else 1e-11), (sch[k], j)


def _resident_model(seed=3, n=200000):
    rng = np.random.default_rng(seed)
    nx = [21, 25, 17]; L = [1.0e5, 1.2e5, 0.8e5]
    tr_x = rng.random((n, 3)) * np.array(L) * 0.999998 + 1e-6 * np.array(L)
    tr_f = np.zeros((n, NF))
    tr_f[:, TR_ID] = np.arange(n)
    tr_f[:, 6] = rng.uniform(3200, 3400, n); tr_f[:, 7] = 3.5e-5; tr_f[:, 8] = rng.integers(1, 3, n); tr_f[:, 10] = 10 ** rng.uniform(19, 21, n)
    tr_f[:, TR_HCD] = rng.uniform(3, 5, n); tr_f[:, TR_HCP] = rng.uniform(1000, 1300, n); tr_f[:, 9] = 120e3; tr_f[:, 11] = 1e-11
    tr_f[:, TR_TMP] = 273 + 1350 * tr_x[:, 0] / L[0] + rng.uniform(-20, 20, n)
    return rng, nx, L, tr_x, tr_f


def test_scatter_is_bitwise_reproducible():
    from pylamp_amd import pylamp3d as P3
    rng, nx, L, tr_x, tr_f = _resident_model()
    grid = [np.linspace(0, L[d], nx[d]) for d in range(3)]
    tr_x[:3000, 1] = grid[1][rng.integers(1, nx[1] - 1, 3000)]              # exactly on cell faces
    M.property_update(tr_f, True, True)
    sub = tr_f[:, [0, 1]]
    a = _t2g(P3, tr_x, sub, grid, [5, 6]); b = _t2g(P3, tr_x, sub, grid, [5, 6])
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
    outs = []
    for rep in range(2):
        sim = P3.Simulation3(nx, L, tr_x, tr_f)
        outs.append(sim.scatter([0, 1], [5, 6]) + sim.scatter([1], [6], sim.gridmp))
        sim.close()
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
    # a different upload order changes the order inside the cells, hence the rounding -- but not beyond it
    perm = rng.permutation(tr_x.shape[0])
    c = _t2g(P3, tr_x[perm], sub[perm], grid, [5, 6])
    assert maxrel(c[0], a[0]) < 1e-12 and maxrel(c[1], a[1]) < 1e-11


def test_resident_stages_equal_module_functions():
    from pylamp_amd import pylamp3d as P3
    rng, nx, L, tr_x, tr_f = _resident_model(4)
    grid = [np.linspace(0, L[d], nx[d]) for d in range(3)]
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_subgrid_heatdiff=False))
    assert sim.count() == tr_x.shape[0] and sim.census().sum() == tr_x.shape[0]
    cells = [M.cell(grid[d], tr_x[:, d]) for d in range(3)]
    cref = np.zeros([v - 1 for v in nx], dtype=np.int64); np.add.at(cref, tuple(cells), 1)
    assert np.array_equal(sim.census(), cref)
    # properties + the field list of a step
    f = sim.scatter_fields()
    ref_f = tr_f.copy(); M.property_update(ref_f, True, True)
    sx, sf = sim.tracers()
    o = np.argsort(sf[:, TR_ID])
    assert np.array_equal(sf[o, TR_ID], tr_f[:, TR_ID]) and np.array_equal(sx[o], tr_x)
    assert maxrel(sf[o, 0], ref_f[:, 0]) < 1e-14 and maxrel(sf[o, 1], ref_f[:, 1]) < 1e-13
    mp = sim.gridmp
    node = _t2g(P3, sx, sf[:, [0, 1, 5, 3, 11, 8]], grid, [5, 6, 5, 5, 5, 5])
    for k, name in enumerate(["rho", "etas", "cp", "T", "H", "mat"]):
        assert np.array_equal(f[name], node[k], equal_nan=True), name       # same kernel, same tracer order: bitwise
    assert maxrel(f["etan"], _t2g(P3, sx, sf[:, [1]], mp, [6])[0]) < 1e-11      # module path: sorted by the centre set's own cells
    for name, tg in (("kz", [mp[0], grid[1], grid[2]]), ("kx", [grid[0], mp[1], grid[2]]), ("ky", [grid[0], grid[1], mp[2]])):
        got = f[name]; ref = _t2g(P3, sx, sf[:, [4]], tg, [5])[0]
        assert maxrel(got, ref) < 1e-12, name          # the module path sorts by the target set's own cells: another order of summation
        assert maxrel(got, M.trac2grid(tr_x, tr_f[:, [4]], tg, [5])[0]) < 1e-12, name
    # temperature: absolute, then increment
    Tn = 1000 + 100 * rng.standard_normal(nx)
    sim.temp_to_tracers(Tn, True)
    _, sf2 = sim.tracers()
    assert maxrel(sf2[:, 3], _g2t(P3, sx, grid, [Tn])[:, 0]) == 0.0
    dT = rng.standard_normal(nx)
    sim.temp_to_tracers(dT, False, 1e12)
    _, sf3 = sim.tracers()
    assert maxrel(sf3[:, 3], sf2[:, 3] + _g2t(P3, sx, grid, [dT])[:, 0]) < 1e-15
    # advection + fence + re-sort
    h = min(L[d] / (nx[d] - 1) for d in range(3)); dt = 1e12
    vel = [rng.standard_normal(nx) * (0.4 * h / dt) for _ in range(3)]
    grids, V = P3.advection_velocity(vel, mp, nx)
    sim.advect(grids, V, dt)
    vr, xr = P3.RK(sx, grids, V, nx, dt)
    xr = M.fence(xr, L)
    ax_, af = sim.tracers(); av = sim.tracer_velocity()
    o2 = np.argsort(af[:, TR_ID]); o1 = np.argsort(sf[:, TR_ID])
    assert np.array_equal(ax_[o2], xr[o1]) and np.array_equal(av[o2], vr[o1])
    assert np.array_equal(af[o2], sf3[o1])
    assert (ax_ > 0).all() and (ax_ < np.array(L)).all() and sim.census().sum() == tr_x.shape[0]
    key = lambda x: (M.cell(grid[0], x[:, 0]) * (nx[1] - 1) + M.cell(grid[1], x[:, 1])) * (nx[2] - 1) + M.cell(grid[2], x[:, 2])
    assert (np.diff(key(ax_)) >= 0).all()            # sorted by cell again
    sim.close()


def test_subgrid_diffusion_stage_matches_model():
    """Stage level, no solve: the resident temperature-to-tracers stage with subgrid diffusion against the NumPy composition."""
    from pylamp_amd import pylamp3d as P3
    rng, nx, L, tr_x, tr_f = _resident_model(5)
    grid = [np.linspace(0, L[d], nx[d]) for d in range(3)]
    M.property_update(tr_f, True, True)
    sim = P3.Simulation3(nx, L, tr_x, tr_f)
    dT = 5 * rng.standard_normal(nx)
    h2 = sum((2 / (L[d] / (nx[d] - 1))) ** 2 for d in range(3))
    tstep = 1.0 * np.median(tr_f[:, TR_HCP] * tr_f[:, TR_RHO] / (tr_f[:, TR_HCD] * h2))        # of the order of the subgrid time scale
    sim.temp_to_tracers(dT, False, tstep)
    sx, sf = sim.tracers()
    o = np.argsort(sf[:, TR_ID])
    ref = M.temp_to_tracers(tr_x, tr_f, grid, dT, False, True, tstep)
    plain = M.temp_to_tracers(tr_x, tr_f, grid, dT, False, False, tstep)
    e = maxrel(sf[o, 3], ref)
    print("subgrid stage: %.3g (effect of the correction: %.3g)" % (e, maxrel(plain, ref)))
    assert e < 1e-12 and maxrel(plain, ref) > 1e-6
    sim.close()


def test_marker_calls_fail_on_a_context_with_several_ranks():
    from pylamp_amd import pylamp3d as P3, _lib
    import ctypes as C
    grid = [np.linspace(0, 1, 9)] * 3
    vc = P3.VirtualCluster3([9, 9, 9], grid, 2, 1, 1)
    try:
        ctx = vc.ctxs[0]
        n = C.c_int64()
        assert ctx.lib.pl3_tracers_count(ctx.handle(), C.byref(n)) != 0
        assert b"one rank" in ctx.lib.pl3_last_error(ctx.handle())
        x = np.full((4, 3), 0.5); f = np.ones((4, NF))
        assert ctx.lib.pl3_tracers_upload(ctx.handle(), 4, _lib.dptr(x), _lib.dptr(f)) != 0
        assert b"pl3_tracers_upload" in ctx.lib.pl3_last_error(ctx.handle())
        with pytest.raises(Exception, match="one rank"):
            P3.RK(x, [np.linspace(0, 1, 10)] * 3, [np.zeros((10, 10, 10))] * 3, [9, 9, 9], 1.0, ctx=ctx)
    finally:
        vc.close()


def test_simulation3_step_matches_2d_oracle_on_y_invariant_mantle(oracle):
    """One step of Simulation3 on driver.mantle_tracers (33 x 41) replicated along y (ny = 9, two copies per cell layer) against
    oracle.step on every y-slice, with the bounds smoke() uses for the same comparison in 2-D: temperature 1e-6, tracer (z, x)
    1e-7 (relative L2), and |v_y| <= 1e-6 of the in-plane maximum.  dy = 21 km >= min(dz, dx) = 20.5 km, so both time-step
    rules pick the 2-D spacing; subgrid diffusion off (its 3-D time scale has a third term).
    Measured on an MI355X: temperature 6.4e-13, tracer (z, x) 2.7e-12, tracer velocities 2.2e-9, |v_y| 7e-10 of the in-plane maximum
    (the heat time step limits this model, so the 3e-8 stopping estimate of the Stokes solve enters the positions only)."""
    from pylamp_amd import pylamp3d as P3, driver
    nx2 = [33, 41]; L2 = [660e3, 820e3]; ny = 9; Ly = 21e3 * (ny - 1)
    x2, f2 = driver.mantle_tracers(nx2, L2, 8, np.random.default_rng(1))
    n2 = x2.shape[0]
    m = 2 * (ny - 1)
    ys = (np.arange(m) + np.random.default_rng(2).uniform(0.1, 0.9, m)) * Ly / m
    x3 = np.concatenate([np.insert(x2, 2, y, axis=1) for y in ys])
    f3 = np.tile(f2, (m, 1)); f3[:, TR_ID] = np.arange(m * n2)
    sim = P3.Simulation3(nx2 + [ny], L2 + [Ly], x3, f3, P3.Options3(do_subgrid_heatdiff=False))
    rep = sim.step()
    st = dict(nx=nx2, L=L2, grid=[np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])], tr_x=x2.copy(), tr_f=f2.copy())
    out = oracle.step(st, oracle.StepConfig(do_subgrid_heatdiff=False), 1)
    assert rep["stokes"]["converged"] == 1 and rep["heat"]["converged"] == 1, rep
    print("tstep 3-D %.9e  2-D %.9e  limiter %s / %s" % (rep["tstep"], out["tstep"], rep["limiter"], out["limiter"]))
    T = sim.field("temp")
    et = max(relerr(T[:, :, k], out["temp"]) for k in range(ny))
    sx, sf = sim.tracers()
    o = np.argsort(sf[:, TR_ID])
    sx = sx[o].reshape(m, n2, 3); sT = sf[o, TR_TMP].reshape(m, n2)
    ex = max(relerr(sx[c][:, :2], st["tr_x"]) for c in range(m))
    eT = max(relerr(sT[c], st["tr_f"][:, TR_TMP]) for c in range(m))
    vmax = max(np.abs(out["velz"]).max(), np.abs(out["velx"]).max())
    vy = np.abs(sim.field("vely")).max() / vmax
    tv = sim.tracer_velocity()[o].reshape(m, n2, 3)
    ev = max(relerr(tv[c][:, :2], out["tr_v"]) for c in range(m))
    print("temp %.3g  tracer (z,x) %.3g  tracer T %.3g  tracer v %.3g  |vy|/|v| %.3g  tracer |vy| %.3g" % (et, ex, eT, ev, vy, np.abs(tv[:, :, 2]).max() / vmax))
    assert et < 1e-6 and ex < 1e-7
    assert vy <= 1e-6 and np.abs(tv[:, :, 2]).max() <= 1e-6 * vmax
    assert np.abs(sx[:, :, 2] - ys[:, None]).max() <= 1e-6 * vmax * rep["tstep"]
    sim.close()


def test_falling_sphere_runs():
    """Does-it-run test, no number pinned: a dense, stiff sphere in a free-slip box, 33^3 nodes, 2 x 2 x 2 jittered tracers per
    cell, 5 steps.  Every solve converges, no tracer is lost or leaves the box, the sphere sinks (gravity is +z) at every step,
    the census sums to the tracer count and no scattered field holds a NaN."""
    from pylamp_amd import pylamp3d as P3
    nx = [33, 33, 33]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))
    n = tr_x.shape[0]
    assert n == 8 * 32 ** 3
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False))
    assert sim.census().min() >= 1
    zs = [tr_x[tr_f[:, 8] == 2, 0].mean()]
    for it in range(5):
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        for name in ("rho", "etas", "etan"):
            assert not np.isnan(sim.field(name)).any(), name
        x, f = sim.tracers()
        assert x.shape[0] == n and sim.census().sum() == n
        assert (x > 0).all() and (x < np.array(L)).all()
        zs.append(x[f[:, 8] == 2, 0].mean())
        print("step %d: tstep %.3e  its %d  sphere z %.6e" % (rep["it"], rep["tstep"], rep["stokes"]["iterations"], zs[-1]))
        assert zs[-1] > zs[-2]
    assert np.array_equal(np.sort(f[:, TR_ID]), np.arange(n))
    sim.close()
