"""3-D markers on rectilinear grids (the per-axis cell search, pl3_mic_set_search / Options3.marker_search) on the GPU, against the
NumPy model tests/mic3_rect_model.py, which tests/test_mic3_rect_model.py ties to the 2-D oracle under oracle.rect_search().

Tolerances are those tests/test_hip_mic3.py, tests/test_hip_mic3_refill.py and tests/test_hip_step3_resident.py use for the same
comparisons on uniform grids; the shapes are the smallest that still have several workgroups, odd sizes, graded, jumping and
shifted axes, and (the thin-cell case) a spacing ratio beyond the bucket table's cap."""
import numpy as np
import pytest

from conftest import maxrel, relerr
import mic3_model as U
import mic3_rect_model as M
import mic3_refill_model as R

pytestmark = pytest.mark.gpu

NF = 13
TR_RHO, TR_ETA, TR_TMP, TR_HCD, TR_HCP, TR_MAT, TR_ID = 0, 1, 3, 4, 5, 8, 12


def _jump(n, L, ratio, origin=0.0):
    """Two zones of equal cell count; the spacing jumps by `ratio` between them."""
    h = np.where(np.arange(n - 1) < (n - 1) // 2, 1.0, float(ratio))
    c = origin + np.concatenate([[0.0], np.cumsum(h)]) * (L / h.sum())
    c[-1] = origin + L
    return c


def _grid(n, L):
    """One axis graded smoothly 5:1, one with an abrupt 4:1 jump, one (mildly graded) with a non-zero origin."""
    return [M.graded(n[0], L[0], 5.0), _jump(n[1], L[1], 4.0), M.graded(n[2], L[2], 0.5, origin=-2.0e3)]


def _mp(grid):
    out = []
    for c in grid:
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


def _sets(grid):
    mp = _mp(grid)
    return {"nodes": grid, "centres": mp, "kz": [mp[0], grid[1], grid[2]], "kx": [grid[0], mp[1], grid[2]], "ky": [grid[0], grid[1], mp[2]]}


def _cloud(rng, grid, n, margin=0.9):
    """As tests/test_hip_mic3.py: random positions up to `margin` end spacings beyond the node set, tracers exactly on cell faces,
    on the first / last coordinate of every axis, and far outside."""
    lo = np.array([c[0] - margin * (c[1] - c[0]) for c in grid]); hi = np.array([c[-1] + margin * (c[-1] - c[-2]) for c in grid])
    p = lo + rng.random((n, 3)) * (hi - lo)
    k = 0
    for d in range(3):
        m = 2000
        p[k:k + m, d] = grid[d][rng.integers(0, len(grid[d]), m)]; k += m
        p[k:k + 50, d] = grid[d][0]; p[k + 50:k + 100, d] = grid[d][-1]; k += 100
    p[k:k + 100] = hi + (hi - lo)
    p[k + 100:k + 150] = lo - (hi - lo)
    return p


def _t2g(P3, tr_x, tr_f, grid, sch, search=True):
    shp = [len(c) for c in grid]
    out = [np.zeros(shp) for _ in sch]
    P3.trac2grid(tr_x, tr_f, None, grid, out, shp, avgscheme=list(sch), search=search)
    return out


def _g2t(P3, tr_x, grid, fields, defval=np.nan, method=16, search=True):
    out = np.zeros((tr_x.shape[0], len(fields)))
    P3.grid2trac(tr_x, out, grid, fields, [len(c) for c in grid], defval=defval, method=method, search=search)
    return out


def _check_scatter(P3, tr_x, vals, grid, sets=("nodes", "centres", "kz", "kx", "ky")):
    for name, tg in _sets(grid).items():
        if name not in sets:
            continue
        sch = [5, 6, 1, 2] if name == "nodes" else [5, 6]
        f = vals[:, [0, 1, 0, 1][:len(sch)]]
        got = _t2g(P3, tr_x, f, tg, sch)
        again = _t2g(P3, tr_x, f, tg, sch)
        ref = M.trac2grid(tr_x, f, tg, sch)
        for k, s in enumerate(sch):
            e = maxrel(got[k], ref[k])
            print("trac2grid %-8s scheme %d: %.3g  (NaN nodes %d)" % (name, s, e, np.isnan(ref[k]).sum()))
            assert e < (1e-12 if s & 1 else 1e-11), (name, s, e)
            assert np.array_equal(got[k], again[k], equal_nan=True), (name, s)


def test_scatter_matches_model_on_a_rectilinear_grid():
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(0)
    grid = _grid([21, 17, 25], [1.0e5, 1.3e5, 0.9e5])
    n = 200000
    tr_x = _cloud(rng, grid, n)
    vals = np.stack([rng.uniform(2900, 3300, n), 10 ** rng.uniform(18, 23, n)], 1)
    _check_scatter(P3, tr_x, vals, grid)
    assert not P3._mic_ctx(None).marker_search()            # the shared carrier context is left as it was


def test_gather_and_rk4_match_model_on_a_rectilinear_grid():
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(1)
    shp = [24, 32, 18]
    grid = _grid(shp, [1.0e5, 1.3e5, 0.9e5])
    n = 200000
    tr_x = _cloud(rng, grid, n, margin=0.3)
    F = [rng.standard_normal(shp) for _ in range(3)]
    for meth, name in ((16, "linear"), (8, "nearest"), (32, "veldiv")):
        got = _g2t(P3, tr_x, grid, F, defval=-7.0, method=meth)
        ref = M.grid2trac(tr_x, grid, F, defval=-7.0, method=meth)
        e = maxrel(got, ref)
        nout = int((ref[:, 0] == -7.0).sum())
        print("grid2trac %s: %.3g (outside: %d)" % (name, e, nout))
        assert e < 1e-13, (name, e)
        assert int((got[:, 0] == -7.0).sum()) == nout > 1000
    # RK4: velocities that move a tracer by about a third of the SMALLEST cell per step
    h = min(np.diff(c).min() for c in grid)
    dt = 3.0e5
    V = [f * (h / 3 / dt) for f in F]
    v, x = P3.RK(tr_x, grid, V, [s - 1 for s in shp], dt, search=True)
    vr, xr = M.rk4(tr_x, grid, V, dt)
    print("rk4: x %.3g  v %.3g" % (maxrel(x, xr), maxrel(v, vr)))
    assert maxrel(x, xr) < 1e-14 and maxrel(v, vr) < 1e-9


def _thin(n, L, at):
    """n coordinates from 0 to L; cell `at` is 1e-5 L wide, the others share the rest equally."""
    h = np.full(n - 1, (1.0 - 1e-5) / (n - 2)); h[at] = 1e-5
    c = np.concatenate([[0.0], np.cumsum(h)]) * L
    c[-1] = L
    return c


def test_a_very_thin_cell():
    """L / min(h) = 1e5 is beyond any bucket count: several cells share a bucket and the walk from the bucket's entry is what finds
    the cell."""
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(2)
    nx = [9, 9, 9]; L = [1.0e5, 1.3e5, 0.9e5]
    grid = [_thin(9, L[0], 3), _thin(9, L[1], 0), _thin(9, L[2], 7)]
    n = 40000
    tr_x = _cloud(rng, grid, n, margin=0.9)
    for d, at in enumerate((3, 0, 7)):            # many tracers inside, and on the faces of, the thin cells
        k = 10000 + 3000 * d
        tr_x[k:k + 3000, d] = grid[d][at] + rng.random(3000) * (grid[d][at + 1] - grid[d][at])
    vals = np.stack([rng.uniform(2900, 3300, n), 10 ** rng.uniform(18, 23, n)], 1)
    _check_scatter(P3, tr_x, vals, grid, sets=("nodes", "centres"))
    F = [rng.standard_normal(nx) for _ in range(3)]
    for meth in (16, 8, 32):
        ref = M.grid2trac(tr_x, grid, F, defval=-7.0, method=meth)
        assert maxrel(_g2t(P3, tr_x, grid, F, defval=-7.0, method=meth), ref) < 1e-13, meth
    tr_f = np.ones((n, NF)); tr_f[:, TR_ID] = np.arange(n)
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(marker_search=True), grid=grid)
    cell, _ = M.cells_of(tr_x, grid)
    cen = np.bincount(cell, minlength=8 ** 3).reshape(8, 8, 8)
    assert np.array_equal(sim.census(), cen) and cen[3, :, :].sum() > 2000
    sim.close()


def test_search_agrees_with_the_formula_on_a_uniform_grid():
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(3)
    shp = [21, 17, 25]
    grid = [np.linspace(0, 1.0e5, 21), np.linspace(1.0e3, 1.3e5, 17), np.linspace(-2.0e3, 0.9e5, 25)]
    n = 200000
    lo = np.array([c[0] - 0.9 * (c[1] - c[0]) for c in grid]); hi = np.array([c[-1] + 0.9 * (c[-1] - c[-2]) for c in grid])
    tr_x = lo + rng.random((n, 3)) * (hi - lo)
    vals = np.stack([rng.uniform(2900, 3300, n), 10 ** rng.uniform(18, 23, n)], 1)
    for name, tg in _sets(grid).items():
        a = _t2g(P3, tr_x, vals, tg, [5, 6], search=True); b = _t2g(P3, tr_x, vals, tg, [5, 6], search=False)
        for k in range(2):
            e = maxrel(a[k], b[k])
            print("uniform %-8s scheme %d: search vs formula %.3g" % (name, 5 + k, e))
            assert e < 1e-12, (name, k, e)
    F = [rng.standard_normal(shp) for _ in range(3)]
    for meth in (16, 32):
        a = _g2t(P3, tr_x, grid, F, defval=-7.0, method=meth, search=True); b = _g2t(P3, tr_x, grid, F, defval=-7.0, method=meth, search=False)
        assert maxrel(a, b) < 1e-12, meth


def _resident_model(seed, nx, L, per_cell=10):
    rng = np.random.default_rng(seed)
    n = per_cell * (nx[0] - 1) * (nx[1] - 1) * (nx[2] - 1)
    tr_x = rng.random((n, 3)) * np.array(L) * 0.999998 + 1e-6 * np.array(L)
    tr_f = np.zeros((n, NF))
    tr_f[:, TR_ID] = np.arange(n)
    tr_f[:, 6] = rng.uniform(3200, 3400, n); tr_f[:, 7] = 3.5e-5; tr_f[:, 8] = rng.integers(1, 3, n); tr_f[:, 10] = 10 ** rng.uniform(19, 21, n)
    tr_f[:, TR_HCD] = rng.uniform(3, 5, n); tr_f[:, TR_HCP] = rng.uniform(1000, 1300, n); tr_f[:, 9] = 120e3; tr_f[:, 11] = 1e-11
    tr_f[:, TR_TMP] = 273 + 1350 * tr_x[:, 0] / L[0] + rng.uniform(-20, 20, n)
    return rng, tr_x, tr_f


def _key(cells_of, x, grid):
    return cells_of(x, grid)[0]


def test_resident_stages_on_a_graded_grid():
    from pylamp_amd import pylamp3d as P3
    nx = [17, 13, 21]; L = [1.0e5, 1.2e5, 0.8e5]
    grid = [M.graded(nx[0], L[0], 5.0), _jump(nx[1], L[1], 4.0), M.refined(nx[2], L[2], 3.0)]
    rng, tr_x, tr_f = _resident_model(4, nx, L)
    n = tr_x.shape[0]
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_subgrid_heatdiff=False, marker_search=True), grid=grid)
    assert all(np.array_equal(a, b) for a, b in zip(sim.grid, grid)) and sim.ctx.marker_search()
    cell, _ = M.cells_of(tr_x, grid)
    cref = np.bincount(cell, minlength=16 * 12 * 20).reshape(16, 12, 20)
    assert sim.count() == n and np.array_equal(sim.census(), cref)
    f = sim.scatter_fields()
    sx, sf = sim.tracers()
    o = np.argsort(sf[:, TR_ID])
    assert np.array_equal(sx[o], tr_x) and (np.diff(_key(M.cells_of, sx, grid)) >= 0).all()
    mp = sim.gridmp
    node = _t2g(P3, sx, sf[:, [0, 1, 5, 3, 11, 8]], grid, [5, 6, 5, 5, 5, 5])
    for k, name in enumerate(["rho", "etas", "cp", "T", "H", "mat"]):
        assert np.array_equal(f[name], node[k], equal_nan=True), name       # same kernel, same tracer order: bitwise
    assert maxrel(f["etan"], _t2g(P3, sx, sf[:, [1]], mp, [6])[0]) < 1e-11
    for name, tg in (("kz", [mp[0], grid[1], grid[2]]), ("kx", [grid[0], mp[1], grid[2]]), ("ky", [grid[0], grid[1], mp[2]])):
        assert maxrel(f[name], _t2g(P3, sx, sf[:, [4]], tg, [5])[0]) < 1e-12, name
        assert maxrel(f[name], M.trac2grid(sx, sf[:, [4]], tg, [5])[0]) < 1e-12, name
    # temperature: absolute, then increment (bitwise the module function), then with subgrid diffusion against the model
    Tn = 1000 + 100 * rng.standard_normal(nx)
    sim.temp_to_tracers(Tn, True)
    _, sf2 = sim.tracers()
    assert np.array_equal(sf2[:, 3], _g2t(P3, sx, grid, [Tn])[:, 0])
    dT = 5 * rng.standard_normal(nx)
    sim.opt.do_subgrid_heatdiff = True
    h2 = sum((2 / (L[d] / (nx[d] - 1))) ** 2 for d in range(3))
    tstep = 1.0 * np.median(sf2[:, TR_HCP] * sf2[:, TR_RHO] / (sf2[:, TR_HCD] * h2))
    sim.temp_to_tracers(dT, False, tstep)
    _, sf3 = sim.tracers()
    ref = M.temp_to_tracers(sx, sf2, grid, dT, False, True, tstep)
    plain = M.temp_to_tracers(sx, sf2, grid, dT, False, False, tstep)
    e = maxrel(sf3[:, 3], ref)
    print("subgrid stage on the graded grid: %.3g (effect of the correction: %.3g)" % (e, maxrel(plain, ref)))
    assert e < 1e-12 and maxrel(plain, ref) > 1e-6
    # advection + fence + re-sort
    h = min(np.diff(c).min() for c in grid); dt = 1e12
    vel = [rng.standard_normal(nx) * (0.4 * h / dt) for _ in range(3)]
    grids, V = P3.advection_velocity(vel, mp, nx)
    sim.advect(grids, V, dt)
    vr, xr = P3.RK(sx, grids, V, nx, dt, search=True)
    xr = U.fence(xr, L)
    ax_, af = sim.tracers(); av = sim.tracer_velocity()
    o2 = np.argsort(af[:, TR_ID]); o1 = np.argsort(sf[:, TR_ID])
    assert np.array_equal(ax_[o2], xr[o1]) and np.array_equal(av[o2], vr[o1]) and np.array_equal(af[o2], sf3[o1])
    assert (np.diff(_key(M.cells_of, ax_, grid)) >= 0).all() and sim.census().sum() == n
    # the switch with tracers resident: the same tracers, sorted by the other rule
    sim.ctx.set_marker_search(False)
    bx, bf = sim.tracers()
    o3 = np.argsort(bf[:, TR_ID])
    assert np.array_equal(bx[o3], ax_[o2]) and np.array_equal(bf[o3], af[o2])
    assert (np.diff(_key(R.cells_of, bx, grid)) >= 0).all() and not (np.diff(_key(M.cells_of, bx, grid)) >= 0).all()
    sim.ctx.set_marker_search(True)
    cx, cf = sim.tracers()
    o4 = np.argsort(cf[:, TR_ID])
    assert np.array_equal(cx[o4], ax_[o2]) and np.array_equal(cf[o4], af[o2]) and (np.diff(_key(M.cells_of, cx, grid)) >= 0).all()
    sim.close()


def test_refill_on_a_graded_grid():
    from pylamp_amd import pylamp3d as P3
    nx = [13, 11, 9]; L = [1.0e5, 1.2e5, 0.8e5]
    grid = [M.graded(nx[0], L[0], 4.0), _jump(nx[1], L[1], 3.0), M.refined(nx[2], L[2], 2.0)]
    rng = np.random.default_rng(21)
    n = 30000
    x = rng.random((n, 3)) * np.array(L) * 0.999998 + 1e-6 * np.array(L)
    keep = np.ones(n, dtype=bool)
    corner = (x[:, 0] < 0.35 * L[0]) & (x[:, 1] < 0.4 * L[1])
    keep &= ~corner | (rng.random(n) < 0.1)
    slab = (x[:, 2] > 0.7 * L[2]) & (x[:, 2] < 0.8 * L[2])
    keep &= ~slab | (rng.random(n) < 0.2)
    _, idx = M.cells_of(x, grid)
    for c in ((3, 4, 5), (10, 2, 7), (11, 9, 0)):
        keep &= ~((idx[0] == c[0]) & (idx[1] == c[1]) & (idx[2] == c[2]))
    tr_x = x[keep]
    tr_f = rng.uniform(1.0, 2.0, (tr_x.shape[0], NF)) * 10.0 ** rng.integers(0, 20, NF)
    tr_f[:, TR_ID] = rng.permutation(tr_x.shape[0]) + 100.0
    dens, dmin, seed, it = 8, 4, 4242, 3
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(tracdens=dens, tracdens_min=dmin, inject_seed=seed, marker_search=True), grid=grid)
    got = sim.refill(it=it)
    xg, fg = sim.tracers(); vg = sim.tracer_velocity(); cen = sim.census()
    rx, rf, rv, info = M.refill(tr_x, tr_f, grid, dens, dmin, seed, it)
    print("refill: %d tracers + %d injected into %d cells (%d empty), smallest count %d" %
          (tr_x.shape[0], got["ninjected"], got["nrefilled"], got["nempty"], got["mincount"]))
    assert info["nempty"] >= 3 and info["nrefilled"] > 50 and info["mincount"] == 0
    assert got == dict(ninjected=info["ninjected"], nrefilled=info["nrefilled"], nempty=info["nempty"], mincount=info["mincount"])
    assert xg.shape[0] == rx.shape[0] == sim.count() == tr_x.shape[0] + info["ninjected"]
    assert np.array_equal(cen, info["census"]) and cen.min() >= dmin
    new = info["new"]
    assert np.array_equal(xg[~new], rx[~new]) and np.array_equal(fg, rf, equal_nan=True) and np.array_equal(vg, rv)
    ex = [float(np.abs(xg[new, d] - rx[new, d]).max()) / L[d] for d in range(3)]
    print("new positions: max |dx| / L = %.3g %.3g %.3g" % tuple(ex))
    assert max(ex) <= 4 * 2.0 ** -52
    assert np.array_equal(M.cells_of(xg[new], grid)[0], info["cell"][new])           # every new tracer inside its own cell
    for d in range(3):
        i = info["cell"][new] // [(nx[1] - 1) * (nx[2] - 1), nx[2] - 1, 1][d] % (nx[d] - 1)
        assert (xg[new, d] >= grid[d][i]).all() and (xg[new, d] < grid[d][i + 1]).all()
    sim.close()


@pytest.fixture(scope="module")
def mantle_step(oracle):
    """One step on the y-invariant mantle model on a graded grid: 2-D oracle, host-staged 3-D and resident 3-D."""
    from pylamp_amd import pylamp3d as P3, driver
    nx2 = [25, 33]; L2 = [660e3, 820e3]; ny = 7; Ly = 26e3 * (ny - 1)
    g2 = [M.refined(nx2[0], L2[0], 2.0), M.graded(nx2[1], L2[1], 2.0)]
    gy = M.graded(ny, Ly, 1.5)
    x2, f2 = driver.mantle_tracers(nx2, L2, 16, np.random.default_rng(1))
    n2 = x2.shape[0]
    assert n2 == 13200
    u = np.random.default_rng(2).uniform(0.1, 0.9, (ny - 1, 2))
    ys = np.concatenate([gy[i] + u[i] * (gy[i + 1] - gy[i]) for i in range(ny - 1)])
    m = ys.size
    x3 = np.concatenate([np.insert(x2, 2, y, axis=1) for y in ys])
    f3 = np.tile(f2, (m, 1)); f3[:, TR_ID] = np.arange(m * n2)
    st = dict(nx=nx2, L=L2, grid=[g2[0].copy(), g2[1].copy()], tr_x=x2.copy(), tr_f=f2.copy())
    with oracle.rect_search():
        out = oracle.step(st, oracle.StepConfig(do_subgrid_heatdiff=False), 1)
    runs = []
    for resident in (False, True):
        sim = P3.Simulation3(nx2 + [ny], L2 + [Ly], x3, f3, P3.Options3(do_subgrid_heatdiff=False, marker_search=True, resident=resident),
                             grid=g2 + [gy])
        rep = sim.step()
        x, f = sim.tracers()
        runs.append(dict(rep=rep, x=x, f=f, v=sim.tracer_velocity(), census=sim.census(),
                         fields={k: sim.field(k).copy() for k in ("rho", "etas", "etan", "T", "kz", "kx", "ky", "velz", "velx", "vely", "pres", "temp")}))
        sim.close()
    return dict(st=st, out=out, runs=runs, ys=ys, n2=n2, ny=ny)


@pytest.mark.parametrize("resident", [False, True])
def test_step_matches_2d_oracle_on_a_graded_y_invariant_mantle(mantle_step, resident):
    ms = mantle_step
    st, out, run, ys, n2, ny = ms["st"], ms["out"], ms["runs"][1 if resident else 0], ms["ys"], ms["n2"], ms["ny"]
    rep = run["rep"]; m = ys.size
    assert rep["stokes"]["converged"] == 1 and rep["heat"]["converged"] == 1, rep
    print("tstep 3-D %.9e  2-D %.9e  limiter %s / %s" % (rep["tstep"], out["tstep"], rep["limiter"], out["limiter"]))
    T = run["fields"]["temp"]
    et = max(relerr(T[:, :, k], out["temp"]) for k in range(ny))
    o = np.argsort(run["f"][:, TR_ID])
    sx = run["x"][o].reshape(m, n2, 3)
    ex = max(relerr(sx[c][:, :2], st["tr_x"]) for c in range(m))
    vmax = max(np.abs(out["velz"]).max(), np.abs(out["velx"]).max())
    vy = np.abs(run["fields"]["vely"]).max() / vmax
    tv = run["v"][o].reshape(m, n2, 3)
    print("temp %.3g  tracer (z,x) %.3g  |vy|/|v| %.3g  tracer |vy| %.3g" % (et, ex, vy, np.abs(tv[:, :, 2]).max() / vmax))
    assert et < 1e-6 and ex < 1e-7
    assert vy <= 1e-6 and np.abs(tv[:, :, 2]).max() <= 1e-6 * vmax


def test_staged_and_resident_steps_agree_bitwise_on_a_graded_grid(mantle_step):
    s, r = mantle_step["runs"]
    assert s["rep"]["tstep"] == r["rep"]["tstep"] and s["rep"]["limiter"] == r["rep"]["limiter"]
    for q in ("iterations", "rel_residual"):
        assert s["rep"]["stokes"][q] == r["rep"]["stokes"][q] and s["rep"]["heat"][q] == r["rep"]["heat"][q]
    for k in s["fields"]:
        assert np.array_equal(s["fields"][k], r["fields"][k], equal_nan=True), k
    for k in ("x", "f", "v", "census"):
        assert np.array_equal(s[k], r[k], equal_nan=True), k


def test_falling_sphere_runs_on_a_refined_grid():
    """Does-it-run test, no number pinned: the falling sphere at 33^3 on a grid refined 3:1 around the sphere's path, 4 x 4 x 4
    jittered tracers per mean cell (8 in the finest cells), tracdens = 8 / tracdens_min = 4, 3 steps."""
    from pylamp_amd import pylamp3d as P3
    nx = [33, 33, 33]; L = [100e3, 100e3, 100e3]
    grid = [P3.refined_grid(33, L[0], 0.45, 3.0, 0.35), P3.refined_grid(33, L[1], 0.5, 3.0, 0.2), P3.refined_grid(33, L[2], 0.5, 3.0, 0.2)]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7), per_axis=4)
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, tracdens=8, tracdens_min=4,
                                                        marker_search=True), grid=grid)
    assert sim.census().min() >= 1
    zs = [tr_x[tr_f[:, TR_MAT] == 2, 0].mean()]
    for it in range(3):
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        for name in ("rho", "etas", "etan"):
            assert not np.isnan(sim.field(name)).any(), name
        x, f = sim.tracers()
        assert x.shape[0] == rep["ntrac"] and sim.census().sum() == x.shape[0]
        assert (x > 0).all() and (x < np.array(L)).all()
        zs.append(x[f[:, TR_MAT] == 2, 0].mean())
        print("step %d: tstep %.3e  its %d  injected %d  sphere z %.6e" % (rep["it"], rep["tstep"], rep["stokes"]["iterations"], rep["ninjected"], zs[-1]))
        assert zs[-1] > zs[-2]
    sim.close()
