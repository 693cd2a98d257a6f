"""3-D census + refill on the GPU (pl3_resident_refill / pl3_resident_advect, Simulation3.refill / advect / step) against the
NumPy model tests/mic3_refill_model.py, which tests/test_mic3_refill_model.py ties to the 2-D oracle.

Bounds.  Counts, counters, census, order, IDs, NaN pattern and everything about the old tracers: exact.  New positions:
4 * 2^-52 * L_d (g + u h may be contracted into one FMA: one rounding of a value below L_d instead of two; 4 is slack over that
one ulp).  New fields: 2 tracdens 2^-52 relative (fewer than tracdens same-sign summands, whatever fixed order the kernel sums
in).  The stages on the grown state use the bounds tests/test_hip_mic3.py uses for the same stages."""
import ctypes as C

import numpy as np
import pytest

from conftest import maxrel
import mic3_model as M
import mic3_refill_model as R

pytestmark = pytest.mark.gpu

NF, TR_ID, TR_MAT = 13, 12, 8
NX = [21, 25, 17]; LL = [1.0e5, 1.2e5, 0.8e5]


def _grid(nx=NX, L=LL):
    return [np.linspace(0, L[d], nx[d]) for d in range(3)]


def _cloud(seed, n=80000, empty=((3, 4, 5), (10, 2, 9), (19, 23, 15))):
    """Random cloud over the anisotropic box, thinned to a quarter in one corner region and to a half in a slab, the cells in
    `empty` emptied; positive values in every column, IDs a permutation starting at 100."""
    rng = np.random.default_rng(seed)
    L = np.array(LL)
    x = rng.random((n, 3)) * L * 0.999998 + 1e-6 * L
    keep = np.ones(n, dtype=bool)
    corner = (x[:, 0] < 0.35 * L[0]) & (x[:, 1] < 0.4 * L[1])
    keep &= ~corner | (rng.random(n) < 0.25)
    slab = (x[:, 2] > 0.7 * L[2]) & (x[:, 2] < 0.8 * L[2])
    keep &= ~slab | (rng.random(n) < 0.5)
    _, idx = R.cells_of(x, _grid())
    for c in empty:
        keep &= ~((idx[0] == c[0]) & (idx[1] == c[1]) & (idx[2] == c[2]))
    x = x[keep]
    f = rng.uniform(1.0, 2.0, (x.shape[0], NF)) * 10.0 ** rng.integers(0, 20, NF)
    f[:, TR_ID] = rng.permutation(x.shape[0]) + 100.0
    return x, f


def _state(sim):
    x, f = sim.tracers()
    return x, f, sim.tracer_velocity(), sim.census()


@pytest.mark.parametrize("unique", [False, True])
def test_refill_matches_model(unique):
    """Measured on an MI355X (both ID rules): new positions differ from the model by at most 1.46e-16 / 1.21e-16 / 1.82e-16 of L_d
    (z, x, y: one ulp, the FMA), new fields by 0 (the kernel sums in resident order, as the model does), everything else exact.
    68 122 tracers, 14 881 injected into 1 672 cells, 100 of them empty."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _cloud(21)
    dens, dmin, seed, it = 12, 6, 4242, 3
    sim = P3.Simulation3(NX, LL, tr_x, tr_f, P3.Options3(tracdens=dens, tracdens_min=dmin, inject_seed=seed, inject_unique_ids=unique))
    cen0 = sim.census()
    got = sim.refill(it=it)
    x, f, v, cen = _state(sim)
    rx, rf, rv, info = R.refill(tr_x, tr_f, _grid(), dens, dmin, seed, it, unique_ids=unique)
    print("refill: %d tracers + %d injected into %d cells (%d empty), smallest count %d" %
          (tr_x.shape[0], got["ninjected"], got["nrefilled"], got["nempty"], got["mincount"]))
    assert info["nempty"] >= 3 and info["nrefilled"] > 500 and info["mincount"] == 0 == cen0.min()
    assert got == dict(ninjected=info["ninjected"], nrefilled=info["nrefilled"], nempty=info["nempty"], mincount=info["mincount"])
    assert x.shape[0] == rx.shape[0] == sim.count() == sim.ntrac == tr_x.shape[0] + info["ninjected"]
    assert np.array_equal(cen, info["census"]) and cen.min() >= dmin and cen.sum() == x.shape[0]
    new = info["new"]
    assert np.array_equal(x[~new], rx[~new]) and np.array_equal(f[~new], rf[~new])            # the old tracers, in their stable order
    assert np.array_equal(f[:, TR_ID], rf[:, TR_ID])
    assert np.array_equal(np.isnan(f), np.isnan(rf)) and np.isnan(f[new]).any() and not np.isnan(x).any()
    ex = [float(np.abs(x[new, d] - rx[new, d]).max()) / LL[d] for d in range(3)]
    cols = [q for q in range(NF) if q != TR_ID]
    a, b = f[new][:, cols], rf[new][:, cols]
    ok = ~np.isnan(b)
    ef = float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))
    print("new positions: max |dx| / L = %.3g %.3g %.3g   new fields: max relative %.3g" % (ex[0], ex[1], ex[2], ef))
    assert max(ex) <= 4 * 2.0 ** -52
    assert ef <= 2 * dens * 2.0 ** -52
    assert not v[new].any() and np.array_equal(v, rv)
    # the new tracers lie in the cells they were made for
    assert np.array_equal(R.cells_of(x[new], _grid())[0], info["cell"][new])
    sim.close()


def test_two_refills_are_bitwise_equal():
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _cloud(22)
    outs = []
    for rep in range(2):
        sim = P3.Simulation3(NX, LL, tr_x, tr_f, P3.Options3(tracdens=12, tracdens_min=6))
        c = sim.refill(it=1)
        assert c["ninjected"] > 0
        outs.append(_state(sim))
        sim.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)


def test_advect_without_work_equals_resident_rk4():
    """pl3_resident_advect with tracdens_min = 0, and with densities that leave no cell deficient, against pl3_resident_rk4."""
    from pylamp_amd import pylamp3d as P3, _lib
    rng = np.random.default_rng(23)
    n = 200000
    tr_x = rng.random((n, 3)) * np.array(LL) * 0.999998 + 1e-6 * np.array(LL)
    tr_f = rng.uniform(1.0, 2.0, (n, NF)); tr_f[:, TR_ID] = np.arange(n)
    h = min(LL[d] / (NX[d] - 1) for d in range(3)); dt = 1e12
    vel = [rng.standard_normal(NX) * (0.4 * h / dt) for _ in range(3)]
    grids, V = P3.advection_velocity(vel, P3.gridmp_of(_grid()), NX)
    shp = tuple(v + 1 for v in NX)
    g = [_lib.f64(c) for c in grids]; Vc = [np.ascontiguousarray(a.reshape(shp)) for a in V]
    ref = P3.Simulation3(NX, LL, tr_x, tr_f)
    ref._lib_call("pl3_resident_rk4", *[_lib.dptr(c) for c in g], *[_lib.dptr(a) for a in Vc], float(dt), 1)
    want = _state(ref)
    ref.close()
    lo = int(want[3].min())
    assert lo >= 2
    for dens, dmin in ((0, 0), (lo + 3, lo)):
        sim = P3.Simulation3(NX, LL, tr_x, tr_f, P3.Options3(tracdens=dens, tracdens_min=dmin))
        c = sim.advect(grids, V, dt, it=1)
        assert c == dict(ninjected=0, nrefilled=0, nempty=0, mincount=lo)
        for a, b in zip(_state(sim), want):
            assert np.array_equal(a, b)
        sim.close()


def test_arrays_grow_inside_the_sort_and_the_stages_run_on_the_grown_state():
    """One tracer per cell refilled to 16: the arrays grow 16-fold inside the sort.  Every old tracer keeps its 13 columns bitwise;
    scatter, temperature stage and RK4 on the grown state against tests/mic3_model.py on the downloaded arrays.
    Measured on an MI355X: scatter 2.3e-15 (arithmetic) / 1.8e-14 (geometric), temperature 3.6e-16, RK4 x 1.2e-16, v 6.0e-15."""
    from pylamp_amd import pylamp3d as P3
    rng = np.random.default_rng(24)
    grid = _grid()
    nc = [v - 1 for v in NX]
    I, J, K = np.meshgrid(*[np.arange(v) for v in nc], indexing="ij")
    tr_x = np.stack([(I.ravel() + rng.uniform(0.1, 0.9, I.size)) * (LL[0] / nc[0]), (J.ravel() + rng.uniform(0.1, 0.9, I.size)) * (LL[1] / nc[1]),
                     (K.ravel() + rng.uniform(0.1, 0.9, I.size)) * (LL[2] / nc[2])], 1)
    n = tr_x.shape[0]
    p = rng.permutation(n); tr_x = tr_x[p]
    tr_f = rng.uniform(1.0, 2.0, (n, NF)) * 10.0 ** rng.integers(0, 20, NF)
    tr_f[:, TR_ID] = np.arange(n)
    tr_f[:, 3] = 273 + 1350 * tr_x[:, 0] / LL[0]
    sim = P3.Simulation3(NX, LL, tr_x, tr_f, P3.Options3(tracdens=16, tracdens_min=2, inject_unique_ids=True))
    assert sim.census().max() == 1
    c = sim.refill(it=1)
    assert c == dict(ninjected=15 * n, nrefilled=n, nempty=0, mincount=1)
    x, f, v, cen = _state(sim)
    assert x.shape[0] == 16 * n and (cen == 16).all()
    old = f[:, TR_ID] < n
    o = np.argsort(f[old, TR_ID])
    assert np.array_equal(f[old][o], tr_f) and np.array_equal(x[old][o], tr_x)
    assert np.array_equal(np.sort(f[~old, TR_ID]), n + np.arange(15 * n))
    # a new tracer of a cell with one resident is a copy of it (the mean of one value), at another place in the same cell
    cell_all = R.cells_of(x, grid)[0]
    assert (np.diff(cell_all) >= 0).all()
    src = np.where(old)[0][np.searchsorted(cell_all[old], cell_all[~old])]
    cols = [q for q in range(NF) if q != TR_ID]
    assert np.array_equal(f[~old][:, cols], f[src][:, cols])
    # stages on the grown state
    got = sim.scatter([0, 1], [5, 6])
    ref = M.trac2grid(x, f[:, [0, 1]], grid, [5, 6])
    es = [maxrel(got[0], ref[0]), maxrel(got[1], ref[1])]
    Tn = 1000 + 100 * rng.standard_normal(NX)
    sim.temp_to_tracers(Tn, True)
    _, f2 = sim.tracers()
    et = maxrel(f2[:, 3], M.grid2trac(x, grid, [Tn])[:, 0])
    h = min(LL[d] / nc[d] for d in range(3)); dt = 1e12
    vel = [rng.standard_normal(NX) * (0.3 * h / dt) for _ in range(3)]
    grids, V = P3.advection_velocity(vel, sim.gridmp, NX)
    sim.opt.tracdens_min = 0; sim.opt.tracdens = 0
    sim.advect(grids, V, dt)
    vr, xr = M.rk4(x, grids, V, dt)
    xr = M.fence(xr, LL)
    ax_, af, av, _ = _state(sim)
    o2 = np.argsort(af[:, TR_ID]); o1 = np.argsort(f[:, TR_ID])
    exx, evv = maxrel(ax_[o2], xr[o1]), maxrel(av[o2], vr[o1])
    print("grown state: scatter %.3g / %.3g  temperature %.3g  rk4 x %.3g  v %.3g" % (es[0], es[1], et, exx, evv))
    assert es[0] < 1e-12 and es[1] < 1e-11 and et < 1e-13 and exx < 1e-14 and evv < 1e-9
    assert np.array_equal(af[o2][:, cols], f2[o1][:, cols]) and sim.census().sum() == 16 * n
    sim.close()


def test_the_stream_of_a_cell_does_not_depend_on_the_other_cells():
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _cloud(25)
    grid = _grid()
    cell = R.cells_of(tr_x, grid)[0]
    cnt = np.bincount(cell, minlength=20 * 24 * 16)
    extra = int(np.where(cnt >= 8)[0][37])                     # a cell that is not deficient: empty it as well
    keep = cell != extra
    sets = [(tr_x, tr_f), (tr_x[keep], tr_f[keep])]
    pos = []
    for x0, f0 in sets:
        sim = P3.Simulation3(NX, LL, x0, f0, P3.Options3(tracdens=12, tracdens_min=6, inject_seed=99))
        sim.refill(it=7)
        x, _ = sim.tracers()
        sim.close()
        info = R.refill(x0, f0, grid, 12, 6, 99, 7)[3]
        assert x.shape[0] == info["new"].size
        new = info["new"]
        pos.append({(int(c), int(q)): tuple(r) for c, q, r in zip(info["cell"][new], info["ordinal"][new], x[new])})
    a, b = pos
    assert set(b) - set(a) == {(extra, q) for q in range(12)}
    assert all(b[k] == a[k] for k in a) and len(a) > 1000


def test_refill_errors_are_named():
    from pylamp_amd import pylamp3d as P3, _lib
    tr_x, tr_f = _cloud(26, n=20000)
    sim = P3.Simulation3(NX, LL, tr_x, tr_f)
    lib, hnd = sim.ctx.lib, sim.ctx.handle()
    out = (C.c_int64 * 4)()
    g = [_lib.f64(np.linspace(0, 1, NX[d] + 1)) for d in range(3)]
    V = [np.zeros([v + 1 for v in NX]) for _ in range(3)]
    args = [_lib.dptr(c) for c in g] + [_lib.dptr(a) for a in V]
    assert lib.pl3_resident_advect(hnd, *args, 1.0, 0, 8, 4, 1, 1, 0, out) != 0
    msg = lib.pl3_last_error(hnd)
    assert b"fence" in msg and b"injection" in msg and b"nearest" in msg, msg
    assert lib.pl3_resident_advect(hnd, *args, 1.0, 0, 0, 0, 1, 1, 0, out) == 0             # fence off is fine without injection
    assert lib.pl3_resident_refill(hnd, 3, 5, 1, 1, 0, out) != 0
    assert b"tracdens < tracdens_min" in lib.pl3_last_error(hnd)
    assert lib.pl3_resident_refill(hnd, -1, 0, 1, 1, 0, out) != 0
    assert sim.count() == tr_x.shape[0]
    sim.close()
    grid = [np.linspace(0, 1, 9)] * 3
    vc = P3.VirtualCluster3([9, 9, 9], grid, 2, 1, 1)
    try:
        ctx = vc.ctxs[0]
        assert ctx.lib.pl3_resident_refill(ctx.handle(), 8, 4, 1, 1, 0, out) != 0
        assert b"one rank" in ctx.lib.pl3_last_error(ctx.handle()) and b"pl3_resident_refill" in ctx.lib.pl3_last_error(ctx.handle())
        g9 = [_lib.f64(np.linspace(0, 1, 10))] * 3; V9 = [np.zeros((10, 10, 10))] * 3
        assert ctx.lib.pl3_resident_advect(ctx.handle(), *[_lib.dptr(c) for c in g9], *[_lib.dptr(a) for a in V9], 1.0, 1, 8, 4, 1, 1, 0, out) != 0
        assert b"one rank" in ctx.lib.pl3_last_error(ctx.handle())
    finally:
        vc.close()


def _sphere_thinned(nx, L, slab=(8, 12)):
    """falling_sphere_tracers (2 x 2 x 2 per cell) with the cells of the z layers slab[0]..slab[1]-1 thinned to 2 of their 8: the
    two on the diagonal of the cell's sub-lattice, so that each of them forms a lattice of one per cell and a cell keeps about two
    under any translation."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))
    m = [2 * (v - 1) for v in nx]
    a, b, c = np.meshgrid(*[np.arange(v) for v in m], indexing="ij")
    a, b, c = a.ravel(), b.ravel(), c.ravel()
    in_slab = (a // 2 >= slab[0]) & (a // 2 < slab[1])
    diag = (a % 2 == b % 2) & (b % 2 == c % 2)
    keep = ~in_slab | diag
    return tr_x[keep], tr_f[keep], tr_x.shape[0]


def test_falling_sphere_with_injection():
    """33^3 nodes, a slab of four cell layers through the sphere thinned to 2 of 8 tracers, refill to 8 below 4, five steps."""
    from pylamp_amd import pylamp3d as P3
    nx = [33, 33, 33]; L = [100e3, 100e3, 100e3]
    grid = [np.linspace(0, L[d], nx[d]) for d in range(3)]
    tr_x, tr_f, nfull = _sphere_thinned(nx, L)
    n0 = tr_x.shape[0]
    assert n0 == nfull - 6 * 4 * 32 * 32
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, tracdens=8, tracdens_min=4,
                                                         inject_unique_ids=True))
    assert sim.census().min() == 2
    sphere = lambda f: (f[:, TR_ID] < nfull) & (f[:, TR_MAT] == 2)
    zs = [tr_x[sphere(tr_f), 0].mean()]
    total = 0
    for it in range(5):
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        for name in ("rho", "etas", "etan"):
            assert not np.isnan(sim.field(name)).any(), name
        total += rep["ninjected"]
        cen = sim.census()
        x, f = sim.tracers()
        print("step %d: tstep %.3e  its %d  injected %d into %d cells (%d empty, smallest count %d)  sphere z %.6e" %
              (rep["it"], rep["tstep"], rep["stokes"]["iterations"], rep["ninjected"], rep["nrefilled"], rep["nempty"], rep["mincount"],
               x[sphere(f), 0].mean()))
        assert cen.min() >= 4 and cen.sum() == rep["ntrac"] == x.shape[0] == n0 + total
        assert (x > 0).all() and (x < np.array(L)).all()
        if it == 0:
            assert rep["ninjected"] > 0 and rep["nrefilled"] > 1000
            # cells whose residents are all sphere material hand exactly that material to their new tracers
            cell = R.cells_of(x, grid)[0]
            isnew = f[:, TR_ID] >= nfull
            m = 32 ** 3
            nres = np.bincount(cell[~isnew], minlength=m)
            nsph = np.bincount(cell[~isnew], weights=(f[~isnew, TR_MAT] == 2).astype(float), minlength=m)
            pure = (nres > 0) & (nsph == nres)
            sel = isnew & pure[cell]
            assert sel.sum() > 100 and (f[sel, TR_MAT] == 2.0).all()
            assert sim.tracer_velocity()[isnew].any() == False and sim.tracer_velocity()[~isnew].any()      # noqa: E712
        zs.append(x[sphere(f), 0].mean())
        assert zs[-1] > zs[-2]
    assert np.unique(f[:, TR_ID]).size == f.shape[0]
    sim.close()


def test_step_names_the_cause_when_cells_without_tracers_make_nan():
    from pylamp_amd import pylamp3d as P3
    nx = [17, 17, 17]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(3))
    idx = R.cells_of(tr_x, [np.linspace(0, L[d], nx[d]) for d in range(3)])[1]
    hole = np.ones(tr_x.shape[0], dtype=bool)
    for d in range(3):
        hole &= (idx[d] >= 6) & (idx[d] < 10)
    sim = P3.Simulation3(nx, L, tr_x[~hole], tr_f[~hole], P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False))
    with pytest.raises(Exception, match="without any marker in reach.*enable injection"):
        sim.step()
    assert sim.it == 0
    sim.close()
