"""3-D fence-off deletion on the GPU (pl3_mic_set_deletion, Options3.tracs_fence_enabled = False + marker_deletion = True) against
the NumPy model tests/mic3_delete_model.py, which tests/test_mic3_delete_model.py ties to the 2-D oracle.

The deletion is "the same sort on the survivors", so the bounds are those of the plain sort and refill: which tracers leave, the
survivors' IDs and order, counts, counters and census are exact; positions after RK4 1e-14 and velocities 1e-9 (relative to the
largest, as tests/test_hip_mic3.py); positions of new tracers 4 * 2^-52 L_d and their fields 2 tracdens 2^-52 (as
tests/test_hip_mic3_refill.py).  Every set is built so that no model end position lies within 1e-9 L of a wall -- the tests assert
it -- so that a rounding difference between kernel and model cannot change who leaves.

Grids: 7 x 6 x 8 nodes (6 x 5 x 7 cells, several workgroups of tracers, one of cells), uniform and graded 4:1 with the search on."""
import ctypes as C

import numpy as np
import pytest

from conftest import maxrel
import mic3_delete_model as D
import mic3_model as M
import mic3_rect_model as S
import mic3_refill_model as R

pytestmark = pytest.mark.gpu

NF, TR_MAT, TR_RH0, TR_ET0, TR_ID = 13, 8, 6, 10, 12
NX = [7, 6, 8]; LL = [1.2e5, 1.0e5, 0.7e5]
NCELL = 6 * 5 * 7
SEARCH = [False, True]


def _grid(search):
    from pylamp_amd import pylamp3d as P3
    return [P3.graded_grid(NX[d], LL[d], 4) for d in range(3)] if search else [np.linspace(0, LL[d], NX[d]) for d in range(3)]


def _sim(search, tr_x=None, tr_f=None, delete=True, **kw):
    from pylamp_amd import pylamp3d as P3
    if delete:
        kw.update(tracs_fence_enabled=False, marker_deletion=True)
    return P3.Simulation3(NX, LL, tr_x, tr_f, P3.Options3(marker_search=search, **kw), grid=_grid(search) if search else None)


def _fields(rng, n):
    f = rng.uniform(1.0, 2.0, (n, NF)) * 10.0 ** rng.integers(0, 20, NF)
    f[:, TR_ID] = rng.permutation(n) + 100.0
    return f


def _cloud(seed, n=4000):
    """Random cloud strictly inside the box, positive values in every column, IDs a permutation starting at 100."""
    rng = np.random.default_rng(seed)
    x = (0.001 + 0.998 * rng.random((n, 3))) * np.array(LL)
    return x, _fields(rng, n)


def _state(sim):
    x, f = sim.tracers()
    return x, f, sim.tracer_velocity(), sim.census()


def _model(search):
    return S if search else M


def _uniform_z(sim, w):
    """The padded centre grid and a velocity w along +z everywhere on it, ghosts equal to the interior."""
    from pylamp_amd import pylamp3d as P3
    grids, V = P3.advection_velocity([np.zeros(NX)] * 3, sim.gridmp, NX)
    V[0][...] = w
    return grids, V


def _clear_of_walls(x):
    """No position within 1e-9 L of a wall."""
    return all(not (np.abs(x[:, d]) <= 1e-9 * LL[d]).any() and not (np.abs(x[:, d] - LL[d]) <= 1e-9 * LL[d]).any() for d in range(3))


def _assert_state(sim, x, f, v, census, tag):
    gx, gf, gv, gc = _state(sim)
    assert gx.shape == x.shape and sim.count() == sim.ntrac == x.shape[0], tag
    assert np.array_equal(gf[:, TR_ID], f[:, TR_ID]), tag + ": IDs and order"
    assert np.array_equal(gx, x, equal_nan=True) and np.array_equal(gf, f), tag + ": rows"
    assert np.array_equal(gv, v, equal_nan=True), tag + ": stored velocities"
    assert np.array_equal(gc, census) and gc.sum() == x.shape[0], tag + ": census"


# ---- 1. boundary values --------------------------------------------------------------------------------------------------------
def _boundary_set():
    x, f = _cloud(41, 3000)
    special = []
    for d in range(3):
        L = LL[d]
        for val in (0.0, L, np.nextafter(0.0, 1.0), np.nextafter(L, 0.0), -1e-3 * L, L * (1 + 1e-3), np.nan):
            p = 0.37 * np.array(LL); p[d] = val
            special.append(p)
    k = len(special)
    pos = np.random.default_rng(42).choice(x.shape[0], k, replace=False)          # scattered through the workgroups
    x[pos] = np.array(special)
    leave = np.zeros(x.shape[0], dtype=bool)
    leave[pos.reshape(3, 7)[:, [0, 1, 4, 5]].ravel()] = True                       # 0, L, -1e-3 L, L (1 + 1e-3): <= 0 or >= L
    return x, f, leave


@pytest.mark.parametrize("search", SEARCH)
def test_boundary_values_leave_exactly_by_the_rule(search):
    """Zero velocity: RK4 returns the positions exactly, so upload, refill() and advect() see the same set.  Per axis 0, L, -1e-3 L and
    L (1 + 1e-3) leave; nextafter(0, 1), nextafter(L, 0) and the NaN coordinate stay.  Switching deletion on with the clamped set
    resident removes the same twelve."""
    x0, f0, leave = _boundary_set()
    grid = _grid(search)
    assert np.array_equal(D.outside(x0, LL), leave) and leave.sum() == 12
    x, f, v, info, kept = D.sort_delete_refill(x0, f0, grid, search=search)
    assert np.array_equal(kept, ~leave) and np.isnan(x).sum() == 3
    sim = _sim(search, x0, f0)
    assert sim.ctx.marker_deletion() and sim.ctx.tracers_removed() == (12, 12)
    _assert_state(sim, x, f, v, info["census"], "upload")
    c = sim.refill(it=1)
    assert c == dict(ninjected=0, nrefilled=0, nempty=info["nempty"], mincount=info["mincount"], nremoved=0)
    assert sim.ctx.tracers_removed() == (0, 12)
    _assert_state(sim, x, f, v, info["census"], "refill")
    grids, V = _uniform_z(sim, 0.0)
    c = sim.advect(grids, V, 1.0e3, it=1)
    assert c["nremoved"] == 0 and c["ninjected"] == 0 and sim.ctx.tracers_removed() == (0, 12)
    _assert_state(sim, x, f, x * 0.0, info["census"], "advect")                    # v = (x - x) / dt: NaN where the coordinate is
    sim.close()
    # the switch itself: resident tracers outside the box (clamped into the nearest cell) go when deletion is switched on
    sim = _sim(search, x0, f0, delete=False)
    assert sim.count() == x0.shape[0] and sim.ctx.tracers_removed() == (0, 0)
    sim.ctx.set_marker_deletion(True)
    assert sim.ctx.tracers_removed() == (12, 12) and sim.count() == x0.shape[0] - 12
    gx, gf, _, gc = _state(sim)
    assert np.array_equal(np.sort(gf[:, TR_ID]), np.sort(f[:, TR_ID])) and np.array_equal(gc, info["census"])
    sim.close()


# ---- 2. layers leaving ---------------------------------------------------------------------------------------------------------
def _resident_order(x0, f0, grid, search):
    x, f, _, _, kept = D.sort_delete_refill(x0, f0, grid, search=search)
    assert kept.all()
    return x, f


@pytest.mark.parametrize("search", SEARCH)
def test_layers_leave_under_a_uniform_velocity(search):
    """w dt = 1.5 times the last cell along z.  With the reference's weights (1,1,1,1)/6 a tracer is carried 2/3 w dt = one cell, less
    where its later stages fall beyond the padded grid (velocity 0 there): the model has the same rules, the outermost layer leaves."""
    x0, f0 = _cloud(43)
    grid = _grid(search)
    sim = _sim(search, x0, f0)
    xs, fs = _resident_order(x0, f0, grid, search)
    dt = 1.0e12
    grids, V = _uniform_z(sim, 1.5 * (grid[0][-1] - grid[0][-2]) / dt)
    vr, xr = _model(search).rk4(xs, grids, V, dt)
    assert _clear_of_walls(xr)
    x, f, v, info, kept = D.sort_delete_refill(xr, fs, grid, tr_v=vr, search=search)
    nout = int((~kept).sum())
    assert 400 < nout < 2000 and (xr[~kept, 0] >= LL[0]).all()
    c = sim.advect(grids, V, dt, it=1)
    gx, gf, gv, gc = _state(sim)
    print("layers: %d of %d leave; x %.3g  v %.3g" % (nout, x0.shape[0], maxrel(gx, x), maxrel(gv, v)))
    assert c["nremoved"] == nout and sim.ctx.tracers_removed() == (nout, nout)
    assert sim.count() == sim.ntrac == x0.shape[0] - nout == gx.shape[0]
    assert np.array_equal(gf, f)                                                   # the survivors' rows, in the model's order
    assert np.array_equal(gc, info["census"]) and gc.sum() == gx.shape[0]
    assert maxrel(gx, x) < 1e-14 and maxrel(gv, v) < 1e-9
    assert (gx > 0).all() and (gx < np.array(LL)).all()
    sim.close()


# ---- 3. deletion and refill in one sort -----------------------------------------------------------------------------------------
TOP_COLUMNS = ((1, 2), (3, 5))


def _refill_set(grid, search):
    """A cloud in which the top z cell of two columns holds tracers only where they leave under a shift s = 0.3 of the last cell, and
    the columns hold nothing that would arrive in their place: the removal empties those two cells.  The largest ID sits on the
    tracer nearest to the wall zL, which leaves."""
    x, f = _cloud(44)
    gz = grid[0]; h = gz[-1] - gz[-2]; s = 0.3 * h
    _, idx = (S if search else R).cells_of(x, grid)
    drop = np.zeros(x.shape[0], dtype=bool)
    for j, k in TOP_COLUMNS:
        drop |= (idx[1] == j) & (idx[2] == k) & (x[:, 0] >= LL[0] - h - s) & (x[:, 0] < LL[0] - s)
    drop |= (idx[0] >= 1) & (idx[0] <= 2) & (idx[1] == 0) & (np.random.default_rng(49).random(x.shape[0]) > 0.15)   # and a sparse slab: cells with 1..3
    x, f = x[~drop], f[~drop]
    extra = []
    for j, k in TOP_COLUMNS:
        for q in range(3):
            t = 0.3 + 0.2 * q
            extra.append([LL[0] - (0.1 + 0.1 * q) * s, grid[1][j] + t * (grid[1][j + 1] - grid[1][j]), grid[2][k] + t * (grid[2][k + 1] - grid[2][k])])
    x = np.concatenate([x, np.array(extra)])
    f = np.concatenate([f, _fields(np.random.default_rng(45), len(extra))])
    f[:, TR_ID] = np.random.default_rng(46).permutation(x.shape[0]) + 100.0
    top = np.argmax(x[:, 0])
    big = np.argmax(f[:, TR_ID])
    f[[top, big], TR_ID] = f[[big, top], TR_ID]
    return x, f, s


def _refill_case(search, unique):
    grid = _grid(search)
    x0, f0, s = _refill_set(grid, search)
    dens, dmin, seed, it, dt = 8, 4, 4242, 3, 1.0e12
    sim = _sim(search, x0, f0, tracdens=dens, tracdens_min=dmin, inject_seed=seed, inject_unique_ids=unique, do_heatdiff=False,
               tdep_rho=False, tdep_eta=False)
    xs, fs = _resident_order(x0, f0, grid, search)
    grids, V = _uniform_z(sim, 1.5 * s / dt)       # the reference's weights (1,1,1,1)/6 carry a tracer 2/3 w dt; every stage stays on the padded grid
    cen0 = sim.census()
    vr, xr = _model(search).rk4(xs, grids, V, dt)
    c = sim.advect(grids, V, dt, it=it)
    return sim, c, cen0, fs, xr, vr, D.sort_delete_refill(xr, fs, grid, dens, dmin, seed, it, unique_ids=unique, tr_v=vr, search=search)


@pytest.mark.parametrize("unique", [False, True])
@pytest.mark.parametrize("search", SEARCH)
def test_deletion_and_refill_in_one_sort(search, unique):
    sim, c, cen0, fs, xr, vr, (x, f, v, info, kept) = _refill_case(search, unique)
    assert _clear_of_walls(xr)
    nout = int((~kept).sum())
    # the top cells of the two prepared columns held tracers, lost all of them to the removal and received none: they are empty
    # in the census the refill saw
    emptied = [(5 * 5 + j) * 7 + k for j, k in TOP_COLUMNS]
    left = np.bincount(info["cell"][~info["new"]], minlength=NCELL)
    assert nout > 50 and all(cen0.ravel()[q] >= 3 and left[q] == 0 and q in info["cells"] for q in emptied)
    assert info["nempty"] >= len(emptied)
    assert fs[~kept, TR_ID].max() == fs[:, TR_ID].max() > fs[kept, TR_ID].max()    # the largest ID leaves with its holder
    gx, gf, gv, gc = _state(sim)
    print("delete + refill: %d leave, %d injected into %d cells (%d empty, %d emptied by the removal), smallest count %d" %
          (nout, c["ninjected"], c["nrefilled"], c["nempty"], len(emptied), c["mincount"]))
    assert c == dict(ninjected=info["ninjected"], nrefilled=info["nrefilled"], nempty=info["nempty"], mincount=info["mincount"], nremoved=nout)
    assert info["mincount"] == 0 and sim.ctx.tracers_removed() == (nout, nout)
    assert gx.shape[0] == x.shape[0] == sim.count() == sim.ntrac == fs.shape[0] - nout + info["ninjected"]
    assert np.array_equal(gc, info["census"]) and gc.min() >= 4 and gc.sum() == gx.shape[0]
    new = info["new"]
    assert np.array_equal(gf[:, TR_ID], f[:, TR_ID])                               # survivors in order, new IDs from the survivors' largest
    first = fs[kept, TR_ID].max() + (1 if unique else 0)
    assert gf[new, TR_ID].min() == first
    assert np.array_equal(gf[~new], f[~new]) and maxrel(gx[~new], x[~new]) < 1e-14 and maxrel(gv[~new], v[~new]) < 1e-9
    assert np.array_equal(np.isnan(gf), np.isnan(f)) and np.isnan(gf[new]).any() and not np.isnan(gx).any()
    for q in emptied:
        assert np.isnan(gf[new & (info["cell"] == q)][:, 0]).all()
    ex = [float(np.abs(gx[new, d] - x[new, d]).max()) / LL[d] for d in range(3)]
    cols = [q for q in range(NF) if q != TR_ID]
    a, b = gf[new][:, cols], f[new][:, cols]
    ok = ~np.isnan(b)
    assert ok.any()
    ef = float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok])))
    print("new positions: max |dx| / L = %.3g %.3g %.3g   new fields: max relative %.3g" % (ex[0], ex[1], ex[2], ef))
    assert max(ex) <= 4 * 2.0 ** -52 and ef <= 2 * 8 * 2.0 ** -52
    assert not gv[new].any()
    # the NaN fields of the new tracers of the empty cells reach the grid: the step names the cause instead of solving
    with pytest.raises(Exception, match="holds NaN.*without any marker in reach"):
        sim.step()
    assert sim.it == 0
    sim.close()


def test_two_deleting_refills_are_bitwise_equal():
    outs = []
    for rep in range(2):
        sim, c = _refill_case(True, False)[:2]
        assert c["ninjected"] > 0 and c["nremoved"] > 0
        outs.append(_state(sim))
        sim.close()
    for a, b in zip(*outs):
        assert np.array_equal(a, b, equal_nan=True)


# ---- 4. everything leaves -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("search", SEARCH)
def test_everything_leaves(search):
    x0, f0 = _cloud(47, 3000)
    sim = _sim(search, x0, f0, tracdens=8, tracdens_min=4)
    dt = 1.0e12
    grids, V = _uniform_z(sim, 12.0 * LL[0] / dt)                                  # the first stage alone carries every tracer 2 L further
    sim.opt.tracdens_min = 0
    c = sim.advect(grids, V, dt, it=1)
    assert c["nremoved"] == 3000 and c["ninjected"] == 0 and sim.ctx.tracers_removed() == (3000, 3000)
    assert sim.count() == sim.ntrac == 0
    x, f, v, cen = _state(sim)
    assert x.shape == (0, 3) and f.shape == (0, NF) and v.shape == (0, 3) and cen.shape == (6, 5, 7) and not cen.any()
    out = sim.scatter([0, 1], [5, 6])
    assert all(np.isnan(a).all() for a in out)                                     # nothing arrives anywhere: 0/0 as for any empty node
    c = sim.advect(grids, V, dt, it=2)                                             # an empty set advects and sorts
    assert c["nremoved"] == 0 and sim.count() == 0
    sim.opt.tracdens_min = 4
    c = sim.refill(it=3)
    assert c == dict(ninjected=8 * NCELL, nrefilled=NCELL, nempty=NCELL, mincount=0, nremoved=0)
    x, f, v, cen = _state(sim)
    rx, rf, _, info = (S if search else R).refill(np.zeros((0, 3)), np.zeros((0, NF)), _grid(search), 8, 4, sim.opt.inject_seed, 3)
    assert sim.count() == 8 * NCELL and (cen == 8).all() and np.isnan(f[:, :TR_ID]).all() and not v.any()
    assert np.array_equal(f[:, TR_ID], rf[:, TR_ID]) and f[0, TR_ID] == -1.0       # no survivor: numbering starts at -1
    assert max(float(np.abs(x[:, d] - rx[:, d]).max()) / LL[d] for d in range(3)) <= 4 * 2.0 ** -52
    assert sim.ctx.tracers_removed() == (0, 3000)
    sim.upload(x0, f0)                                                             # an upload starts the count again
    assert sim.ctx.tracers_removed() == (0, 0) and sim.count() == 3000
    sim.close()


# ---- 5. off means off -----------------------------------------------------------------------------------------------------------
def test_without_the_switch_nothing_is_removed():
    """Deletion never set: after an advection without the fence the tracers outside are counted in the nearest cell, as before this
    switch existed.  Switched on, the sort removes them; switched off again, later leavers stay."""
    from pylamp_amd import _lib
    x0, f0 = _cloud(48)
    grid = _grid(False)
    sim = _sim(False, x0, f0, delete=False)
    assert sim.ctx.marker_deletion() is False
    xs, fs = _resident_order(x0, f0, grid, False)
    dt = 1.0e12
    grids, V = _uniform_z(sim, 1.5 * (grid[0][1] - grid[0][0]) / dt)
    gl = [_lib.f64(c) for c in grids]; Vl = [np.ascontiguousarray(a, dtype=np.float64) for a in V]
    args = [_lib.dptr(c) for c in gl] + [_lib.dptr(a) for a in Vl]
    out = (C.c_int64 * 4)()

    def advect_unfenced():
        sim._lib_call("pl3_resident_advect", *args, float(dt), 0, 0, 0, 1, 1, 0, out)

    def clamped(xm, fm, vm):
        """The plain stable sort by the clamped cell of mic3_refill_model.cells_of."""
        o = np.argsort(R.cells_of(xm, grid)[0], kind="stable")
        return xm[o], fm[o], vm[o], np.bincount(R.cells_of(xm, grid)[0], minlength=NCELL).reshape(6, 5, 7)
    advect_unfenced()
    vr, xr = M.rk4(xs, grids, V, dt)
    assert _clear_of_walls(xr)
    gone = D.outside(xr, LL)
    x1, f1, v1, cen1 = clamped(xr, fs, vr)
    gx, gf, gv, gc = _state(sim)
    assert 400 < gone.sum() and sim.count() == x0.shape[0] and sim.ctx.tracers_removed() == (0, 0)
    assert np.array_equal(gf, f1) and np.array_equal(gc, cen1) and maxrel(gx, x1) < 1e-14 and maxrel(gv, v1) < 1e-9
    assert (gx[:, 0] >= LL[0]).sum() == gone.sum()                                 # ... and are carried along, in the last layer's cells
    sim.ctx.set_marker_deletion(True)
    n1 = x0.shape[0] - int(gone.sum())
    assert sim.ctx.tracers_removed() == (int(gone.sum()), int(gone.sum())) and sim.count() == n1
    gx, gf, gv, gc = _state(sim)
    keep1 = ~D.outside(x1, LL)
    assert np.array_equal(gf, f1[keep1]) and (gx[:, 0] < LL[0]).all()
    sim.ctx.set_marker_deletion(False)
    assert sim.ctx.marker_deletion() is False and sim.count() == n1
    advect_unfenced()
    vr2, xr2 = M.rk4(gx, grids, V, dt)
    assert _clear_of_walls(xr2) and D.outside(xr2, LL).sum() > 400
    x2, f2, v2, cen2 = clamped(xr2, gf, vr2)
    hx, hf, hv, hc = _state(sim)
    assert sim.count() == n1 and sim.ctx.tracers_removed() == (0, int(gone.sum()))
    assert np.array_equal(hf, f2) and np.array_equal(hc, cen2) and maxrel(hx, x2) < 1e-14
    sim.close()


# ---- 6. step level --------------------------------------------------------------------------------------------------------------
SNX = [9, 9, 9]; SL = [100e3, 100e3, 100e3]
STEP_FIELDS = ("rho", "etas", "etan", "velz", "velx", "vely", "pres")


def _sphere_with_sheet():
    """The falling-sphere set (IDs below n) and a sheet of 5 x 5 tracers 1e-9 of a cell above the zL wall under the sphere."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = P3.falling_sphere_tracers(SNX, SL, np.random.default_rng(7))
    n = tr_x.shape[0]
    h = SL[0] / (SNX[0] - 1)
    cell = [np.floor(tr_x[:, d] / h).astype(int) for d in range(3)]
    keep = np.ones(n, dtype=bool)
    for c in ((2, 2, 2), (5, 3, 6)):                     # two cells thinned to 2 of their 8: the refill fires inside the deleting sort
        keep[np.flatnonzero((cell[0] == c[0]) & (cell[1] == c[1]) & (cell[2] == c[2]))[2:]] = False
    tr_x, tr_f = tr_x[keep], tr_f[keep]
    a = np.linspace(0.42, 0.58, 5)
    X, Y = np.meshgrid(a * SL[1], a * SL[2], indexing="ij")
    sheet = np.stack([np.full(25, SL[0] - 1e-9 * h), X.ravel(), Y.ravel()], axis=1)
    sf = np.zeros((25, NF)); sf[:, TR_ID] = n + np.arange(25); sf[:, TR_RH0] = 3300; sf[:, TR_MAT] = 1; sf[:, TR_ET0] = 1e19
    return np.concatenate([tr_x, sheet]), np.concatenate([tr_f, sf]), n


def _run_steps(resident, nstep=2):
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f, n = _sphere_with_sheet()
    bc = [P3.BC_TYPE_NOSLIP, P3.BC_TYPE_FREESLIP, P3.BC_TYPE_FREESLIP, P3.BC_TYPE_NOSLIP, P3.BC_TYPE_FREESLIP, P3.BC_TYPE_FREESLIP]
    sim = P3.Simulation3(SNX, SL, tr_x, tr_f, P3.Options3(bcstokes=bc, tracs_fence_enabled=False, marker_deletion=True, tracdens=8, tracdens_min=4,
                                                          do_heatdiff=False, tdep_rho=False, tdep_eta=False, resident=resident))
    steps = []
    for it in range(nstep):
        before = sim.tracers()
        rep = sim.step()
        x, f = sim.tracers()
        steps.append(dict(rep=rep, before=before, x=x, f=f, v=sim.tracer_velocity(), census=sim.census(),
                          fields={k: sim.field(k).copy() for k in STEP_FIELDS}, removed=sim.ctx.tracers_removed()))
    gridmp = sim.gridmp
    sim.close()
    return steps, gridmp, bc, n


@pytest.fixture(scope="module")
def stepped():
    return _run_steps(False), _run_steps(True)


def test_steps_with_deletion_staged_and_resident_are_bitwise_equal(stepped):
    (staged, _, _, _), (resident, _, _, _) = stepped
    for it, (s, r) in enumerate(zip(staged, resident)):
        tag = "step %d: " % (it + 1)
        assert list(s["rep"]) == list(r["rep"]), tag + "report keys"
        for k in ("it", "limiter", "ninjected", "nrefilled", "nempty", "mincount", "nremoved", "ntrac", "tstep", "time"):
            assert s["rep"][k] == r["rep"][k], tag + k
        for q in ("iterations", "converged", "operator_applies", "precond_applies", "rel_residual", "error_estimate"):
            assert s["rep"]["stokes"][q] == r["rep"]["stokes"][q], tag + "stokes " + q
        assert s["rep"]["stokes"]["converged"] == 1 and s["removed"] == r["removed"]
        for k in STEP_FIELDS:
            assert np.array_equal(s["fields"][k], r["fields"][k]), tag + "field " + k
        for k in ("x", "f", "v", "census"):
            assert np.array_equal(s[k], r[k], equal_nan=True), tag + k
        assert s["rep"]["ntrac"] == s["x"].shape[0] == s["census"].sum()
    assert staged[0]["rep"]["ninjected"] == 12 and staged[0]["rep"]["nrefilled"] == 2 and staged[0]["rep"]["nremoved"] == 25


def test_a_step_removes_what_the_model_predicts_from_its_own_velocity(stepped):
    """advection_velocity -> mic3_model.rk4 -> outside on the tracers as they were before the step, with the step's own solved
    velocity and time step.  The sheet under the sphere is carried through the no-slip wall zL (the velocity interpolated onto a
    no-slip wall at rest is half the last centre value): nremoved > 0 is a condition of this test."""
    from pylamp_amd import pylamp3d as P3
    for steps, gridmp, bc, n in stepped:
        total = 0
        for it, s in enumerate(steps):
            xb, fb = s["before"]
            vel = [s["fields"][k] for k in ("velz", "velx", "vely")]
            grids, V = P3.advection_velocity(vel, gridmp, SNX, bc)
            _, xr = M.rk4(xb, grids, V, s["rep"]["tstep"])
            sheet = (fb[:, TR_ID] >= n) & (fb[:, TR_ID] < n + 25)
            for d in range(3):
                near = (np.abs(xr[~sheet, d]) <= 1e-9 * SL[d]) | (np.abs(xr[~sheet, d] - SL[d]) <= 1e-9 * SL[d])
                assert not near.any()
            gone = D.outside(xr, SL)
            print("step %d: the model removes %d (%d of the sheet), the step %d; injected %d" %
                  (it + 1, gone.sum(), (gone & sheet).sum(), s["rep"]["nremoved"], s["rep"]["ninjected"]))
            assert s["rep"]["nremoved"] == int(gone.sum()) == s["removed"][0]
            assert s["rep"]["ntrac"] == xb.shape[0] - int(gone.sum()) + s["rep"]["ninjected"]
            assert not np.isin(fb[gone, TR_ID], s["f"][:, TR_ID]).any() or s["rep"]["ninjected"] > 0       # (the reference's ID rule may repeat an ID)
            total += s["rep"]["nremoved"]
        assert steps[0]["rep"]["nremoved"] > 0 and steps[-1]["removed"][1] == total


# ---- 7. named errors ------------------------------------------------------------------------------------------------------------
def test_deletion_errors_are_named():
    from pylamp_amd import pylamp3d as P3
    grid = [np.linspace(0, 1, 9)] * 3
    vc = P3.VirtualCluster3([9, 9, 9], grid, 2, 1, 1)
    try:
        ctx = vc.ctxs[0]
        assert ctx.lib.pl3_mic_set_deletion(ctx.handle(), 1) != 0
        msg = ctx.lib.pl3_last_error(ctx.handle())
        assert b"one rank" in msg and b"pl3_mic_set_deletion" in msg, msg
        on = C.c_int(7)
        assert ctx.lib.pl3_mic_get_deletion(ctx.handle(), C.byref(on)) != 0 and b"one rank" in ctx.lib.pl3_last_error(ctx.handle())
    finally:
        vc.close()
    ctx = P3.Context3([5, 5, 5], [np.linspace(0, 1, 5)] * 3)
    assert ctx.lib.pl3_tracers_removed(ctx.handle(), None) != 0
    assert b"pl3_tracers_removed" in ctx.lib.pl3_last_error(ctx.handle())
    assert ctx.lib.pl3_mic_get_deletion(ctx.handle(), None) != 0 and b"pl3_mic_get_deletion" in ctx.lib.pl3_last_error(ctx.handle())
    assert ctx.marker_deletion() is False and ctx.tracers_removed() == (0, 0)
    ctx.set_marker_deletion(True)                                                  # no tracers resident: only the state changes
    assert ctx.marker_deletion() is True
    # fence == 0 with injection: refused without the switch (the message keeps its words), allowed with it
    out = (C.c_int64 * 4)()
    from pylamp_amd import _lib
    g = [_lib.f64(np.linspace(0, 1, 6))] * 3; V = [np.zeros((6, 6, 6))] * 3
    args = [_lib.dptr(c) for c in g] + [_lib.dptr(a) for a in V]
    x = np.random.default_rng(1).random((500, 3)) * 0.98 + 0.01
    f = np.ones((500, NF)); f[:, TR_ID] = np.arange(500)
    ctx.check(ctx.lib.pl3_tracers_upload(ctx.handle(), 500, _lib.dptr(x), _lib.dptr(f)))
    assert ctx.lib.pl3_resident_advect(ctx.handle(), *args, 1.0, 0, 8, 4, 1, 1, 0, out) == 0
    ctx.set_marker_deletion(False)
    assert ctx.lib.pl3_resident_advect(ctx.handle(), *args, 1.0, 0, 8, 4, 1, 1, 0, out) != 0
    msg = ctx.lib.pl3_last_error(ctx.handle())
    assert b"fence" in msg and b"injection" in msg and b"nearest" in msg and b"pl3_mic_set_deletion" in msg, msg
    ctx.close()
