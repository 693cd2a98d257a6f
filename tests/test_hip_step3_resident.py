"""The device-resident 3-D step (Options3.resident = True, pl3_resident_step) against the host-staged Simulation3.step(), which
is its yardstick: the same kernels and solvers in the same order, so the two must agree BITWISE.

Why bitwise is the bound: the scatter sums in a fixed order and pl_3d.hip has no floating-point atomics, so the staged step
repeats itself bit for bit from run to run (measured on an MI355X on the commit before this feature: two staged runs of models A
and B from scratch, three steps each -- every field, tstep, tracer array, iteration count and counter identical).  The resident
step changes where the fields live, not what is computed: the reductions behind the time-step rules are exact (min / max), the
diffusivity is evaluated with one rounding per operation as NumPy does, and the scalars are combined in Python's order.

Three models, three steps each (the wall carry, the increment path and the subgrid diffusion all run from step 2 on):
  A  falling sphere, 33^3, heat on, tracdens = 8 / tracdens_min = 4, thinned in three cells so that the refill fires inside a step;
  B  driver.mantle_tracers (33 x 41) replicated along y (ny = 9) with a genuinely 3-D temperature perturbation, subgrid diffusion on;
  C  falling sphere, 17^3, heat off: the two-field scatter and the unweighted geometric etan.
Each pair of runs is made once and shared by the tests."""
import os

import numpy as np
import pytest

from conftest import relerr

pytestmark = pytest.mark.gpu

TR_TMP, TR_HCD, TR_HCP, TR_RH0, TR_ALP, TR_MAT, TR_ET0, TR_IHT, TR_ID = 3, 4, 5, 6, 7, 8, 10, 11, 12
SCATTERED = ("rho", "etas", "etan", "cp", "T", "H", "mat", "kz", "kx", "ky")
SOLVED = ("velz", "velx", "vely", "pres", "temp")
NSTEP = 3


def _sphere(n, heat, thin=()):
    from pylamp_amd import pylamp3d as P3
    nx = [n, n, n]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))
    if heat:
        z, x, y = (tr_x[:, d] / L[d] for d in range(3))
        tr_f[:, TR_TMP] = 273 + 1350 * z + 40 * np.sin(2 * np.pi * x) * np.sin(np.pi * z) * np.cos(2 * np.pi * y)
        tr_f[:, TR_HCD] = 4.0; tr_f[:, TR_HCP] = 1250.0; tr_f[:, TR_ALP] = 3.5e-5; tr_f[:, TR_IHT] = 1e-9
    h = L[0] / (n - 1)
    cell = [np.floor(tr_x[:, d] / h).astype(int) for d in range(3)]
    keep = np.ones(tr_x.shape[0], bool)
    for c in thin:                               # leave two tracers in the cell
        inside = np.flatnonzero((cell[0] == c[0]) & (cell[1] == c[1]) & (cell[2] == c[2]))
        keep[inside[2:]] = False
    return nx, L, tr_x[keep], tr_f[keep]


def _mantle3():
    from pylamp_amd import driver
    nx2 = [33, 41]; L2 = [660e3, 820e3]; ny = 9; Ly = 21e3 * (ny - 1)
    x2, f2 = driver.mantle_tracers(nx2, L2, 8, np.random.default_rng(1))
    n2 = x2.shape[0]
    m = 2 * (ny - 1)
    ys = (np.arange(m) + np.random.default_rng(2).uniform(0.1, 0.9, m)) * Ly / m
    x3 = np.concatenate([np.insert(x2, 2, y, axis=1) for y in ys])
    f3 = np.tile(f2, (m, 1)); f3[:, TR_ID] = np.arange(m * n2)
    return nx2, L2, ny, Ly, x2, f2, ys, x3, f3


def _run(nx, L, tr_x, tr_f, kw, resident, outdir=None):
    """NSTEP steps; what every step leaves behind, by tracer ID where the order could differ."""
    from pylamp_amd import pylamp3d as P3
    sim = P3.Simulation3(nx, L, tr_x.copy(), tr_f.copy(), P3.Options3(resident=resident, **kw))
    steps = []
    for it in range(NSTEP):
        sim.transfer_stats(reset=True)
        rep = sim.step()
        xf = sim.transfer_stats(reset=True)
        names = [k for k in SCATTERED + SOLVED if resident or k in sim.fields]
        if resident and not kw.get("do_heatdiff", True):
            names = ["rho", "etas", "etan", "velz", "velx", "vely", "pres"]
        x, f = sim.tracers(); v = sim.tracer_velocity()
        steps.append(dict(rep=rep, xfer=xf, fields={k: sim.field(k).copy() for k in names}, x=x, f=f, v=v, census=sim.census(),
                          times=sim.stage_times()))
        if outdir is not None and it == NSTEP - 1:
            sim.write_snapshot(outdir)
    sim.close()
    return steps


@pytest.fixture(scope="module")
def model_a(tmp_path_factory):
    nx, L, x, f = _sphere(33, True, thin=[(5, 5, 5), (10, 20, 7), (20, 8, 30)])
    kw = dict(tracdens=8, tracdens_min=4)
    d = tmp_path_factory.mktemp("snap")
    return (_run(nx, L, x, f, kw, False, str(d / "staged")), _run(nx, L, x, f, kw, True, str(d / "resident")), str(d))


@pytest.fixture(scope="module")
def model_b():
    nx2, L2, ny, Ly, _, _, _, x3, f3 = _mantle3()
    z, x, y = x3[:, 0] / L2[0], x3[:, 1] / L2[1], x3[:, 2] / Ly
    f3 = f3.copy()
    f3[:, TR_TMP] += 30 * np.sin(np.pi * z) * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y)
    kw = dict(do_subgrid_heatdiff=True)
    return _run(nx2 + [ny], L2 + [Ly], x3, f3, kw, False), _run(nx2 + [ny], L2 + [Ly], x3, f3, kw, True)


@pytest.fixture(scope="module")
def model_c():
    nx, L, x, f = _sphere(17, False)
    kw = dict(do_heatdiff=False, tdep_rho=False, tdep_eta=False)
    return _run(nx, L, x, f, kw, False), _run(nx, L, x, f, kw, True)


def _assert_steps_equal(staged, resident, scattered, solved):
    for it, (s, r) in enumerate(zip(staged, resident)):
        tag = "step %d: " % (it + 1)
        assert list(s["rep"]) == list(r["rep"]), tag + "report keys"
        for k in ("it", "limiter", "ninjected", "nrefilled", "nempty", "mincount", "ntrac"):
            assert s["rep"][k] == r["rep"][k], tag + k
        for k in ("stokes", "heat"):
            if s["rep"][k] is None:
                assert r["rep"][k] is None
                continue
            for q in ("iterations", "converged", "operator_applies", "precond_applies", "rel_residual", "error_estimate"):
                assert s["rep"][k][q] == r["rep"][k][q], tag + k + " " + q
            assert s["rep"][k]["converged"] == 1
        print(tag + "tstep staged %.17g resident %.17g  limiter %s  stokes its %d  injected %d" % (
            s["rep"]["tstep"], r["rep"]["tstep"], s["rep"]["limiter"], s["rep"]["stokes"]["iterations"], s["rep"]["ninjected"]))
        assert s["rep"]["tstep"] == r["rep"]["tstep"] and s["rep"]["time"] == r["rep"]["time"], tag + "tstep"
        assert isinstance(r["rep"]["tstep"], float) and isinstance(r["rep"]["ntrac"], int)
        for k in scattered + solved:
            assert np.array_equal(s["fields"][k], r["fields"][k], equal_nan=True), tag + "field " + k
        assert sorted(r["fields"]) == sorted(scattered + solved)
        assert np.array_equal(s["census"], r["census"]), tag + "census"
        so, ro = np.argsort(s["f"][:, TR_ID], kind="stable"), np.argsort(r["f"][:, TR_ID], kind="stable")
        for k in ("x", "f", "v"):
            assert np.array_equal(s[k][so], r[k][ro], equal_nan=True), tag + "tracer " + k
        assert sorted(s["times"]) == sorted(r["times"]) and all(t >= 0 for t in r["times"].values())


def test_fields_before_the_first_solve_are_bitwise_equal(model_a, model_b):
    for staged, resident in (model_a[:2], model_b):
        for k in SCATTERED:
            assert np.array_equal(staged[0]["fields"][k], resident[0]["fields"][k]), k
            assert not np.isnan(resident[0]["fields"][k]).any(), k


def test_sphere_with_refill_equals_staged(model_a):
    staged, resident = model_a[:2]
    _assert_steps_equal(staged, resident, list(SCATTERED), list(SOLVED))
    assert sum(s["rep"]["ninjected"] for s in staged) > 0 and staged[0]["rep"]["nrefilled"] >= 3      # the refill fired inside a step


def test_mantle_with_subgrid_diffusion_equals_staged(model_b):
    staged, resident = model_b
    _assert_steps_equal(staged, resident, list(SCATTERED), list(SOLVED))
    # the walls of T carry the previous solved temperature from step 2 on
    T2, prev = resident[1]["fields"]["T"], resident[0]["fields"]["temp"]
    for d in range(3):
        for w in (0, -1):
            s = [slice(None)] * 3; s[d] = w
            assert np.array_equal(T2[tuple(s)], prev[tuple(s)])
    assert not np.array_equal(T2[1:-1, 1:-1, 1:-1], prev[1:-1, 1:-1, 1:-1])


def test_heat_off_equals_staged(model_c):
    staged, resident = model_c
    _assert_steps_equal(staged, resident, ["rho", "etas", "etan"], ["velz", "velx", "vely", "pres"])
    assert all(s["rep"]["heat"] is None and s["rep"]["limiter"] == "S" for s in resident)


def test_snapshots_are_equal(model_a):
    d = model_a[2]
    for name in ("griddata.%06d.npz" % NSTEP, "tracs.%06d.npz" % NSTEP):
        a, b = np.load(os.path.join(d, "staged", name)), np.load(os.path.join(d, "resident", name))
        assert sorted(a.files) == sorted(b.files)
        for k in a.files:
            assert np.array_equal(a[k], b[k], equal_nan=True), name + " " + k


def test_nothing_grid_sized_crosses_the_bus(model_a):
    """33^3: a node field is 287 KB, the solver's largest scalar read-back 90 KB."""
    from pylamp_amd import pylamp3d as P3
    staged, resident = model_a[:2]
    for it in range(NSTEP):
        print("step %d: staged %s  resident %s" % (it + 1, staged[it]["xfer"], resident[it]["xfer"]))
        assert resident[it]["xfer"]["large"] == 0 and resident[it]["xfer"]["large_bytes"] == 0
        assert resident[it]["xfer"]["small"] > 0 and resident[it]["xfer"]["small_bytes"] < 8 * 33 ** 3 * resident[it]["xfer"]["small"]
        assert staged[it]["xfer"]["large"] > 0                   # the same library, host-staged: the counter counts
    nx, L, x, f = _sphere(33, True)
    sim = P3.Simulation3(nx, L, x, f, P3.Options3(resident=True))
    sim.step()
    sim.transfer_stats(reset=True)
    sim.step()
    assert sim.transfer_stats()["large"] == 0
    sim.field("temp")
    assert sim.transfer_stats()["large"] == 1 and sim.transfer_stats()["large_bytes"] == 8 * 33 ** 3
    sim.field("temp")                            # cached until the next step
    assert sim.transfer_stats(reset=True)["large"] == 1
    sim.close()


def test_advection_velocity_kernel_matches_numpy_bitwise():
    """Random fields, three unequal node counts: every inner value, every ghost plane, edge and corner."""
    from pylamp_amd import pylamp3d as P3, _lib
    rng = np.random.default_rng(5)
    for nx in ([7, 9, 12], [6, 5, 70]):
        grid = [np.linspace(0, 1.0 + d, nx[d]) for d in range(3)]
        ctx = P3.Context3(nx, grid)
        vel = [rng.standard_normal(nx) for _ in range(3)]
        _, ref = P3.advection_velocity(vel, P3.gridmp_of(grid), nx)
        out = [np.full([v + 1 for v in nx], np.nan) for _ in range(3)]
        ctx.check(ctx.lib.pl3_advection_velocity(ctx.handle(), *[_lib.dptr(v) for v in vel], *[_lib.dptr(v) for v in out]))
        for q in range(3):
            assert np.array_equal(out[q], ref[q]), (nx, q)
            assert np.array_equal(np.signbit(out[q]), np.signbit(ref[q])), (nx, q)
            # the order of the walls shows at the corners: the corner (0, 0, 0) is the inner value, negated once per own-axis wall
            assert out[q][0, 0, 0] == -ref[q][1, 1, 1] and out[q][-1, -1, -1] == -ref[q][-2, -2, -2]
        ctx.close()


def test_resident_step_matches_2d_oracle_on_y_invariant_mantle(oracle):
    """The comparison of test_simulation3_step_matches_2d_oracle_on_y_invariant_mantle with resident=True, same bounds:
    temperature < 1e-6, tracer (z, x) < 1e-7 (relative L2), |v_y| <= 1e-6 of the in-plane maximum."""
    from pylamp_amd import pylamp3d as P3
    nx2, L2, ny, Ly, x2, f2, ys, x3, f3 = _mantle3()
    n2 = x2.shape[0]; m = ys.size
    sim = P3.Simulation3(nx2 + [ny], L2 + [Ly], x3, f3, P3.Options3(do_subgrid_heatdiff=False, resident=True))
    rep = sim.step()
    st = dict(nx=nx2, L=L2, grid=[np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])], tr_x=x2.copy(), tr_f=f2.copy())
    out = oracle.step(st, oracle.StepConfig(do_subgrid_heatdiff=False), 1)
    assert rep["stokes"]["converged"] == 1 and rep["heat"]["converged"] == 1, rep
    print("tstep 3-D %.9e  2-D %.9e  limiter %s / %s" % (rep["tstep"], out["tstep"], rep["limiter"], out["limiter"]))
    T = sim.field("temp")
    et = max(relerr(T[:, :, k], out["temp"]) for k in range(ny))
    sx, sf = sim.tracers()
    o = np.argsort(sf[:, TR_ID])
    sx = sx[o].reshape(m, n2, 3)
    ex = max(relerr(sx[c][:, :2], st["tr_x"]) for c in range(m))
    vmax = max(np.abs(out["velz"]).max(), np.abs(out["velx"]).max())
    vy = np.abs(sim.field("vely")).max() / vmax
    tv = sim.tracer_velocity()[o].reshape(m, n2, 3)
    print("temp %.3g  tracer (z,x) %.3g  |vy|/|v| %.3g  tracer |vy| %.3g" % (et, ex, vy, np.abs(tv[:, :, 2]).max() / vmax))
    assert et < 1e-6 and ex < 1e-7
    assert vy <= 1e-6 and np.abs(tv[:, :, 2]).max() <= 1e-6 * vmax
    sim.close()


def test_a_hole_in_the_tracers_raises_and_leaves_the_state():
    from pylamp_amd import pylamp3d as P3
    nx, L, x, f = _sphere(17, False)
    h = L[0] / 16
    hole = np.all(np.abs(x - 8 * h) < h, axis=1)              # the eight cells around node (8, 8, 8)
    x, f = x[~hole], f[~hole]
    sim = P3.Simulation3(nx, L, x, f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, resident=True))
    x0, f0 = sim.tracers(); n0 = sim.count()
    with pytest.raises(Exception, match=r"scattered field 'rho' holds NaN at 1 nodes.*without any marker in reach.*enable injection"):
        sim.step()
    assert sim.it == 0 and sim.count() == n0
    x1, f1 = sim.tracers()
    assert np.array_equal(x0, x1) and np.array_equal(f0, f1)
    msg = sim.ctx.lib.pl3_last_error(sim.ctx.handle()).decode()
    assert "pl3_resident_step" in msg and "'rho'" in msg and " 1 nodes" in msg
    with pytest.raises(Exception, match="no field 'nonsense'.*have: rho, etas, etan"):
        sim.field("nonsense")
    sim.close()


def test_unknown_field_lists_the_names():
    from pylamp_amd import pylamp3d as P3
    nx, L, x, f = _sphere(17, False)
    sim = P3.Simulation3(nx, L, x, f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, resident=True))
    with pytest.raises(Exception, match="no field"):
        sim.field("rho")                         # nothing computed yet
    sim.step()
    with pytest.raises(Exception, match="no field 'viscosity'.*have: rho, etas, etan, velz, velx, vely, pres"):
        sim.field("viscosity")
    with pytest.raises(Exception, match="no field 'temp'"):
        sim.field("temp")                        # heat is off: not computed
    sim.close()


def test_resident_step_is_rejected_on_a_context_with_several_ranks():
    from pylamp_amd import pylamp3d as P3, _lib
    import ctypes as C
    grid = [np.linspace(0, 1, 9)] * 3
    vc = P3.VirtualCluster3([9, 9, 9], grid, 2, 1, 1)
    try:
        ctx = vc.ctxs[0]
        cfg, rep = _lib.Step3Config(), _lib.Step3Report()
        assert ctx.lib.pl3_resident_step(ctx.handle(), C.byref(cfg), 1, C.byref(rep)) != 0
        msg = ctx.lib.pl3_last_error(ctx.handle())
        assert b"pl3_resident_step" in msg and b"one rank" in msg and b"pl3_set_comm" in msg
        out = np.zeros((9, 9, 9))
        assert ctx.lib.pl3_get_field(ctx.handle(), b"rho", _lib.dptr(out)) != 0
        assert b"pl3_get_field" in ctx.lib.pl3_last_error(ctx.handle())
    finally:
        vc.close()
