"""The opt-in warm start of the 3-D Stokes solve (pl3_stokes_set_warm_start): the extrapolated start vector against Lagrange
weights derived here, the guard that falls back to the cold solve bit for bit, the accuracy of warm solves against the direct solve
of the independent model (tests/stokes3_model.py), and the errors by name.  [17, 13, 21], falling-sphere coefficients."""
import numpy as np
import pytest

import stokes3_model as M

pytestmark = pytest.mark.gpu

NX = [17, 13, 21]
L = [100e3, 100e3, 100e3]
TR_TMP, TR_HCD, TR_HCP, TR_ALP, TR_IHT = 3, 4, 5, 7, 11
COUNTERS = ("iterations", "converged", "operator_applies", "precond_applies", "rel_residual", "error_estimate", "used_direct")


def _tracers(heat):
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = P3.falling_sphere_tracers(NX, L, np.random.default_rng(7))
    if heat:
        z, x, y = (tr_x[:, d] / L[d] for d in range(3))
        tr_f[:, TR_TMP] = 273 + 1350 * z + 40 * np.sin(2 * np.pi * x) * np.sin(np.pi * z) * np.cos(2 * np.pi * y)
        tr_f[:, TR_HCD] = 4.0; tr_f[:, TR_HCP] = 1250.0; tr_f[:, TR_ALP] = 3.5e-5; tr_f[:, TR_IHT] = 1e-9
    return tr_x, tr_f


@pytest.fixture(scope="module")
def coeffs():
    """rho, etas (nodes) and etan (cell centres) of the falling sphere, scattered once."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _tracers(False)
    sim = P3.Simulation3(NX, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False))
    f = sim.scatter_fields()
    grid = [g.copy() for g in sim.grid]
    sim.close()
    assert not any(np.isnan(f[k]).any() for k in ("rho", "etas", "etan"))
    return dict(grid=grid, rho=f["rho"], etas=f["etas"], etan=f["etan"])


def _perturbed(c, k):
    """The density with the k.th of a family of smooth perturbations of 0.3 % (k = 0: none)."""
    z, x, y = np.meshgrid(*[g / g[-1] for g in c["grid"]], indexing="ij")
    return c["rho"] * (1.0 + 3e-3 * np.sin(k * np.pi * z) * np.cos((k + 1) * np.pi * x) * np.cos(k * np.pi * y))


def _solve(P3, ctx, c, rho, grav=None):
    A, _ = P3.makeStokesMatrix(NX, c["grid"], c["etas"], c["etan"], rho, grav=grav, ctx=ctx)
    assert P3.solve(A, resident=True) is None
    assert A.last_stats["converged"] == 1, A.last_stats
    return P3.solution(A), A.last_stats


def lagrange(times, target):
    """Values at `target` of the Lagrange basis polynomials on the nodes `times`."""
    t = np.asarray(times, dtype=np.longdouble)
    return [np.prod([(np.longdouble(target) - t[j]) / (t[i] - t[j]) for j in range(t.size) if j != i]) for i in range(t.size)]


def _check_start(got, weights, levels, what):
    ld = np.longdouble
    terms = [ld(w) * x.astype(ld) for w, x in zip(weights, levels)]
    ref = sum(terms)
    bound = 8 * np.finfo(np.float64).eps * sum(np.abs(t) for t in terms)
    err = np.abs(got.astype(ld) - ref)
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))))
    print("%s: weights %s, worst error / bound %.3f" % (what, [float(w) for w in weights], worst))
    assert np.all(err <= bound), what


def test_start_vector_is_the_lagrange_extrapolation(coeffs):
    """Solves at model times 0, 1 and 1.5 (commits with dt = 1, then 0.5), the next one 0.25 later: the start vector is x_0 with one
    level, 1.5 x_1 - 0.5 x_0 with two (1 + c, -c with c = min(2, dt0 / dt1) = 0.5) and the quadratic through the three with three,
    each within 8 eps sum |L_k x_k| (three products, two sums) of the Lagrange combination formed here in longdouble.  A time step
    that tripled takes c = 2.  The rings of the work vectors stay zero through warm solves."""
    from pylamp_amd import pylamp3d as P3
    ctx = P3.Context3(NX, coeffs["grid"])
    try:
        ctx.set_warm_start(3, 2)
        assert ctx.warm_start() == (3, 2)
        A = P3.StokesOperator3
        x0, _ = _solve(P3, ctx, coeffs, _perturbed(coeffs, 0))
        info = ctx.history_info()
        assert info["held"] == 0 and info["start"] == "cold" and info["used"] == 0
        ctx.commit_solution(1.0)
        assert ctx.history_info()["held"] == 1
        assert np.array_equal(ctx.start_vector(), x0)                         # one level: the solution itself
        x1, _ = _solve(P3, ctx, coeffs, _perturbed(coeffs, 1))
        info = ctx.history_info()
        assert info["start"] in ("warm", "rejected") and info["used"] == 1 and info["weights"] == [1.0, 0.0, 0.0], info
        ctx.commit_solution(0.5)
        w2 = lagrange([1.0, 0.0], 1.5)
        assert [float(w) for w in w2] == [1.5, -0.5]
        _check_start(ctx.start_vector(), w2, [x1, x0], "two levels")
        x2, _ = _solve(P3, ctx, coeffs, _perturbed(coeffs, 2))
        info = ctx.history_info()
        assert info["used"] == 2 and info["weights"] == [1.5, -0.5, 0.0], info   # (1 + c, -c), c = min(2, 0.5 / 1)
        ctx.commit_solution(0.25)
        assert ctx.history_info()["held"] == 3
        w3 = lagrange([1.5, 1.0, 0.0], 1.75)
        _check_start(ctx.start_vector(), w3, [x2, x1, x0], "three levels")
        x3, _ = _solve(P3, ctx, coeffs, _perturbed(coeffs, 3))
        info = ctx.history_info()
        print("three levels: solve started %s, |r0| %.3e, ref %.3e, weights %s" % (info["start"], info["r0"], info["ref"], info["weights"]))
        assert info["used"] == 3 and info["start"] in ("warm", "rejected")
        assert np.allclose(info["weights"], [float(w) for w in w3], rtol=1e-12, atol=0)
        assert (info["start"] == "warm") == (info["r0"] < info["ref"])
        assert A(ctx).ring_sum() == 0.0
        # a time step that tripled: the linear formula with its weight capped at 2, on two fresh levels
        ctx.clear_history()
        assert ctx.history_info()["held"] == 0
        ctx.commit_solution(1.0)
        x4, _ = _solve(P3, ctx, coeffs, _perturbed(coeffs, 4))
        ctx.commit_solution(3.0)
        _check_start(ctx.start_vector(), [3.0, -2.0], [x4, x3], "capped")
        assert A(ctx).ring_sum() == 0.0
        ctx.set_warm_start(0)
        assert ctx.warm_start() == (0, 0) and ctx.history_info()["held"] == 0
        ctx.commit_solution(1.0)                                               # off: nothing happens
        assert ctx.history_info()["held"] == 0
    finally:
        ctx.close()


def test_guard_falls_back_to_the_cold_solve_bit_for_bit(coeffs):
    """Solve, commit, then the same coefficients under reversed gravity: the kept solution answers the opposite load, so its
    residual is about twice |b| and cannot be below the hydrostatic reference.  The solve reports the rejection with both numbers,
    and its solution and counters are those of the same two solves on a context without warm start."""
    from pylamp_amd import pylamp3d as P3
    out = {}
    for warm in (True, False):
        ctx = P3.Context3(NX, coeffs["grid"])
        try:
            if warm:
                ctx.set_warm_start(3, 2)
            _solve(P3, ctx, coeffs, coeffs["rho"])
            ctx.commit_solution(1.0)
            out[warm] = _solve(P3, ctx, coeffs, coeffs["rho"], grav=(-9.81, 0.0, 0.0)) + (ctx.history_info(),)
        finally:
            ctx.close()
    info = out[True][2]
    print("guard: start %s, |r0| %.6e, ref %.6e" % (info["start"], info["r0"], info["ref"]))
    assert info["start"] == "rejected" and info["used"] == 1 and info["held"] == 1
    assert info["ref"] > 0 and info["r0"] >= info["ref"]
    assert out[False][2]["start"] == "cold" and out[False][2]["held"] == 0
    assert np.array_equal(out[True][0], out[False][0])
    for k in COUNTERS:
        assert out[True][1][k] == out[False][1][k], k


def _velocity_error(sim):
    """Relative L2 error of the velocities of sim's last step against the direct solve of the model's system for sim.fields."""
    f = sim.fields
    ap = lambda x, rounded=True: M.stokes_apply(NX, sim.grid, f["etas"], f["etan"], x, strict=True, rounded=rounded)
    xr = M.direct_solve(M.assemble(ap, NX), ap, M.stokes_rhs(NX, sim.grid, f["etas"], f["etan"], f["rho"], strict=True))
    R = xr.reshape(NX + [4])[..., :3]
    V = np.stack([f["velz"], f["velx"], f["vely"]], axis=-1)
    return float(np.sqrt(np.sum((V - R) ** 2) / np.sum(R ** 2)))


@pytest.fixture(scope="module")
def six_steps():
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _tracers(True)
    runs = {}
    for warm in (True, False):
        sim = P3.Simulation3(NX, L, tr_x.copy(), tr_f.copy(), P3.Options3(stokes_warm_start=warm))
        reps, errs = [], {}
        for it in range(1, 7):
            reps.append(sim.step())
            if it in (3, 6):
                errs[it] = _velocity_error(sim)
        sim.close()
        runs[warm] = (reps, errs)
    return runs


def test_warm_steps_are_as_accurate_and_take_fewer_iterations(six_steps):
    """Six steps of the sphere with heat on, warm start on and off on the same tracers.  After steps 3 and 6 the velocities are
    within 1e-6 (relative L2; the bound of the README's "Accuracy" row) of the direct solve of the model's system rebuilt from that
    step's fields -- warm, and cold as the control.  Steps 2 .. 6 start warm, the cold run carries no stokes_start key, and the
    iterations summed over steps 3 .. 6 are strictly fewer warm than cold.
    Measured on MI355X: velocity error after step 3 warm 3.7e-8, cold 1.6e-8; after step 6 warm 2.9e-8, cold 4.0e-8; iterations per
    step warm 43, 47, 44, 34, 33, 33, cold 43, 47, 57, 50, 54, 43; summed over steps 3 .. 6: warm 144, cold 204."""
    (wr, we), (cr, ce) = six_steps[True], six_steps[False]
    for it in (3, 6):
        print("step %d: velocity error warm %.3e cold %.3e" % (it, we[it], ce[it]))
    print("starts:", [r["stokes_start"] for r in wr])
    print("iterations warm %s cold %s" % ([r["stokes"]["iterations"] for r in wr], [r["stokes"]["iterations"] for r in cr]))
    nw, nc = (sum(r["stokes"]["iterations"] for r in reps[2:]) for reps in (wr, cr))
    print("iterations over steps 3 .. 6: warm %d cold %d" % (nw, nc))
    for it in (3, 6):
        assert we[it] <= 1e-6 and ce[it] <= 1e-6, (it, we[it], ce[it])
    assert all(r["stokes"]["converged"] == 1 for r in wr + cr)
    assert [r["stokes_start"] for r in wr] == ["cold"] + ["warm"] * 5
    assert all("stokes_start" not in r for r in cr)
    assert nw < nc, (nw, nc)


def test_reset_and_upload_clear_the_history():
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _tracers(False)
    sim = P3.Simulation3(NX, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, stokes_warm_start=(4, 3)))
    try:
        assert sim.ctx.warm_start() == (4, 3)
        assert sim.step()["stokes_start"] == "cold" and sim.ctx.history_info()["held"] == 1
        sim.reset_stokes_history()
        assert sim.ctx.history_info()["held"] == 0
        assert sim.step()["stokes_start"] == "cold" and sim.ctx.history_info()["held"] == 1
        sim.upload(tr_x, tr_f)
        assert sim.ctx.history_info()["held"] == 0
        # a wall that changes its kind clears it, a wall velocity does not
        sim.step()
        sim.ctx.set_wall_velocity(None)
        assert sim.ctx.history_info()["held"] == 1
        sim.ctx.set_stokes_walls([P3.BC_TYPE_NOSLIP] + [P3.BC_TYPE_FREESLIP] * 5)
        assert sim.ctx.history_info()["held"] == 0
    finally:
        sim.close()


def test_errors_name_the_argument(coeffs):
    from pylamp_amd import pylamp3d as P3
    ctx = P3.Context3(NX, coeffs["grid"])
    try:
        for points, order, word in ((1, 1, "points = 1"), (7, 2, "points = 7"), (-1, 1, "points = -1"), (3, 0, "order = 0"),
                                    (5, 4, "order = 4"), (2, 2, "order = 2 needs points >= 3"), (3, 3, "order = 3 needs points >= 4")):
            with pytest.raises(Exception, match="pl3_stokes_set_warm_start: .*" + word):
                ctx.set_warm_start(points, order)
        assert ctx.warm_start() == (0, 0)
        with pytest.raises(Exception, match="pl3_stokes_start_vector: warm start is off"):
            ctx.start_vector()
        ctx.set_warm_start(6, 3)
        with pytest.raises(Exception, match="pl3_stokes_history_commit: no Stokes solution"):
            ctx.commit_solution(1.0)
        with pytest.raises(Exception, match="pl3_stokes_start_vector: the history is empty"):
            ctx.start_vector()
        for dt in (0.0, -1.0, float("nan")):
            with pytest.raises(Exception, match="pl3_stokes_history_commit: dt = "):
                ctx.commit_solution(dt)
    finally:
        ctx.close()
    grid = [np.linspace(0, 1, 9)] * 3
    vc = P3.VirtualCluster3([9, 9, 9], grid, 2, 1, 1)
    try:
        with pytest.raises(Exception, match="pl3_stokes_set_warm_start: .*pl3_set_comm"):
            vc.ctxs[0].set_warm_start(3, 2)
    finally:
        vc.close()
