"""The 3-D yield stress on the GPU (pl3_stokes_set_yield / pl3_stokes_yield_update, pylamp3d.yield_update, Options3.yield_stress) against
the NumPy model tests/stokes3_yield_model.py: the kernel entry by entry, the resident solution, Couette flow, the Picard loop against the
model's, Simulation3 staged against resident, and the rejections.

Bounds.  Per entry B = ((32 mag_e / e + 4) eps) tau_y / (2 e) from the model (its docstring derives it); the inputs of the kernel test
have no entry within B of the switch and yield 10 .. 90 % of their entries (tests/test_yield3_model.py checks both on the CPU), so the
yielded sets must be equal and an unyielded entry is its material value bit for bit.  The change is max |ln(eta_new / eta_prev)|: with
eta_new within B the logarithm moves by B / eta_eff, twice for safety against the second-order term, plus 8 eps for the quotient and the
library logarithm.  The Picard test takes its bound from the model itself: the model loop is rerun three times with every direct solution
perturbed by a seeded random vector of relative size 1e-6 per velocity component (the README's promise for the velocity error of a
solve); twice the largest deviation of the final velocities and effective viscosities from the unperturbed run is the bound, the factor
allowing for the direction the solver's error actually takes."""
import numpy as np
import pytest

import stokes3_yield_model as Y
from test_yield3_model import KINDS, LEN, SHAPES, WALLS, blob, blob_tau0, couette, kernel_case, model_of

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
N_, F_ = 0, 1                                  # NOSLIP, FREESLIP
TR_TMP, TR_HCD, TR_HCP, TR_ALP, TR_IHT, TR_ID = 3, 4, 5, 7, 11, 12


# ---- 1. the kernel against the model ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SHAPES, ids=lambda n: "x".join(str(v) for v in n))
def test_kernel_matches_the_model(n, kind):
    from pylamp_amd import pylamp3d as P3
    rho = np.full(n, 3300.0)
    ctx = None
    try:
        for wall in WALLS:
            c = kernel_case(n, kind, wall)
            ctx = ctx or P3.Context3(n, c["grid"])
            A, _ = P3.makeStokesMatrix(n, c["grid"], c["etas"], c["etan"], rho, bc=c["bc"], ctx=ctx, strict_reference=c["strict"],
                                       wallvel=np.zeros((6, 3)) if c["wallvel"] is None else c["wallvel"],
                                       wallflow=[None] * 6 if c["wallflow"] is None else c["wallflow"],
                                       yield_stress=(c["tau0"], c["dtau_dz"], c["eta_floor"]))
            assert ctx.yield_setting() == (c["tau0"], c["dtau_dz"], c["eta_floor"])
            x = np.stack(c["v"] + [c["P"]], axis=-1).reshape(-1)
            strainrate = P3.strain_fields(A, x)["strainrate"]
            got = P3.yield_update(A, x)
            es, en = P3.coefficients(A)
            ref = model_of(c)
            tag = "%s %s:" % (kind, wall)
            for name, g, r, B, yld, mat in (("etas", es, ref["etas_eff"], ref["B_s"], ref["yielded_s"], c["etas"]),
                                            ("etan", en, ref["etan_eff"], ref["B_n"], ref["yielded_n"], c["etan"])):
                err = np.abs(g.astype(LD) - r)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = np.where(err > 0, err / B, 0)
                print("%s %s worst error / B = %.3f, yielded %d of %d" % (tag, name, float(ratio.max()), int(yld.sum()), yld.size))
                assert np.all(err <= B), (tag, name, float(ratio.max()))
                assert np.array_equal(g[~yld], mat[~yld]), (tag, name)                   # unyielded: the material value, bit for bit
                assert np.array_equal(g < mat, yld), (tag, name)
            assert got["yielded_nodes"] == int(ref["yielded_s"].sum()) and got["yielded_cells"] == int(ref["yielded_n"].sum()), tag
            # the minimum, at the model's arg-min
            both = np.concatenate([ref["etas_eff"].ravel(), ref["etan_eff"].ravel()]); Bb = np.concatenate([ref["B_s"].ravel(), ref["B_n"].ravel()])
            at = int(np.argmin(both))
            assert abs(LD(got["min_eta"]) - both[at]) <= Bb[at], tag
            assert got["min_eta"] == min(es.min(), en.min())
            # the change against the material viscosities
            cells = tuple(slice(0, k - 1) for k in n)
            rel = max(float((ref["B_s"] / ref["etas_eff"]).max()), float((ref["B_n"] / ref["etan_eff"])[cells].max()))
            print("%s change %.17g, model %.17g, allowed %.3e" % (tag, got["change"], ref["change"], 2 * rel + 8 * EPS))
            assert abs(got["change"] - ref["change"]) <= 2 * rel + 8 * EPS, tag
            assert got["max_strainrate_nodes"] == strainrate.max(), tag              # the node invariant IS the strainrate field
            assert abs(LD(got["max_strainrate_cells"]) - ref["e_c"].max()) <= 32 * EPS * float(ref["e_c"].max()) * 4
            # stateless: a second call derives the same arrays from the material ones (its change is against the first call's: 0)
            again = P3.yield_update(A, x)
            es2, en2 = P3.coefficients(A)
            assert np.array_equal(es, es2) and np.array_equal(en, en2) and again["change"] == 0.0, tag
            assert {k: again[k] for k in again if k != "change"} == {k: got[k] for k in got if k != "change"}, tag
            # the ghost entries of etan, and the material arrays
            for a in range(3):
                sl = [slice(None)] * 3; sl[a] = -1
                assert np.array_equal(en[tuple(sl)], c["etan"][tuple(sl)]), (tag, a)
            ms, mn = P3.coefficients(A, material=True)
            assert np.array_equal(ms, c["etas"]) and np.array_equal(mn, c["etan"]), tag
        assert A.ring_sum() == 0.0               # nothing was written outside the nodes
    finally:
        if ctx is not None:
            ctx.close()


# ---- 2. the resident solution -------------------------------------------------------------------------------------------------------------
def test_last_solve_and_given_velocities_agree_bitwise():
    from pylamp_amd import pylamp3d as P3
    n = [17, 13, 21]
    grid, etas, etan, rho = blob(n, LEN)
    bc = [N_, F_, F_, N_, F_, F_]
    ctx = P3.Context3(n, grid)
    try:
        A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=bc, ctx=ctx, yield_stress=(1e6, 0.0, 1e19))
        x = P3.solve(A)
        assert A.last_stats["converged"] == 1
        dev = P3.yield_update(A)
        dev_c = P3.coefficients(A)
        assert dev["yielded_nodes"] > 0 and dev["yielded_cells"] > 0 and dev["change"] > 0
        A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=bc, ctx=ctx)             # fresh coefficients: both are the material ones again
        assert all(np.array_equal(a, b) for a, b in zip(P3.coefficients(A), (etas, etan)))
        host = P3.yield_update(A, x)
        host_c = P3.coefficients(A)
        assert dev == host
        assert np.array_equal(dev_c[0], host_c[0]) and np.array_equal(dev_c[1], host_c[1])
    finally:
        ctx.close()


# ---- 3. Couette -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("strict", [False, True])
def test_couette_flow_carries_the_yield_stress(strict):
    """The lid z0 dragged along x over a uniform fluid, gravity off (the x walls carry the linear profile as a flow through them: a closed
    box would make it a cavity flow): e = U / (2 Lz) everywhere, so with tau_y below 2 eta e everything yields to tau_y / (2 e), the
    velocities stay what they are and the stress is tau_y.  The loop's tolerance 1e-4: a velocity error of 1e-6 U over a cell of Lz / 8
    moves a strain rate by up to 2 x 8 x 1e-6 of U / Lz."""
    from pylamp_amd import pylamp3d as P3
    n, L, U, eta0 = [9, 9, 9], [1.0e5, 1.0e5, 1.0e5], 1e-9, 1e21
    c = couette(n, L, U, eta0)
    tau = 0.5 * 2 * eta0 * U / (2 * L[0])
    A, _ = P3.makeStokesMatrix(n, c["grid"], c["eta"], c["eta"], c["rho"], bc=c["bc"], grav=[0.0, 0.0, 0.0], strict_reference=strict,
                               wallvel=c["wallvel"], wallflow=c["wallflow"], yield_stress=(tau, 0.0, 1e15))
    try:
        P3.solve(A)
        assert A.last_stats["converged"] == 1
        rep = P3.picard_loop(A, 3, 1e-4)
        print("Couette, strict %s: %s" % (strict, rep))
        assert rep["converged"] and rep["iterations"] <= 3
        assert rep["yielded_nodes"][-1] == 9 ** 3 and rep["yielded_cells"][-1] == 8 ** 3
        stress = P3.strain_fields(A)["stress"]
        worst_s = float(np.abs(stress - tau).max() / tau)
        vx = P3.x2vp(P3.solution(A), n)[0][1]
        worst_v = float(np.abs(vx - c["v"][1])[:-1, :, :-1].max() / U)
        print("Couette, strict %s: stress off tau_y by %.3e, profile off linear by %.3e of U" % (strict, worst_s, worst_v))
        assert worst_s <= 1e-6 and worst_v <= 1e-6
        es, en = P3.coefficients(A)
        assert abs(es - 0.5 * eta0).max() <= 1e-4 * eta0 and abs(en[:-1, :-1, :-1] - 0.5 * eta0).max() <= 1e-4 * eta0
    finally:
        A._ctx.close()


# ---- 4. the Picard loop against the model's ---------------------------------------------------------------------------------------------
def test_picard_loop_matches_the_model():
    """GPU deviation / bound, printed below and recorded in DESIGN.md 6c.  Measured on MI355X: velocities 4.9e-9 of a bound of 3.3e-6
    (ratio 0.0015), ln(eta_eff) 6.9e-8 of 2.2e-4 (ratio 0.0003)."""
    from pylamp_amd import pylamp3d as P3
    n = [17, 13, 21]
    grid, etas, etan, rho = blob(n, LEN)
    bc = [N_, F_, F_, N_, F_, F_]
    floor, its = 1e19, 3
    tau0, first = blob_tau0(n, grid, etas, etan, rho, bc)
    ref = Y.picard(n, grid, etas, etan, rho, tau0, 0.0, floor, its, tol=0.0, bc=bc, reuse=[first])
    solvers = [first] + ref["solvers"]

    def deviation(x, es, en):
        v0 = ref["x"].reshape(n + [4])[..., :3]
        v = np.asarray(x).reshape(n + [4])[..., :3]
        cells = tuple(slice(0, k - 1) for k in n)
        return (float(np.abs(v - v0).max() / np.abs(v0).max()),
                max(float(np.abs(np.log(es / ref["etas_eff"])).max()), float(np.abs(np.log(en / ref["etan_eff"]))[cells].max())))

    bound_v = bound_e = 0.0
    for seed in range(3):
        rng = np.random.default_rng(100 + seed)

        def perturb(x):
            X = x.reshape(n + [4]).copy()
            for q in range(3):
                X[..., q] += 1e-6 * np.abs(X[..., q]).max() * rng.uniform(-1.0, 1.0, n)
            return X.reshape(-1)
        o = Y.picard(n, grid, etas, etan, rho, tau0, 0.0, floor, its, tol=0.0, bc=bc, reuse=solvers, perturb=perturb)
        dv, de = deviation(o["x"], o["etas_eff"], o["etan_eff"])
        bound_v, bound_e = max(bound_v, 2 * dv), max(bound_e, 2 * de)
    A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=bc, yield_stress=(tau0, 0.0, floor))
    try:
        P3.solve(A)
        rep = P3.picard_loop(A, its, 0.0)
        es, en = P3.coefficients(A)
        dv, de = deviation(P3.solution(A), es, en)
    finally:
        A._ctx.close()
    print("Picard, model: change %s, yielded nodes %s" % (ref["change"], ref["yielded_nodes"]))
    print("Picard, GPU:   change %s, yielded nodes %s, Stokes iterations %s" % (rep["change"], rep["yielded_nodes"], rep["stokes_iterations"]))
    print("Picard: velocity deviation %.3e of bound %.3e (ratio %.4f); ln(eta_eff) deviation %.3e of bound %.3e (ratio %.4f)"
          % (dv, bound_v, dv / bound_v, de, bound_e, de / bound_e))
    assert rep["iterations"] == its and not rep["converged"]
    assert dv <= bound_v and de <= bound_e


# ---- 5. Simulation3 ---------------------------------------------------------------------------------------------------------------------
NSTEP = 3
BITE = dict(yield_stress=2e6, picard_maxit=3, picard_tol=1e-3)


def _sphere17():
    from pylamp_amd import pylamp3d as P3
    nx = [17, 17, 17]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))
    z, x, y = (tr_x[:, d] / L[d] for d in range(3))
    tr_f[:, TR_TMP] = 273 + 1350 * z + 40 * np.sin(2 * np.pi * x) * np.sin(np.pi * z) * np.cos(2 * np.pi * y)
    tr_f[:, TR_HCD] = 4.0; tr_f[:, TR_HCP] = 1250.0; tr_f[:, TR_ALP] = 3.5e-5; tr_f[:, TR_IHT] = 1e-9
    return nx, L, tr_x, tr_f


def _run(resident, **kw):
    from pylamp_amd import pylamp3d as P3
    nx, L, tr_x, tr_f = _sphere17()
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(resident=resident, **kw))
    names = ["rho", "etas", "etan", "cp", "T", "H", "mat", "kz", "kx", "ky", "velz", "velx", "vely", "pres", "temp"]
    if kw.get("yield_stress") is not None:
        names += ["etas_eff", "etan_eff"]
    steps = []
    try:
        for _ in range(NSTEP):
            rep = sim.step()
            x, f = sim.tracers()
            steps.append(dict(rep=rep, fields={k: sim.field(k).copy() for k in names}, x=x, f=f))
    finally:
        sim.close()
    return steps


@pytest.fixture(scope="module")
def runs():
    return dict(staged=_run(False, **BITE), resident=_run(True, **BITE), plain=_run(True), high=_run(True, yield_stress=1e30, picard_maxit=3, picard_tol=1e-3),
                defaults=_run(True, yield_stress=None, yield_eta_floor=None, picard_maxit=10, picard_tol=1e-2),
                warm=_run(True, stokes_warm_start=True, **BITE))


def _same(a, b, skip=()):
    """Every step: the fields that both runs have, the tracers and the time step, array for array."""
    for it, (s, r) in enumerate(zip(a, b)):
        for k in s["fields"]:
            if k in r["fields"] and k not in skip:
                assert np.array_equal(s["fields"][k], r["fields"][k]), (it + 1, k)
        so, ro = np.argsort(s["f"][:, TR_ID], kind="stable"), np.argsort(r["f"][:, TR_ID], kind="stable")
        assert np.array_equal(s["x"][so], r["x"][ro]) and np.array_equal(s["f"][so], r["f"][ro], equal_nan=True), it + 1
        assert s["rep"]["tstep"] == r["rep"]["tstep"], it + 1


def test_staged_and_resident_agree_bitwise(runs):
    a, b = runs["staged"], runs["resident"]
    _same(a, b)
    for s, r in zip(a, b):
        assert list(s["rep"]) == list(r["rep"]) and sorted(s["fields"]) == sorted(r["fields"])
        assert s["rep"]["picard"] == r["rep"]["picard"]
        for k in ("iterations", "rel_residual"):
            assert s["rep"]["heat"][k] == r["rep"]["heat"][k] and s["rep"]["stokes"][k] == r["rep"]["stokes"][k]


def test_a_yield_stress_out_of_reach_changes_nothing(runs):
    _same(runs["plain"], runs["high"])
    for s, r in zip(runs["plain"], runs["high"]):
        assert "picard" not in s["rep"]
        p = r["rep"]["picard"]
        assert p["iterations"] == 1 and p["converged"] and p["change"] == [0.0] and p["yielded_nodes"] == [0] and p["yielded_cells"] == [0]
        assert p["stokes_iterations"] == [r["rep"]["stokes"]["iterations"]]
        assert {k: v for k, v in r["rep"].items() if k not in ("picard", "stokes", "heat")} == {k: v for k, v in s["rep"].items() if k not in ("stokes", "heat")}
        for k in ("iterations", "rel_residual", "converged"):
            assert s["rep"]["stokes"][k] == r["rep"]["stokes"][k] and s["rep"]["heat"][k] == r["rep"]["heat"][k]
        assert np.array_equal(r["fields"]["etas_eff"], r["fields"]["etas"]) and np.array_equal(r["fields"]["etan_eff"], r["fields"]["etan"])


def test_the_option_unset_is_every_new_option_at_its_default(runs):
    _same(runs["plain"], runs["defaults"])
    for s, r in zip(runs["plain"], runs["defaults"]):
        assert list(s["rep"]) == list(r["rep"]) and "picard" not in r["rep"] and sorted(s["fields"]) == sorted(r["fields"])


def test_a_yield_stress_that_bites(runs):
    for it, s in enumerate(runs["resident"]):
        p, f = s["rep"]["picard"], s["fields"]
        print("step %d: Picard %s; Stokes %d iterations" % (it + 1, p, s["rep"]["stokes"]["iterations"]))
        assert p["yielded_nodes"][0] > 0 and 1 <= p["iterations"] <= 3
        assert len(p["change"]) == len(p["yielded_nodes"]) == len(p["yielded_cells"]) == len(p["stokes_iterations"]) == p["iterations"]
        assert np.all(f["etas_eff"] <= f["etas"]) and np.any(f["etas_eff"] < f["etas"])
        assert np.all(f["etan_eff"] <= f["etan"]) and np.any(f["etan_eff"] < f["etan"])
        assert np.all(f["etas_eff"] >= 1e17)                                         # yield_eta_floor = None: Options3.etamin
        assert all(np.all(np.isfinite(a)) for a in f.values())
    assert any(not np.array_equal(a["fields"]["velz"], b["fields"]["velz"]) for a, b in zip(runs["resident"], runs["plain"]))


def test_a_yield_stress_with_the_warm_start(runs):
    for s in runs["warm"]:
        p = s["rep"]["picard"]
        assert s["rep"]["stokes"]["converged"] == 1 and "stokes_start" in s["rep"] and p["iterations"] >= 1 and p["yielded_nodes"][0] > 0
        assert np.isfinite(s["rep"]["tstep"]) and all(np.all(np.isfinite(a)) for a in s["fields"].values())
        assert np.all(np.isfinite(s["x"])) and np.all(np.isfinite(p["change"]))


# ---- 6. rejections, each by its name --------------------------------------------------------------------------------------------------------
def test_rejections():
    from pylamp_amd import _lib, pylamp3d as P3
    nx, L, tr_x, tr_f = _sphere17()
    for bad in (0, 33, 2.5, True):
        with pytest.raises(Exception, match="Simulation3: Options3.picard_maxit = .* must be an integer 1 .. 32"):
            P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(yield_stress=1e6, picard_maxit=bad))
    with pytest.raises(Exception, match="Simulation3: Options3.picard_tol = -1e-06 must be >= 0"):
        P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(yield_stress=1e6, picard_tol=-1e-6))
    with pytest.raises(Exception, match="Options3.yield_stress: expected None, a yield stress tau0 .* or a pair"):
        P3.Options3(yield_stress=(1e6, 0.0, 1e19))
    with pytest.raises(Exception, match="pl3_stokes_set_yield: eta_floor = -1 must be positive"):
        P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(yield_stress=1e6, yield_eta_floor=-1.0))
    n = [9, 9, 9]
    grid = [np.linspace(0, 1e5, 9)] * 3
    one = np.ones(n)
    ctx = P3.Context3(n, grid)
    try:
        assert ctx.yield_setting() is None
        with pytest.raises(Exception, match="pl3_stokes_set_yield: the yield stress tau_y = .* must be positive throughout the box, got 1000000 at z\\[0\\] and -1000000 at"):
            ctx.set_yield(1e6, -2e6 / 1e5, 1e19)
        with pytest.raises(Exception, match="pl3_stokes_set_yield: the yield stress tau_y = .* must be positive"):
            ctx.set_yield(0.0, 0.0, 1e19)
        with pytest.raises(Exception, match="pl3_stokes_set_yield: eta_floor = 0 must be positive"):
            ctx.set_yield(1e6, 0.0, 0.0)
        for bad in ((np.nan, 0.0, 1e19), (1e6, np.inf, 1e19), (1e6, 0.0, np.inf)):
            with pytest.raises(Exception, match="pl3_stokes_set_yield: .* must all be finite"):
                ctx.set_yield(*bad)
        assert ctx.yield_setting() is None                                  # a rejected call changes nothing
        with pytest.raises(Exception, match="pl3_step_set_picard: maxit = 0 must be 1 .. 32"):
            ctx.set_picard(0, 1e-2)
        with pytest.raises(Exception, match="pl3_step_set_picard: maxit = 33 must be 1 .. 32"):
            ctx.set_picard(33, 1e-2)
        with pytest.raises(Exception, match="pl3_step_set_picard: tol = -.* must be >= 0"):
            ctx.set_picard(3, -1e-3)
        ctx.set_picard(32, 0.0)
        assert ctx.picard_report()["iterations"] == 0
        o = np.zeros(6)
        assert ctx.lib.pl3_stokes_yield_update(ctx.handle(), None, None, None, _lib.dptr(o)) != 0
        assert b"pl3_stokes_yield_update: no Stokes coefficients set" in ctx.lib.pl3_last_error(ctx.handle())
        A, _ = P3.makeStokesMatrix(n, grid, one, one, one, ctx=ctx)
        with pytest.raises(Exception, match="pl3_stokes_yield_update: no yield stress set"):
            P3.yield_update(A, np.zeros(4 * 9 ** 3))
        ctx.set_yield(1e6, 10.0, 1e19)
        assert ctx.yield_setting() == (1e6, 10.0, 1e19)
        with pytest.raises(Exception, match="pl3_stokes_yield_update: NULL velocities .*no solve has run"):
            P3.yield_update(A)
        assert ctx.lib.pl3_stokes_yield_update(ctx.handle(), _lib.dptr(one), None, None, _lib.dptr(o)) != 0
        assert b"all three or all NULL" in ctx.lib.pl3_last_error(ctx.handle())
        with pytest.raises(Exception, match="picard_loop: picard_maxit = 0 must be an integer 1 .. 32"):
            P3.picard_loop(A, 0, 1e-2)
        with pytest.raises(Exception, match="picard_loop: picard_tol = -1 must be >= 0"):
            P3.picard_loop(A, 3, -1)
        rest = P3.yield_update(A, np.zeros(4 * 9 ** 3))                      # a fluid at rest: nothing yields
        assert rest["change"] == 0.0 and rest["yielded_nodes"] == 0 and rest["yielded_cells"] == 0 and rest["min_eta"] == 1.0
        ctx.set_yield(None)
        assert ctx.yield_setting() is None
    finally:
        ctx.close()
    vc = P3.VirtualCluster3(n, grid, 2, 1, 1)
    try:
        c0 = vc.ctxs[0]
        with pytest.raises(Exception, match="pl3_stokes_set_yield: the yield stress runs on one rank .*pl3_set_comm"):
            c0.set_yield(1e6, 0.0, 1e19)
    finally:
        vc.close()
