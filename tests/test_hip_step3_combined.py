"""The 3-D step with every opt-in feature switched on together (rectilinear grid with the marker search, fence-off deletion, flow through
the walls, inflow material, a moving no-slip lid, heat-wall profiles with the budget, classical RK4, the warm start, strain fields, shear
heating and the yield stress with its Picard loop) on the GPU: the staged Simulation3.step() against the resident one bit for bit, and every
stage of every resident step against tests/step3_stage_model.py, which holds the order of a step and takes the arithmetic of each stage
from the existing NumPy models.  The cases K1 and K2 and the CPU checks of their inputs are in tests/test_step3_stage_model.py.

Every stage model is fed with the device's own inputs (the tracers downloaded before the step, the fields and the time step the device
reports), so no discrete decision of an earlier stage can flip the comparison of a later one.  The end positions of the tracers the step
deleted cannot be downloaded; for those rows the deletion model takes the model's end positions, which the CPU checks keep 1e-9 L away from
every wall and face, five decades above the position bar.

Bars.  None is invented here; each is the bar of the single-feature GPU test that compares the same quantity with the same model:
  scatter            maxrel < 1e-12 (arithmetic schemes), < 1e-11 (geometric)                     tests/test_hip_mic3_rect.py
  gather             maxrel < 1e-13 (absolute), < 1e-12 (increment with subgrid diffusion)        tests/test_hip_mic3_rect.py
  strain fields      32 eps x the model's magnitude per entry; the total (36 + sqrt(N)) eps x the summed magnitude   tests/test_hip_3d_strain.py
  heat solve         relerr < 1e-6                                           tests/test_hip_3d_heatwalls.py, tests/test_hip_3d_model.py
  heat budget        each output within 1e-12 of the sum of |terms|; normalised imbalance <= 1e-10 in a step         tests/test_hip_3d_heatwalls.py
  RK4                positions maxrel < 1e-14, velocities maxrel < 1e-9                           tests/test_hip_3d_flow.py
  refill             new positions within 4 x 2^-52 L, every column of a new tracer bit for bit   tests/test_hip_mic3_rect.py, tests/test_hip_mic3_inflow.py
  Picard             twice the largest deviation of the model's own loop under three perturbations of 1e-6 of its intermediate
                     solutions (the recipe of test_picard_loop_matches_the_model in tests/test_hip_3d_yield.py), per case and step
  tstep, limiter, counters, IDs   equal
Every test prints the largest ratio of deviation to bar that it saw.

The dissipation in the heat budget.  pl3_heat_budget sums H over the control volumes of the INTERIOR nodes, dissipation_total over the whole
box (the wall nodes' half volumes included), so source - sum(scattered H) is dissipation_total minus the wall nodes' share; the test adds
that share from the device's own dissipation field and holds the sum to the reduction bound of tests/test_hip_3d_strain.py.
"""
import numpy as np
import pytest

from conftest import maxrel, relerr
import step3_stage_model as G
import stokes3_yield_model as Y
import test_step3_stage_model as K
from test_hip_step3_resident import _assert_steps_equal

pytestmark = pytest.mark.gpu

LD = np.longdouble
EPS = np.finfo(np.float64).eps
TR_TMP, TR_ID = G.TR_TMP, G.TR_ID
SOLVED = ("velz", "velx", "vely", "pres", "temp", "strainrate", "stress", "dissipation", "etas_eff", "etan_eff")
VEL = ("velz", "velx", "vely")
STEP_CONSERVATION_BOUND = 1e-10                # tests/test_hip_3d_heatwalls.py


def _run(c, resident, warm=True):
    """Every step of a run; held / start: the levels of the warm start's history before the step and the start vector its first solve
    will form (None without a level)."""
    from pylamp_amd import pylamp3d as P3
    sim = P3.Simulation3(c["nx"], c["L"], c["tr_x"], c["tr_f"], P3.Options3(resident=resident, **dict(c["options"], stokes_warm_start=warm)),
                         grid=c["grid"])
    steps = []
    try:
        for it in range(1, c["nsteps"] + 1):
            K.apply_setters(sim, c, it)
            x0, f0 = sim.tracers()
            held = sim.ctx.history_info()["held"]
            start = sim.ctx.start_vector() if held > 0 else None
            rep = sim.step()
            x, f = sim.tracers()
            steps.append(dict(rep=rep, x0=x0, f0=f0, x=x, f=f, v=sim.tracer_velocity(), census=sim.census(), times=sim.stage_times(), held=held, start=start,
                              fields={k: sim.field(k).copy() for k in G.SCATTERED + SOLVED}, budget=sim.heat_budget()))
    finally:
        sim.close()
    return steps


def _stages(c, steps):
    """The stage model of every step of a run, each stage fed with the run's own inputs."""
    n = c["nx"]
    cells = tuple(slice(0, k - 1) for k in n)
    out = []
    for it, d in enumerate(steps, start=1):
        s, F = K.settings_of(c, it), d["fields"]
        m = dict(s=s)
        m["fields"], fu = G.scatter(s, d["x0"], d["f0"], steps[it - 2]["fields"]["temp"] if it > 1 else None)
        # Stokes + Picard from the device's scattered fields, and the bound from the model's own sensitivity
        st = G.stokes(s, F["rho"], F["etas"], F["etan"])
        v0 = np.stack([st[k] for k in VEL], axis=-1)
        bound_v = bound_e = 0.0
        for seed in range(3):
            rng = np.random.default_rng(100 + seed)

            def perturb(x):
                X = x.reshape(n + [4]).copy()
                for q in range(3):
                    X[..., q] += 1e-6 * np.abs(X[..., q]).max() * rng.uniform(-1.0, 1.0, n)
                return X.reshape(-1)
            o = G.stokes(s, F["rho"], F["etas"], F["etan"], perturb=perturb, reuse=st["picard"]["solvers"])
            dv = float(np.abs(np.stack([o[k] for k in VEL], axis=-1) - v0).max() / np.abs(v0).max())
            de = max(float(np.abs(np.log(o["etas_eff"] / st["etas_eff"])).max()), float(np.abs(np.log(o["etan_eff"] / st["etan_eff"]))[cells].max()))
            bound_v, bound_e = max(bound_v, 2 * dv), max(bound_e, 2 * de)
        m.update(stokes=st, bound_v=bound_v, bound_e=bound_e)
        vel = [F[k] for k in VEL]
        m["strain"] = G.strain(s, vel, F["etas_eff"], F["etan_eff"], m["fields"]["H"])
        m["strain_material"] = G.strain(s, vel, F["etas"], F["etan"])
        m["tstep"], m["limiter"] = G.timestep(s, F["kz"], F["rho"], F["cp"], vel)
        tstep, k = d["rep"]["tstep"], [F["kz"], F["kx"], F["ky"]]
        m["temp"] = G.heat(s, F["T"], k, F["cp"], F["rho"], F["H"], tstep)
        m["budget"] = G.budget(s, F["T"], k, F["cp"], F["rho"], F["H"], tstep, F["temp"])
        m["Hsum"] = G.budget(s, F["T"], k, F["cp"], F["rho"], m["fields"]["H"], tstep, F["temp"])[0][7]          # the scattered H alone
        m["tmp"] = G.gather(s, it, d["x0"], fu, F["temp"], F["T"], tstep)
        m["v"], m["x_end"], _ = G.advect(s, d["x0"], vel, tstep)
        # the end of the step: the device's end positions, velocities and columns for the rows it kept, the model's for the rows it deleted
        row = {int(i): r for r, i in enumerate(d["f0"][:, TR_ID])}
        old = np.array([int(i) in row for i in d["f"][:, TR_ID]])
        at = np.array([row[int(i)] for i in d["f"][old, TR_ID]], dtype=np.int64)
        xe, fe, ve = m["x_end"].copy(), fu.copy(), m["v"].copy()
        fe[:, TR_TMP] = m["tmp"]
        xe[at], fe[at], ve[at] = d["x"][old], d["f"][old], d["v"][old]
        m["old"], m["at"], m["fu"] = old, at, fu
        m["x"], m["f"], m["vv"], m["info"], m["kept"] = G.markers(s, it, xe, fe, ve)
        out.append(m)
    return out


@pytest.fixture(scope="module", params=K.CASES)
def runs(request):
    import time
    c = K.case(request.param)
    t0 = time.time()
    staged, resident, cold = _run(c, False), _run(c, True), _run(c, True, warm=False)
    t1 = time.time()
    model = _stages(c, resident)
    print("%s: the three runs took %.1f s, the stage models %.1f s" % (c["name"], t1 - t0, time.time() - t1))
    return dict(case=c, staged=staged, resident=resident, cold=cold, model=model)


def _tag(runs, it):
    return "%s step %d:" % (runs["case"]["name"], it + 1)


def test_staged_and_resident_agree_bitwise(runs):
    staged, resident = runs["staged"], runs["resident"]
    _assert_steps_equal(staged, resident, list(G.SCATTERED), list(SOLVED))
    for it, (s, r) in enumerate(zip(staged, resident)):
        for k in ("picard", "dissipation_total", "nremoved", "ninflow", "stokes_start"):
            assert s["rep"][k] == r["rep"][k], _tag(runs, it) + k
        assert s["budget"] == r["budget"], _tag(runs, it) + "heat budget"
        p = r["rep"]["picard"]
        assert p["iterations"] == 3 and not p["converged"] and r["rep"]["nempty"] == 0
        print(_tag(runs, it), "stokes_start %s, Picard %s" % (r["rep"]["stokes_start"], p))
        # stokes_start is that of the step's LAST solve, a Picard solve from the resident solution, which reports "cold" 
        assert r["rep"]["stokes_start"] == "cold", _tag(runs, it)
        assert s["held"] == r["held"] and (s["start"] is None) == (r["start"] is None)
        assert s["start"] is None or np.array_equal(s["start"], r["start"]), _tag(runs, it) + "start vector"


def test_the_warm_start_extrapolates_the_committed_solutions(runs):
    """What stokes_start cannot tell in a step with a yield stress, from the calls that can.  Before step k the history holds min(k - 1, 3)
    levels: it survives the four setters before K1's step 3.  The start vector the step's first solve forms is the Lagrange extrapolation of
    the solutions the earlier steps ended with -- the velocities and the RESCALED pressure after the Picard loop's last update, which is
    the vector the step commits -- to the bar of tests/test_hip_3d_warm.py (8 eps sum |L_k x_k|): the level itself with one, (1 + c, -c)
    with c = min(2, dt0 / dt1) with two, the quadratic through three in K1's step 4.  Whether the guard kept a start shows against a third run with the warm start
    off: a rejected start is the cold solve bit for bit (tests/test_hip_3d_warm.py), a kept one is not; the steps solved from a kept start
    match the model like the cold ones (test_picard_solution_matches_the_model)."""
    from test_hip_3d_warm import _check_start, lagrange
    c, resident = runs["case"], runs["resident"]
    sol = [np.stack([r["fields"][k] for k in VEL + ("pres",)], axis=-1).reshape(-1) for r in resident]
    dt = [r["rep"]["tstep"] for r in resident]
    for it, r in enumerate(resident):
        assert r["held"] == min(it, 3), (_tag(runs, it), r["held"])
        if it == 0:
            assert r["start"] is None
        elif it == 1:
            assert np.array_equal(r["start"], sol[0]), _tag(runs, it)
        elif it == 2:
            w = min(2.0, dt[1] / dt[0])
            _check_start(r["start"], [1.0 + w, -w], [sol[1], sol[0]], _tag(runs, it) + " two levels")
        else:
            times = [0.0, -dt[it - 2], -dt[it - 2] - dt[it - 3]]
            _check_start(r["start"], lagrange(times, dt[it - 1]), [sol[it - 1], sol[it - 2], sol[it - 3]], _tag(runs, it) + " three levels")
    differs = [not np.array_equal(r["fields"]["velz"], q["fields"]["velz"]) for r, q in zip(resident, runs["cold"])]
    its = [(r["rep"]["picard"]["stokes_iterations"][0], q["rep"]["picard"]["stokes_iterations"][0]) for r, q in zip(resident, runs["cold"])]
    print("%s: first-solve Stokes iterations (warm start on, off) per step %s; the fields differ from the cold run's in steps %s"
          % (c["name"], its, [k + 1 for k, v in enumerate(differs) if v]))
    # Recorded on MI355X, and reproducible bit for bit: the guard rejects the one-level start of step 2 in both cases (the solution of a
    # yielded step is a worse start for the next step's first solve, with the material viscosities, than the hydrostatic state), so
    # steps 1 and 2 equal the cold run's and K2 never solves from a kept start; it keeps the extrapolated start of K1's step 3 (59 Stokes
    # iterations against 67), from where the two runs part, and step 4 starts from three levels.
    assert differs[:2] == [False, False], differs
    if c["nsteps"] >= 4:
        assert differs[2] and differs[3] and resident[3]["held"] == 3, differs


def test_scatter_matches_the_model(runs):
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        for k in G.SCATTERED:
            if k == "H":
                continue                         # (with the dissipation: test_strain_fields_use_the_effective_viscosities)
            bar = 1e-11 if k in ("etas", "etan") else 1e-12          # tests/test_hip_mic3_rect.py: geometric / arithmetic schemes
            e = maxrel(d["fields"][k], m["fields"][k])
            worst = max(worst, e / bar)
            assert e < bar, (_tag(runs, it), k, e)
        # the scattered H, which the device reports with the dissipation added, to the same bar: taking the dissipation off again rounds by
        # eps |H| <= 1.2e-14 of max |scattered H| (the dissipation is at most 53 x that; tests/test_step3_stage_model.py prints it)
        e = maxrel(d["fields"]["H"] - d["fields"]["dissipation"], m["fields"]["H"])
        worst = max(worst, e / 1e-12)
        assert e < 1e-12, (_tag(runs, it), "H", e)
        if it > 0:                            # the wall carry: the six walls of T are the previous solved temperature, bit for bit
            prev = runs["resident"][it - 1]["fields"]["temp"]
            assert np.array_equal(d["fields"]["T"], G.wall_carry(d["fields"]["T"], prev)), _tag(runs, it)
            assert not np.array_equal(d["fields"]["T"][1:-1, 1:-1, 1:-1], prev[1:-1, 1:-1, 1:-1])
    print("%s scatter: largest deviation / bar %.3g" % (runs["case"]["name"], worst))


def test_picard_solution_matches_the_model(runs):
    """The same for the cold first step and the warm-started later ones: the start vector must not change the answer."""
    n = runs["case"]["nx"]
    cells = tuple(slice(0, k - 1) for k in n)
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        F, st = d["fields"], m["stokes"]
        v0 = np.stack([st[k] for k in VEL], axis=-1)
        dv = float(np.abs(np.stack([F[k] for k in VEL], axis=-1) - v0).max() / np.abs(v0).max())
        de = max(float(np.abs(np.log(F["etas_eff"] / st["etas_eff"])).max()), float(np.abs(np.log(F["etan_eff"] / st["etan_eff"]))[cells].max()))
        p = d["rep"]["picard"]
        print("%s velocities %.3e of bound %.3e (ratio %.4f); ln(eta_eff) %.3e of bound %.3e (ratio %.4f); start %s; yielded nodes %s (model %s)"
              % (_tag(runs, it), dv, m["bound_v"], dv / m["bound_v"], de, m["bound_e"], de / m["bound_e"], d["rep"]["stokes_start"], p["yielded_nodes"],
                 st["picard"]["yielded_nodes"]))
        worst = max(worst, dv / m["bound_v"], de / m["bound_e"])
        assert dv <= m["bound_v"] and de <= m["bound_e"], _tag(runs, it)
        assert d["rep"]["stokes"]["converged"] == 1
        for a in range(3):                       # the entries of etan beyond the cells keep the material value
            sl = [slice(None)] * 3; sl[a] = -1
            assert np.array_equal(F["etan_eff"][tuple(sl)], F["etan"][tuple(sl)])
    print("%s Picard: largest deviation / bound %.4f" % (runs["case"]["name"], worst))


def test_strain_fields_use_the_effective_viscosities(runs):
    """Stress, dissipation, dissipation_total and the shear heating of a yielded step are those of the viscosities AFTER the loop's last
    update: within the kernel test's bound of the model with etas_eff / etan_eff, and far outside it of the model with the material ones."""
    n = runs["case"]["nx"]
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        F, ref, mat = d["fields"], m["strain"], m["strain_material"]
        for k in ("strainrate", "stress", "dissipation"):
            err = np.abs(F[k].astype(LD) - ref[k])
            bound = 32 * EPS * ref["mag"][k]                            # tests/test_hip_3d_strain.py
            worst = max(worst, float((err / bound).max()))
            assert np.all(err <= bound), (_tag(runs, it), k, float((err / bound).max()))
        for k in ("stress", "dissipation"):                             # the positive control: the material viscosities give other fields
            assert float((np.abs(F[k].astype(LD) - mat[k]) / (32 * EPS * mat["mag"][k])).max()) > 1e6, (_tag(runs, it), k)
        factor = 32 + 4 + np.sqrt(np.prod(n))
        e = float(abs(LD(d["rep"]["dissipation_total"]) - ref["total"]) / (EPS * ref["mag_total"]))
        worst = max(worst, e / factor)
        assert e <= factor, (_tag(runs, it), e)
        # H of the step = the scattered H + that dissipation: the scatter's bar on the first part, the strain bound on the second, one
        # rounding of the sum
        Hs = m["fields"]["H"]
        err = np.abs(F["H"].astype(LD) - ref["H"])
        bound = 1e-12 * np.abs(Hs).max() + 32 * EPS * ref["mag"]["dissipation"] + EPS * np.abs(ref["H"])
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (_tag(runs, it), "H", float((err / bound).max()))
        assert float(np.abs(F["H"] - Hs).max()) > 0.01 * np.abs(Hs).max()          # (the dissipation is no rounding error of H)
    print("%s strain fields: largest deviation / bar %.3g" % (runs["case"]["name"], worst))


def test_time_step_is_the_formula_of_the_staged_step(runs):
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        print("%s tstep %.17g (model %.17g), limiter %s" % (_tag(runs, it), d["rep"]["tstep"], m["tstep"], d["rep"]["limiter"]))
        assert d["rep"]["tstep"] == m["tstep"] and d["rep"]["limiter"] == m["limiter"], _tag(runs, it)


def test_heat_solve_and_budget_match_the_model(runs):
    c = runs["case"]
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        s, F, b = m["s"], d["fields"], d["budget"]
        e = relerr(F["temp"], m["temp"])
        worst = max(worst, e / 1e-6)
        assert d["rep"]["heat"]["converged"] == 1 and e < 1e-6, (_tag(runs, it), e)          # tests/test_hip_3d_heatwalls.py
        # the wall rows: the hot patch holds the nodes of z0 at its entries (1e-6 K, as the step test of tests/test_hip_3d_heatwalls.py)
        assert np.abs(F["temp"][0] - s["planes"][0]).max() <= 1e-6, _tag(runs, it)
        assert np.abs(F["temp"][-1] - c["bcheatvals"][3]).max() <= 1e-6
        out, mag = m["budget"]
        got = np.array(b["wall_flow"] + [b["storage"], b["source"]])
        dev = np.abs(LD(1) * got - out)
        assert np.all(dev <= 1e-12 * mag), (_tag(runs, it), dev, mag)
        err = np.where(mag > 0, dev / np.where(mag > 0, mag, 1), 0)
        worst = max(worst, float(err.max() / 1e-12))
        a = c["flow_axis"]
        assert b["wall_flow"][a] > 0                                      # the flux plane feeds heat in
        print("%s heat solve relerr %.3e; budget |gpu - model| / sum|terms| at most %.2e" % (_tag(runs, it), e, float(err.max())))
    print("%s heat: largest deviation / bar %.3g" % (c["name"], worst))


def test_heat_budget_of_the_combined_step_closes(runs):
    n = runs["case"]["nx"]
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        b, ref = d["budget"], m["strain"]
        scale = max(abs(b["storage"]), abs(b["source"]), max(abs(v) for v in b["wall_flow"]))
        rel = abs(b["imbalance"]) / scale
        worst = max(worst, rel / STEP_CONSERVATION_BOUND)
        assert rel <= STEP_CONSERVATION_BOUND, (_tag(runs, it), rel)
        # source = the scattered H + the dissipation over the interior control volumes; with the wall nodes' share of the dissipation
        # (from the device's field) that is dissipation_total, to the reduction bound of tests/test_hip_3d_strain.py plus the scatter's
        # bar on the sum of H
        wall = np.ones(n, dtype=bool); wall[1:-1, 1:-1, 1:-1] = False
        share = np.sum((d["fields"]["dissipation"].astype(LD) * ref["vol_nodes"])[wall])
        err = abs(LD(b["source"]) - m["Hsum"] + share - LD(d["rep"]["dissipation_total"]))
        bound = (36 + np.sqrt(np.prod(n))) * EPS * ref["mag_total"] + 1e-12 * abs(m["Hsum"])
        worst = max(worst, float(err / bound))
        print("%s imbalance / largest term %.3e; source %.6e, scattered H %.6e, dissipation_total %.6e (wall nodes %.6e): off by %.3g of the bound"
              % (_tag(runs, it), rel, b["source"], float(m["Hsum"]), d["rep"]["dissipation_total"], float(share), float(err / bound)))
        assert err <= bound, (_tag(runs, it), float(err / bound))
        assert d["rep"]["dissipation_total"] > 0.01 * abs(float(m["Hsum"]))
    print("%s heat budget: largest deviation / bar %.3g" % (runs["case"]["name"], worst))


def test_temperature_reaches_the_tracers(runs):
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        bar = 1e-13 if it == 0 else 1e-12                                  # tests/test_hip_mic3_rect.py: absolute / increment with subgrid diffusion
        e = maxrel(d["f"][m["old"], TR_TMP], m["tmp"][m["at"]])
        worst = max(worst, e / bar)
        assert e < bar, (_tag(runs, it), e)
        if it > 0:                               # (the subgrid correction is no rounding error)
            plain = G.gather(dict(m["s"], subgrid=False), it + 1, d["x0"], m["fu"], d["fields"]["temp"], d["fields"]["T"], d["rep"]["tstep"])
            assert maxrel(plain, m["tmp"]) > 1e-6
    print("%s temperature to tracers: largest deviation / bar %.3g" % (runs["case"]["name"], worst))


def test_advection_matches_the_model(runs):
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        ex, ev = maxrel(d["x"][m["old"]], m["x_end"][m["at"]]), maxrel(d["v"][m["old"]], m["v"][m["at"]])
        worst = max(worst, ex / 1e-14, ev / 1e-9)                           # tests/test_hip_3d_flow.py
        print("%s rk4: x %.3g  v %.3g" % (_tag(runs, it), ex, ev))
        assert ex < 1e-14 and ev < 1e-9, _tag(runs, it)
    print("%s advection: largest deviation / bar %.3g" % (runs["case"]["name"], worst))


def test_deletion_refill_and_inflow_match_the_model(runs):
    c = runs["case"]
    worst = 0.0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        info, rep = m["info"], d["rep"]
        want = {k: info[k] for k in ("ninjected", "nrefilled", "nempty", "mincount", "nremoved", "ninflow")}
        print(_tag(runs, it), want)
        assert {k: rep[k] for k in want} == want, (_tag(runs, it), {k: rep[k] for k in want})
        assert rep["ntrac"] == m["x"].shape[0] == d["x"].shape[0] and np.array_equal(d["census"], info["census"])
        assert info["nremoved"] >= 1 and info["nrefilled"] >= 1 and info["ninflow"] >= 1
        # the survivors are the rows the model keeps; IDs are equal row for row, the new ones included
        assert np.array_equal(np.sort(d["f0"][m["kept"], TR_ID]), np.sort(d["f"][m["old"], TR_ID])), _tag(runs, it)
        assert np.array_equal(d["f"][:, TR_ID], m["f"][:, TR_ID]) and np.array_equal(~m["old"], info["new"]), _tag(runs, it)
        new = info["new"]
        assert np.array_equal(d["x"][~new], m["x"][~new]) and np.array_equal(d["v"], m["vv"])
        ex = max(float(np.abs(d["x"][new, a] - m["x"][new, a]).max()) / c["L"][a] for a in range(3))
        worst = max(worst, ex / (4 * 2.0 ** -52))
        assert ex <= 4 * 2.0 ** -52, (_tag(runs, it), ex)                  # tests/test_hip_mic3_rect.py
        assert np.array_equal(d["f"], m["f"], equal_nan=True), _tag(runs, it)          # tests/test_hip_mic3_inflow.py: every column, bit for bit
        marked = d["f"][:, G.TR_MAT] == 2.0
        assert np.array_equal(marked & new, info["inflow"]), _tag(runs, it)
    print("%s refill: largest position deviation / bar %.3g" % (c["name"], worst))


def test_the_yield_stress_limits_the_flow(runs):
    """2 etas_eff e_n of the device's effective viscosities, with the model's node invariant of the device's velocities, is at most tau_y
    where the floor does not bind and above tau_y where it does (tests/test_step3_stage_model.py evaluates both on the model first).  The
    allowance is the Picard bound of the step on ln(eta_eff), which covers the solver's error in the velocities the last update saw."""
    worst, bound_nodes = 0.0, 0
    for it, (d, m) in enumerate(zip(runs["resident"], runs["model"])):
        F = d["fields"]
        measure, tau, binds = K.yield_measure(m["s"], [F[k] for k in VEL], F["etas_eff"])
        over = float(((measure - tau) / tau)[~binds].max())
        worst = max(worst, over / m["bound_e"])
        print("%s stress measure / tau_y - 1 at most %.3e where the floor does not bind (allowed %.3e); the floor binds at %d nodes, measure / tau_y >= %.4f there"
              % (_tag(runs, it), over, m["bound_e"], int(binds.sum()), float((measure / tau)[binds].min()) if binds.any() else np.nan))
        assert over <= m["bound_e"], _tag(runs, it)
        assert np.all(measure[binds] > tau[binds]), _tag(runs, it)
        # and to the kernel's own bound B (tests/test_hip_3d_yield.py): the effective viscosities are the model's update of the material
        # ones for exactly the velocities the step reports -- one update ahead of the solution, none behind
        s = m["s"]
        u = Y.effective(s["nx"], s["grid"], F["etas"], F["etan"], [F[k] for k in VEL], *s["yield_stress"], bc=s["bc"], wallvel=s["wallvel"])
        for name, B in (("etas_eff", u["B_s"]), ("etan_eff", u["B_n"])):
            err = np.abs(F[name].astype(LD) - u[name])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = float(np.where(err > 0, err / B, 0).max())
            print("%s %s against the update of the reported velocities: worst error / B = %.3f" % (_tag(runs, it), name, ratio))
            assert np.all(err <= B), (_tag(runs, it), name, ratio)
        assert np.all((measure - tau)[~binds] <= 2 * u["e_n"][~binds] * u["B_s"][~binds] + 4 * EPS * tau[~binds]), _tag(runs, it)
        bound_nodes += int(binds.sum())
    assert bound_nodes > 0
    print("%s yield: largest excess / bound %.3g" % (runs["case"]["name"], worst))
