"""One 3-D time step, stage by stage, in NumPy (plain helper module, no fixtures, no project code).  This module holds the ORDER of a
step and the plumbing between its stages; the arithmetic of every stage is that of the existing models:

    scatter     mic3_model.property_update + trac2grid (under mic3_rect_model's search), wall carry of T from step 2 on
    stokes      stokes3_yield_model.direct / picard with wallflow= (right-hand side: stokes3_flow_model.stokes_rhs)
    strain      stokes3_strain_model.strain_fields with the viscosities AFTER the loop's last update; H = scattered H + dissipation
    timestep    the formulas of Simulation3.step(): mean spacing, 2 kz / (rho cp), clamps, limiter
    heat        stokes3_model.heat_apply + stokes3_heatwall_model.heat_rhs_planes, solved directly; heat_budget
    gather      mic3_model.temp_to_tracers: absolute at step 1, the increment (with subgrid diffusion) later
    advect      stokes3_flow_model.advection_velocity + rk4_classic (mic3_model.rk4 without the option) under the search
    markers     mic3_delete_model's rule (mic3_model.fence without the option) + mic3_inflow_model.refill

Each function takes the inputs of ONE stage and returns what the stage must produce.  tests/test_hip_step3_combined.py feeds every stage
with the device's own inputs (the tracers before the step, the fields and the time step the device reports), so that no discrete
decision of an earlier stage can flip the comparison of a later one; tests/test_step3_stage_model.py chains the stages into a model
trajectory to check that the test inputs reach what they are meant to reach.

A step's settings are a dict `s` (settings() gives the defaults, every opt-in off):
    nx, grid, search, bc, wallvel (6, 3), wallflow (six entries or None), grav (None: the model's default)
    tdep_rho, tdep_eta, Tref, etamin, etamax
    yield_stress (None or (tau0, dtau_dz, eta_floor)), picard_maxit         (the loop runs with tol = 0: always picard_maxit solves)
    shear_heating
    modifier, adv_max, adv_min, dif_max, dif_min
    bcheat, bcheatvals, planes (six entries or None)
    subgrid, classic, deletion, tracdens, tracdens_min, seed, unique_ids, material (six entries or None)
"""
import numpy as np

import mic3_delete_model as D
import mic3_inflow_model as I
import mic3_model as U
import mic3_rect_model as RS
import stokes3_flow_model as Q
import stokes3_heatwall_model as HW
import stokes3_model as M
import stokes3_strain_model as S
import stokes3_yield_model as Y

SECINYR = 60 * 60 * 24 * 365.25
TR_RHO, TR_ETA, TR_TMP, TR_HCD, TR_HCP, TR_RH0, TR_ALP, TR_MAT, TR_ACE, TR_ET0, TR_IHT, TR_ID = 0, 1, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
ARITHW, GEOMW = U.AVG_ARITH | U.AVG_WEIGHTED, U.AVG_GEOM | U.AVG_WEIGHTED
SCATTERED = ("rho", "etas", "etan", "cp", "T", "H", "mat", "kz", "kx", "ky")
FIXTEMP, FIXFLOW = M.FIXTEMP, M.FIXFLOW


def settings(nx, grid, **kw):
    s = dict(nx=[int(v) for v in nx], grid=[np.asarray(c, dtype=np.float64) for c in grid], search=False, bc=None, wallvel=None, wallflow=None,
             grav=None, tdep_rho=True, tdep_eta=True, Tref=1623.0, etamin=1e17, etamax=1e23, yield_stress=None, picard_maxit=1,
             shear_heating=False, modifier=0.67, adv_max=50e9 * SECINYR, adv_min=50e-9 * SECINYR, dif_max=50e9 * SECINYR,
             dif_min=50e-9 * SECINYR, bcheat=[FIXTEMP, FIXFLOW, FIXFLOW, FIXTEMP, FIXFLOW, FIXFLOW], bcheatvals=[273.0, 0.0, 0.0, 1623.0, 0.0, 0.0],
             planes=None, subgrid=True, classic=False, deletion=False, tracdens=0, tracdens_min=0, seed=12345, unique_ids=False, material=None)
    for k in kw:
        if k not in s:
            raise Exception("unknown setting " + k)
    s.update(kw)
    return s


def gridmp(grid):
    """Mid-points with one extrapolated entry per axis, the node set of the cell-centred fields."""
    out = []
    for c in grid:
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


def _marker(s):
    """The marker models of the step: the searching ones on a rectilinear grid."""
    return RS if s["search"] else U


# ---- scatter --------------------------------------------------------------------------------------------------------------------------------
def scatter(s, tr_x, tr_f, prev_temp=None):
    """(fields, tr_f after the property update).  fields: the ten sets of Simulation3.scatter_fields(); prev_temp (from step 2 on): the
    temperature the previous step solved, which the six walls of T keep."""
    f = np.array(tr_f, dtype=np.float64)
    U.property_update(f, s["tdep_rho"], s["tdep_eta"], Tref=s["Tref"], etamin=s["etamin"], etamax=s["etamax"])
    g, mp = s["grid"], gridmp(s["grid"])
    t2g = _marker(s).trac2grid
    out = {}
    out["rho"], out["etas"], out["cp"], out["T"], out["H"], out["mat"] = t2g(tr_x, f[:, [TR_RHO, TR_ETA, TR_HCP, TR_TMP, TR_IHT, TR_MAT]], g,
                                                                          [ARITHW, GEOMW, ARITHW, ARITHW, ARITHW, ARITHW])
    out["etan"], = t2g(tr_x, f[:, [TR_ETA]], mp, [GEOMW])
    out["kz"], = t2g(tr_x, f[:, [TR_HCD]], [mp[0], g[1], g[2]], [ARITHW])
    out["kx"], = t2g(tr_x, f[:, [TR_HCD]], [g[0], mp[1], g[2]], [ARITHW])
    out["ky"], = t2g(tr_x, f[:, [TR_HCD]], [g[0], g[1], mp[2]], [ARITHW])
    if prev_temp is not None:
        out["T"] = wall_carry(out["T"], prev_temp)
    return out, f


def wall_carry(T, prev_temp):
    T = np.array(T, dtype=np.float64)
    for d in range(3):
        for w in (0, -1):
            sl = [slice(None)] * 3; sl[d] = w
            T[tuple(sl)] = np.asarray(prev_temp)[tuple(sl)]
    return T


# ---- Stokes + Picard --------------------------------------------------------------------------------------------------------------------------
def stokes(s, rho, etas, etan, perturb=None, reuse=None):
    """The solution of the step's Stokes stage from the scattered rho, etas, etan: a dict with velz, velx, vely, pres (Kcont-scaled),
    etas_eff, etan_eff (the material arrays without a yield stress) and, with one, `picard` (stokes3_yield_model.picard's report: change,
    yielded_nodes, yielded_cells per update, solvers).  The loop runs picard_maxit solves (tol = 0).  The start vector of a solve is no
    input: a cold and a warm-started step have the same answer.  perturb, reuse: as in stokes3_yield_model.picard."""
    n = s["nx"]
    kw = dict(bc=s["bc"], wallvel=s["wallvel"], grav=s["grav"])
    if s["wallflow"] is not None:
        kw["wallflow"] = s["wallflow"]
    if s["yield_stress"] is None:
        x = Y.direct(n, s["grid"], etas, etan, rho, **kw)
        es, en, rep = np.asarray(etas, dtype=np.float64), np.asarray(etan, dtype=np.float64), None
    else:
        tau0, dtau_dz, floor = s["yield_stress"]
        rep = Y.picard(n, s["grid"], etas, etan, rho, tau0, dtau_dz, floor, s["picard_maxit"], tol=0.0, perturb=perturb, reuse=reuse, **kw)
        x, es, en = rep["x"], rep["etas_eff"], rep["etan_eff"]
    X = np.asarray(x).reshape(n + [4])
    return dict(velz=X[..., 0], velx=X[..., 1], vely=X[..., 2], pres=X[..., 3], etas_eff=es, etan_eff=en, picard=rep)


# ---- strain fields and shear heating ----------------------------------------------------------------------------------------------------------
def strain(s, vel, etas_eff, etan_eff, H=None):
    """stokes3_strain_model.strain_fields of the velocities with the viscosities the step ends with (after the loop's last update), and
    H of the step: the scattered H plus that dissipation where shear heating is on, the scattered H where it is off."""
    res = S.strain_fields(s["nx"], s["grid"], etas_eff, etan_eff, vel, bc=s["bc"], wallvel=s["wallvel"])
    if H is not None:
        res["H"] = S._ld(H) + res["dissipation"] if s["shear_heating"] else S._ld(H)
    return res


# ---- time step ----------------------------------------------------------------------------------------------------------------------------------
def timestep(s, kz, rho, cp, vel):
    """(tstep, limiter) by the formulas of Simulation3.step(), operation for operation in float64."""
    g = s["grid"]
    dx = [float(g[d][-1]) / (s["nx"][d] - 1) for d in range(3)]
    diffusivity = kz / (rho * cp)
    tstep_temp = s["modifier"] * np.min(dx) ** 2 / np.max(2 * diffusivity)
    tstep_temp = max(min(tstep_temp, s["dif_max"]), s["dif_min"])
    with np.errstate(divide="ignore"):
        tstep_stokes = s["modifier"] * np.min(dx) / max(np.max(v) for v in vel)
    tstep_stokes = max(min(tstep_stokes, s["adv_max"]), s["adv_min"])
    return min(tstep_temp, tstep_stokes), ("H" if tstep_temp < tstep_stokes else "S")


# ---- heat ---------------------------------------------------------------------------------------------------------------------------------------
def heat(s, T, k, cp, rho, H, tstep):
    """The temperature after the step's heat solve (direct), (nz, nx, ny) float64: T the scattered temperature (with its wall carry), k =
    [kz, kx, ky], H with the dissipation where shear heating is on."""
    n, g = s["nx"], s["grid"]
    mp = gridmp(g)
    ap = lambda x, rounded=True: M.heat_apply(n, g, mp, k, cp, rho, s["bcheat"], tstep, x, rounded=rounded)
    if s["planes"] is None:
        rhs = M.heat_rhs(n, T, cp, rho, H, s["bcheat"], s["bcheatvals"], tstep)
    else:
        rhs = HW.heat_rhs_planes(n, T, cp, rho, H, s["bcheat"], s["bcheatvals"], tstep, s["planes"])
    return np.asarray(M.direct_solve(M.assemble(ap, n, ncomp=1), ap, rhs), dtype=np.float64).reshape(n)


def budget(s, T, k, cp, rho, H, tstep, temp):
    """(out, mag) of stokes3_heatwall_model.heat_budget for the step's heat solve."""
    return HW.heat_budget(s["nx"], s["grid"], gridmp(s["grid"]), k, cp, rho, H, T, tstep, temp)


# ---- temperature to the tracers -------------------------------------------------------------------------------------------------------------
def gather(s, it, tr_x, tr_f, temp, T, tstep):
    """The tracer temperatures after the step: tr_f the tracers after the property update, temp the solved temperature, T the one the
    solve started from; absolute at step it = 1, the increment temp - T later (with subgrid diffusion where it is on)."""
    ttt = _marker(s).temp_to_tracers
    if it == 1:
        return ttt(tr_x, tr_f, s["grid"], temp, True, False, 0.0)
    return ttt(tr_x, tr_f, s["grid"], temp - T, False, s["subgrid"], tstep)


# ---- advection ------------------------------------------------------------------------------------------------------------------------------
def advect(s, tr_x, vel, tstep):
    """(tracer velocities, end positions, (grids, vels) of the padded advection field)."""
    grids, vels = Q.advection_velocity(vel, gridmp(s["grid"]), s["nx"], s["bc"], s["wallvel"], s["wallflow"])
    if s["classic"]:
        if s["search"]:
            with RS._search():
                v, x = Q.rk4_classic(tr_x, grids, vels, tstep)
        else:
            v, x = Q.rk4_classic(tr_x, grids, vels, tstep)
    else:
        v, x = _marker(s).rk4(tr_x, grids, vels, tstep)
    return v, x, (grids, vels)


# ---- deletion, refill, inflow ---------------------------------------------------------------------------------------------------------------
def flow_planes(s):
    return None if s["wallflow"] is None else Q.flows(s["wallflow"], s["nx"])


def material_planes(s):
    """{column: plane} per wall with scalars broadcast, the form mic3_inflow_model.refill takes."""
    if s["material"] is None:
        return None
    out = []
    for w, m in enumerate(s["material"]):
        if m is None:
            out.append(None)
            continue
        p, q = I.AXES[w % 3]
        out.append({int(c): np.broadcast_to(np.asarray(v, dtype=np.float64), (s["nx"][p] - 1, s["nx"][q] - 1)) for c, v in m.items()})
    return out


def markers(s, it, x_end, tr_f, tr_v):
    """The end of the step from the end positions of the advection, in the order the step's sort leaves: (x, f, v, info, kept).  With
    the deletion, the tracers outside the box go (mic3_delete_model.outside) and the refill runs on the survivors; without it the fence
    holds them (mic3_model.fence).  info: mic3_inflow_model.refill's, with nremoved; kept: the mask of the rows of x_end that stay."""
    g = s["grid"]
    x_end = np.asarray(x_end, dtype=np.float64)
    if s["deletion"]:
        kept = ~D.outside(x_end, [c[-1] for c in g])
        x0 = x_end[kept]
    else:
        kept = np.ones(x_end.shape[0], dtype=bool)
        x0 = U.fence(x_end, [c[-1] for c in g])
    x, f, v, info = I.refill(x0, np.asarray(tr_f)[kept], g, s["tracdens"], s["tracdens_min"], s["seed"], it, unique_ids=s["unique_ids"],
                             tr_v=np.asarray(tr_v)[kept], material=material_planes(s), flow=flow_planes(s), search=s["search"])
    info["nremoved"] = int((~kept).sum())
    return x, f, v, info, kept
