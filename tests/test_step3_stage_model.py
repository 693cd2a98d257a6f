"""CPU checks of tests/step3_stage_model.py (one 3-D step, stage by stage, from the existing NumPy models) and of the two cases that
tests/test_hip_step3_combined.py runs on the GPU with every opt-in feature of the 3-D step switched on together.

The cases (case("K1"), case("K2")) are built here and imported by the GPU test.  This module runs a whole MODEL trajectory of each --
every stage fed by the previous model stage, direct solves -- and asserts with the models alone that the inputs are fit for the
purpose: the yield stress bites partly at every Picard update, the floor binds, every step deletes, refills and marks inflow tracers,
no cell runs empty, no end position sits on a face, the dissipation matters to H, the profile walls matter to the temperature.  With
every opt-in off the stage functions are the existing models with their default arguments.

K1  [13, 11, 9], four steps: z graded 2 : 1, x refined, y uniform; lid z0 moves along y; flow x0 -> xL; hot patch on z0, flux plane on
    x0; inflow material on x0; before step 3 the lid speed, the flow, the heat profile and the inflow material change.
K2  [6, 7, 67], two steps: y graded (a y-line crosses the 64-lane tile), z refined; lid z0 moves along x; flow y0 -> yL; flux plane and
    inflow material on y0.
"""
import functools

import numpy as np
import pytest

from conftest import relerr

import mic3_model as U
import mic3_rect_model as RS
import mic3_refill_model as R
import step3_stage_model as G
import stokes3_flow_model as Q
import stokes3_model as M
import stokes3_strain_model as S
import stokes3_walls_model as W
import stokes3_yield_model as Y
from test_yield3_model import between

LD = np.longdouble
N_, F_ = W.NOSLIP, W.FREESLIP
NF = 13
HEAT_BAR = 1e-6                                # relerr of the heat solve (tests/test_hip_3d_heatwalls.py, tests/test_hip_3d_model.py)
FACE_MARGIN = 1e-9                             # of L: no end position nearer to a wall or a cell face
ULID = 1.0e-8                                  # m/s
TTOP, TBOT = 1400.0, 1800.0                    # K: with TR_ACE below the material viscosity spans three decades
ACE = 4.2e5
MODIFIER = 0.3                                 # tstep_modifier: the lid moves a tracer by a quarter of a cell per step, no cell under it runs empty


# ---- the cases ------------------------------------------------------------------------------------------------------------------------------
def _face_plane(n, a, amp, phase):
    """A positive plane over the faces of a wall of axis a, (n_p - 1, n_q - 1): 1 + amp sin cos, never uniform."""
    p, q = Q.AXES[a]
    i, j = np.meshgrid((np.arange(n[p] - 1) + 0.5) / (n[p] - 1), (np.arange(n[q] - 1) + 0.5) / (n[q] - 1), indexing="ij")
    return 1.0 + amp * np.sin(np.pi * (i + phase)) * np.cos(np.pi * (j - phase))


def _node_plane(n, a, centre, width):
    """A bump over the nodes of a wall of axis a, (n_p, n_q), between 0 and 1."""
    p, q = Q.AXES[a]
    i, j = np.meshgrid(np.linspace(0, 1, n[p]), np.linspace(0, 1, n[q]), indexing="ij")
    return np.exp(-((i - centre[0]) ** 2 + (j - centre[1]) ** 2) / width ** 2)


def _walls(n, a, c, lid, uin, phase, patch):
    """The four wall settings of a case: the lid z0 moves along component c with speed lid; the walls a and a + 3 carry the same plane
    Un > 0 (in at the low wall, out at the high one: the net flux is zero on any grid); a hot patch is the temperature plane on z0 and a
    flux plane lies on wall a; the inflow material of wall a names TR_TMP (a plane), TR_MAT and TR_RH0."""
    wallvel = np.zeros((6, 3)); wallvel[0, c] = lid
    un = uin * _face_plane(n, a, 0.4, phase)
    wallflow = [None] * 6; wallflow[a] = un; wallflow[a + 3] = un.copy()
    planes = [None] * 6
    planes[0] = TTOP + 250.0 * _node_plane(n, 0, patch, 0.3)
    planes[a] = -0.08 * (1.0 + 0.5 * _node_plane(n, a, (0.5, 0.5), 0.4))          # k dT/dx_a along +a: heat flows in
    material = [None] * 6
    material[a] = {G.TR_TMP: 1500.0 + 100.0 * _face_plane(n, a, 0.5, 0.25 + phase), G.TR_MAT: 2.0, G.TR_RH0: 3250.0}
    return dict(wallvel=wallvel, wallflow=wallflow, planes=planes, material=material)


def _tracers(n, grid, L, seed, thin, flow_axis=1):
    """Eight per cell, one in each octant of the cell at a seeded uniform position (so that no two leave a cell in step); a cell in `thin`
    = {cell: count} keeps that many.  The temperature rises with depth and varies along x and y."""
    rng = np.random.default_rng(seed)
    nc = [k - 1 for k in n]
    ci = np.indices(nc + [2, 2, 2]).reshape(6, -1)
    x = np.empty((ci.shape[1], 3))
    for d in range(3):
        u = (ci[3 + d] + rng.uniform(0.02, 0.98, ci.shape[1])) / 2
        x[:, d] = grid[d][ci[d]] + u * (grid[d][ci[d] + 1] - grid[d][ci[d]])
    keep = np.ones(x.shape[0], dtype=bool)
    for c, count in thin.items():
        inside = np.flatnonzero((ci[0] == c[0]) & (ci[1] == c[1]) & (ci[2] == c[2]))
        keep[inside[count:]] = False
    # three more in the far corner cell, beyond its mid-point on every axis and close to the walls zL and yL, where they stay: the corner
    # entry of the cell-centred set (etan) hears of no other tracers, and a NaN there makes min(eta), and with it Kcont, NaN
    far = np.array([[0.9, 0.9, 0.9], [0.85, 0.88, 0.92], [0.93, 0.86, 0.84]])
    far[:, flow_axis] = [0.56, 0.62, 0.58]
    far = np.stack([grid[d][-2] + far[:, d] * (grid[d][-1] - grid[d][-2]) for d in range(3)], axis=1)
    x = np.concatenate([x[keep], far])
    x = x[rng.permutation(x.shape[0])]
    f = np.zeros((x.shape[0], NF))
    z, xx, y = (x[:, d] / L[d] for d in range(3))
    f[:, G.TR_TMP] = TTOP + (TBOT - TTOP) * z + 30.0 * np.sin(2 * np.pi * xx) * np.sin(np.pi * z) * np.cos(2 * np.pi * y)
    f[:, G.TR_HCD] = 4.0; f[:, G.TR_HCP] = 1250.0; f[:, G.TR_RH0] = 3300.0; f[:, G.TR_ALP] = 3.0e-5; f[:, G.TR_MAT] = 1.0
    f[:, G.TR_ACE] = ACE; f[:, G.TR_ET0] = 1e20; f[:, G.TR_IHT] = 2e-5
    f[:, G.TR_ID] = np.arange(x.shape[0])
    return x, f


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of a combined run: nx, L, grid, nsteps, tr_x, tr_f, early / late (the wall settings of steps 1 .. 2 and from step 3 on;
    late is None for K2), yield_stress = (tau0, dtau_dz, eta_floor), and options: the keywords of Options3 (without `resident`)."""
    if name == "K1":
        n, L, nsteps, a, c, seed = [13, 11, 9], [1.0e5, 1.2e5, 0.8e5], 4, 1, 2, 11
        grid = [RS.graded(n[0], L[0], 2.0), RS.refined(n[1], L[1], 2.0), np.linspace(0, L[2], n[2])]
        # an inner cell starts with two tracers, and cells on the inflow wall with two to six: they fall below tracdens_min step after step
        thin = {(6, 5, 4): 2, (3, 0, 2): 2, (7, 0, 5): 3, (9, 0, 1): 4, (1, 0, 6): 4, (5, 0, 3): 5, (10, 0, 4): 5, (2, 0, 0): 6, (8, 0, 7): 6}
    elif name == "K2":
        n, L, nsteps, a, c, seed = [6, 7, 67], [0.5e5, 0.6e5, 6.6e5], 2, 2, 1, 23
        grid = [RS.refined(n[0], L[0], 2.0), np.linspace(0, L[1], n[1]), RS.graded(n[2], L[2], 2.0)]
        thin = {(2, 3, 30): 2, (3, 2, 0): 2, (1, 4, 0): 3, (0, 1, 0): 4, (4, 3, 0): 4, (2, 5, 0): 5}
    else:
        raise Exception("no case " + name)
    # the flow moves a tracer by about 0.15 of the cell at the inflow wall per step (Un varies by 0.6 .. 1.4 over the wall): the cells there
    # fall below tracdens_min one after the other and none loses its last four tracers in one step
    early = _walls(n, a, c, ULID, 0.36 * ULID, 0.0, (0.4, 0.5))
    late = _walls(n, a, c, 1.25 * ULID, 0.45 * ULID, 0.2, (0.6, 0.4)) if name == "K1" else None
    tr_x, tr_f = _tracers(n, grid, L, seed, thin, a)
    bc = [N_, F_, F_, N_, F_, F_]
    out = dict(name=name, nx=n, L=L, grid=grid, nsteps=nsteps, flow_axis=a, tr_x=tr_x, tr_f=tr_f, early=early, late=late, bc=bc,
               bcheatvals=[TTOP, 0.0, 0.0, TBOT, 0.0, 0.0])
    # the yield stress from the model's first solve with the material viscosities: tau0 between two neighbouring values of
    # 2 eta e / (1 + z / Lz) over the nodes and the cells (the recipe of test_yield3_model.kernel_case), the floor likewise from tau_y / (2 e)
    s = settings_of(dict(out, yield_stress=None), 1)
    f, _ = G.scatter(s, tr_x, tr_f)
    x = Y.direct(n, grid, f["etas"], f["etan"], f["rho"], bc=bc, wallvel=early["wallvel"], wallflow=early["wallflow"]).reshape(n + [4])
    res = S.strain_fields(n, grid, f["etas"], f["etan"], [x[..., q] for q in range(3)], bc=bc, wallvel=early["wallvel"])
    e_c, _ = Y.centre_invariant(res)
    cells = tuple(slice(0, k - 1) for k in n)
    un, uc = Y.tau_y(grid, n, 1.0, 1.0 / L[0])          # tau_y / tau0 with dtau_dz = tau0 / Lz: doubles over the depth
    s2 = np.concatenate([(2 * S._ld(f["etas"]) * res["strainrate"] / un).ravel(), (2 * S._ld(f["etan"])[cells] * e_c / uc).ravel()]).astype(np.float64)
    tau0 = between(s2, 0.5)
    lim = np.concatenate([(tau0 * un / (2 * res["strainrate"])).ravel(), (tau0 * uc / (2 * e_c)).ravel()]).astype(np.float64)
    out["yield_stress"] = (tau0, tau0 / L[0], between(lim, 0.1))
    out["options"] = dict(marker_search=True, tracs_fence_enabled=False, marker_deletion=True, tracdens=8, tracdens_min=4, inject_unique_ids=True,
                          rk4_classic=True, do_subgrid_heatdiff=True, tdep_rho=True, tdep_eta=True, stokes_warm_start=True, shear_heating=True,
                          strain_fields=True, yield_stress=out["yield_stress"][:2], yield_eta_floor=out["yield_stress"][2], picard_maxit=3,
                          picard_tol=0.0, tstep_modifier=MODIFIER, bcstokes=bc, bcstokesvel=early["wallvel"], bcstokesflow=early["wallflow"], bcinflow=early["material"],
                          bcheatvals=out["bcheatvals"], bcheatprofile=early["planes"])
    return out


def walls_of(c, it):
    return c["late"] if c["late"] is not None and it >= 3 else c["early"]


def settings_of(c, it):
    """The stage model's settings of step `it` (1-based)."""
    w = walls_of(c, it)
    return G.settings(c["nx"], c["grid"], search=True, bc=c["bc"], wallvel=w["wallvel"], wallflow=w["wallflow"], yield_stress=c["yield_stress"],
                      picard_maxit=3, shear_heating=True, modifier=MODIFIER, bcheatvals=c["bcheatvals"], planes=w["planes"], subgrid=True, classic=True,
                      deletion=True, tracdens=8, tracdens_min=4, unique_ids=True, material=w["material"])


def apply_setters(sim, c, it):
    """What a run calls before step `it`: the four setters before step 3 where the case has late settings."""
    if c["late"] is not None and it == 3:
        w = c["late"]
        sim.set_wall_velocity(w["wallvel"]); sim.set_wall_flow(w["wallflow"]); sim.set_heat_profile(w["planes"]); sim.set_inflow_material(w["material"])


def yield_measure(s, vel, etas_eff):
    """(2 etas_eff e_n, tau_y at the nodes, binds): the node stress measure of the effective viscosities with the node invariant e_n of
    the velocities they were derived from; binds: where etas_eff is the floor."""
    n = s["nx"]
    res = S.strain_fields(n, s["grid"], etas_eff, etas_eff, vel, bc=s["bc"], wallvel=s["wallvel"])
    tau0, dtau_dz, floor = s["yield_stress"]
    tn, _ = Y.tau_y(s["grid"], n, tau0, dtau_dz)
    return 2 * S._ld(etas_eff) * res["strainrate"], tn + np.zeros(n, dtype=LD), np.asarray(etas_eff) == floor


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """The model's own run of the case: per step a dict of what every stage produced."""
    c = case(name)
    x, f, temp = c["tr_x"], c["tr_f"], None
    steps = []
    for it in range(1, c["nsteps"] + 1):
        s = settings_of(c, it)
        fl, fu = G.scatter(s, x, f, temp)
        for k, a in fl.items():                  # (a condition on the inputs: the device's step takes min(eta) and max(kz) over whole arrays)
            assert not np.isnan(a).any(), "%s step %d: the scattered field %s holds NaN at %s" % (name, it, k, np.argwhere(np.isnan(a))[:4].tolist())
        st = G.stokes(s, fl["rho"], fl["etas"], fl["etan"])
        vel = [st["velz"], st["velx"], st["vely"]]
        sr = G.strain(s, vel, st["etas_eff"], st["etan_eff"], fl["H"])
        H = sr["H"].astype(np.float64)
        tstep, limiter = G.timestep(s, fl["kz"], fl["rho"], fl["cp"], vel)
        k = [fl["kz"], fl["kx"], fl["ky"]]
        temp = G.heat(s, fl["T"], k, fl["cp"], fl["rho"], H, tstep)
        plain = G.heat(dict(s, planes=None), fl["T"], k, fl["cp"], fl["rho"], H, tstep)
        unheated = G.heat(s, fl["T"], k, fl["cp"], fl["rho"], fl["H"], tstep)
        fu[:, G.TR_TMP] = G.gather(s, it, x, fu, temp, fl["T"], tstep)
        v, xe, _ = G.advect(s, x, vel, tstep)
        before = RS.cells_of(xe[~G.D.outside(xe, [g[-1] for g in c["grid"]])], c["grid"])[0]
        x, f, _, info, kept = G.markers(s, it, xe, fu, v)
        steps.append(dict(s=s, fields=fl, stokes=st, strain=sr, H=H, tstep=tstep, limiter=limiter, temp=temp, temp_plain=plain, temp_unheated=unheated, x_end=xe, v=v,
                          info=info, kept=kept, cells_before=before, x=x, f=f))
    return steps


CASES = ("K1", "K2")


# ---- the inputs are fit for the purpose -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_yield_stress_bites_partly_and_the_floor_binds(name):
    c, steps = case(name), trajectory(name)
    nn, ncell = int(np.prod(c["nx"])), int(np.prod([k - 1 for k in c["nx"]]))
    binds = 0
    for it, st in enumerate(steps):
        p = st["stokes"]["picard"]
        print("%s step %d: yielded nodes %s of %d, cells %s of %d, change %s" % (name, it + 1, p["yielded_nodes"], nn, p["yielded_cells"], ncell,
                                                                                  ["%.3g" % v for v in p["change"]]))
        assert p["iterations"] == 3
        assert all(0.1 * nn <= v <= 0.9 * nn for v in p["yielded_nodes"]) and all(0.1 * ncell <= v <= 0.9 * ncell for v in p["yielded_cells"])
        floor = c["yield_stress"][2]
        binds += int((st["stokes"]["etas_eff"] == floor).sum()) + int((st["stokes"]["etan_eff"] == floor).sum())
        assert np.all(st["stokes"]["etas_eff"] <= st["fields"]["etas"]) and np.all(st["stokes"]["etan_eff"] <= st["fields"]["etan"])
    assert binds > 0
    # the material viscosity spans three decades
    e = steps[0]["fields"]["etas"]
    assert e.max() / e.min() > 1e3


@pytest.mark.parametrize("name", CASES)
def test_yield_stress_limits_the_stress_measure_of_the_model(name):
    """2 etas_eff e_n, with e_n of the velocities the last update saw, is at most tau_y where the floor does not bind (within the
    model's own bound B of the limit) and above tau_y where it does: the positive control of the GPU test's check."""
    for it, st in enumerate(trajectory(name)):
        s, so = st["s"], st["stokes"]
        vel = [so["velz"], so["velx"], so["vely"]]
        m, tau, binds = yield_measure(s, vel, so["etas_eff"])
        u = Y.effective(s["nx"], s["grid"], st["fields"]["etas"], st["fields"]["etan"], vel, *s["yield_stress"], bc=s["bc"], wallvel=s["wallvel"])
        assert np.array_equal(u["etas_eff"].astype(np.float64), so["etas_eff"])              # one update ahead of the solution
        over = float(((m - tau) / tau)[~binds].max())
        print("%s step %d: stress measure / tau_y - 1 at most %.3e where the floor does not bind; floor binds at %d nodes, measure / tau_y there >= %.4f"
              % (name, it + 1, over, int(binds.sum()), float((m / tau)[binds].min()) if binds.any() else np.nan))
        assert np.all((m - tau)[~binds] <= 2 * u["e_n"][~binds] * u["B_s"][~binds] + 4 * Y.EPS * tau[~binds])
        assert np.all(m[binds] > tau[binds])
    assert any(yield_measure(st["s"], [st["stokes"][k] for k in ("velz", "velx", "vely")], st["stokes"]["etas_eff"])[2].any() for st in trajectory(name))


@pytest.mark.parametrize("name", CASES)
def test_markers_leave_enter_and_are_refilled_in_every_step(name):
    c, steps = case(name), trajectory(name)
    nc = [k - 1 for k in c["nx"]]
    a = c["flow_axis"]
    inner_deficit = False
    for it, st in enumerate(steps):
        info = st["info"]
        print("%s step %d: removed %d, injected %d into %d cells (%d empty, smallest count %d), %d inflow tracers, %d tracers" % (
            name, it + 1, info["nremoved"], info["ninjected"], info["nrefilled"], info["nempty"], info["mincount"], info["ninflow"], st["x"].shape[0]))
        assert info["nremoved"] >= 1 and info["nrefilled"] >= 1 and info["ninflow"] >= 1 and info["nempty"] == 0
        cnt = np.bincount(st["cells_before"], minlength=int(np.prod(nc))).reshape(nc)
        assert cnt.min() == info["mincount"] > 0
        away = np.delete(cnt, 0, axis=a)                       # the cells that do not touch the inflow wall (the low wall of the flow axis)
        inner_deficit |= bool((away < 4).any())
    assert inner_deficit


@pytest.mark.parametrize("name", CASES)
def test_no_end_position_sits_on_a_wall_or_a_face(name):
    """A condition on the seed, not a tolerance: the deletion and the per-cell census of the device and of the model then decide alike."""
    c = case(name)
    for it, st in enumerate(trajectory(name)):
        worst = min(float(np.abs(st["x_end"][:, d, None] - c["grid"][d][None, :]).min()) / c["L"][d] for d in range(3))
        print("%s step %d: nearest end position to a face %.3e of L" % (name, it + 1, worst))
        assert worst > FACE_MARGIN


@pytest.mark.parametrize("name", CASES)
def test_sources_matter(name):
    for it, st in enumerate(trajectory(name)):
        d, H = np.abs(st["strain"]["dissipation"]).max(), np.abs(st["fields"]["H"]).max()
        dT, dD = relerr(st["temp_plain"], st["temp"]), relerr(st["temp_unheated"], st["temp"])          # the norm of the heat bar
        print("%s step %d: max dissipation / max scattered H = %.3g; relerr of the temperature without the profile walls %.3g, without the dissipation %.3g; limiter %s, tstep %.4g"
              % (name, it + 1, float(d / H), dT, dD, st["limiter"], st["tstep"]))
        assert d >= 0.01 * H and dT > 100 * HEAT_BAR and dD > 100 * HEAT_BAR


# ---- the switched-off model ---------------------------------------------------------------------------------------------------------------
def test_with_every_option_off_the_stages_are_the_existing_models():
    n, L = [6, 5, 7], [1.0e5, 1.2e5, 0.8e5]
    grid = [np.linspace(0, L[d], n[d]) for d in range(3)]
    x, f = _tracers(n, grid, L, 3, {(2, 2, 2): 2})
    s = G.settings(n, grid, tracdens=8, tracdens_min=4)
    mp = G.gridmp(grid)
    fl, fu = G.scatter(s, x, f)
    ref = f.copy(); U.property_update(ref, True, True)
    assert np.array_equal(fu, ref)
    node = U.trac2grid(x, ref[:, [0, 1, 5, 3, 11, 8]], grid, [5, 6, 5, 5, 5, 5])
    for k, name in enumerate(("rho", "etas", "cp", "T", "H", "mat")):
        assert np.array_equal(fl[name], node[k]), name
    assert np.array_equal(fl["etan"], U.trac2grid(x, ref[:, [1]], mp, [6])[0])
    for name, tg in (("kz", [mp[0], grid[1], grid[2]]), ("kx", [grid[0], mp[1], grid[2]]), ("ky", [grid[0], grid[1], mp[2]])):
        assert np.array_equal(fl[name], U.trac2grid(x, ref[:, [4]], tg, [5])[0]), name
    st = G.stokes(s, fl["rho"], fl["etas"], fl["etan"])
    xs = Y.direct(n, grid, fl["etas"], fl["etan"], fl["rho"]).reshape(n + [4])
    for q, name in enumerate(("velz", "velx", "vely", "pres")):
        assert np.array_equal(st[name], xs[..., q]), name
    assert st["picard"] is None and np.array_equal(st["etas_eff"], fl["etas"]) and np.array_equal(st["etan_eff"], fl["etan"])
    vel = [st["velz"], st["velx"], st["vely"]]
    sr = G.strain(s, vel, st["etas_eff"], st["etan_eff"], fl["H"])
    plain = S.strain_fields(n, grid, fl["etas"], fl["etan"], vel)
    assert all(np.array_equal(sr[k], plain[k]) for k in ("strainrate", "stress", "dissipation")) and np.array_equal(sr["H"], S._ld(fl["H"]))
    tstep, limiter = G.timestep(s, fl["kz"], fl["rho"], fl["cp"], vel)
    k = [fl["kz"], fl["kx"], fl["ky"]]
    temp = G.heat(s, fl["T"], k, fl["cp"], fl["rho"], fl["H"], tstep)
    ap = lambda v, rounded=True: M.heat_apply(n, grid, mp, k, fl["cp"], fl["rho"], s["bcheat"], tstep, v, rounded=rounded)
    rhs = M.heat_rhs(n, fl["T"], fl["cp"], fl["rho"], fl["H"], s["bcheat"], s["bcheatvals"], tstep)
    assert np.array_equal(temp.ravel(), np.asarray(M.direct_solve(M.assemble(ap, n, ncomp=1), ap, rhs), dtype=np.float64))
    assert np.array_equal(G.gather(s, 1, x, fu, temp, fl["T"], tstep), U.temp_to_tracers(x, fu, grid, temp, True, False, 0.0))
    assert np.array_equal(G.gather(s, 2, x, fu, temp, fl["T"], tstep), U.temp_to_tracers(x, fu, grid, temp - fl["T"], False, True, tstep))
    v, xe, (grids, vels) = G.advect(s, x, vel, tstep)
    g0, v0 = W.advection_velocity(vel, mp, n)
    assert all(np.array_equal(a, b) for a, b in zip(grids, g0)) and all(np.array_equal(a, b) for a, b in zip(vels, v0))
    vr, xr = U.rk4(x, g0, v0, tstep)
    assert np.array_equal(v, vr) and np.array_equal(xe, xr)
    xm, fm, vm, info, kept = G.markers(s, 1, xe, fu, v)
    rx, rf, rv, rinfo = R.refill(U.fence(xe, L), fu, grid, 8, 4, 12345, 1, tr_v=v)
    assert kept.all() and info["nremoved"] == 0 and info["ninflow"] == 0 and info["nrefilled"] == rinfo["nrefilled"] >= 1
    assert np.array_equal(xm, rx) and np.array_equal(fm, rf, equal_nan=True) and np.array_equal(vm, rv)
