"""Flow through the walls of the 3-D Stokes kernels (pl3_stokes_set_wall_flow) against the NumPy model tests/stokes3_flow_model.py,
which tests/test_stokes3_flow_model.py earns its authority: the right-hand side unscaled and row-scaled (every rank of a block
decomposition too), the advection ghosts bit for bit, solutions against the refined direct solve of the model's assembled matrix, and
Simulation3 as a plug flow with deletion at the outflow and refill at the inflow.  Problems are those of tests/test_hip_3d_model.py:
non-uniform in all axes, 3 decades of viscosity."""
import functools
import re

import numpy as np
import pytest

import stokes3_flow_model as Q
import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W
from test_hip_3d_model import _problem, _solution_errors
from test_hip_3d_moving import _check_rhs

pytestmark = pytest.mark.gpu

N, F = W.NOSLIP, W.FREESLIP
GRAV = (3.0, -4.0, 5.0)                                     # the gravity of tests/test_hip_3d_walls.py
ZERO = (0.0, 0.0, 0.0)
U0 = 3e-7                                                   # m/s: the size of the buoyant velocities of these problems
BIG = (37, 45, 131)


def _mid(c):
    return (c[1:] + c[:-1]) / 2


@functools.lru_cache(maxsize=None)
def _case(n, case, u0=U0):
    """(bc, wallvel, wallflow) on the grid of _problem(n):
    plug: a uniform flow in at z0 and out at zL, all walls free-slip;
    parabolic: the profile 4 s (1 - s), s = z / Lz, in at x0 and out at xL between no-slip z-walls (it vanishes towards them);
    corner: in at z0 and out at xL, scaled by the ratio of the areas, all walls no-slip and z0 sliding as well."""
    grid = _problem(n)["grid"]
    if case == "plug":
        return [F] * 6, None, [u0, None, None, u0, None, None]
    if case == "parabolic":
        s = _mid(grid[0]) / grid[0][-1]
        prof = u0 * (4 * s * (1 - s))[:, None] * np.ones(n[2] - 1)[None, :]
        return [N, F, F, N, F, F], None, [None, prof, None, None, prof.copy(), None]
    assert case == "corner"
    U = np.zeros((6, 3)); U[0] = (0.0, u0, -0.5 * u0)
    return [N] * 6, U, [u0, None, None, None, u0 * (grid[1][-1] / grid[0][-1]), None]


CASES = ("plug", "parabolic", "corner")


@functools.lru_cache(maxsize=None)
def _divisor(n, case, strict):
    p = _problem(n)
    return V.row_divisor(p["n"], p["grid"], p["etas"], p["etan"], _case(n, case)[0], strict)


def _model_rhs(n, case, strict, grav, scaled, flow=True):
    p = _problem(n)
    bc, U, fl = _case(n, case)
    kw = dict(grav=grav, bc=bc, wallvel=U, wallflow=fl if flow else None, strict=strict)
    if not scaled:
        return Q.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], **kw)
    plain = grav == ZERO and U is None                      # (no row but the walls' own is non-zero: the model needs no divisor)
    return Q.stokes_rhs_scaled(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], divisor=None if plain else _divisor(n, case, strict), **kw)


def _gpu_rhs(P3, ctx, n, case):
    """[(strict, grav, unscaled, scaled, unscaled without flow, scaled without flow)] from one context"""
    p = _problem(n)
    bc, U, fl = _case(n, case)
    U = np.zeros((6, 3)) if U is None else U
    out = []
    for strict in (True, False):
        for grav in (GRAV, ZERO):
            A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx,
                                         strict_reference=strict, wallvel=U, wallflow=fl)
            scaled = A.rhs(scaled=True)
            got = ctx.wall_flow()
            want = P3.wall_flows(fl, p["n"])
            assert all((g is None) == (w is None) and (g is None or np.array_equal(g, w)) for g, w in zip(got, want))
            A0, rest = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx,
                                           strict_reference=strict, wallvel=U, wallflow=[None] * 6)
            assert ctx.wall_flow() == [None] * 6
            out.append((strict, grav, rhs, scaled, rest, A0.rhs(scaled=True)))
    return out


def _check_case(res, n, case, what):
    p = _problem(n)
    bc, U, fl = _case(n, case)
    big = tuple(n) == BIG
    for strict, grav, rhs, scaled, rest, rest_scaled in res:
        tag = "%s %s strict=%s grav=%s" % (what, case, strict, grav)
        _check_rhs(rhs, _model_rhs(n, case, strict, grav, False), n, tag + " unscaled")
        # without the flow the right-hand side is the moving-wall model's
        ref0 = V.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, strict=strict)
        _check_rhs(rest, ref0, n, tag + " unscaled, without the flow")
        assert np.abs(rhs - rest).max() > 0
        if not big or (grav == ZERO and U is None):
            _check_rhs(scaled, _model_rhs(n, case, strict, grav, True), n, tag + " scaled")
        else:
            # BIG with gravity or a sliding wall: the model's divisor (an assembled matrix) takes a minute there.  The flow's rows are
            # disjoint from every other row's, so the flow's own part is compared with the model: Un on its rows and nothing else.
            part = scaled - rest_scaled
            _check_rhs(part, Q.flow_rhs(p["n"], fl).reshape(-1).astype(np.float64), n, tag + " scaled, the flow's part")
            rows = part != 0
            assert np.array_equal(scaled[rows], part[rows]) and not rest_scaled[rows].any()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("n", [[5, 5, 5], [6, 5, 7], [13, 10, 70], list(BIG)])
def test_rhs_matches_model(n, case):
    """Unscaled (pl3_stokes_rhs) and row-scaled (pl3_stokes_rhs_scaled, what the solve iterates on), both wall-row modes, gravity
    (3, -4, 5) and zero.  [5, 5, 5]: every layer is a wall layer; [6, 5, 7]: odd sizes; [13, 10, 70]: more than one 64-lane tile
    along y; [37, 45, 131]: the size at which the operator runs as the marching kernel with its rim.  Bound: the model's zero pattern
    and 1e-14 of the largest entry per component (the criterion of tests/test_hip_3d_moving.py)."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    p = _problem(n)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        res = _gpu_rhs(P3, ctx, n, case)
    finally:
        ctx.close()
    _check_case(res, n, case, "rhs %s" % list(n))


def test_rhs_on_every_rank_of_a_block_decomposition():
    """2 x 2 x 2 blocks at [13, 11, 141], the corner flow: the planes are indexed by global face indices, so every rank, given the
    same six planes, returns the model's right-hand side."""
    from pylamp_amd import pylamp3d as P3
    n = (13, 11, 141)
    p = _problem(n)
    vc = P3.VirtualCluster3(p["n"], p["grid"], 2, 2, 2)
    try:
        res = vc.all(lambda ctx, rank: _gpu_rhs(P3, ctx, n, "corner"))
    finally:
        vc.close()
    assert len(res) == 8
    for rank, out in enumerate(res):
        _check_case(out, n, "corner", "blocks rank %d" % rank)


@pytest.mark.parametrize("case", CASES)
def test_advection_ghosts_bitwise(case):
    """pl3_advection_velocity after pl3_stokes_set_wall_flow is advection_velocity(wallflow=...) and the model bit for bit, at
    [6, 7, 9] with flows of the size of the field; without a flow the result is that of the same walls alone.  A third of the field is
    exactly zero, and the sign of the zeros is compared as well (-V against 2 0 - V) -- but for the ghost planes of the walls whose
    pass is skipped: a later pass that copies from there finds a source no pass has written, where the kernel has always written +0
    and NumPy's negation gives -0."""
    from pylamp_amd import pylamp3d as P3, _lib
    n = (6, 7, 9)
    rng = np.random.default_rng(91)
    grid = [np.linspace(0, 1.0, n[a]) for a in range(3)]
    bc, U, fl = _case(n, case, 1.0)
    if case == "parabolic":                                 # a profile that varies along both axes of the wall
        fl = [None, fl[1] * rng.uniform(0.5, 1.5, fl[1].shape), None, None, fl[4] * rng.uniform(0.5, 1.5, fl[4].shape), None]
    vel = [rng.standard_normal(n) * (rng.uniform(size=n) > 0.33) for _ in range(3)]
    ctx = P3.Context3(list(n), grid)
    try:
        ctx.set_stokes_walls(bc)
        ctx.set_wall_velocity(U)
        got = {}
        for name, f in (("flow", fl), ("none", None)):
            # (the ghosts need no balanced flow, but the setting does: the unbalanced parabolic pair goes in through one more wall)
            ctx.set_wall_flow(_balanced(grid, f))
            adv = [np.full([v + 1 for v in n], np.nan) for _ in range(3)]
            ctx.check(ctx.lib.pl3_advection_velocity(ctx.handle(), *[_lib.dptr(v) for v in vel], *[_lib.dptr(v) for v in adv]))
            got[name] = adv
    finally:
        ctx.close()
    gm = P3.gridmp_of(grid)
    for name, f in (("flow", _balanced(grid, fl)), ("none", None)):
        _, ref = P3.advection_velocity(vel, gm, n, bc, U, f)
        _, mod = Q.advection_velocity(vel, gm, n, bc=bc, wallvel=U, wallflow=f)
        _, old = V.advection_velocity(vel, gm, n, bc=bc, wallvel=U)
        written = np.ones([v + 1 for v in n], dtype=bool)
        for w in range(6):
            if bc[w] == N and not (U is not None and U[w].any()) and (f is None or f[w] is None):
                np.moveaxis(written, w % 3, 0)[0 if w < 3 else -1] = False
        for q in range(3):
            assert np.array_equal(got[name][q], ref[q]) and np.array_equal(ref[q], mod[q]), (name, q)
            assert np.array_equal(np.signbit(ref[q]), np.signbit(mod[q])), (name, q)
            assert np.array_equal(np.signbit(got[name][q])[written], np.signbit(mod[q])[written]), (name, q)
            assert (got[name][q][written] == 0).any()
            if f is None:
                assert np.array_equal(got[name][q], old[q]) and np.array_equal(np.signbit(mod[q]), np.signbit(old[q])), q
    assert any(not np.array_equal(got["flow"][q], got["none"][q]) for q in range(3))


def _balanced(grid, fl):
    """fl with the wall y0 (free of flow in every case here) taking up what is left of the net flux."""
    if fl is None:
        return None
    phi, _, tot = Q.net_flux(grid, fl)
    if abs(phi) <= np.longdouble(1e-11) * tot:
        return fl
    assert fl[2] is None
    out = list(fl)
    out[2] = float(-phi / (np.longdouble(grid[0][-1]) * np.longdouble(grid[1][-1])))
    return out


# ---- solutions -------------------------------------------------------------------------------------------------------
SOLVE_N = (17, 13, 21)


@functools.lru_cache(maxsize=None)
def _direct(case, strict):
    p = _problem(SOLVE_N)
    bc = _case(SOLVE_N, case)[0]
    ap = lambda x, rounded=True: W.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, bc=bc, strict=strict, rounded=rounded)
    return M.DirectSolver(M.assemble(ap, p["n"]), ap)


@pytest.mark.parametrize("buoyancy", [True, False], ids=["buoyant", "channel"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "natural"])
@pytest.mark.parametrize("case", CASES)
def test_solution_matches_direct_solve_of_the_model(case, strict, buoyancy):
    """[17, 13, 21], the three flows, both wall-row modes, with buoyancy (default gravity) and without (gravity zero): P3.solve against
    the refined direct solution of the model's assembled matrix for the model's right-hand side.  Bounds of
    tests/test_hip_3d_walls.py: converged == 1 within DEFAULT_MAXIT, velocity relative L2 < 1e-6, pressure on the non-ghost cells
    < 1e-5 (plug flow without gravity has the exact pressure zero: there the error is taken relative to eta U / h).  The start vector, the hydrostatic guess and the error estimate all meet non-zero wall-normal entries here.  Plug flow
    without gravity returns U to 1e-6 U on every v_z entry; parabolic / strict / channel is solved device-resident as well.  The
    iteration counts are printed, not capped (DESIGN.md 6c records them)."""
    from pylamp_amd import pylamp3d as P3
    p = _problem(SOLVE_N)
    bc, U, fl = _case(SOLVE_N, case)
    grav = None if buoyancy else ZERO
    rr = Q.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, wallflow=fl, strict=strict)
    xr = _direct(case, strict).solve(rr)
    what = "%s %s %s" % (case, "strict" if strict else "natural", "buoyant" if buoyancy else "channel")
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx, strict_reference=strict,
                                     wallvel=np.zeros((6, 3)) if U is None else U, wallflow=fl)
        x = P3.solve(A)
        st = A.last_stats
        print("solve %s: %d iterations, converged %d, residual %.3e, estimate %.3e" % (what, st["iterations"], st["converged"],
                                                                                       st["rel_residual"], st["error_estimate"]))
        ev, ep = _solution_errors(x, xr, SOLVE_N)
        print("  velocity %.3e pressure %.3e" % (ev, ep))
        assert st["converged"] == 1 and st["iterations"] <= P3.DEFAULT_MAXIT, st
        X = x.reshape(p["n"] + [4])
        if case == "plug" and not buoyancy:
            # The exact pressure is zero, so an error relative to it has no denominator.  It is taken relative to the viscous pressure
            # of this flow instead, eta U / h with the median viscosity and the smallest cell width (in the solution's units, over Kcont),
            # as a root mean square over the non-ghost cells: the size of the pressures the other two channel flows have.
            h = min(float(np.diff(g).min()) for g in p["grid"])
            scale = float(np.median(p["etan"])) * U0 / h / A.Kcont
            ep = float(np.sqrt(np.mean((X[:-1, :-1, :-1, 3] - xr.reshape(p["n"] + [4])[:-1, :-1, :-1, 3]) ** 2))) / scale
            print("  plug: pressure error %.3e of the viscous pressure scale %.3e" % (ep, scale))
        assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        # the wall-normal entries are the profile itself (an identity row: to the residual bound, 1e-6 of the largest entry is ample)
        for w, un in enumerate(P3.wall_flows(fl, p["n"])):
            plane = np.moveaxis(X[..., w % 3], w % 3, 0)[0 if w < 3 else -1]
            assert np.abs(plane[:-1, :-1] - (0.0 if un is None else un)).max() <= 1e-6 * U0, w
        if case == "plug" and not buoyancy:
            dev = np.abs(X[:, :-1, :-1, 0] - U0).max()
            print("  plug: largest |v_z - U| = %.3e U" % (dev / U0))
            assert dev <= 1e-6 * U0
            assert np.abs(X[..., 1:3]).max() <= 1e-6 * U0
        if case == "parabolic" and strict and not buoyancy:
            assert P3.solve(A, resident=True) is None and A.last_stats["converged"] == 1, A.last_stats
            ev, ep = _solution_errors(P3.solution(A), xr, SOLVE_N)
            print("  resident: velocity %.3e pressure %.3e (%d iterations)" % (ev, ep, A.last_stats["iterations"]))
            assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        # the flow is in the answer, and a right-hand side that is given stays as given: the flow of the context does not enter it
        given = V.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, strict=strict)
        if given.any():
            xg = P3.solve(A, rhs=given)
            assert np.abs(xg - x).max() > 1e-3 * np.abs(x).max()
            A0, _ = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx, strict_reference=strict,
                                        wallflow=[None] * 6)
            eg = _solution_errors(xg, P3.solve(A0), SOLVE_N)
            print("  without the flow: %d iterations" % A0.last_stats["iterations"])
            assert eg[0] < 1e-5 and eg[1] < 1e-4, eg
    finally:
        ctx.close()


# ---- Simulation3 -----------------------------------------------------------------------------------------------------
SIM_NX = [17, 17, 17]
SIM_L = [100e3, 100e3, 100e3]
SIM_U = 1e-9
SIM_MOD = 0.3                                               # tstep_modifier: a step carries the tracers 0.3 cells along z
FLOWS = {"plug": [SIM_U, None, None, SIM_U, None, None], "none": None}


def _sim_tracers():
    """8 tracers per cell, each at its own height (k + 0.5) / 8 of the cell, on a 2 x 2 lattice in x, y; uniform density and viscosity.
    With steps of 0.3 cells the cells along z0 hold 6 tracers after the first step and 3 after the second, which the refill
    (tracdens_min = 4) tops up: no cell runs empty, and what the run reports does not depend on a random stream."""
    from pylamp_amd import pylamp3d as P3
    m = [v - 1 for v in SIM_NX]
    dz, dx, dy = (SIM_L[a] / m[a] for a in range(3))
    ci, cj, ck, k = np.meshgrid(np.arange(m[0]), np.arange(m[1]), np.arange(m[2]), np.arange(8), indexing="ij")
    tr_x = np.stack([(ci + (k + 0.5) / 8) * dz, (cj + 0.25 + 0.5 * (k & 1)) * dx, (ck + 0.25 + 0.5 * ((k >> 1) & 1)) * dy], axis=-1).reshape(-1, 3)
    tr_f = np.zeros((tr_x.shape[0], P3.NFTRAC))
    tr_f[:, P3.TR__ID] = np.arange(tr_x.shape[0])[::-1]    # (new IDs count from the largest one left: the outflow must not take it)
    tr_f[:, 6] = 3300.0; tr_f[:, P3.TR_RHO] = 3300.0; tr_f[:, P3.TR_MAT] = 1; tr_f[:, 10] = 1e19            # TR_RH0, TR_ET0
    return tr_x, tr_f


@functools.lru_cache(maxsize=None)
def _flow_run(resident, flows, classic=True, mod=SIM_MOD):
    """One step per name in `flows` (keys of FLOWS): the first is Options3.bcstokesflow ("never": the option is not given), the later
    ones are set with set_wall_flow before their step.  classic: Options3.rk4_classic, the RK4 weights with which a tracer moves by
    U tstep.  Cached: nobody writes to the result."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _sim_tracers()
    kw = {} if flows[0] == "never" else dict(bcstokesflow=FLOWS[flows[0]])
    opt = P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, resident=resident, grav=ZERO, tracdens=8, tracdens_min=4,
                      tracs_fence_enabled=False, marker_deletion=True, inject_unique_ids=True, tstep_modifier=mod, rk4_classic=classic, **kw)
    sim = P3.Simulation3(SIM_NX, SIM_L, tr_x, tr_f, opt)
    out = []
    x, f = sim.tracers()
    o = np.argsort(f[:, P3.TR__ID], kind="stable")
    before = dict(x=x[o], id=f[o, P3.TR__ID])
    for it, name in enumerate(flows):
        if it > 0:
            sim.set_wall_flow(FLOWS[name])
        n0 = sim.ntrac
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        x, f = sim.tracers()
        o = np.argsort(f[:, P3.TR__ID], kind="stable")
        out.append(dict(rep=rep, n0=n0, x=x[o], f=f[o], id=f[o, P3.TR__ID], v=sim.tracer_velocity()[o], before=before,
                        fields={k: sim.field(k).copy() for k in ("rho", "etas", "etan", "velz", "velx", "vely", "pres")}))
        before = dict(x=x[o], id=f[o, P3.TR__ID])
    sim.close()
    return out


def _same(a, b):
    for it, (s, r) in enumerate(zip(a, b)):
        for k in ("iterations", "converged", "rel_residual", "error_estimate"):
            assert s["rep"]["stokes"][k] == r["rep"]["stokes"][k], (it, k)
        for k in ("tstep", "ntrac", "ninjected", "nrefilled", "nempty", "nremoved"):
            assert s["rep"][k] == r["rep"][k], (it, k)
        for k in s["fields"]:
            assert np.array_equal(s["fields"][k], r["fields"][k]), (it, k)
        for k in ("x", "f", "v"):
            assert np.array_equal(s[k], r[k], equal_nan=True), (it, k)


def _survivors(s):
    """(displacement of the tracers that survived the step, in ID order; the positions before the step of those that did not)"""
    keep = np.isin(s["before"]["id"], s["id"])
    mine = np.isin(s["id"], s["before"]["id"])
    assert keep.sum() == mine.sum() == s["n0"] - s["rep"]["nremoved"] and (~mine).sum() == s["rep"]["ninjected"]
    return s["x"][mine] - s["before"]["x"][keep], s["before"]["x"][~keep]


def test_simulation3_plug_flow_staged_and_resident():
    """[17, 17, 17], 8 tracers per cell, tracdens = 8, tracdens_min = 4, fence off with deletion, gravity zero, uniform density, the
    classical RK4 weights: two steps of plug flow z0 -> zL.  Staged and resident agree bit for bit; tracers leave through zL and are
    removed, the cells along z0 are refilled and none runs empty; ntrac follows + ninjected - nremoved; the velocity field is U on
    every v_z entry to 1e-6 U, so U tstep is tstep_modifier cells."""
    staged = _flow_run(False, ("plug", "plug"))
    resident = _flow_run(True, ("plug", "plug"))
    _same(staged, resident)
    dz = SIM_L[0] / (SIM_NX[0] - 1)
    for s in staged:
        rep = s["rep"]
        print("plug step %d: %d iterations, tstep %.6e, removed %d, injected %d in %d cells, empty %d, ntrac %d" % (
            rep["it"], rep["stokes"]["iterations"], rep["tstep"], rep["nremoved"], rep["ninjected"], rep["nrefilled"], rep["nempty"], rep["ntrac"]))
        assert rep["nempty"] == 0 and rep["nremoved"] > 0
        assert rep["ntrac"] == s["n0"] + rep["ninjected"] - rep["nremoved"] == s["x"].shape[0]
        assert abs(SIM_U * rep["tstep"] - SIM_MOD * dz) <= 1e-6 * SIM_MOD * dz
        assert np.abs(s["fields"]["velz"][:, :-1, :-1] - SIM_U).max() <= 1e-6 * SIM_U
        d, gone = _survivors(s)
        # the removed ones are those that the step carried past zL
        assert gone.shape[0] == rep["nremoved"] and np.all(gone[:, 0] + SIM_U * rep["tstep"] >= SIM_L[0] * (1 - 1e-9))
    assert sum(s["rep"]["ninjected"] for s in staged) > 0
    assert staged[1]["rep"]["nrefilled"] == (SIM_NX[1] - 1) * (SIM_NX[2] - 1)          # the whole layer of cells along z0


def test_simulation3_plug_flow_carries_the_tracers_by_u_tstep():
    """The same run: every tracer that survives a step has moved by U tstep along z, within 1e-6 of that, and not sideways -- with
    Options3.rk4_classic = True.  The reference's RK4 weights (1, 1, 1, 1) / 6 (pylamp_trac.py:385; the default, pinned by
    tests/golden/rk4.npz) sum to 4 / 6 and carry a tracer by 4 / 6 U tstep in the same velocity field: that run is held to that figure,
    to the same 1e-6 (tstep_modifier 0.45, so that its steps are 0.3 cells as well)."""
    for s in _flow_run(False, ("plug", "plug")):
        d, _ = _survivors(s)
        move = SIM_U * s["rep"]["tstep"]
        print("step %d: dz / (U tstep) - 1 in [%.3e, %.3e], sideways %.3e" % (s["rep"]["it"], (d[:, 0] / move - 1).min(), (d[:, 0] / move - 1).max(),
                                                                           np.abs(d[:, 1:]).max() / move))
        assert np.all(np.abs(d[:, 0] - move) <= 1e-6 * move) and np.abs(d[:, 1:]).max() <= 1e-6 * move
    for s in _flow_run(False, ("plug", "plug"), classic=False, mod=0.45):
        d, _ = _survivors(s)
        move = (4.0 / 6.0) * SIM_U * s["rep"]["tstep"]
        print("reference weights, step %d: dz / (4/6 U tstep) - 1 in [%.3e, %.3e]" % (s["rep"]["it"], (d[:, 0] / move - 1).min(), (d[:, 0] / move - 1).max()))
        assert np.all(np.abs(d[:, 0] - move) <= 1e-6 * move) and s["rep"]["nempty"] == 0


def test_rk4_classic_matches_model_and_is_off_by_default():
    """pl3_rk4 with pl3_mic_set_rk4_classic against the NumPy composition Q.rk4_classic on a random velocity field that moves a tracer
    by about a third of a cell: the bounds of tests/test_hip_mic3.py (positions 1e-14, velocities 1e-9 of the maximum).  Switched off
    again, and on a fresh context, the result is the reference's weights', mic3_model.rk4."""
    import mic3_model
    from pylamp_amd import pylamp3d as P3
    from test_hip_mic3 import _cloud
    from conftest import maxrel
    rng = np.random.default_rng(5)
    grid = [np.linspace(-2.0e3, 1.0e5, 24), np.linspace(1.0e3, 1.3e5, 32), np.linspace(0, 0.9e5, 18)]
    shp = [24, 32, 18]
    tr_x = _cloud(rng, grid, 20000, margin=0.3)
    dt = 3.0e5
    h = min(c[1] - c[0] for c in grid)
    V = [rng.standard_normal(shp) * (h / 3 / dt) for _ in range(3)]
    nx = [v - 1 for v in shp]
    ctx = P3.Context3([5, 5, 5], [np.linspace(0, 1, 5)] * 3)
    try:
        assert not ctx.rk4_classic()
        v0, x0 = P3.RK(tr_x, grid, V, nx, dt, ctx=ctx)
        ctx.set_rk4_classic(True)
        assert ctx.rk4_classic()
        v1, x1 = P3.RK(tr_x, grid, V, nx, dt, ctx=ctx)
        ctx.set_rk4_classic(False)
        v2, x2 = P3.RK(tr_x, grid, V, nx, dt, ctx=ctx)
    finally:
        ctx.close()
    vr, xr = Q.rk4_classic(tr_x, grid, V, dt)
    print("rk4 classic: x %.3g  v %.3g" % (maxrel(x1, xr), maxrel(v1, vr)))
    assert maxrel(x1, xr) < 1e-14 and maxrel(v1, vr) < 1e-9
    vr0, xr0 = mic3_model.rk4(tr_x, grid, V, dt)
    assert maxrel(x0, xr0) < 1e-14 and maxrel(v0, vr0) < 1e-9
    assert np.array_equal(x0, x2) and np.array_equal(v0, v2) and not np.array_equal(x0, x1)


@pytest.mark.parametrize("resident", [False, True], ids=["staged", "resident"])
def test_set_wall_flow_between_steps_starts_and_stops_the_flow(resident):
    """No flow, the plug, no flow: at rest every velocity is exactly zero and no tracer moves or is removed; the step in between
    carries them.  A run that never names bcstokesflow is the run with None."""
    run = _flow_run(resident, ("none", "plug", "none"))
    for it in (0, 2):
        for k in ("velz", "velx", "vely"):
            assert not run[it]["fields"][k].any(), (it, k)
        assert not run[it]["v"].any() and run[it]["rep"]["nremoved"] == 0
        assert np.array_equal(run[it]["x"], run[it]["before"]["x"])
    assert np.abs(run[1]["fields"]["velz"][:, :-1, :-1] - SIM_U).max() <= 1e-6 * SIM_U and run[1]["rep"]["nremoved"] > 0
    if not resident:
        _same(run[:1], _flow_run(False, ("never",)))


# ---- rejections ------------------------------------------------------------------------------------------------------
def test_rejections_by_message():
    """Shape, a non-finite entry and the net flux -- through the library and through the Python layers --, the fence, tracdens_min,
    and the normal component of wallvel, which keeps its old text.  A rejected call changes nothing."""
    from pylamp_amd import pylamp3d as P3, _lib
    nx = [5, 6, 7]; L = [1.0, 2.0, 3.0]
    grid = [np.linspace(0, L[a], nx[a]) for a in range(3)]
    one = np.ones(nx)
    ctx = P3.Context3(nx, grid)

    def set_flow(planes):
        planes = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in planes]
        ptr = (_lib.c_double_p * 6)(*[None if a is None else _lib.dptr(a) for a in planes])
        ctx.check(ctx.lib.pl3_stokes_set_wall_flow(ctx.handle(), ptr))

    try:
        assert ctx.lib.pl3_stokes_set_wall_flow(None, None) != 0
        assert b"pl3_stokes_set_wall_flow: NULL context" in ctx.lib.pl3_last_error(None)
        assert ctx.wall_flow() == [None] * 6
        good = [np.full((5, 6), 3e-9), None, None, np.full((5, 6), 3e-9), None, None]
        set_flow(good)
        bad = np.full((4, 6), 1e-9); bad[3, 2] = np.nan
        with pytest.raises(Exception, match=r"pl3_stokes_set_wall_flow: wall xL has a non-finite flow entry \[3, 2\] = nan"):
            set_flow([None, np.full((4, 6), 1e-9), None, None, bad, None])
        # in at z0 (area 2 x 3) and out at xL (area 1 x 3) with the same speed: 3e-9 is left over
        with pytest.raises(Exception) as e:
            set_flow([np.full((5, 6), 1e-9), None, None, None, np.full((4, 6), 1e-9), None])
        m = re.fullmatch(r"pl3_stokes_set_wall_flow: the net flux through the walls is (\S+) \(inflow positive\), more than 1e-10 of the sum (\S+) of "
                         r"\|Un\| over the wall faces: .*; fluxes into the box: z0 (\S+), x0 0, y0 0, zL 0, xL (\S+), yL 0", str(e.value))
        assert m, str(e.value)
        assert np.allclose([float(v) for v in m.groups()], [3e-9, 9e-9, 6e-9, -3e-9], rtol=1e-14, atol=0)
        with pytest.raises(Exception, match=r"the net flux through the walls is 6(\.0+\d)?e-09 "):
            ctx.set_wall_flow([1e-9, None, None, None, None, None])
        got = ctx.wall_flow()                                # the rejected calls changed nothing
        assert all((g is None) == (w is None) and (g is None or np.array_equal(g, w)) for g, w in zip(got, good))
        # the setting survives pl3_stokes_set_coeffs and pl3_stokes_set_walls; six None clear it
        P3.makeStokesMatrix(nx, grid, one, one, one, bc=[N] * 6, ctx=ctx)
        assert np.array_equal(ctx.wall_flow()[3], good[3])
        with pytest.raises(Exception, match=r"3-D Stokes: the flow of wall y0 needs the shape \(nz - 1, nx - 1\) = \(4, 5\) or a scalar \(got \(5, 4\)\)"):
            P3.makeStokesMatrix(nx, grid, one, one, one, ctx=ctx, wallflow=[None, None, np.zeros((5, 4)), None, None, None])
        P3.makeStokesMatrix(nx, grid, one, one, one, ctx=ctx, wallflow=[None] * 6)
        assert ctx.wall_flow() == [None] * 6
        # the old entry keeps its behaviour and its text
        U = np.zeros((6, 3)); U[3, 0] = 1e-9
        with pytest.raises(Exception, match=r"wall zL has the normal velocity component Uz = 1e-09: .*marker deletion path, which is not built in 3-D"):
            ctx.check(ctx.lib.pl3_stokes_set_wall_velocity(ctx.handle(), _lib.dptr(np.ascontiguousarray(U))))
    finally:
        ctx.close()
    f, phi = P3.wall_fluxes(grid, [1e-9, None, None, None, 1e-9, None])
    assert np.allclose(f, [6e-9, 0, 0, 0, -3e-9, 0], rtol=1e-14, atol=0) and abs(phi - 3e-9) < 1e-22
    free = dict(tracs_fence_enabled=False, marker_deletion=True, tracdens=8, tracdens_min=4)
    flow = [1e-9, None, None, 1e-9, None, None]
    with pytest.raises(Exception, match=r"Options3.bcstokesflow: a flow through the walls needs tracs_fence_enabled = False together with marker_deletion = True"):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokesflow=flow, tracdens=8, tracdens_min=4))
    with pytest.raises(Exception, match=r"Options3.bcstokesflow: a flow through the walls needs the refill of depleted cells, tracdens >= tracdens_min > 0 \(got tracdens_min = 0\)"):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokesflow=flow, tracs_fence_enabled=False, marker_deletion=True))
    with pytest.raises(Exception, match=r"Options3.bcstokesflow: wall z0 has a non-finite flow entry \[0, 0\] = inf"):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokesflow=[np.inf, None, None, None, None, None], **free))
    with pytest.raises(Exception, match=r"the net flux through the walls is 6(\.0+\d)?e-09 "):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokesflow=[1e-9, None, None, None, None, None], **free))
    sim = P3.Simulation3(nx, L, options=P3.Options3(**free))
    try:
        with pytest.raises(Exception, match=r"Simulation3.set_wall_flow: the flow of wall zL needs the shape \(nx - 1, ny - 1\) = \(5, 6\)"):
            sim.set_wall_flow([None, None, None, np.zeros((6, 5)), None, None])
        sim.set_wall_flow(flow)
        assert np.array_equal(sim.ctx.wall_flow()[0], np.full((5, 6), 1e-9))
        with pytest.raises(Exception, match=r"wall zL has the normal velocity component Uz"):
            sim.set_wall_velocity(U)
    finally:
        sim.close()
    fenced = P3.Simulation3(nx, L, options=P3.Options3(tracdens=8, tracdens_min=4))
    try:
        with pytest.raises(Exception, match=r"Simulation3.set_wall_flow: a flow through the walls needs tracs_fence_enabled = False"):
            fenced.set_wall_flow(flow)
    finally:
        fenced.close()
