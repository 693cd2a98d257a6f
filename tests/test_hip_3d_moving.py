"""Moving no-slip walls of the 3-D Stokes kernels (pl3_stokes_set_wall_velocity) against the NumPy model
tests/stokes3_moving_model.py, which tests/test_stokes3_moving_model.py ties to the 2-D oracle: the right-hand side unscaled and
row-scaled (per-node kernels, every rank of a block decomposition), the advection ghosts bit for bit, solutions against the refined
direct solve of the model's assembled matrix, and Simulation3 as a lid-driven cavity.  Problems are those of
tests/test_hip_3d_model.py: non-uniform in all axes, 3 decades of viscosity."""
import ctypes as C
import functools

import numpy as np
import pytest

import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W
from test_hip_3d_model import _problem, _solution_errors

pytestmark = pytest.mark.gpu

N, F = W.NOSLIP, W.FREESLIP
GRAV = (3.0, -4.0, 5.0)                                     # the gravity of tests/test_hip_3d_walls.py
ZERO = (0.0, 0.0, 0.0)
U0 = 3e-7                                                   # m/s: the size of the buoyant velocities of these problems


def _vel(**kw):
    U = np.zeros((6, 3))
    for k, v in kw.items():
        U[W.WALLS.index(k)] = v
    return U


# walls, velocities: z0 alone moving in x and y; all six no-slip with z0 and xL moving (they share a cube edge); the mixed set (every
# cube edge joins two kinds) with z0 moving; for the solves the lid z0 over no-slip z-walls
CASES = {"z0": ([N, F, F, F, F, F], _vel(z0=(0.0, U0, -0.5 * U0))),
         "all2": ([N] * 6, _vel(z0=(0.0, U0, -0.5 * U0), xL=(0.7 * U0, 0.0, 0.4 * U0))),
         "mixed": ([N, F, N, F, N, F], _vel(z0=(0.0, -0.8 * U0, U0))),
         "lid": ([N, F, F, N, F, F], _vel(z0=(0.0, U0, -0.5 * U0)))}


@functools.lru_cache(maxsize=None)
def _divisor(n, case, strict):
    p = _problem(n)
    return V.row_divisor(p["n"], p["grid"], p["etas"], p["etan"], CASES[case][0], strict)


@functools.lru_cache(maxsize=None)
def _model_rhs(n, case, strict, grav, scaled):
    p = _problem(n)
    bc, U = CASES[case]
    if scaled:
        return V.stokes_rhs_scaled(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, strict=strict,
                                   divisor=_divisor(n, case, strict))
    return V.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, strict=strict)


def _gpu_rhs(P3, ctx, n, case):
    """[(strict, grav, unscaled, scaled, unscaled at rest)] from one context"""
    p = _problem(n)
    bc, U = CASES[case]
    out = []
    for strict in (True, False):
        for grav in (GRAV, ZERO):
            A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx,
                                         strict_reference=strict, wallvel=U)
            scaled = A.rhs(scaled=True)
            assert np.array_equal(ctx.wall_velocity(), U)
            A0, rest = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx,
                                           strict_reference=strict, wallvel=np.zeros((6, 3)))
            out.append((strict, grav, rhs, scaled, rest))
    return out


def _check_rhs(r, rr, n, what):
    """The same zero pattern, and per component max |r - r_ref| <= 1e-14 max |r_ref|."""
    R, RR = r.reshape(list(n) + [4]), rr.reshape(list(n) + [4])
    assert np.array_equal(R == 0, RR == 0), what + ": zero pattern differs at %d entries" % int(np.sum((R == 0) != (RR == 0)))
    assert not R[..., 3].any()
    for q in range(3):
        d, s = np.abs(R[..., q] - RR[..., q]), np.abs(RR[..., q]).max()
        node = np.unravel_index(int(np.argmax(d)), d.shape)
        print("%s component %d: max err %.3e of max %.3e" % (what, q, d.max(), s))
        assert d.max() <= 1e-14 * s, "%s: component %d, node %s: gpu %r model %r" % (what, q, node, R[node + (q,)], RR[node + (q,)])


def _check_case(res, n, case, what):
    p = _problem(n)
    for strict, grav, rhs, scaled, rest in res:
        tag = "%s %s strict=%s grav=%s" % (what, case, strict, grav)
        _check_rhs(rhs, _model_rhs(n, case, strict, grav, False), n, tag + " unscaled")
        _check_rhs(scaled, _model_rhs(n, case, strict, grav, True), n, tag + " scaled")
        # at rest the right-hand side is the one of the walls model, and the comparison above sees the velocities
        ref0 = W.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=CASES[case][0], strict=strict)
        assert np.array_equal(rest == 0, ref0 == 0) and np.allclose(rest, ref0, rtol=1e-14, atol=0), tag
        assert np.abs(rhs - rest).max() > 0


@pytest.mark.parametrize("case", ["z0", "all2", "mixed"])
@pytest.mark.parametrize("n", [[5, 5, 5], [6, 5, 7], [13, 10, 70]])
def test_rhs_matches_model(n, case):
    """Unscaled (pl3_stokes_rhs) and row-scaled (pl3_stokes_rhs_scaled, what the solve iterates on), both wall-row modes, gravity
    (3, -4, 5) and zero.  [5, 5, 5]: every layer is a wall layer; [6, 5, 7]: odd sizes; [13, 10, 70]: more than one 64-lane tile
    along y.  Bound: the model's zero pattern and 1e-14 of the largest entry per component."""
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
    """2 x 2 x 2 blocks at the grid of test_blocks_match_model_on_every_rank, [13, 11, 141], the mixed set with z0 moving: layer tests
    and tables use global indices, so every rank gives the model's right-hand side."""
    from pylamp_amd import pylamp3d as P3
    n = (13, 11, 141)
    p = _problem(n)
    vc = P3.VirtualCluster3(p["n"], p["grid"], 2, 2, 2)
    try:
        res = vc.all(lambda ctx, rank: _gpu_rhs(P3, ctx, n, "mixed"))
    finally:
        vc.close()
    assert len(res) == 8
    for rank, out in enumerate(res):
        _check_case(out, n, "mixed", "blocks rank %d" % rank)


@pytest.mark.parametrize("case", ["z0", "all2"])
def test_advection_ghosts_bitwise(case):
    """pl3_advection_velocity after pl3_stokes_set_wall_velocity is advection_velocity(wallvel=...) (and the model) bit for bit: one
    moving wall next to free-slip walls, and two moving walls that share a cube edge (the chain of passes is replayed in order)."""
    from pylamp_amd import pylamp3d as P3, _lib
    n = [6, 7, 9]
    bc, U = CASES[case]
    U = U / U0                                              # velocities of the size of the field
    rng = np.random.default_rng(77)
    grid = [np.linspace(0, 1.0, n[a]) for a in range(3)]
    vel = [rng.standard_normal(n) for _ in range(3)]
    ctx = P3.Context3(n, grid)
    try:
        ctx.set_stokes_walls(bc)
        got = {}
        for name, u in (("moving", U), ("rest", None)):
            ctx.set_wall_velocity(u)
            adv = [np.full([v + 1 for v in n], np.nan) for _ in range(3)]
            ctx.check(ctx.lib.pl3_advection_velocity(ctx.handle(), *[_lib.dptr(v) for v in vel], *[_lib.dptr(v) for v in adv]))
            got[name] = adv
    finally:
        ctx.close()
    gm = P3.gridmp_of(grid)
    for name, u in (("moving", U), ("rest", None)):
        _, ref = P3.advection_velocity(vel, gm, n, bc, u)
        _, mod = V.advection_velocity(vel, gm, n, bc=bc, wallvel=u)
        for q in range(3):
            assert np.array_equal(got[name][q], ref[q]) and np.array_equal(ref[q], mod[q]), (name, q)
    assert any(not np.array_equal(got["moving"][q], got["rest"][q]) for q in range(3))
    assert got["moving"][1][0, 1:-1, 1:-1].all() and not got["rest"][1][0, 1:-1, 1:-1].any()


# ---- solutions -------------------------------------------------------------------------------------------------------
SOLVE_N = (17, 13, 21)


@functools.lru_cache(maxsize=None)
def _direct(case, strict):
    p = _problem(SOLVE_N)
    ap = lambda x, rounded=True: W.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, bc=CASES[case][0], strict=strict, rounded=rounded)
    return M.DirectSolver(M.assemble(ap, p["n"]), ap)


@pytest.mark.parametrize("buoyancy", [True, False], ids=["buoyant", "cavity"])
@pytest.mark.parametrize("strict", [True, False], ids=["strict", "natural"])
@pytest.mark.parametrize("case", ["lid", "all2"])
def test_solution_matches_direct_solve_of_the_model(case, strict, buoyancy):
    """[17, 13, 21], the lid z0 moving over no-slip z-walls and all six no-slip with z0 and xL moving, both wall-row modes, with
    buoyancy (default gravity) and as a pure cavity (gravity zero): P3.solve against the refined direct solution of the model's
    assembled matrix for the model's right-hand side.  Bounds of tests/test_hip_3d_walls.py: converged == 1 within DEFAULT_MAXIT,
    velocity relative L2 < 1e-6, pressure on the non-ghost cells < 1e-5; strict mode: |v - gamma v_nb - (1 - gamma) U| <= 1e-10 of the
    largest velocity on the slaved rows of the no-slip walls.  lid / strict / cavity is solved device-resident as well.  The
    iteration counts are printed, not capped (DESIGN.md 6c records them)."""
    from pylamp_amd import pylamp3d as P3
    p = _problem(SOLVE_N)
    bc, U = CASES[case]
    grav = None if buoyancy else ZERO
    rr = V.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, wallvel=U, strict=strict)
    xr = _direct(case, strict).solve(rr)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx, strict_reference=strict,
                                     wallvel=U)
        x = P3.solve(A)
        st = A.last_stats
        print("solve %s %s %s: %d iterations, converged %d, residual %.3e" % (case, "strict" if strict else "natural",
                                                                            "buoyant" if buoyancy else "cavity", st["iterations"],
                                                                            st["converged"], st["rel_residual"]))
        assert st["converged"] == 1 and st["iterations"] <= P3.DEFAULT_MAXIT, st
        ev, ep = _solution_errors(x, xr, SOLVE_N)
        print("  velocity %.3e pressure %.3e" % (ev, ep))
        assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        if strict:
            vmax = np.abs(x.reshape(p["n"] + [4])[..., :3]).max()
            dn = V.extrapolation_defect(p["n"], p["grid"], x, bc, U)
            print("  slaved rows of the no-slip walls: defect %.3e of the largest velocity" % (dn / vmax))
            assert dn <= 1e-10 * vmax, dn / vmax
        if case == "lid" and strict and not buoyancy:
            assert P3.solve(A, resident=True) is None and A.last_stats["converged"] == 1, A.last_stats
            ev, ep = _solution_errors(P3.solution(A), xr, SOLVE_N)
            print("  resident: velocity %.3e pressure %.3e (%d iterations)" % (ev, ep, A.last_stats["iterations"]))
            assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        # the walls' motion is in the answer: the same problem at rest differs (a cavity at rest does not flow at all)
        A0, _ = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=grav, ctx=ctx, strict_reference=strict,
                                    wallvel=np.zeros((6, 3)))
        x0 = P3.solve(A0)
        print("  at rest: %d iterations" % A0.last_stats["iterations"])
        assert np.abs(x0 - x).max() > 1e-3 * np.abs(x).max()
        if not buoyancy:
            assert not x0.any() and A0.last_stats["converged"] == 1
        if buoyancy:
            # a right-hand side that is given stays as given: the velocities of the context do not enter it
            ctx.set_wall_velocity(U)
            xg = P3.solve(A0, rhs=V.stokes_rhs(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=grav, bc=bc, strict=strict))
            eg = _solution_errors(xg, x0, SOLVE_N)
            assert eg[0] < 1e-5 and eg[1] < 1e-4, eg
    finally:
        ctx.close()


# ---- Simulation3 -----------------------------------------------------------------------------------------------------
LID_BC = [N, F, F, N, F, F]
LID_U = 1e-9


def _cavity_run(resident, vel, nstep=2, grav=ZERO, never=False, then=None):
    """The sizes of _sphere_run (tests/test_hip_3d_walls.py): [17, 17, 17], 8 tracers per cell; uniform density."""
    from pylamp_amd import pylamp3d as P3
    nx = [17, 17, 17]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))
    if grav == ZERO:
        tr_f[:, P3.TR_RHO] = 3300.0
    kw = {} if never else dict(bcstokesvel=vel)
    opt = P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, bcstokes=LID_BC, resident=resident, grav=grav, **kw)
    sim = P3.Simulation3(nx, L, tr_x, tr_f, opt)
    out = []
    for it in range(nstep):
        if then is not None and it == nstep - 1:
            sim.set_wall_velocity(then)
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        x, f = sim.tracers()
        o = np.argsort(f[:, 12], kind="stable")                                        # TR__ID
        out.append(dict(rep=rep, x=x[o], f=f[o], v=sim.tracer_velocity()[o],
                        fields={k: sim.field(k).copy() for k in ("rho", "etas", "etan", "velz", "velx", "vely", "pres")}))
    sim.close()
    return out, L[0] / (nx[0] - 1)


def _same(a, b):
    for it, (s, r) in enumerate(zip(a, b)):
        for k in ("iterations", "converged", "rel_residual", "error_estimate"):
            assert s["rep"]["stokes"][k] == r["rep"]["stokes"][k], (it, k)
        assert s["rep"]["tstep"] == r["rep"]["tstep"] and s["rep"]["ntrac"] == r["rep"]["ntrac"]
        for k in s["fields"]:
            assert np.array_equal(s["fields"][k], r["fields"][k]), (it, k)
        for k in ("x", "f", "v"):
            assert np.array_equal(s[k], r[k], equal_nan=True), (it, k)


def test_simulation3_lid_driven_cavity_staged_and_resident():
    """Gravity zero, uniform density, the lid z0 moving along x: two steps staged and resident agree bit for bit; the tracers of the
    top cell layer move with the sign of U, and the lid's speed bounds every velocity."""
    U = _vel(z0=(0.0, LID_U, 0.0))
    staged, dz = _cavity_run(False, U)
    resident, _ = _cavity_run(True, U)
    _same(staged, resident)
    for s in staged:
        top = s["x"][:, 0] < dz
        print("cavity step %d: %d iterations, tstep %.3e, top-layer tracer vx in [%.3e, %.3e]" % (
            s["rep"]["it"], s["rep"]["stokes"]["iterations"], s["rep"]["tstep"], s["v"][top, 1].min(), s["v"][top, 1].max()))
        assert top.sum() > 1000 and np.all(s["v"][top, 1] > 0)
        assert np.abs(s["fields"]["velx"]).max() <= LID_U * (1 + 1e-6)
    assert not np.array_equal(staged[0]["x"], staged[1]["x"])


def test_simulation3_walls_at_rest_and_set_wall_velocity_between_steps():
    """Gravity zero and U = 0: every velocity is exactly zero and no tracer moves, staged and resident; set_wall_velocity before the
    second step starts the cavity.  With gravity on, bcstokesvel all zeros is bit for bit the run that never sets it."""
    U = _vel(z0=(0.0, LID_U, 0.0))
    for resident in (False, True):
        run, _ = _cavity_run(resident, np.zeros((6, 3)), nstep=2, then=U)
        first, second = run
        for k in ("velz", "velx", "vely"):
            assert not first["fields"][k].any(), k
        assert not first["v"].any()
        assert second["fields"]["velx"].any() and second["v"][:, 1].max() > 0
    zeros, _ = _cavity_run(False, np.zeros((6, 3)), nstep=1, grav=None)
    never, _ = _cavity_run(False, None, nstep=1, grav=None, never=True)
    _same(zeros, never)
    assert zeros[0]["fields"]["velz"].any()


def test_rejections_by_message():
    """The four errors of the library, each naming the wall and the value, and the same through the Python layers."""
    from pylamp_amd import pylamp3d as P3, _lib
    nx = [5, 5, 5]; L = [1.0, 1.0, 1.0]
    grid = [np.linspace(0, 1, 5)] * 3
    one = np.ones(nx)
    ctx = P3.Context3(nx, grid)

    def set_vel(u):
        u = np.ascontiguousarray(u, dtype=np.float64)
        ctx.check(ctx.lib.pl3_stokes_set_wall_velocity(ctx.handle(), _lib.dptr(u)))

    try:
        ctx.set_stokes_walls([N] * 6)
        assert not ctx.wall_velocity().any()
        U = np.zeros((6, 3)); U[4, 2] = np.nan
        with pytest.raises(Exception, match=r"pl3_stokes_set_wall_velocity: wall xL has a non-finite velocity component Uy = nan"):
            set_vel(U)
        U = np.zeros((6, 3)); U[3, 0] = 1e-9
        with pytest.raises(Exception, match=r"wall zL has the normal velocity component Uz = 1e-09: .*marker deletion path, which is not built in 3-D"):
            set_vel(U)
        ctx.set_stokes_walls([N, N, F, N, N, N])
        U = np.zeros((6, 3)); U[2, 1] = 1e-9
        with pytest.raises(Exception, match=r"wall y0 is FREESLIP and cannot move with velocity \(0, 1e-09, 0\)"):
            set_vel(U)
        assert not ctx.wall_velocity().any()                 # a rejected setting changes nothing
        U = _vel(z0=(0.0, 2e-9, -1e-9), xL=(3e-9, 0.0, 5e-10))
        set_vel(U)
        assert np.array_equal(ctx.wall_velocity(), U)
        with pytest.raises(Exception, match=r"pl3_stokes_set_walls: wall xL moves with velocity \(3e-09, 0, 5e-10\) and cannot become FREESLIP"):
            ctx.check(ctx.lib.pl3_stokes_set_walls(ctx.handle(), (C.c_int * 6)(0, 0, 1, 0, 1, 0)))
        with pytest.raises(Exception, match=r"wall z0 moves with velocity"):
            P3.makeStokesMatrix(nx, grid, one, one, one, bc=[F] * 6, ctx=ctx)
        # the velocities survive pl3_stokes_set_coeffs, as the kinds do; kinds and velocities given together replace both
        P3.makeStokesMatrix(nx, grid, one, one, one, ctx=ctx)
        assert np.array_equal(ctx.wall_velocity(), U)
        P3.makeStokesMatrix(nx, grid, one, one, one, bc=[F] * 6, wallvel=np.zeros((6, 3)), ctx=ctx)
        assert not ctx.wall_velocity().any()
    finally:
        ctx.close()
    with pytest.raises(Exception, match=r"wall zL has the normal velocity component Uz"):
        P3.makeStokesMatrix(nx, grid, one, one, one, bc=[N] * 6, wallvel=_vel(zL=(1e-9, 0, 0)))
    with pytest.raises(Exception, match=r"Options3.bcstokesvel: wall x0 is FREESLIP and cannot move"):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokes=LID_BC, bcstokesvel=_vel(x0=(1e-9, 0, 0))))
    sim = P3.Simulation3(nx, L, options=P3.Options3(bcstokes=LID_BC))
    try:
        with pytest.raises(Exception, match=r"Simulation3.set_wall_velocity: wall z0 has a non-finite velocity component Ux = inf"):
            sim.set_wall_velocity(_vel(z0=(0, np.inf, 0)))
        sim.set_wall_velocity(_vel(zL=(0, 0, 2e-9)))
        assert np.array_equal(sim.ctx.wall_velocity(), _vel(zL=(0, 0, 2e-9)))
    finally:
        sim.close()
