"""Per-wall no-slip boundaries of the 3-D Stokes kernels (pl3_stokes_set_walls) against the NumPy model
tests/stokes3_walls_model.py, which tests/test_stokes3_walls_model.py ties to the 2-D oracle: operator and right-hand side row by
row (per-node kernels, the rim behind the marching kernel, every rank of a block decomposition), solutions against the refined
direct solve of the model's assembled matrix, and Simulation3 with a rigid lid and base.  Problems are those of
tests/test_hip_3d_model.py: non-uniform in all axes, 3 decades of viscosity, a random vector on all entries."""
import ctypes as C
import functools

import numpy as np
import pytest

import stokes3_model as M
import stokes3_walls_model as W
from test_hip_3d_model import LDS_THRESHOLD, _check_apply, _check_rhs, _model_rhs, _problem, _solution_errors

pytestmark = pytest.mark.gpu

N, F = W.NOSLIP, W.FREESLIP
WALLSETS = {"all": [N] * 6, "z0": [N, F, F, F, F, F], "mixed": [N, F, N, F, N, F],      # mixed: every cube edge joins two kinds
            "zz": [N, F, F, N, F, F], "free": [F] * 6}
GRAV = (3.0, -4.0, 5.0)


@functools.lru_cache(maxsize=None)
def _walls_apply(n, strict, walls):
    p = _problem(n)
    return W.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], p["x"], bc=WALLSETS[walls], strict=strict)


def _against_model(P3, ctx, n, walls):
    p = _problem(n)
    out = []
    for strict in (True, False):
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=WALLSETS[walls], grav=GRAV, ctx=ctx,
                                     strict_reference=strict)
        out.append((strict, A @ p["x"], rhs, A.Kcont, A.Kbond))
    return out


def _check_against_model(res, n, walls, what):
    p = _problem(n)
    kc, kb = M.scaling(p["grid"], p["etas"], p["etan"])
    for strict, y, rhs, kcg, kbg in res:
        tag = "%s walls=%s strict=%s" % (what, walls, strict)
        assert kcg == pytest.approx(kc, rel=1e-13) and kbg == pytest.approx(kb, rel=1e-13)
        yr = _walls_apply(n, strict, walls)
        _check_apply(y, yr, n, tag)
        ident = W.identity_rows(p["n"], strict, WALLSETS[walls]).reshape(-1)
        assert np.array_equal(y[ident], kcg * p["x"][ident]), tag + ": identity rows are not exactly Kcont * x"
        _check_rhs(rhs, _model_rhs(n, strict, GRAV), tag + " rhs")
        # the comparison sees the walls: the model with these walls is not the free-slip model
        assert np.abs(yr - _walls_apply(n, strict, "free")).max() > 1e-6 * np.abs(yr).max(), tag


@pytest.mark.parametrize("walls", ["all", "z0", "mixed"])
@pytest.mark.parametrize("n", [[5, 5, 5], [6, 7, 9], [13, 10, 70], [37, 45, 131]])
def test_operator_and_rhs_match_model(n, walls):
    """Both wall-row modes.  [5, 5, 5]: every node on the rim, the slaved layers at 0 and 3; [6, 7, 9], [13, 10, 70]: the per-node
    kernels; [37, 45, 131]: k3_rim behind the marching kernel.  Bounds of tests/test_hip_3d_model.py: 1e-12 of the maximum per
    component, identity rows exactly Kcont x, right-hand side rtol 1e-14 with the same zero pattern."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    p = _problem(n)
    assert (int(np.prod(n)) >= LDS_THRESHOLD) == (n == (37, 45, 131))
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        res = _against_model(P3, ctx, n, walls)
    finally:
        ctx.close()
    _check_against_model(res, n, walls, "apply %s" % list(n))


def test_blocks_match_model_on_every_rank():
    """2 x 2 x 2 blocks, the mixed set, [13, 11, 141]: (nodes - 1) has to be divisible by the block count along every axis, which
    [13, 10, 70] is not; the y-blocks of 70 cells still cross the 64-lane tile.  Row classes, wall tests and spacing tables are
    global: every rank gives the model's rows."""
    from pylamp_amd import pylamp3d as P3
    n = (13, 11, 141)
    p = _problem(n)
    vc = P3.VirtualCluster3(p["n"], p["grid"], 2, 2, 2)
    try:
        res = vc.all(lambda ctx, rank: _against_model(P3, ctx, n, "mixed"))
    finally:
        vc.close()
    assert len(res) == 8
    for rank, out in enumerate(res):
        _check_against_model(out, n, "mixed", "blocks rank %d" % rank)


@pytest.mark.parametrize("n", [[6, 7, 9], [37, 45, 131]])
def test_freeslip_is_untouched(n):
    """bc=None (a new context) and bc=[1]*6 (after a no-slip setting on the same context): the same operator output, right-hand side,
    Kcont / Kbond and -- through the solve of a given right-hand side, which k3_scale_rows scales and the scaled operator iterates
    on -- row scaling, bit for bit; and the free-slip model's rows.  bc=None on a context leaves its walls as they are."""
    from pylamp_amd import pylamp3d as P3
    n = tuple(n)
    p = _problem(n)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        for strict in (True, False):
            got = []
            for bc in ([N] * 6, None, [F] * 6):
                A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=GRAV, ctx=ctx, strict_reference=strict)
                got.append((A @ p["x"], rhs, A.Kcont, A.Kbond))
            assert np.array_equal(got[0][0], got[1][0])         # bc=None left the context's no-slip walls alone
            fresh = []
            for bc in (None, [F] * 6):                          # two new contexts: the same history, so the solves are comparable
                c = P3.Context3(p["n"], p["grid"])
                try:
                    A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=bc, grav=GRAV, ctx=c, strict_reference=strict)
                    sol = P3.solve(A, rhs=rhs) if int(np.prod(n)) < 1000 else None
                    fresh.append((A @ p["x"], rhs, A.Kcont, A.Kbond, sol))
                finally:
                    c.close()
            for q in range(2):
                assert np.array_equal(fresh[0][q], fresh[1][q]) and np.array_equal(fresh[0][q], got[2][q]), (strict, q)
            assert fresh[0][2:4] == fresh[1][2:4] == got[2][2:4]
            if fresh[0][4] is not None:
                assert np.array_equal(fresh[0][4], fresh[1][4]) and np.abs(fresh[0][4]).max() > 0
            assert not np.array_equal(got[0][0], got[2][0])
            _check_apply(got[2][0], _walls_apply(n, strict, "free"), n, "free-slip %s strict=%s" % (list(n), strict))
    finally:
        ctx.close()


# ---- solutions -------------------------------------------------------------------------------------------------------
SOLVE_N = (17, 13, 21)
# BiCGStab iterations measured on MI355X: (walls, strict) -> (no-slip, free-slip solve of the same problem)
MEASURED = {("zz", True): (47, 46), ("zz", False): (43, 38), ("all", True): (53, 45), ("all", False): (51, 40)}
MEASURED_LDS = (58, 55)                                      # [37, 45, 131], no-slip z-walls / free-slip


@functools.lru_cache(maxsize=None)
def _direct_solution(walls, strict):
    p = _problem(SOLVE_N)
    ap = lambda x, rounded=True: W.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, bc=WALLSETS[walls], strict=strict, rounded=rounded)
    return M.DirectSolver(M.assemble(ap, p["n"]), ap).solve(_model_rhs(SOLVE_N, strict, None))


def _extrapolation_defect(x, walls):
    """Strict mode: the largest |v - gamma v_nb| over the slaved rows of the no-slip walls (gamma = rD / (rD + rd): the row divided
    by Kcont times its coefficient of v), and the largest |v - v_nb| over those of the free-slip walls."""
    p = _problem(SOLVE_N)
    n = p["n"]
    X = x.reshape(n + [4])
    worst = [0.0, 0.0]
    count = 0
    for D, lst in enumerate(W.slaved_rows(n, WALLSETS[walls])):
        v = X[..., D]
        for rows, a, hi, kind in lst:
            c = p["grid"][a]
            nb = M._shift(v, a, -1 if hi else 1)
            if kind == N:
                rD, rd = (1 / (c[-1] - c[-3]), 1 / (c[-1] - c[-2])) if hi else (1 / (c[2] - c[0]), 1 / (c[1] - c[0]))
                worst[0] = max(worst[0], float(np.abs(v - rD / (rD + rd) * nb)[rows].max()))
                count += int(rows.sum())
            else:
                worst[1] = max(worst[1], float(np.abs(v - nb)[rows].max()))
    assert count > 0
    return worst


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("walls", ["zz", "all"])
def test_solution_matches_direct_solve_of_the_model(walls, strict):
    """[17, 13, 21], walls z0 + zL no-slip and all six no-slip, both wall-row modes: P3.solve against the refined direct solution of
    the model's assembled matrix: converged == 1, velocity relative L2 < 1e-6, pressure on the non-ghost cells < 1e-5 (the bounds
    of tests/test_hip_3d_model.py); zz / strict is solved device-resident as well.  Strict mode: the solved slaved values satisfy
    their extrapolation row to 1e-10 of the largest velocity.  The iteration count is capped at 1.25 x the measured one.
    Measured on MI355X (velocity, pressure; iterations no-slip / free-slip solve of the same problem): zz strict 3.7e-9, 1.2e-10
    (47 / 46), device-resident 4.9e-9, 3.0e-10; zz natural 4.3e-9, 1.2e-11 (43 / 38); all strict 6.5e-9, 8.0e-11 (53 / 45); all natural
    2.3e-9, 8.0e-12 (51 / 40).  Slaved rows of the no-slip walls: defect 3e-15 of the largest velocity, of the free-slip walls 0."""
    from pylamp_amd import pylamp3d as P3
    p = _problem(SOLVE_N)
    xr = _direct_solution(walls, strict)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=WALLSETS[walls], ctx=ctx, strict_reference=strict)
        x = P3.solve(A)
        st = A.last_stats
        assert st["converged"] == 1 and st["iterations"] <= P3.DEFAULT_MAXIT, st
        ev, ep = _solution_errors(x, xr, SOLVE_N)
        print("solve walls=%s strict=%s: velocity %.3e pressure %.3e (%d iterations)" % (walls, strict, ev, ep, st["iterations"]))
        assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        if strict:
            vmax = np.abs(x.reshape(p["n"] + [4])[..., :3]).max()
            dn, df = _extrapolation_defect(x, walls)
            print("  slaved rows: no-slip defect %.3e, free-slip defect %.3e of the largest velocity" % (dn / vmax, df / vmax))
            assert dn <= 1e-10 * vmax and df <= 1e-10 * vmax, (dn / vmax, df / vmax)
        assert st["iterations"] <= 1.25 * MEASURED[(walls, strict)][0], st
        if strict and walls == "zz":
            assert P3.solve(A, resident=True) is None and A.last_stats["converged"] == 1, A.last_stats
            ev, ep = _solution_errors(P3.solution(A), xr, SOLVE_N)
            print("solve resident: velocity %.3e pressure %.3e" % (ev, ep))
            assert ev < 1e-6 and ep < 1e-5, (ev, ep)
        # the free-slip solve of the same problem, for the count beside it
        A0, _ = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=WALLSETS["free"], ctx=ctx, strict_reference=strict)
        x0 = P3.solve(A0)
        print("  free-slip: %d iterations" % A0.last_stats["iterations"])
        assert np.abs(x0 - x).max() > 1e-3 * np.abs(x).max()
    finally:
        ctx.close()


def test_lds_solve_residual_by_the_model():
    """[37, 45, 131] with no-slip z-walls: the rim behind the LDS smoother and residual inside the V-cycle.  The residual is the
    MODEL's: ||rhs_ref - A_ref x_gpu|| / ||rhs_ref|| < 1e-6; converged within the default maxit; iterations capped at 1.25 x the
    measured count.  Measured on MI355X: model residual 7.0e-12, 58 iterations (free-slip walls: 55);
    on the 129^3 problem of bench.py --config 3d257 (too large for this suite) no-slip z-walls take 33 iterations, free-slip 22."""
    from pylamp_amd import pylamp3d as P3
    n = (37, 45, 131)
    p = _problem(n)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        A, rhs = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=WALLSETS["zz"], ctx=ctx)
        x = P3.solve(A)
        st = A.last_stats
    finally:
        ctx.close()
    assert st["converged"] == 1 and st["rel_residual"] <= P3.DEFAULT_RTOL and st["iterations"] <= P3.DEFAULT_MAXIT, st
    rr = _model_rhs(n, True, None)
    res = rr.astype(np.longdouble) - W.stokes_apply(p["n"], p["grid"], p["etas"], p["etan"], x, bc=WALLSETS["zz"], strict=True, rounded=False)
    rel = float(np.sqrt(np.sum(res * res)) / np.linalg.norm(rr))
    print("lds solve, no-slip z-walls: model residual %.3e, %d iterations" % (rel, st["iterations"]))
    assert rel < 1e-6, rel
    assert st["iterations"] <= 1.25 * MEASURED_LDS[0], st


# ---- Simulation3 -----------------------------------------------------------------------------------------------------
def _sphere_run(bc, resident, nstep=2):
    from pylamp_amd import pylamp3d as P3, _lib
    nx = [17, 17, 17]; L = [100e3, 100e3, 100e3]
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(7))           # 2 x 2 x 2 = 8 tracers per cell
    opt = P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, bcstokes=bc, resident=resident)
    sim = P3.Simulation3(nx, L, tr_x, tr_f, opt)
    out = []
    for it in range(nstep):
        rep = sim.step()
        assert rep["stokes"]["converged"] == 1, rep
        x, f = sim.tracers()
        o = np.argsort(f[:, 12], kind="stable")                                        # TR__ID
        out.append(dict(rep=rep, x=x[o], f=f[o], v=sim.tracer_velocity()[o],
                        fields={k: sim.field(k).copy() for k in ("rho", "etas", "etan", "velz", "velx", "vely", "pres")}))
    # the device advection velocity of this context (its walls) on the last velocities
    vel = [out[-1]["fields"][k] for k in ("velz", "velx", "vely")]
    adv = [np.full([v + 1 for v in nx], np.nan) for _ in range(3)]
    sim.ctx.check(sim.ctx.lib.pl3_advection_velocity(sim.ctx.handle(), *[_lib.dptr(v) for v in vel], *[_lib.dptr(v) for v in adv]))
    _, ref = P3.advection_velocity(vel, sim.gridmp, nx, bc)
    _, mod = W.advection_velocity(vel, sim.gridmp, nx, bc)
    sim.close()
    return out, adv, ref, mod


def test_simulation3_falling_sphere_with_rigid_lid_and_base():
    """[17, 17, 17], 8 tracers per cell, z0 and zL no-slip, two steps: the resident and the staged step agree bit for bit (as in
    tests/test_hip_step3_resident.py), the device advection velocity is the Python one (and the model's), and the flow is not
    the free-slip one.  Measured on MI355X: 32 iterations in the first step (free-slip: 38)."""
    bc = WALLSETS["zz"]
    staged, adv_s, ref, mod = _sphere_run(bc, False)
    resident, adv_r, _, _ = _sphere_run(bc, True)
    free, _, _, _ = _sphere_run([F] * 6, False, nstep=1)
    for it, (s, r) in enumerate(zip(staged, resident)):
        for k in ("iterations", "converged", "rel_residual", "error_estimate"):
            assert s["rep"]["stokes"][k] == r["rep"]["stokes"][k], (it, k)
        assert s["rep"]["tstep"] == r["rep"]["tstep"] and s["rep"]["ntrac"] == r["rep"]["ntrac"]
        for k in s["fields"]:
            assert np.array_equal(s["fields"][k], r["fields"][k]), (it, k)
        for k in ("x", "f", "v"):
            assert np.array_equal(s[k], r[k], equal_nan=True), (it, k)
    for q in range(3):
        assert np.array_equal(adv_s[q], ref[q]) and np.array_equal(adv_r[q], ref[q]) and np.array_equal(ref[q], mod[q]), q
        assert not adv_s[q][0].any() and not adv_s[q][-1].any()                       # the skipped z passes leave their ghost planes zero
    assert adv_s[1][1:-1, 0, 1:-1].any()                                               # ... and the free-slip x0 pass wrote its own
    vx, vx0 = staged[0]["fields"]["velx"], free[0]["fields"]["velx"]
    print("velx: max %.3e, differs from free-slip by %.3e; iterations %d (no-slip) %d (free-slip)" % (
        np.abs(vx).max(), np.abs(vx - vx0).max(), staged[0]["rep"]["stokes"]["iterations"], free[0]["rep"]["stokes"]["iterations"]))
    assert np.abs(vx - vx0).max() > 1e-2 * np.abs(vx0).max()
    # a rigid lid: the slaved layer of vx next to z0 is a third of the layer below (uniform grid), free-slip copies it
    assert np.allclose(vx[0, 2:-2, 2:-3], vx[1, 2:-2, 2:-3] / 3, rtol=1e-9, atol=1e-12 * np.abs(vx).max())
    assert np.array_equal(vx0[0, 2:-2, 2:-3], vx0[1, 2:-2, 2:-3])


def test_other_wall_kinds_are_rejected_by_name():
    from pylamp_amd import pylamp3d as P3
    nx = [5, 5, 5]; L = [1.0, 1.0, 1.0]
    with pytest.raises(Exception, match=r"wall xL has kind 2"):
        P3.Simulation3(nx, L, options=P3.Options3(bcstokes=[1, 1, 1, 1, 2, 1]))          # CYCLIC
    grid = [np.linspace(0, 1, 5)] * 3
    one = np.ones(nx)
    with pytest.raises(Exception, match=r"wall y0 has kind 4"):
        P3.makeStokesMatrix(nx, grid, one, one, one, bc=[1, 1, 4, 1, 1, 1])              # FLOWTHRU
    with pytest.raises(Exception, match=r"wall z0 has kind 2"):
        P3.advection_velocity([one, one, one], P3.gridmp_of(grid), nx, bc=[2, 1, 1, 1, 1, 1])
    ctx = P3.Context3(nx, grid)
    try:
        with pytest.raises(Exception, match=r"wall zL has kind 3"):
            ctx.check(ctx.lib.pl3_stokes_set_walls(ctx.handle(), (C.c_int * 6)(1, 1, 1, 3, 1, 1)))
    finally:
        ctx.close()
