"""The 3-D strain-rate, stress and dissipation fields on the GPU (pl3_stokes_strain_fields, pylamp3d.strain_fields) against the NumPy
model tests/stokes3_strain_model.py, and the opt-in shear heating of Simulation3 (Options3.shear_heating / strain_fields), staged
against resident.

Bounds.  The kernels evaluate the model's expressions in float64.  Per entry: a strain rate is a rounded difference times a table entry
1 / (c[i+1] - c[i]) that carries two roundings, summed with a second one and squared (about 10 half-units of the last place of its
magnitude squared), then weighted by up to three quotients of table entries, multiplied by the viscosity and accumulated over at most 14
terms: below 32 eps of the entry's magnitude (the model's `mag`, the same expressions with |a| + |b| for every difference a - b), the
bound the issue sets.  The total is sum_nodes Phi V_node: every Phi within 32 eps of its magnitude, V_node three products of rounded
quotients (4 eps), and N - 1 additions of the fixed-order reduction, each rounding by at most eps / 2 of a partial sum <= the summed
magnitude, taken as a random walk: (32 + 4 + sqrt(N)) eps x the summed magnitude."""
import ctypes as C

import numpy as np
import pytest

import stokes3_strain_model as S
from test_strain3_model import make_grid, random_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
N_, F_ = 0, 1                                  # NOSLIP, FREESLIP
FIELDS = ("strainrate", "stress", "dissipation")
SHAPES = ([17, 13, 21], [7, 9, 67], [5, 5, 5], [6, 70, 5])          # standard | across the 64-wide y block and the 4-row x block | all rim | 70 along x
TR_TMP, TR_HCD, TR_HCP, TR_ALP, TR_IHT, TR_ID = 3, 4, 5, 7, 11, 12


def _wall_cases(n, rng):
    """(name, bc, strict, wallvel, wallflow)"""
    U = 2e-9
    mv = np.zeros((6, 3)); mv[0] = (0.0, U, U / 2)
    prof = rng.uniform(0.5, 1.5, (n[0] - 1, n[2] - 1)) * 1e-9        # the same plane on x0 and xL: the net flux vanishes
    flow = [None, prof, None, None, prof, None]
    return [("freeslip strict", [F_] * 6, True, None, None), ("freeslip natural", [F_] * 6, False, None, None),
            ("noslip z", [N_, F_, F_, N_, F_, F_], True, None, None), ("noslip all", [N_] * 6, False, None, None),
            ("moving z0", [N_, F_, F_, N_, F_, F_], False, mv, None), ("through-flow x", [F_] * 6, True, None, flow)]


def _check(got, ref, n, tag):
    for k in FIELDS:
        err = np.abs(got[k].astype(np.longdouble) - ref[k])
        bound = 32 * EPS * ref["mag"][k]
        worst = float((err / bound).max())
        print("%s %-11s worst error / (32 eps magnitude) = %.3f" % (tag, k, worst))
        assert np.all(err <= bound), (tag, k, worst)
    N = int(np.prod(n))
    factor = 32 + 4 + np.sqrt(N)
    err = abs(np.longdouble(got["dissipation_total"]) - ref["total"])
    print("%s total       error / (eps summed magnitude) = %.3f of %.1f" % (tag, float(err / (EPS * ref["mag_total"])), factor))
    assert err <= factor * EPS * ref["mag_total"], tag


@pytest.mark.parametrize("kind", ["regular", "graded"])
@pytest.mark.parametrize("n", SHAPES, ids=lambda n: "x".join(str(v) for v in n))
def test_kernel_matches_the_model(n, kind):
    from pylamp_amd import pylamp3d as P3
    L = [1.0e5, 1.3e5, 0.9e5]
    grid = make_grid(n, L, kind)
    etas, etan, v, P = random_case(n, grid, 31 + n[2])
    rho = np.full(n, 3300.0)
    ctx = P3.Context3(n, grid)
    try:
        for name, bc, strict, mv, flow in _wall_cases(n, np.random.default_rng(5)):
            A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=bc, ctx=ctx, strict_reference=strict,
                                       wallvel=np.zeros((6, 3)) if mv is None else mv, wallflow=[None] * 6 if flow is None else flow)
            vv = [a.copy() for a in v]
            if flow is not None:                 # the wall-normal velocities of the solution vector carry the flow
                vv[1][:-1, 0, :-1] = flow[1]; vv[1][:-1, -1, :-1] = flow[4]
            x = np.stack(vv + [P], axis=-1).reshape(-1)
            got = P3.strain_fields(A, x)
            ref = S.strain_fields(n, grid, etas, etan, vv, bc=bc, wallvel=mv)
            _check(got, ref, n, "%s %s:" % (kind, name))
            again = P3.strain_fields(A, x)
            assert all(np.array_equal(got[k], again[k]) for k in FIELDS) and got["dissipation_total"] == again["dissipation_total"], name
        assert A.ring_sum() == 0.0               # nothing was written outside the nodes
    finally:
        ctx.close()


def _blob(n, L):
    grid = [np.linspace(0, L[a], n[a]) for a in range(3)]
    Z, X, Y = np.meshgrid(*grid, indexing="ij")
    r2 = (Z - 0.4 * L[0]) ** 2 + (X - 0.5 * L[1]) ** 2 + (Y - 0.45 * L[2]) ** 2
    inside = r2 < (0.25 * L[0]) ** 2
    return grid, np.where(inside, 1e21, 1e20), np.where(inside, 1e21, 1e20), np.where(inside, 3400.0, 3300.0)


def test_last_solve_and_given_velocities_agree_bitwise():
    from pylamp_amd import pylamp3d as P3
    n = [17, 13, 21]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _blob(n, L)
    A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=[N_, F_, F_, N_, F_, F_])
    try:
        x = P3.solve(A)
        assert A.last_stats["converged"] == 1
        dev = P3.strain_fields(A)
        host = P3.strain_fields(A, x)
        for k in FIELDS:
            assert np.array_equal(dev[k], host[k]), k
            assert np.all(np.isfinite(dev[k])) and dev[k].max() > 0
        assert dev["dissipation_total"] == host["dissipation_total"] > 0
        # and the model on the solved velocities
        ref = S.strain_fields(n, grid, etas, etan, P3.x2vp(x, n)[0], bc=[N_, F_, F_, N_, F_, F_])
        assert abs(dev["dissipation_total"] - float(ref["total"])) <= (36 + np.sqrt(np.prod(n))) * EPS * float(ref["mag_total"])
    finally:
        A._ctx.close()


# ---- Simulation3: shear heating, staged against resident ------------------------------------------------------------------------------
NSTEP = 3


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
    if kw.get("shear_heating") or kw.get("strain_fields"):
        names += list(FIELDS)
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
    return dict(staged_sh=_run(False, shear_heating=True), resident_sh=_run(True, shear_heating=True), plain=_run(True),
                off=_run(True, shear_heating=False, strain_fields=False), fields=_run(True, strain_fields=True))


def _same(a, b):
    """Every step: the fields that run `a` has, the tracers and the time step, array for array."""
    for it, (s, r) in enumerate(zip(a, b)):
        for k in s["fields"]:
            assert np.array_equal(s["fields"][k], r["fields"][k]), (it + 1, k)
        so, ro = np.argsort(s["f"][:, TR_ID], kind="stable"), np.argsort(r["f"][:, TR_ID], kind="stable")
        assert np.array_equal(s["x"][so], r["x"][ro]) and np.array_equal(s["f"][so], r["f"][ro], equal_nan=True), it + 1
        assert s["rep"]["tstep"] == r["rep"]["tstep"], it + 1


def test_staged_and_resident_shear_heating_agree_bitwise(runs):
    a, b = runs["staged_sh"], runs["resident_sh"]
    _same(a, b)
    for s, r in zip(a, b):
        assert list(s["rep"]) == list(r["rep"]) and sorted(s["fields"]) == sorted(r["fields"])
        assert s["rep"]["dissipation_total"] == r["rep"]["dissipation_total"] > 0
        for k in ("iterations", "rel_residual"):
            assert s["rep"]["heat"][k] == r["rep"]["heat"][k] and s["rep"]["stokes"][k] == r["rep"]["stokes"][k]


def test_H_is_the_scattered_H_plus_the_dissipation(runs):
    sh, fo = runs["resident_sh"][0], runs["fields"][0]                     # the first step: the same tracers, so the same scattered H
    assert np.array_equal(sh["fields"]["dissipation"], fo["fields"]["dissipation"])
    assert np.array_equal(sh["fields"]["H"], fo["fields"]["H"] + sh["fields"]["dissipation"])
    assert np.all(sh["fields"]["dissipation"] >= 0) and sh["fields"]["dissipation"].max() > 0
    inner = (slice(1, -1),) * 3
    assert np.any(sh["fields"]["temp"][inner] != fo["fields"]["temp"][inner])      # and the heat solve saw it


def test_switches_off_change_nothing(runs):
    _same(runs["plain"], runs["off"])
    for s, r in zip(runs["plain"], runs["off"]):
        assert "dissipation_total" not in s["rep"] and list(s["rep"]) == list(r["rep"]) and sorted(s["fields"]) == sorted(r["fields"])
        assert not set(FIELDS) & set(s["fields"])


def test_strain_fields_alone_leave_the_physics_unchanged(runs):
    _same(runs["plain"], runs["fields"])
    for s in runs["fields"]:
        assert s["rep"]["dissipation_total"] > 0
        for k in FIELDS:
            assert np.all(np.isfinite(s["fields"][k])) and s["fields"][k].max() > 0


def test_lid_driven_cavity_heats_up():
    """A uniform fluid at 1000 K between z walls held at 1000 K, gravity off, the lid z0 dragged along x: without shear heating only the
    small H0 warms it, with it the temperature inside is strictly higher after two steps."""
    from pylamp_amd import pylamp3d as P3
    nx = [13, 13, 13]; L = [100e3, 100e3, 100e3]
    temps, totals = {}, {}
    for on in (False, True):
        tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(1))
        tr_f[:, P3.TR_RHO] = 3300.0; tr_f[:, P3.TR_ETA] = 1e21; tr_f[:, 6] = 3300.0; tr_f[:, 10] = 1e21
        tr_f[:, TR_TMP] = 1000.0; tr_f[:, TR_HCD] = 40.0; tr_f[:, TR_HCP] = 1250.0; tr_f[:, TR_IHT] = 1e-8
        lid = np.zeros((6, 3)); lid[0] = (0.0, 1e-9, 0.0)
        opt = P3.Options3(tdep_rho=False, tdep_eta=False, grav=(0.0, 0.0, 0.0), resident=True, bcstokes=[P3.BC_TYPE_NOSLIP] * 6,
                          bcstokesvel=lid, bcheatvals=[1000.0, 0.0, 0.0, 1000.0, 0.0, 0.0], shear_heating=on)
        opt.tstep_adv_max = opt.tstep_modifier * (L[0] / (nx[0] - 1)) / 1e-9
        sim = P3.Simulation3(nx, L, tr_x, tr_f, opt)
        try:
            for _ in range(2):
                rep = sim.step()
            temps[on] = sim.field("temp").copy()
            totals[on] = rep.get("dissipation_total")
        finally:
            sim.close()
    inner = (slice(1, -1),) * 3
    print("interior temperature after two steps: %.6f .. %.6f K without, %.6f .. %.6f K with shear heating; dissipation %.4e W" % (
        temps[False][inner].min(), temps[False][inner].max(), temps[True][inner].min(), temps[True][inner].max(), totals[True]))
    assert totals[False] is None and totals[True] > 0
    assert np.all(temps[True][inner] > temps[False][inner])


# ---- rejections, each by name -----------------------------------------------------------------------------------------------------------
def test_rejections():
    from pylamp_amd import _lib, pylamp3d as P3
    nx, L, tr_x, tr_f = _sphere17()
    with pytest.raises(Exception, match="shear_heating = True needs .*do_heatdiff"):
        P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, shear_heating=True))
    # the library's own check, for a caller of the C ABI
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False, resident=True))
    try:
        assert sim.ctx.shear_heating() is False
        sim.ctx.set_shear_heating(True)
        assert sim.ctx.shear_heating() is True
        with pytest.raises(Exception, match="pl3_resident_step: shear heating .*do_heatdiff"):
            sim.step()
        sim.ctx.set_shear_heating(False)
        sim.step()
        with pytest.raises(Exception, match="no field 'dissipation'.*have: rho, etas, etan, velz, velx, vely, pres"):
            sim.field("dissipation")
        with pytest.raises(Exception, match="pl3_step_dissipation_total: no resident step has run with"):
            sim.ctx.dissipation_total()
    finally:
        sim.close()
    n = [9, 9, 9]
    grid = [np.linspace(0, 1, 9)] * 3
    out = np.empty(n); tot = C.c_double()
    ctx = P3.Context3(n, grid)
    try:
        args = (None, None, None, _lib.dptr(out), None, None, C.byref(tot))
        assert ctx.lib.pl3_stokes_strain_fields(ctx.handle(), *args) != 0
        msg = ctx.lib.pl3_last_error(ctx.handle())
        assert b"pl3_stokes_strain_fields" in msg and b"no Stokes coefficients" in msg, msg
        one = np.ones(n)
        A, _ = P3.makeStokesMatrix(n, grid, one, one, one, ctx=ctx)
        with pytest.raises(Exception, match="pl3_stokes_strain_fields: NULL velocities .*no solve has run"):
            P3.strain_fields(A)
        assert ctx.lib.pl3_stokes_strain_fields(ctx.handle(), _lib.dptr(one), None, None, _lib.dptr(out), None, None, None) != 0
        assert b"all three or all NULL" in ctx.lib.pl3_last_error(ctx.handle())
        only = P3.strain_fields(A, np.zeros(4 * 9 ** 3))                   # a fluid at rest
        assert all(not only[k].any() for k in FIELDS) and only["dissipation_total"] == 0.0
    finally:
        ctx.close()
    vc = P3.VirtualCluster3(n, grid, 2, 1, 1)
    try:
        c0 = vc.ctxs[0]
        assert c0.lib.pl3_stokes_strain_fields(c0.handle(), *args) != 0
        msg = c0.lib.pl3_last_error(c0.handle())
        assert b"pl3_stokes_strain_fields" in msg and b"one rank" in msg and b"pl3_set_comm" in msg, msg
    finally:
        vc.close()
