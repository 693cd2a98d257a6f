"""3-D heat walls with a profile (pl3_heat_set_wall_values) and the heat budget (pl3_heat_budget) against the NumPy model
tests/stokes3_heatwall_model.py, on the grids of tests/test_hip_3d_model.py (graded in all axes, random k, rho, Cp, H).

Sizes: [5, 5, 5] the smallest with an interior; [9, 6, 70] y crosses the 64-lane row of the per-node kernels and the three extents
differ, so a transposed plane cannot pass; [17, 13, 21] for the direct solves.  Every plane carries NaN at the entries another wall
owns: a kernel that read one would spoil its row.  References are computed once and shared; nobody writes to them."""
import functools

import numpy as np
import pytest

from conftest import relerr
import stokes3_model as M
import stokes3_heatwall_model as HW
from test_hip_3d_model import WALLS, _heat_problem

gpu = pytest.mark.gpu
SIZES = [(5, 5, 5), (9, 6, 70), (17, 13, 21)]
NAMES = ("z0", "x0", "y0", "zL", "xL", "yL")
# Conservation (test_solved_field_conserves_heat): the normalised imbalance |storage - source - sum wall_flow| / (|storage| + |source|
# + sum |wall_flow|) of the solved field.  Ten times the largest value measured on MI355X (see that test), rounded up to a power of ten:
# 4.0e-13 over the three sizes and wall sets.  The steps of Simulation3 at 9^3 by the same rule: 3.8e-12 over three steps on either path
# (1.7e-12, 3.8e-12, 3.8e-12).
CONSERVATION_BOUND = 1e-11
STEP_CONSERVATION_BOUND = 1e-10


def _planes(n, walls, nan=True, seed=0):
    """A plane for every wall, a distinct random value per node: temperatures U(300, 1500) on the FIXTEMP walls of the set, fluxes
    U(-0.02, 0.02) on its FIXFLOW walls; NaN at every entry another wall owns."""
    bc = WALLS[walls][0]
    rng = np.random.default_rng(77 + seed + n[0] * 10007 + n[1] * 101 + n[2])
    out = []
    for w in range(6):
        shp = HW.plane_shape(n, w)
        v = rng.uniform(300, 1500, shp) if bc[w] == M.FIXTEMP else rng.uniform(-0.02, 0.02, shp)
        if nan:
            v[~HW.read_mask(n, w)] = np.nan
        out.append(v)
    return out


def _apply(h, bc):
    return lambda x, rounded=True: M.heat_apply(h["n"], h["grid"], h["mid"], h["k"], h["Cp"], h["rho"], bc, h["dt"], x, rounded=rounded)


@functools.lru_cache(maxsize=None)
def _model_rhs(n, walls):
    h = _heat_problem(n)
    bc, bv = WALLS[walls]
    return HW.heat_rhs_planes(h["n"], h["T0"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"], _planes(n, walls))


@functools.lru_cache(maxsize=None)
def _model_solution(n, walls):
    h = _heat_problem(n)
    ap = _apply(h, WALLS[walls][0])
    return M.direct_solve(M.assemble(ap, h["n"], ncomp=1), ap, _model_rhs(n, walls))


def _model_budget(n, T):
    h = _heat_problem(n)
    return HW.heat_budget(h["n"], h["grid"], h["mid"], h["k"], h["Cp"], h["rho"], h["H"], h["T0"], h["dt"], T)


def _make(P3, n, walls, ctx, wallvalues=None, bcvalue=None):
    h = _heat_problem(n)
    bc, bv = WALLS[walls]
    return P3.makeDiffusionMatrix(h["n"], h["grid"], h["mid"], h["T0"], h["k"], h["Cp"], h["rho"], h["H"], bc, bv if bcvalue is None else bcvalue,
                                  h["dt"], ctx=ctx, wallvalues=wallvalues)


def _out8(b):
    return np.array(b["wall_flow"] + [b["storage"], b["source"]])


def _normalised(b):
    return abs(b["imbalance"]) / (abs(b["storage"]) + abs(b["source"]) + sum(abs(v) for v in b["wall_flow"]))


@functools.lru_cache(maxsize=None)
def _gpu_solved(n, walls):
    """The GPU's solution with planes on all six walls, and its budget from the field still on the device."""
    from pylamp_amd import pylamp3d as P3
    h = _heat_problem(n)
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        A, rhs = _make(P3, n, walls, ctx, wallvalues=_planes(n, walls))
        T = P3.solve_heat(A)
        return dict(T=T, rhs=rhs, stats=A.last_stats, budget=P3.heat_budget(A))
    finally:
        ctx.close()


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_validator_shapes_broadcasts_and_named_errors():
    from pylamp_amd import pylamp3d as P3
    n = [9, 6, 70]
    assert P3.wall_heat_values(None, n) == [None] * 6
    V = P3.wall_heat_values([1.5, None, np.zeros((9, 6)), np.ones((6, 70)), 2, None], n)
    assert [None if v is None else v.shape for v in V] == [(6, 70), None, (9, 6), (6, 70), (9, 70), None]
    assert np.array_equal(V[0], np.full((6, 70), 1.5)) and np.array_equal(V[4], np.full((9, 70), 2.0))
    assert all(v is None or (v.dtype == np.float64 and v.flags["C_CONTIGUOUS"]) for v in V)
    D = P3.wall_heat_values({"zL": 7.0, "y0": np.arange(54.0).reshape(9, 6)}, n)
    assert [v is not None for v in D] == [False, False, True, True, False, False] and D[2][3, 4] == 22.0
    with pytest.raises(Exception, match="who: the heat wall values name a wall 'top'"):
        P3.wall_heat_values({"top": 1.0}, n, "who")
    with pytest.raises(Exception, match=r"six entries \[z0, x0, y0, zL, xL, yL\] \(got 5\)"):
        P3.wall_heat_values([None] * 5, n)
    with pytest.raises(Exception, match=r"heat wall x0 need the shape \(nz, ny\) = \(9, 70\) or a scalar \(got \(70, 9\)\)"):
        P3.wall_heat_values([None, np.zeros((70, 9)), None, None, None, None], n)
    with pytest.raises(Exception, match=r"heat wall yL need the shape \(nz, nx\) = \(9, 6\) or a scalar \(got \(6, 9\)\)"):
        P3.wall_heat_values({"yL": np.zeros((6, 9))}, n)
    with pytest.raises(Exception, match=r"heat wall zL need the shape \(nx, ny\) = \(6, 70\) or a scalar \(got an object that is no array\)"):
        P3.wall_heat_values({"zL": "hot"}, n)
    # entries another wall owns are not looked at; one that is read is rejected with wall and indices
    for w in range(6):
        v = np.zeros(HW.plane_shape(n, w))
        v[~HW.read_mask(n, w)] = np.nan
        P3.wall_heat_values([v if u == w else None for u in range(6)], n)
    v = np.zeros((9, 70)); v[0, 5] = np.nan; v[8, 69] = np.inf
    P3.wall_heat_values({"xL": v}, n)
    v[4, 0] = np.inf                                     # an x-wall owns its y-edges
    with pytest.raises(Exception, match=r"heat wall xL has a non-finite entry \[4, 0\] = inf"):
        P3.wall_heat_values({"xL": v}, n)
    v = np.zeros((9, 6)); v[3, 0] = v[0, 2] = np.nan     # a y-wall owns neither
    P3.wall_heat_values({"y0": v}, n)
    v[3, 1] = np.nan
    with pytest.raises(Exception, match=r"heat wall y0 has a non-finite entry \[3, 1\] = nan"):
        P3.wall_heat_values({"y0": v}, n)
    v = np.zeros((6, 70)); v[0, 0] = np.nan              # a z-wall owns all of its nodes
    with pytest.raises(Exception, match=r"heat wall z0 has a non-finite entry \[0, 0\] = nan"):
        P3.wall_heat_values({"z0": v}, n)
    assert P3.Options3().bcheatprofile is None


def test_model_read_mask_is_the_ownership_of_the_rows():
    n = [5, 6, 7]
    own = M._owner(n)
    for w in range(6):
        m = HW.read_mask(n, w)
        assert m.shape == HW.plane_shape(n, w)
        assert m.sum() == (own == w).sum()
    assert HW.read_mask(n, 0).all() and HW.read_mask(n, 3).all()
    x = HW.read_mask(n, 1)
    assert not x[0].any() and not x[-1].any() and x[1:-1].all()
    y = HW.read_mask(n, 5)
    assert y[1:-1, 1:-1].all() and y.sum() == 3 * 4


def test_model_budget_telescopes_for_the_direct_solve():
    """The model's own identity at [9, 6, 70], mixed walls with planes: the normalised imbalance of the refined direct solve (residual
    <= 1e-12) is the reference value for the GPU's.  Measured: 7.6e-17."""
    n = (9, 6, 70)
    out, mag = _model_budget(n, _model_solution(n, "mixed"))
    im, rel = HW.imbalance(out)
    print("model budget [9, 6, 70] mixed: wall flows %s storage %.6e source %.6e imbalance %.3e normalised %.3e"
          % (" ".join("%.4e" % float(v) for v in out[:6]), float(out[6]), float(out[7]), float(im), float(rel)))
    assert np.all(mag > 0)
    assert rel <= 1e-12
    # a field that does not satisfy the rows does not balance: the identity is not a tautology of the sums
    h = _heat_problem(n)
    assert HW.imbalance(_model_budget(n, h["T0"])[0])[1] > 1e-3


def test_model_planes_rhs_keeps_scalars_where_no_plane_is_given():
    n = (5, 5, 5)
    h = _heat_problem(n)
    bc, bv = WALLS["mixed"]
    r0 = M.heat_rhs(h["n"], h["T0"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"])
    assert np.array_equal(HW.heat_rhs_planes(h["n"], h["T0"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"], None), r0)
    pl = _planes(n, "mixed")
    r1 = HW.heat_rhs_planes(h["n"], h["T0"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"], [pl[0]] + [None] * 5).reshape(n)
    assert np.array_equal(r1[0], pl[0]) and np.array_equal(r1[1:], r0.reshape(n)[1:])


# ---- GPU ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("walls", ["mixed", "flow"])
def test_rhs_wall_rows_are_the_plane_entries(n, walls):
    """Unscaled pl3_heat_rhs: wall rows equal the entries of the planes exactly, interior rows are the scalar run's bits, nothing is NaN
    although every entry another wall owns is."""
    from pylamp_amd import pylamp3d as P3
    h = _heat_problem(n)
    pl = _planes(n, walls)
    own = M._owner(h["n"])
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        _, r_scalar = _make(P3, n, walls, ctx)
        _, r = _make(P3, n, walls, ctx, wallvalues=pl)
        assert not np.isnan(r).any()
        assert np.allclose(r, _model_rhs(n, walls), rtol=1e-14, atol=0)              # (the bound of the scalar right-hand side's test)
        r3, rs3 = r.reshape(h["n"]), r_scalar.reshape(h["n"])
        assert np.array_equal(r3[own < 0], rs3[own < 0])
        for w in range(6):
            a = w % 3
            full = np.broadcast_to(np.expand_dims(pl[w], a), h["n"])
            assert np.array_equal(r3[own == w], full[own == w]), NAMES[w]
        back = ctx.heat_wall_values()
        assert all(np.array_equal(b, p, equal_nan=True) for b, p in zip(back, pl))
        # one wall alone: the others keep their scalars
        _, r1 = _make(P3, n, walls, ctx, wallvalues=[None, None, None, None, pl[4], None])
        r13 = r1.reshape(h["n"])
        assert np.array_equal(r13[own != 4], rs3[own != 4]) and np.array_equal(r13[own == 4], r3[own == 4])
        assert [b is not None for b in ctx.heat_wall_values()] == [False, False, False, False, True, False]
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_a_constant_plane_is_the_scalar(n):
    """np.full(shape, v) on every wall: the right-hand side and the solution bits of bcvalue = v; after clearing the planes the scalar
    run's bits return, and the planes survive a new set of coefficients."""
    from pylamp_amd import pylamp3d as P3
    h = _heat_problem(n)
    bc, bv = WALLS["mixed"]
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        A, r_scalar = _make(P3, n, "mixed", ctx)
        T_scalar = P3.solve_heat(A)
        const = [np.full(HW.plane_shape(n, w), bv[w]) for w in range(6)]
        A, r = _make(P3, n, "mixed", ctx, wallvalues=const, bcvalue=[1e300] * 6)       # (a wall with a plane ignores its scalar)
        assert np.array_equal(r, r_scalar)
        assert np.array_equal(P3.solve_heat(A), T_scalar)
        A, r = _make(P3, n, "mixed", ctx, bcvalue=[-1.0] * 6)                          # wallvalues=None: the planes stay
        assert np.array_equal(r, r_scalar)
        A, r = _make(P3, n, "mixed", ctx, wallvalues=[None] * 6)
        assert ctx.heat_wall_values() == [None] * 6
        assert np.array_equal(r, r_scalar) and np.array_equal(P3.solve_heat(A), T_scalar)
    finally:
        ctx.close()


@gpu
@pytest.mark.parametrize("n", [(9, 6, 70), (17, 13, 21)])
def test_solution_with_planes_matches_direct_solve_of_the_model(n):
    """relerr < 1e-6 (the project's bound for the heat solve, as test_heat_solution_matches_direct_solve_of_the_model) against the
    refined direct solve of the model's matrix with heat_rhs_planes, planes on all six walls.
    Measured on MI355X: [9, 6, 70] 4.1e-13 (fixed) 8.8e-13 (flux) 1.0e-12 (mixed); [17, 13, 21] 2.0e-13, 7.4e-13, 2.2e-13."""
    for walls in WALLS:
        g = _gpu_solved(n, walls)
        assert g["stats"]["converged"] == 1, g["stats"]
        assert not np.isnan(g["T"]).any()
        e = relerr(g["T"], _model_solution(n, walls))
        print("heat solve with planes %s %s: relerr %.3e" % (list(n), walls, e))
        assert e < 1e-6, (walls, e)


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_budget_matches_model_on_the_same_field(n):
    """Each of the eight outputs within 1e-12 of the sum of the absolute values of its terms of the longdouble model (the apply test's
    convention; a fixed-order tree sum of N terms errs by about log2 N ulps of that sum), for a random field and for the solved one;
    two calls are bitwise equal, and the field on the device gives the bits of the same field from the host."""
    from pylamp_amd import pylamp3d as P3
    h = _heat_problem(n)
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        A, _ = _make(P3, n, "mixed", ctx, wallvalues=_planes(n, "mixed"))
        Ts = P3.solve_heat(A)
        rng = np.random.default_rng(5)
        for what, T in (("random", rng.uniform(273, 1623, h["n"])), ("solved", Ts)):
            b = P3.heat_budget(A, T)
            out, mag = _model_budget(n, T)
            err = np.abs(HW.LD(1) * _out8(b) - out) / mag
            print("budget %s %s: |gpu - model| / sum|terms| = %s" % (list(n), what, " ".join("%.2e" % float(e) for e in err)))
            assert np.all(err <= 1e-12), (what, err)
            assert b["imbalance"] == b["storage"] - b["source"] - sum(b["wall_flow"])
            assert P3.heat_budget(A, T) == b
        assert P3.heat_budget(A) == b
        assert np.array_equal(Ts, _gpu_solved(n, "mixed")["T"]) and b == _gpu_solved(n, "mixed")["budget"]
    finally:
        ctx.close()


@gpu
def test_solved_field_conserves_heat():
    """The normalised imbalance of the GPU's solved field (planes on all six walls) at the three sizes and wall sets.  The model's own
    value is 7.6e-17 (test_model_budget_telescopes_for_the_direct_solve); the GPU's is the residual of its Krylov solve (rtol 1e-12)
    summed over the interior rows.  Measured on MI355X (fixed, flux, mixed): [5, 5, 5] 4.9e-16, 3.4e-14, 1.1e-13; [9, 6, 70] 1.3e-13,
    1.6e-13, 4.0e-13; [17, 13, 21] 2.7e-13, 2.6e-13, 3.3e-14 (also in profiles/heat_walls3.json); the bound is ten times the largest,
    rounded up to a power of ten."""
    worst = 0.0
    for n in SIZES:
        for walls in WALLS:
            g = _gpu_solved(n, walls)
            v = _normalised(g["budget"])
            print("conservation %s %s: normalised imbalance %.3e (solve residual %.2e, %d iterations)"
                  % (list(n), walls, v, g["stats"]["rel_residual"], g["stats"]["iterations"]))
            worst = max(worst, v)
    assert worst <= CONSERVATION_BOUND <= 1e-6, worst


@gpu
@pytest.mark.parametrize("n", SIZES)
def test_fixflow_wall_flow_is_the_prescribed_flux(n):
    """On a FIXFLOW wall with plane v the flux row pins k dT/dx_a = v at every node, so wall_flow[w] = -+ sum v w_p w_q over its interior
    nodes (- on a low wall, + on a high one), within the conservation bound in the budget's own normalisation.
    Measured on MI355X: at most 3.5e-14 ([9, 6, 70] mixed, xL)."""
    h = _heat_problem(n)
    for walls in ("flow", "mixed"):
        bc = WALLS[walls][0]
        g = _gpu_solved(n, walls)
        b = g["budget"]
        scale = abs(b["storage"]) + abs(b["source"]) + sum(abs(v) for v in b["wall_flow"])
        pl = _planes(n, walls)
        for w in range(6):
            if bc[w] != M.FIXFLOW:
                continue
            want, _ = HW.fixflow_wall_flow(h["n"], h["mid"], w, pl[w])
            e = abs(b["wall_flow"][w] - float(want)) / scale
            print("fixflow %s %s wall %s: flow %.6e prescribed %.6e, difference / scale %.3e" % (list(n), walls, NAMES[w], b["wall_flow"][w], float(want), e))
            assert np.sign(b["wall_flow"][w]) == np.sign(float(want))
            assert e <= CONSERVATION_BOUND, (walls, NAMES[w], e)


# ---- steps -------------------------------------------------------------------------------------------------------------
TR_TMP, TR_HCD, TR_HCP, TR_ALP, TR_IHT = 3, 4, 5, 7, 11
STEP_N = [9, 9, 9]
STEP_L = [100e3, 100e3, 100e3]
REPORT_KEYS = ("it", "tstep", "limiter", "ninjected", "nrefilled", "nempty", "mincount", "nremoved", "time", "ntrac")
SOLVE_KEYS = ("iterations", "converged", "operator_applies", "precond_applies", "rel_residual", "error_estimate")


def _step_tracers():
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = P3.falling_sphere_tracers(STEP_N, STEP_L, np.random.default_rng(7))         # 2 x 2 x 2 tracers per cell
    z, x, y = (tr_x[:, d] / STEP_L[d] for d in range(3))
    tr_f[:, TR_TMP] = 273 + 1350 * z + 40 * np.sin(2 * np.pi * x) * np.sin(np.pi * z) * np.cos(2 * np.pi * y)
    tr_f[:, TR_HCD] = 4.0; tr_f[:, TR_HCP] = 1250.0; tr_f[:, TR_ALP] = 3.5e-5; tr_f[:, TR_IHT] = 1e-9
    return tr_x, tr_f


def _step_profile(shift=0.0):
    """A hot disc on zL (a FIXTEMP wall) and a strip of heat entering through x0 (a FIXFLOW wall: into the box is a negative entry)."""
    g = np.linspace(0, 1, 9)
    X, Y = np.meshgrid(g, g, indexing="ij")
    disc = 1623.0 + 300.0 * ((X - 0.5 - shift) ** 2 + (Y - 0.5) ** 2 < 0.3 ** 2)
    strip = np.zeros((9, 9)); strip[3:6, :] = -0.02
    return {"zL": disc, "x0": strip}


def _run_steps(resident, profile, change=None, nstep=3):
    """nstep steps; `change`: the profile set between steps 2 and 3."""
    from pylamp_amd import pylamp3d as P3
    tr_x, tr_f = _step_tracers()
    sim = P3.Simulation3(STEP_N, STEP_L, tr_x, tr_f, P3.Options3(resident=resident, bcheatprofile=profile))
    out = []
    try:
        for it in range(nstep):
            if it == 2 and change is not None:
                sim.set_heat_profile(change)
            sim.transfer_stats(reset=True)
            rep = sim.step()
            xf = sim.transfer_stats(reset=True)
            out.append(dict(rep=rep, xfer=xf, temp=sim.field("temp").copy(), budget=sim.heat_budget() if profile is not None else None))
    finally:
        sim.close()
    return out


class _counted:
    """Counts the calls of library entries through ctypes while the block runs."""

    def __init__(self, *names):
        from pylamp_amd import _lib
        self.lib, self.names, self.calls = _lib.load(), names, []

    def __enter__(self):
        self.real = {k: getattr(self.lib, k) for k in self.names}
        for k, f in self.real.items():
            setattr(self.lib, k, lambda *a, _k=k, _f=f: (self.calls.append(_k), _f(*a))[1])
        return self.calls

    def __exit__(self, *exc):
        for k, f in self.real.items():
            setattr(self.lib, k, f)


@pytest.fixture(scope="module")
def stepped():
    prof = _step_profile()
    out = {}
    for path, resident in (("staged", False), ("resident", True)):
        with _counted("pl3_heat_set_wall_values") as calls:
            out[path] = _run_steps(resident, prof)
            out[path + "_sets"] = len(calls)
            out[path + "_moved"] = _run_steps(resident, prof, _step_profile(0.2))
            out[path + "_moved_sets"] = len(calls) - out[path + "_sets"]
    return out


def _assert_same_steps(a, b):
    for it, (s, r) in enumerate(zip(a, b)):
        tag = "step %d: " % (it + 1)
        assert list(s["rep"]) == list(r["rep"]), tag + "report keys"
        for k in REPORT_KEYS:
            assert s["rep"][k] == r["rep"][k], tag + k
        for k in ("stokes", "heat"):
            for q in SOLVE_KEYS:
                assert s["rep"][k][q] == r["rep"][k][q], tag + k + " " + q
            assert s["rep"][k]["converged"] == 1
        assert np.array_equal(s["temp"], r["temp"]), tag + "temp"
        assert s["budget"] == r["budget"], tag + "budget"


@gpu
def test_steps_with_a_profile_agree_bitwise_between_the_paths(stepped):
    _assert_same_steps(stepped["staged"], stepped["resident"])
    _assert_same_steps(stepped["staged_moved"], stepped["resident_moved"])
    for s in stepped["resident"]:
        b = s["budget"]
        print("step %d: wall flows %s storage %.4e source %.4e normalised imbalance %.2e"
              % (s["rep"]["it"], " ".join("%.3e" % v for v in b["wall_flow"]), b["storage"], b["source"], _normalised(b)))
        assert _normalised(b) <= STEP_CONSERVATION_BOUND
        # The disc holds the nodes of zL at their plane entries, the strip feeds heat in through x0, and xL stays insulating.  The wall
        # rows are met to the solve's residual: 1e-12 of |b| <= 1923 sqrt(729) is 5e-8 K on an identity row; 1e-6 leaves a margin.
        assert np.abs(s["temp"][-1] - _step_profile()["zL"]).max() <= 1e-6
        assert b["wall_flow"][1] > 0 and abs(b["wall_flow"][4]) < 1e-6 * b["wall_flow"][1]
    # the planes go to the context once, at construction, and once more per set_heat_profile: never per step
    assert stepped["staged_sets"] == 1 and stepped["resident_sets"] == 1
    assert stepped["staged_moved_sets"] == 2 and stepped["resident_moved_sets"] == 2


@gpu
def test_set_heat_profile_acts_from_the_next_step(stepped):
    for path in ("staged", "resident"):
        same, moved = stepped[path], stepped[path + "_moved"]
        for it in (0, 1):
            assert np.array_equal(same[it]["temp"], moved[it]["temp"]) and same[it]["budget"] == moved[it]["budget"]
        assert not np.array_equal(same[2]["temp"], moved[2]["temp"])
        assert np.abs(moved[2]["temp"][-1] - _step_profile(0.2)["zL"]).max() <= 1e-6


@gpu
def test_without_a_profile_the_new_entries_are_not_called(stepped):
    """Options3.bcheatprofile = None: neither path touches pl3_heat_set_wall_values / pl3_heat_get_wall_values / pl3_heat_budget, and
    the errors of Simulation3.heat_budget are raised before the library is asked."""
    from pylamp_amd import pylamp3d as P3
    with _counted("pl3_heat_set_wall_values", "pl3_heat_get_wall_values", "pl3_heat_budget") as calls:
        plain = {path: _run_steps(path == "resident", None, nstep=2) for path in ("staged", "resident")}
        for it in range(2):
            assert np.array_equal(plain["staged"][it]["temp"], plain["resident"][it]["temp"])
            assert not np.array_equal(plain["resident"][it]["temp"], stepped["resident"][it]["temp"])
        tr_x, tr_f = _step_tracers()
        sim = P3.Simulation3(STEP_N, STEP_L, tr_x, tr_f, P3.Options3())
        try:
            with pytest.raises(Exception, match="Simulation3.heat_budget: no step has run yet"):
                sim.heat_budget()
            sim.set_heat_profile(None)                     # nothing set, nothing to clear
        finally:
            sim.close()
        sim = P3.Simulation3(STEP_N, STEP_L, tr_x, tr_f, P3.Options3(do_heatdiff=False))
        try:
            with pytest.raises(Exception, match="Simulation3.heat_budget: the heat solve is off"):
                sim.heat_budget()
            with pytest.raises(Exception, match="Simulation3.set_heat_profile: a profile over the heat walls needs the heat solve"):
                sim.set_heat_profile({"zL": 1700.0})
        finally:
            sim.close()
        assert calls == []


# ---- errors ------------------------------------------------------------------------------------------------------------
@gpu
def test_errors_name_the_entry():
    from pylamp_amd import pylamp3d as P3, _lib
    n = (9, 6, 70)
    h = _heat_problem(n)
    ctx = P3.Context3(h["n"], h["grid"])
    try:
        out = np.zeros(8)
        assert ctx.lib.pl3_heat_budget(ctx.handle(), None, _lib.dptr(out)) != 0
        msg = ctx.lib.pl3_last_error(ctx.handle())
        assert b"pl3_heat_budget" in msg and b"heat operator not set" in msg, msg
        with pytest.raises(Exception, match=r"heat wall y0 need the shape \(nz, nx\) = \(9, 6\)"):
            ctx.set_heat_wall_values({"y0": np.zeros((6, 9))})
        # the library's own check of the entries that are read (handed over without the Python validator)
        v = np.zeros((9, 70)); v[0, 3] = v[8, 0] = np.nan
        ptr = (_lib.c_double_p * 6)(None, _lib.dptr(v), None, None, None, None)
        assert ctx.lib.pl3_heat_set_wall_values(ctx.handle(), ptr) == 0
        assert [b is not None for b in ctx.heat_wall_values()] == [False, True, False, False, False, False]
        v[5, 69] = np.inf
        assert ctx.lib.pl3_heat_set_wall_values(ctx.handle(), ptr) != 0
        msg = ctx.lib.pl3_last_error(ctx.handle())
        assert b"pl3_heat_set_wall_values: wall x0 has a non-finite entry [5, 69] = inf" in msg, msg
        assert np.array_equal(ctx.heat_wall_values()[1][5], np.zeros(70))              # a rejected call changes nothing
        ctx.set_heat_wall_values(None)
        assert ctx.heat_wall_values() == [None] * 6
        A, _ = _make(P3, n, "mixed", ctx)
        with pytest.raises(Exception, match="pl3_heat_budget: NULL T means the solution of the last heat solve, and no heat solve has run"):
            P3.heat_budget(A)
        with pytest.raises(Exception, match="dimension mismatch"):
            P3.heat_budget(A, np.zeros(7))
        assert np.isfinite(_out8(P3.heat_budget(A, h["T0"]))).all()                   # a given field needs no solve
    finally:
        ctx.close()
    vc = P3.VirtualCluster3(h["n"], h["grid"], 2, 1, 1)
    try:
        c0 = vc.ctxs[0]
        with pytest.raises(Exception, match="pl3_heat_set_wall_values: .*one rank .*pl3_set_comm"):
            c0.set_heat_wall_values({"zL": 1.0})
        with pytest.raises(Exception, match="pl3_heat_get_wall_values: .*one rank .*pl3_set_comm"):
            c0.heat_wall_values()
        assert c0.lib.pl3_heat_budget(c0.handle(), _lib.dptr(h["T0"]), _lib.dptr(out)) != 0
        msg = c0.lib.pl3_last_error(c0.handle())
        assert b"pl3_heat_budget" in msg and b"one rank" in msg and b"pl3_set_comm" in msg, msg
    finally:
        vc.close()
