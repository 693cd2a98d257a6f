"""CPU checks of tests/stokes3_yield_model.py (the NumPy model of the 3-D yield stress) and of the inputs that tests/test_hip_3d_yield.py
gives the HIP kernel: (a) discrete Couette flow yields uniformly to tau_y / (2 e), (b) centre and node invariants agree on a uniform strain
field, (c) eta_eff never exceeds eta_mat and e = 0 keeps it, (d) eta_eff is continuous across the switch, (e) every kernel test input has
no ambiguous entry and yields between 10 % and 90 % of its entries, (f) the model's Picard loop on the blob reduces its change
monotonically."""
import numpy as np
import pytest

import stokes3_moving_model as V
import stokes3_strain_model as S
import stokes3_walls_model as W
import stokes3_yield_model as Y
from test_strain3_model import make_grid, random_case, _positions

LD = np.longdouble
EPS = np.finfo(np.float64).eps
N_, F_ = W.NOSLIP, W.FREESLIP
LEN = [1.0e5, 1.3e5, 0.9e5]
# the shapes of tests/test_hip_3d_strain.py, and one whose per-node grid has 1 x 6 x 33 = 198 workgroups: more than the 128 groups of the
# first finishing launch of the yield reduction, so that a group combines two partials and 29 groups hold none
SHAPES = ([17, 13, 21], [7, 9, 67], [5, 5, 5], [6, 70, 5], [33, 21, 5])
KINDS = ("regular", "graded")
WALLS = ("freeslip strict", "noslip all", "moving z0", "through-flow x")


def between(values, q):
    """The geometric mean of the two neighbours in the sorted values at the quantile q: a threshold that is none of the values."""
    s = np.sort(np.asarray(values, dtype=np.float64).ravel())
    i = min(max(int(q * s.size), 0), s.size - 2)
    return float(np.sqrt(s[i] * s[i + 1]))


def kernel_case(n, kind, wall):
    """One input of the kernel test: a dict with grid, etas, etan, v (the wall-normal velocities carry the flow), P, bc, strict, wallvel,
    wallflow and the yield setting tau0, dtau_dz, eta_floor.  tau0 lies at a quantile of 2 eta e over the nodes and cells of the case (between
    two neighbouring values, so that no entry sits on the switch), so that
    a good part of the entries yields; dtau_dz is zero for two wall cases and doubles tau_y over the depth for the two others; the floor
    binds in the "noslip all" case (the 30 % quantile of tau_y / (2 e) over the entries)."""
    grid = make_grid(n, LEN, kind)
    etas, etan, v, P = random_case(n, grid, 31 + n[2])
    rng = np.random.default_rng(5)
    U = 2e-9
    mv = np.zeros((6, 3)); mv[0] = (0.0, U, U / 2)
    prof = rng.uniform(0.5, 1.5, (n[0] - 1, n[2] - 1)) * 1e-9        # the same plane on x0 and xL: the net flux vanishes
    bc, strict, wallvel, flow = {"freeslip strict": ([F_] * 6, True, None, None), "noslip all": ([N_] * 6, False, None, None),
                                 "moving z0": ([N_, F_, F_, N_, F_, F_], False, mv, None),
                                 "through-flow x": ([F_] * 6, True, None, [None, prof, None, None, prof, None])}[wall]
    vv = [a.copy() for a in v]
    if flow is not None:
        vv[1][:-1, 0, :-1] = flow[1]; vv[1][:-1, -1, :-1] = flow[4]
    res = S.strain_fields(n, grid, etas, etan, vv, bc=bc, wallvel=wallvel)
    e_c, _ = Y.centre_invariant(res)
    cells = tuple(slice(0, k - 1) for k in n)
    s2 = np.concatenate([(2 * S._ld(etas) * res["strainrate"]).ravel(), (2 * S._ld(etan)[cells] * e_c).ravel()]).astype(np.float64)
    gradient = wall in ("noslip all", "through-flow x")
    tau0 = between(s2, 0.35 if gradient else 0.5)
    dtau_dz = tau0 / LEN[0] if gradient else 0.0
    floor = float(np.finfo(np.float64).tiny)
    if wall == "noslip all":
        tn, tc = Y.tau_y(grid, n, tau0, dtau_dz)
        lim = np.concatenate([((tn + np.zeros(n, dtype=LD)) / (2 * res["strainrate"])).ravel(), ((tc + np.zeros(e_c.shape, dtype=LD)) / (2 * e_c)).ravel()])
        floor = between(lim, 0.3)
    return dict(n=n, grid=grid, etas=etas, etan=etan, v=vv, P=P, bc=bc, strict=strict, wallvel=wallvel, wallflow=flow, tau0=tau0,
                dtau_dz=dtau_dz, eta_floor=floor)


def model_of(case):
    return Y.effective(case["n"], case["grid"], case["etas"], case["etan"], case["v"], case["tau0"], case["dtau_dz"], case["eta_floor"],
                       bc=case["bc"], wallvel=case["wallvel"])


# ---- (a) Couette ------------------------------------------------------------------------------------------------------------------------
def couette(n, L, U, eta0):
    """Discrete Couette flow: the lid z0 moves along x with U, the wall zL rests, both NOSLIP; x and y walls free-slip, the x walls carry
    the profile as a flow through them (a closed box would turn the shear flow into a cavity flow), gravity off, uniform viscosity.
    v_x = U (1 - z / Lz) at the mid-points of the cells along z."""
    grid = [np.linspace(0.0, L[a], n[a]) for a in range(3)]
    zm = (grid[0][1:] + grid[0][:-1]) / 2
    prof = np.repeat((U * (1 - zm / L[0]))[:, None], n[2] - 1, axis=1)
    vx = np.zeros(n); vx[:-1, :, :-1] = (U * (1 - zm / L[0]))[:, None, None]
    wallvel = np.zeros((6, 3)); wallvel[0, 1] = U
    eta = np.full(n, eta0)
    return dict(grid=grid, eta=eta, v=[np.zeros(n), vx, np.zeros(n)], bc=[N_, F_, F_, N_, F_, F_], wallvel=wallvel,
                wallflow=[None, prof, None, None, prof, None], rho=np.full(n, 3300.0))


@pytest.mark.parametrize("strict", [False, True])
def test_couette_flow_yields_uniformly(strict):
    n, L, U, eta0 = [9, 9, 9], [1.0e5, 1.0e5, 1.0e5], 1e-9, 1e21
    c = couette(n, L, U, eta0)
    e = U / (2 * L[0])
    # it is the discrete solution: the momentum rows of the operator model vanish on it (the pressure is zero)
    x = np.stack(c["v"] + [np.zeros(n)], axis=-1).reshape(-1)
    Ax = np.asarray(W.stokes_apply(n, c["grid"], c["eta"], c["eta"], x, bc=c["bc"], strict=strict, rounded=False), dtype=LD).reshape(n + [4])
    b = np.asarray(V.stokes_rhs(n, c["grid"], c["eta"], c["eta"], c["rho"], grav=[0.0, 0.0, 0.0], bc=c["bc"], wallvel=c["wallvel"], strict=strict,
                                rounded=False), dtype=LD).reshape(n + [4])
    inner = (slice(None, -1), slice(1, -1), slice(None, -1))            # the rows of v_x inside (the wall-normal ones carry the flow)
    scale = float(np.abs(Ax[..., 1]).max()) + 2 * eta0 * U / (L[0] / (n[0] - 1)) ** 2
    assert float(np.abs(Ax[..., 1] - b[..., 1])[inner].max()) <= 1e-12 * scale
    for tau, yields in ((0.5 * 2 * eta0 * e, True), (2.0 * 2 * eta0 * e, False)):
        u = Y.effective(n, c["grid"], c["eta"], c["eta"], c["v"], tau, 0.0, 1e15, bc=c["bc"], wallvel=c["wallvel"])
        assert float(np.abs(u["e_n"] - e).max()) <= 1e-14 * e and float(np.abs(u["e_c"] - e).max()) <= 1e-14 * e
        cells = (slice(0, -1),) * 3
        if yields:
            assert u["yielded_s"].all() and u["yielded_n"][cells].all() and not u["yielded_n"][-1].any()
            assert float(np.abs(u["etas_eff"] - tau / (2 * e)).max()) <= 1e-14 * tau / (2 * e)
            assert float(np.abs(u["etan_eff"][cells] - tau / (2 * e)).max()) <= 1e-14 * tau / (2 * e)
            stress = Y.node_stress(n, c["grid"], u["etas_eff"], u["etan_eff"], c["v"], bc=c["bc"], wallvel=c["wallvel"])
            assert float(np.abs(stress - tau).max()) <= 1e-14 * tau                  # the flow carries exactly the yield stress
        else:
            assert not u["yielded_s"].any() and not u["yielded_n"].any()
            assert np.array_equal(u["etas_eff"], c["eta"]) and np.array_equal(u["etan_eff"], c["eta"]) and u["change"] == 0.0


# ---- (b) uniform strain -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", ["simple shear", "pure shear"])
def test_centre_and_node_invariants_agree_on_a_uniform_strain_field(kind, field):
    """Simple shear v_x = g z between no-slip z walls that move with it (both invariants g / 2), and pure shear v_z = a z, v_x = -a x in a
    free-slip box (both |a|): every component is constant, so centres and nodes see the same invariant."""
    n = [9, 7, 11]
    grid = make_grid(n, LEN, kind)
    pos = _positions(grid)
    a, g = LD(2e-14), LD(3e-14)
    zero = np.zeros(n, dtype=LD)
    if field == "simple shear":
        v, bc, want = [zero, g * pos[1][0] + zero, zero], [N_, F_, F_, N_, F_, F_], g / 2
        U = np.zeros((6, 3), dtype=LD); U[3, 1] = g * LD(grid[0][-1])
    else:
        v, bc, U, want = [a * pos[0][0] + zero, -a * pos[1][1] + zero, zero], None, None, a
    res = S.strain_fields(n, grid, np.full(n, 1e21), np.full(n, 1e21), v, bc=bc, wallvel=U)
    e_c, mag_c = Y.centre_invariant(res)
    assert float(np.abs(e_c - want).max()) <= 1e-15 * want
    assert float(np.abs(res["strainrate"] - want).max()) <= 1e-15 * want
    assert np.all(mag_c >= e_c * (1 - 1e-15))


# ---- (c), (d) properties ------------------------------------------------------------------------------------------------------------------
def test_eta_eff_never_exceeds_the_material_viscosity_and_rest_keeps_it():
    n = [9, 7, 11]
    case = kernel_case(n, "graded", "noslip all")
    u = model_of(case)
    assert np.all(u["etas_eff"] <= S._ld(case["etas"])) and np.all(u["etan_eff"] <= S._ld(case["etan"]))
    assert np.all(u["etas_eff"] >= min(case["eta_floor"], case["etas"].min())) and u["min_eta"] > 0
    assert np.array_equal(u["etan_eff"][-1], case["etan"][-1]) and np.array_equal(u["etan_eff"][:, :, -1], case["etan"][:, :, -1])
    rest = Y.effective(n, case["grid"], case["etas"], case["etan"], [np.zeros(n)] * 3, case["tau0"], case["dtau_dz"], case["eta_floor"])
    assert np.array_equal(rest["etas_eff"], case["etas"]) and np.array_equal(rest["etan_eff"], case["etan"])
    assert not rest["yielded_s"].any() and not rest["yielded_n"].any() and rest["change"] == 0.0
    assert not rest["B_s"].any() and not rest["ambiguous_s"].any()


def test_eta_eff_is_continuous_across_the_switch():
    """Scale a velocity field through the point where a node starts to yield: eta_eff at that node moves by no more than the scaling."""
    n = [9, 7, 11]
    case = kernel_case(n, "regular", "freeslip strict")
    u = model_of(case)
    ratio = (2 * S._ld(case["etas"]) * u["e_n"]) / LD(case["tau0"])           # > 1: yielded
    at = np.unravel_index(np.argmin(np.abs(np.log(ratio))), n)
    s0 = float(1 / ratio[at])                                                # scaling the velocities by s0 puts the node on the switch
    vals = []
    for s in (s0 * (1 - 1e-9), s0, s0 * (1 + 1e-9)):
        w = Y.effective(n, case["grid"], case["etas"], case["etan"], [a * s for a in case["v"]], case["tau0"], 0.0, case["eta_floor"])
        vals.append((w["etas_eff"][at], bool(w["yielded_s"][at])))
    mat = LD(case["etas"][at])
    assert vals[0] == (mat, False) and vals[2][1]
    assert abs(vals[2][0] - mat) <= 2e-9 * mat and abs(vals[1][0] - mat) <= 1e-15 * mat


# ---- (e) the inputs of the kernel test ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", SHAPES, ids=lambda n: "x".join(str(v) for v in n))
def test_kernel_test_inputs_are_unambiguous_and_yield_partly(n, kind):
    floor_binds = 0
    for wall in WALLS:
        case = kernel_case(n, kind, wall)
        u = model_of(case)
        cells = tuple(slice(0, k - 1) for k in n)
        assert int(u["ambiguous_s"].sum()) == 0 and int(u["ambiguous_n"].sum()) == 0, wall
        entries = u["yielded_s"].size + u["yielded_n"][cells].size
        frac = (int(u["yielded_s"].sum()) + int(u["yielded_n"].sum())) / entries
        print("%s %s %s: %.1f %% of the entries yield" % (n, kind, wall, 100 * frac))
        assert 0.1 <= frac <= 0.9, (wall, frac)
        assert (case["dtau_dz"] != 0.0) == (wall in ("noslip all", "through-flow x"))
        assert np.all(np.isfinite(u["B_s"])) and np.all(u["B_s"][u["yielded_s"]] > 0)
        floor_binds += int((u["etas_eff"] == LD(case["eta_floor"])).sum())
        if wall == "noslip all":
            assert int((u["etas_eff"] == LD(case["eta_floor"])).sum()) > 0 and int((u["etan_eff"] == LD(case["eta_floor"])).sum()) > 0
    assert floor_binds > 0


# ---- (f) the fixed point ------------------------------------------------------------------------------------------------------------------
def blob(n, L):
    """The blob of tests/test_hip_3d_strain.py: a dense, stiff sphere given at the nodes (etan takes the node values)."""
    grid = [np.linspace(0, L[a], n[a]) for a in range(3)]
    Z, X, Yc = np.meshgrid(*grid, indexing="ij")
    inside = ((Z - 0.4 * L[0]) ** 2 + (X - 0.5 * L[1]) ** 2 + (Yc - 0.45 * L[2]) ** 2) < (0.25 * L[0]) ** 2
    return grid, np.where(inside, 1e21, 1e20), np.where(inside, 1e21, 1e20), np.where(inside, 3400.0, 3300.0)


def blob_tau0(n, grid, etas, etan, rho, bc):
    """The median of the model's node stress after the model's first direct solve, and that solve's solver (for Y.picard(reuse=...))."""
    keep = []
    x = Y.direct(n, grid, etas, etan, rho, bc=bc, keep=keep)
    X = x.reshape(list(n) + [4])
    return float(np.median(Y.node_stress(n, grid, etas, etan, [X[..., q] for q in range(3)], bc=bc).astype(np.float64))), keep[0]


def test_picard_loop_of_the_model_contracts_on_the_blob():
    n, L = [9, 7, 11], LEN
    grid, etas, etan, rho = blob(n, L)
    bc = [N_, F_, F_, N_, F_, F_]
    tau0, _ = blob_tau0(n, grid, etas, etan, rho, bc)
    out = Y.picard(n, grid, etas, etan, rho, tau0, 0.0, 1e19, 3, tol=0.0, bc=bc)
    print("model Picard loop on the blob: change", out["change"], "yielded nodes", out["yielded_nodes"])
    assert out["iterations"] == 3 and not out["converged"]
    assert out["change"][0] > out["change"][1] > out["change"][2] > 0
    assert 0 < out["yielded_nodes"][0] < int(np.prod(n))
