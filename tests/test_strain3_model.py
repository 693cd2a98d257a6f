"""CPU checks that earn tests/stokes3_strain_model.py (the NumPy model of the 3-D strain-rate, stress and dissipation fields) its
authority: (a) the divergence of its stresses plus the pressure gradient IS the momentum row of the operator models (free-slip, no-slip,
moving walls; natural and strict rows), (b) it is exact on fields with constant velocity gradients, (c) the node fields conserve the
integral of the dissipation, (d) on a direct solve of a closed box the dissipation balances the work of buoyancy."""
import numpy as np
import pytest

import stokes3_model as M
import stokes3_moving_model as V
import stokes3_strain_model as S
import stokes3_walls_model as W

LD = np.longdouble
EPS = np.finfo(np.float64).eps
N, F = W.NOSLIP, W.FREESLIP
STD = [9, 7, 11]
LEN = [1.0e5, 1.3e5, 0.9e5]


def graded(n, L, ratio=4.0):
    """Spacings that grow geometrically by `ratio` from the first cell to the last."""
    h = float(ratio) ** np.linspace(0.0, 1.0, int(n) - 1)
    c = np.concatenate([[0.0], np.cumsum(h)]) * (float(L) / h.sum())
    c[-1] = float(L)
    return c


def make_grid(n, L, kind):
    return [np.linspace(0.0, L[a], n[a]) if kind == "regular" else graded(n[a], L[a]) for a in range(3)]


def random_case(n, grid, seed, contrast=3.0):
    """Random viscosities with 10^contrast between the smallest and the largest, random velocities and pressure."""
    rng = np.random.default_rng(seed)
    etas = 1e19 * 10 ** rng.uniform(0.0, contrast, n)
    etan = 1e19 * 10 ** rng.uniform(0.0, contrast, n)
    etas.flat[0], etas.flat[-1] = 1e19, 1e19 * 10 ** contrast
    v = [rng.standard_normal(n) * 1e-9 for _ in range(3)]
    P = rng.standard_normal(n) * 1e-3
    return etas, etan, v, P


def tangential(seed, walls=range(6)):
    """Random tangential velocities of the given walls, (6, 3)."""
    rng = np.random.default_rng(seed)
    U = np.zeros((6, 3))
    for w in walls:
        U[w] = rng.standard_normal(3) * 1e-9
        U[w, w % 3] = 0.0
    return U


# ---- (a) the stresses' divergence is the operator's row ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "graded"])
@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("walls", ["freeslip", "noslip", "mixed", "moving"])
def test_divergence_of_the_stresses_is_the_momentum_row(kind, strict, walls):
    n = STD
    grid = make_grid(n, LEN, kind)
    etas, etan, v, P = random_case(n, grid, 11)
    bc = dict(freeslip=None, noslip=[N] * 6, mixed=[N, F, N, F, N, F], moving=[N] * 6)[walls]
    U = tangential(12) if walls == "moving" else None
    Kc = M.scaling(grid, etas, etan)[0]
    x = np.stack(v + [P], axis=-1).reshape(-1)
    res = S.strain_fields(n, grid, etas, etan, v, bc=bc, wallvel=U)
    rows, mags = S.stress_divergence(n, grid, etan, res, P, Kc)
    ref = np.array(W.stokes_apply(n, grid, etas, etan, x, bc=bc, strict=strict, rounded=False), dtype=LD).reshape(n + [4])
    if U is not None:        # the operator keeps the wall's velocity on the right-hand side: div(stress) = A v - (the walls' terms)
        ref = ref - V.wall_rhs(n, grid, etas, etan, bc, U, strict)
    count = 0
    for D in range(3):
        interior = M.velocity_classes(D, n, strict)[0]
        err = np.abs(rows[..., D] - ref[..., D])[interior]
        bound = (32 * EPS * mags[..., D])[interior]
        assert np.all(mags[..., D][interior] > 0)
        assert np.all(err <= bound), (D, float((err / bound).max()))
        count += int(interior.sum())
    assert count > 0
    if walls != "freeslip" and not strict:         # the walls' terms are in the rows that were compared
        free = S.strain_fields(n, grid, etas, etan, v)
        assert any(np.abs(res["eDE"][p] - free["eDE"][p]).max() > 0 for p in range(3))


# ---- (b) exact fields -----------------------------------------------------------------------------------------------------------------
def _positions(grid):
    """Per component the coordinate arrays of its staggered position, broadcastable: pos[D][a] is the coordinate along a of v_D."""
    c = [np.asarray(g, dtype=LD) for g in grid]
    mid = [np.append((g[1:] + g[:-1]) / 2, g[-1]) for g in c]           # (the last midpoint is a ghost)
    pos = []
    for D in range(3):
        pos.append([S._along(c[a] if a == D else mid[a], a) for a in range(3)])
    return pos


@pytest.mark.parametrize("kind", ["regular", "graded"])
def test_rigid_rotation_has_no_strain(kind):
    """v = Omega r with an antisymmetric Omega: every component vanishes inside.  (On a wall edge the definition drops the half of the
    shear that the free-slip rows drop, so the nodes ON the walls see half the rotation: they are left out.)"""
    n = STD
    grid = make_grid(n, LEN, kind)
    pos = _positions(grid)
    om = np.array([[0.0, 3.0, -2.0], [-3.0, 0.0, 1.5], [2.0, -1.5, 0.0]], dtype=LD) * 1e-14
    v = [sum(om[D, a] * pos[D][a] for a in range(3)) + np.zeros(n, dtype=LD) for D in range(3)]
    eta = np.full(n, 1e21)
    res = S.strain_fields(n, grid, eta, eta, v)
    inner = (slice(1, -1),) * 3
    w = float(np.abs(om).max())
    assert float(res["strainrate"][inner].max()) <= 1e-15 * w
    assert float(res["stress"][inner].max()) <= 1e-15 * w * 2e21
    assert float(res["dissipation"][inner].max()) <= 1e-30 * w * w * 1e21
    assert float(res["strainrate"][0, 1:-1, 1:-1].min()) > 0.1 * w                     # (the z0 wall nodes: not rigid by the definition)


@pytest.mark.parametrize("kind", ["regular", "graded"])
@pytest.mark.parametrize("zwalls", ["moving", "freeslip"])
def test_simple_shear(kind, zwalls):
    """v_x = gamma z: eps_II = gamma / 2, tau_II = eta gamma and Phi = eta gamma^2 at every node when the z walls are no-slip and move
    with the field; with free-slip z walls at every node off those walls."""
    n = STD
    grid = make_grid(n, LEN, kind)
    pos = _positions(grid)
    gam, eta0 = LD(3e-14), 1e21
    v = [np.zeros(n, dtype=LD), gam * pos[1][0] + np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)]
    eta = np.full(n, eta0)
    bc, U = None, None
    if zwalls == "moving":
        bc = [N, F, F, N, F, F]
        U = np.zeros((6, 3), dtype=LD); U[3, 1] = gam * LD(grid[0][-1])
    res = S.strain_fields(n, grid, eta, eta, v, bc=bc, wallvel=U)
    sel = (slice(None),) * 3 if zwalls == "moving" else (slice(1, -1), slice(None), slice(None))
    assert np.all(np.abs(res["strainrate"][sel] - gam / 2) <= 1e-15 * gam)
    assert np.all(np.abs(res["stress"][sel] - eta0 * gam) <= 1e-15 * eta0 * gam)
    assert np.all(np.abs(res["dissipation"][sel] - eta0 * gam * gam) <= 1e-15 * eta0 * gam * gam)
    if zwalls == "freeslip":
        assert np.all(res["strainrate"][0] == 0)                            # all of the shear of a free-slip wall edge is dropped here
    vol = np.prod([float(g[-1] - g[0]) for g in grid])
    if zwalls == "moving":
        assert abs(res["total"] - eta0 * gam * gam * vol) <= 1e-15 * eta0 * gam * gam * vol


@pytest.mark.parametrize("kind", ["regular", "graded"])
def test_pure_shear(kind):
    """v_z = a z, v_x = -a x: eps_zz = a, eps_xx = -a, so eps_II = |a|, tau_II = 2 eta |a|, Phi = 4 eta a^2 at every node."""
    n = STD
    grid = make_grid(n, LEN, kind)
    pos = _positions(grid)
    a, eta0 = LD(2e-14), 1e20
    v = [a * pos[0][0] + np.zeros(n, dtype=LD), -a * pos[1][1] + np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)]
    eta = np.full(n, eta0)
    res = S.strain_fields(n, grid, eta, eta, v)
    assert np.all(np.abs(res["strainrate"] - a) <= 1e-15 * a)
    assert np.all(np.abs(res["stress"] - 2 * eta0 * a) <= 1e-15 * 2 * eta0 * a)
    assert np.all(np.abs(res["dissipation"] - 4 * eta0 * a * a) <= 1e-15 * 4 * eta0 * a * a)
    assert all(np.all(e == 0) for e in res["eDE"])


# ---- (c) the node fields conserve the integral ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "graded"])
@pytest.mark.parametrize("walls", ["freeslip", "moving"])
def test_node_sum_is_centres_plus_edges(kind, walls):
    n = STD
    grid = make_grid(n, LEN, kind)
    etas, etan, v, _ = random_case(n, grid, 21)
    bc, U = ([N] * 6, tangential(22)) if walls == "moving" else (None, None)
    res = S.strain_fields(n, grid, etas, etan, v, bc=bc, wallvel=U)
    assert res["total_centres"] > 0 and res["total_edges"] > 0
    assert abs(res["total_nodes"] - res["total"]) <= 1e-16 * res["total"]
    assert res["mag_total"] >= res["total"]
    for k in ("strainrate", "stress", "dissipation"):
        assert np.all(np.isfinite(res["mag"][k])) and np.all(res["mag"][k] > 0)
    assert abs(np.sum(res["vol_nodes"]) - np.prod([LD(g[-1]) - LD(g[0]) for g in grid])) <= 1e-17 * np.prod(LEN)


# ---- (d) energy ---------------------------------------------------------------------------------------------------------------------------
def test_dissipation_balances_the_work_of_buoyancy():
    """A closed free-slip box, natural rows, a dense stiff blob, solved directly: multiply every momentum row by its velocity and its
    control volume and sum -- the stresses integrate by parts into -(the integral of the dissipation), the pressure term into Kc sum P
    div v V = 0, so the integral of Phi = -sum v b V with b the right-hand side.  The identity holds to the residual of the solve."""
    n = STD
    grid = make_grid(n, LEN, "regular")
    Z, X, Y = np.meshgrid(*grid, indexing="ij")
    blob = ((Z - 0.4 * LEN[0]) ** 2 + (X - 0.5 * LEN[1]) ** 2 + (Y - 0.45 * LEN[2]) ** 2) < (0.25 * LEN[0]) ** 2
    rho = np.where(blob, 3400.0, 3300.0)
    etas = np.where(blob, 1e21, 1e20)
    mid = [np.append((g[1:] + g[:-1]) / 2, g[-1]) for g in grid]
    Zc, Xc, Yc = np.meshgrid(*mid, indexing="ij")
    etan = np.where(((Zc - 0.4 * LEN[0]) ** 2 + (Xc - 0.5 * LEN[1]) ** 2 + (Yc - 0.45 * LEN[2]) ** 2) < (0.25 * LEN[0]) ** 2, 1e21, 1e20)
    ap = lambda x, rounded=True: M.stokes_apply(n, grid, etas, etan, x, strict=False, rounded=rounded)
    b = M.stokes_rhs(n, grid, etas, etan, rho, strict=False)
    solver = M.DirectSolver(M.assemble(ap, n), ap)
    x = solver.solve(b)
    assert 0 < solver.residual <= 1e-12
    X4 = np.asarray(x).reshape(n + [4])
    v = [X4[..., q] for q in range(3)]
    res = S.strain_fields(n, grid, etas, etan, v)
    d, h = S.widths(grid)
    B = np.asarray(b, dtype=LD).reshape(n + [4])
    work = LD(0)
    for D, E, Fq in S.PAIRS:
        vol = S._along(h[D], D) * S._along(np.append(d[E], 0), E) * S._along(np.append(d[Fq], 0), Fq)
        work = work + np.sum(S._ld(v[D]) * B[..., D] * vol)
    total = res["total"]
    assert total > 0 and work < 0
    defect = abs(total + work) / total
    print("dissipation %.6e W, work of buoyancy %.6e W, defect %.3e, residual of the solve %.3e" % (float(total), float(-work), float(defect), solver.residual))
    assert defect <= 100 * solver.residual
