"""CPU checks that earn tests/stokes3_moving_model.py (the NumPy model of moving no-slip walls) its authority: at rest it IS
tests/stokes3_walls_model.py, its right-hand side is linear in the wall velocities wall by wall, its rows vanish for the field that is
linear in the wall distance and equals U on the wall, a y-invariant lid-driven problem reproduces the 2-D oracle's solution, and its
advection ghosts put U on the wall.  The rejections of the model and of the pure-Python validation of pylamp3d are checked by message."""
import numpy as np
import pytest
import scipy.sparse.linalg as spla

import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W
from test_stokes3_model import _extrude, _fields3, _nonuniform

LD = np.longdouble
N, F = W.NOSLIP, W.FREESLIP
ALL = [N] * 6
GRAV = (3.0, -4.0, 5.0)


def _vel(**kw):
    """_vel(z0=(0, 1, 2), xL=...) -> (6, 3)"""
    U = np.zeros((6, 3))
    for k, v in kw.items():
        U[W.WALLS.index(k)] = v
    return U


TWO = _vel(z0=(0.0, 2e-9, -1e-9), xL=(3e-9, 0.0, 0.5e-9))          # z0 and xL share a cube edge


def test_walls_at_rest_are_the_walls_model():
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 231)
    rng = np.random.default_rng(232)
    vel = [rng.standard_normal(n) for _ in range(3)]
    gm = [np.append((c[1:] + c[:-1]) / 2, c[-1] + (c[-1] - c[-2]) / 2) for c in grid]
    for bc in (None, ALL, [N, F, N, F, N, F]):
        for strict in (True, False):
            ref = W.stokes_rhs(n, grid, etas, etan, rho, grav=GRAV, bc=bc, strict=strict, rounded=False)
            for U in (None, np.zeros((6, 3))):
                r = V.stokes_rhs(n, grid, etas, etan, rho, grav=GRAV, bc=bc, wallvel=U, strict=strict, rounded=False)
                assert r.dtype == ref.dtype and np.array_equal(r, ref)
        g0, V0 = W.advection_velocity(vel, gm, n, bc=bc)
        for U in (None, np.zeros((6, 3))):
            g1, V1 = V.advection_velocity(vel, gm, n, bc=bc, wallvel=U)
            for q in range(3):
                assert np.array_equal(g0[q], g1[q]) and np.array_equal(V0[q], V1[q])


@pytest.mark.parametrize("strict", [True, False])
def test_rhs_is_linear_in_the_velocities_wall_by_wall(strict):
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 241)
    rng = np.random.default_rng(242)
    per_wall = []
    for w in range(6):
        U = np.zeros((6, 3))
        U[w] = rng.standard_normal(3) * 1e-9
        U[w, w % 3] = 0.0
        per_wall.append(U)
    part = [V.wall_rhs(n, grid, etas, etan, ALL, U, strict) for U in per_wall]
    scale = max(float(np.abs(p).max()) for p in part)
    for w, p in enumerate(part):
        assert np.abs(p).max() > 0, w
        assert not p[..., w % 3].any() and not p[..., 3].any()          # a wall moves its two tangential components only
        assert np.array_equal(V.wall_rhs(n, grid, etas, etan, ALL, -4.0 * per_wall[w], strict), -4.0 * p)      # (a power of two: exact)
    tot = V.wall_rhs(n, grid, etas, etan, ALL, sum(per_wall), strict)
    # no entry takes more than two walls' terms, so the sum is the same in any order
    assert np.array_equal(tot, sum(part)) and scale > 0
    if strict:
        # a slaved row takes its U from one wall: the walls' rows are disjoint
        assert all(not ((part[a] != 0) & (part[b] != 0)).any() for a in range(6) for b in range(a))
    else:
        assert ((part[0] != 0) & (part[4] != 0)).any()                  # on a cube edge both walls contribute
    # the whole right-hand side is gravity's plus the walls'
    g = V.stokes_rhs(n, grid, etas, etan, rho, grav=GRAV, bc=ALL, strict=strict, rounded=False)
    r = V.stokes_rhs(n, grid, etas, etan, rho, grav=GRAV, bc=ALL, wallvel=sum(per_wall), strict=strict, rounded=False)
    assert np.array_equal(r, g + tot.reshape(-1))


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("D", [0, 1, 2])
def test_rows_vanish_for_the_linear_field_that_is_U_on_the_wall(D, strict):
    """v_D = U + s x (distance from the wall), grids non-uniform in all axes, the viscosity varying along the two axes other than the
    wall's: the slaved row (strict) and the near-wall momentum row (natural) of the moving wall are satisfied, at the low and the high
    side; with U left out of the right-hand side they are not."""
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    rng = np.random.default_rng(250 + D)
    grid = [_nonuniform(n[a], L[a], rng) for a in range(3)]
    s, U0 = 3e-14, 2e-9
    ix = M._index(n)
    for a in ((D + 1) % 3, (D + 2) % 3):
        b = 3 - D - a
        prof = [1e21 * 10 ** rng.uniform(-1, 1, n[q]) for q in range(3)]
        es = M._along(prof[D], D) * M._along(prof[b], b) * np.ones(n) / 1e21
        en = es.copy()
        c = grid[a].astype(LD)
        mid = np.append((c[1:] + c[:-1]) / 2, c[-1])
        for hi in (0, 1):
            w = a + 3 * hi
            dist = (c[-1] - mid) if hi else (mid - c[0])
            X = np.zeros(n + [4], dtype=LD)
            X[..., D] = U0 + s * M._along(dist, a)
            bc = [F] * 6; bc[w] = N
            U = np.zeros((6, 3)); U[w, D] = U0
            layer = ix[a] == (n[a] - 2 if hi else 0)
            if strict:
                rows = [r for r, ax, h, kind in W.slaved_rows(n, bc)[D] if ax == a and h == hi][0]
            else:
                # away from the other tangential axis' walls, where the free-slip mirror rows see the field's variation along a only
                rows = M.velocity_classes(D, n, False)[0] & layer
            y = W.stokes_apply(n, grid, es, en, X.reshape(-1), bc=bc, strict=strict, rounded=False).reshape(n + [4])
            r = V.stokes_rhs(n, grid, es, en, np.zeros(n), grav=(0, 0, 0), bc=bc, wallvel=U, strict=strict, rounded=False).reshape(n + [4])
            scale = float(np.abs(r[..., D][rows]).max())
            assert rows.any() and scale > 0
            assert np.abs((y - r)[..., D][rows]).max() <= 1e-15 * scale, (a, hi)
            assert np.abs(y[..., D][rows]).min() > 0.5 * float(np.abs(r[..., D][rows]).min())      # (the rows need the term)


def _lid_problem(oracle):
    nx2 = [12, 10]; L2 = [660e3, 500e3]; n_inv = 9
    rng = np.random.default_rng(260)
    grid2 = [_nonuniform(nx2[d], L2[d], rng) for d in range(2)]
    Z, X = np.meshgrid(*grid2, indexing="ij")
    Zc, Xc = np.meshgrid(*oracle.gridmp_of(grid2), indexing="ij")
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / L2[1]) * np.cos(np.pi * z / L2[0]))
    etas2, etan2 = f(Z, X), f(Zc, Xc)
    rho2 = 3300 + 40 * np.sin(2 * np.pi * X / L2[1]) * np.sin(np.pi * Z / L2[0])
    avg = 0.5 * sum((grid2[d][-1] - grid2[d][0]) / grid2[d].size for d in range(2))
    return nx2, grid2, etas2, etan2, rho2, n_inv, np.linspace(0, avg * n_inv, n_inv)


@pytest.mark.parametrize("buoyancy", [True, False], ids=["buoyant", "cavity"])
def test_extruded_lid_reproduces_the_2d_oracle_solution(oracle, buoyancy):
    """Lid z0 NOSLIP moving along x, everything invariant along y: on every physical y-slice the direct solution of the model's matrix
    is spsolve of the oracle's 2-D matrix for a NOSLIP z0, whose right-hand side gets -Kcont rd_z[0] U on its v_x extrapolation rows.
    Bound 1e-8 (velocity, relative L2 per slice; the pressure to 1e-8 of its largest value).

    The extruded 2-D solution satisfies the 3-D rows of the slices interior along y, the continuity rows of the cells (3, 2, k != 2)
    included, which the 2-D system replaces by its anchor."""
    nx2, grid2, etas2, etan2, rho2, ny, gy = _lid_problem(oracle)
    U0 = 2e-9
    if not buoyancy:
        rho2 = np.zeros(nx2)
    bc2 = [N, F, F, F]
    A2, rhs2 = oracle.stokes_csr(nx2, grid2, etas2, etan2, rho2, bc2)
    kc2 = oracle.stokes_scaling(grid2, etas2, etan2)[0]
    R2 = rhs2.reshape(nx2 + [3])
    z = grid2[0]
    R2[0, 1:nx2[1] - 1, 1] += -kc2 * (1 / (z[1] - z[0])) * U0
    x2 = spla.spsolve(A2.tocsc(), R2.reshape(-1)).reshape(nx2 + [3])
    n3 = nx2 + [ny]; grid3 = grid2 + [gy]
    ext = lambda a: _extrude(a, 2, ny)
    etas, etan, rho = ext(etas2), ext(etan2), ext(rho2)
    assert M.scaling(grid3, etas, etan)[0] == pytest.approx(kc2, rel=1e-13)
    bc3 = [N, F, F, F, F, F]
    U = _vel(z0=(0.0, U0, 0.0))
    ap = lambda x, rounded=True: W.stokes_apply(n3, grid3, etas, etan, x, bc=bc3, strict=True, rounded=rounded)
    rhs3 = V.stokes_rhs(n3, grid3, etas, etan, rho, grav=(oracle.G[0], 0.0, 0.0), bc=bc3, wallvel=U, strict=True)
    x3 = M.DirectSolver(M.assemble(ap, n3), ap).solve(rhs3).reshape(n3 + [4])
    vn = np.sqrt(np.sum(x2[..., :2] ** 2))
    pmax = np.abs(x2[:-1, :-1, 2]).max()
    worst = [0.0, 0.0]
    for k in range(ny - 1):
        ev = np.sqrt(np.sum((x3[:, :, k, 0] - x2[..., 0]) ** 2) + np.sum((x3[:, :, k, 1] - x2[..., 1]) ** 2)) / vn
        ep = np.abs(x3[:-1, :-1, k, 3] - x2[:-1, :-1, 2]).max() / pmax
        worst = [max(worst[0], ev), max(worst[1], ep)]
    print("extruded lid (%s): velocity %.3e, pressure %.3e, largest v_y %.3e of the largest velocity" % (
        "buoyant" if buoyancy else "cavity", worst[0], worst[1], np.abs(x3[..., 2]).max() / np.abs(x2[..., :2]).max()))
    assert worst[0] < 1e-8 and worst[1] < 1e-8, worst
    assert np.abs(x3[..., 2]).max() < 1e-8 * np.abs(x2[..., :2]).max()
    if not buoyancy:                                           # the lid alone drives the flow: v_x next to it has the sign of U
        assert np.all(x3[0, 2:-2, 1:ny - 2, 1] > 0)
    X3 = np.zeros(n3 + [4])
    X3[..., 0], X3[..., 1], X3[..., 3] = ext(x2[..., 0]), ext(x2[..., 1]), ext(x2[..., 2])
    res = (ap(X3.reshape(-1), rounded=False) - M._ld(rhs3)).reshape(n3 + [4])
    assert np.abs(res[:, :, 1:ny - 2]).max() <= 1e-8 * np.abs(rhs3).max()


def test_ghost_planes_of_a_moving_wall_put_U_on_the_wall():
    n = [6, 7, 8]
    rng = np.random.default_rng(270)
    vel = [rng.standard_normal(n) for _ in range(3)]
    gm = [(np.arange(n[a]) + 0.5) * 1e4 for a in range(3)]
    U = TWO * 1e9
    bc = [N, F, F, F, N, F]
    g, A = V.advection_velocity(vel, gm, n, bc=bc, wallvel=U)
    for w in (0, 4):
        a = w % 3
        for q in range(3):
            Am = np.moveaxis(A[q], a, 0)
            ghost, inner = (Am[0], Am[1]) if w < 3 else (Am[-1], Am[-2])
            mean = (0.5 * (ghost + inner))[1:-1, 1:-1]     # (the lines on the plane's rim belong to the other walls' passes)
            assert np.abs(mean - U[w, q]).max() <= 4e-16 * max(1.0, float(np.abs(inner).max())), (w, q)
    # at rest the passes are skipped
    _, R = V.advection_velocity(vel, gm, n, bc=bc, wallvel=None)
    assert not R[1][0].any() and not R[0][:, -1].any()
    assert A[1][0, 1:-1, 1:-1].all()


def test_the_four_rejections():
    z = np.zeros((6, 3))
    U = z.copy(); U[4, 2] = np.nan
    with pytest.raises(Exception, match=r"wall xL: non-finite velocity component Uy"):
        V.velocities(U, ALL)
    U = z.copy(); U[3, 0] = 1e-9
    with pytest.raises(Exception, match=r"wall zL: normal velocity component Uz = 1e-09.*marker deletion path, which is not built in 3-D"):
        V.velocities(U, ALL)
    U = z.copy(); U[2, 1] = 1e-9
    with pytest.raises(Exception, match=r"wall y0: FREESLIP walls cannot move"):
        V.velocities(U, [N, N, F, N, N, N])
    st = V.WallState()
    st.set_walls(ALL)
    st.set_wall_velocity(TWO)
    with pytest.raises(Exception, match=r"wall xL: moves with velocity \(3e-09, 0.0, 5e-10\) and cannot become FREESLIP"):
        st.set_walls([N, N, N, N, F, N])
    st.set_walls([N, F, F, F, N, F])                           # the walls at rest may change
    st.set_wall_velocity(None)
    st.set_walls([F] * 6)


def test_python_validation_gives_the_same_rejections():
    """pylamp3d.wall_velocities is pure Python (no library call): the three checks of a velocity setting, by message."""
    from pylamp_amd import pylamp3d as P3
    z = np.zeros((6, 3))
    assert np.array_equal(P3.wall_velocities(None), z) and np.array_equal(P3.wall_velocities(TWO, ALL), TWO)
    U = z.copy(); U[4, 2] = np.inf
    with pytest.raises(Exception, match=r"wall xL has a non-finite velocity component Uy = inf"):
        P3.wall_velocities(U, ALL)
    U = z.copy(); U[3, 0] = 1e-9
    with pytest.raises(Exception, match=r"wall zL has the normal velocity component Uz = 1e-09.*marker deletion path, which is not built in 3-D"):
        P3.wall_velocities(U, ALL)
    U = z.copy(); U[2, 1] = 1e-9
    with pytest.raises(Exception, match=r"wall y0 is FREESLIP and cannot move with velocity \(0.0, 1e-09, 0.0\)"):
        P3.wall_velocities(U, [N, N, F, N, N, N])
    with pytest.raises(Exception, match=r"shape \(6, 3\)"):
        P3.wall_velocities(np.zeros((6, 2)), ALL)
    one = np.ones([5, 5, 5])
    with pytest.raises(Exception, match=r"advection_velocity: wall z0 is FREESLIP and cannot move"):
        P3.advection_velocity([one, one, one], P3.gridmp_of([np.linspace(0, 1, 5)] * 3), [5, 5, 5], bc=None, wallvel=_vel(z0=(0, 1, 0)))
    # the Python ghosts are the model's
    rng = np.random.default_rng(280)
    n = [6, 7, 8]
    vel = [rng.standard_normal(n) for _ in range(3)]
    gm = [(np.arange(n[a]) + 0.5) * 1e4 for a in range(3)]
    for bc, U in (([N, F, F, F, N, F], TWO * 1e9), (ALL, _vel(zL=(0, -1.5, 0.25))), (ALL, None)):
        _, A = P3.advection_velocity(vel, gm, n, bc, U)
        _, B = V.advection_velocity(vel, gm, n, bc=bc, wallvel=U)
        for q in range(3):
            assert np.array_equal(A[q], B[q])
