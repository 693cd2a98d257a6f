"""CPU checks that earn tests/stokes3_model.py (the NumPy model the 3-D Stokes and heat kernels are compared with) its authority:
it reduces to the 2-D oracle under extrusion along each of the three axes, is covariant under cyclic permutation of the axes, has
the symmetries and null space of the continuous operator, is second-order consistent, and reproduces constant and linear
temperature fields."""
import numpy as np
import pytest

import stokes3_model as M

LD = np.longdouble


def _nonuniform(n, L, rng):
    w = rng.uniform(0.7, 1.3, n - 1)
    g = np.concatenate([[0.0], np.cumsum(w)])
    return g * (L / g[-1])


def _mid(grid):
    out = []
    for c in grid:
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


def _fields3(n, L, seed, uniform=False):
    """Non-uniform grid, one smooth viscosity function with 3 decades and different wavenumbers along every axis, sampled at
    the nodes and at the centres; density smooth + noise."""
    rng = np.random.default_rng(seed)
    grid = [np.linspace(0, L[a], n[a]) if uniform else _nonuniform(n[a], L[a], rng) for a in range(3)]
    f = lambda z, x, y: 1e20 * 10 ** (1.5 * np.cos(np.pi * z / L[0]) * np.sin(2 * np.pi * x / L[1] + 0.3) * np.cos(3 * np.pi * y / L[2] + 0.7))
    Z, X, Y = np.meshgrid(*grid, indexing="ij")
    Zc, Xc, Yc = np.meshgrid(*_mid(grid), indexing="ij")
    rho = 3300 + 40 * np.sin(np.pi * Z / L[0]) * np.sin(2 * np.pi * X / L[1]) * np.cos(np.pi * Y / L[2]) + rng.uniform(-1, 1, n)
    return grid, f(Z, X, Y), f(Zc, Xc, Yc), rho


# ---- extrusion along each axis ---------------------------------------------------------------------------------------
def _extrude(a2, inv, n_inv):
    return np.repeat(np.expand_dims(a2, inv), n_inv, axis=inv)


@pytest.mark.parametrize("inv", [2, 1, 0])
def test_extrusion_reduces_to_2d_oracle(oracle, inv):
    """A problem invariant along axis `inv` reproduces the 2-D oracle on the slices whose rows are interior along `inv`; the two
    active axes, in their 3-D order, take the roles of the oracle's z and x.  What each axis pins to the reference:
      inv = y: the z-x plane -- vz / vx rows, their slaved rows at the x- and z-walls, the corner rule on z-x cube edges, the
               viscosity of the z-x edges (averaged along y), gravity along z;
      inv = x: the y-walls and the z-y edges -- the vz row's terms along its SECOND tangential axis (F = y), the vy row's along
               its first (E = z), vz slaved at the y-walls, vy slaved at the z-walls, pressure symmetry inward along y on the
               z-y cube edges, the viscosity of the z-y edges (averaged along x);
      inv = z: the x-y plane -- vx rows along E = y, vy rows along F = x, vx slaved at the y-walls, vy at the x-walls, pressure
               symmetry inward along y on the x-y cube edges, the viscosity of the x-y edges (averaged along z), gravity along x."""
    act = [a for a in range(3) if a != inv]
    nx2 = [12, 10]; L2 = [660e3, 500e3]; n_inv = 9
    rng = np.random.default_rng(10 + inv)
    grid2 = [_nonuniform(nx2[d], L2[d], rng) for d in range(2)]
    Z, X = np.meshgrid(*grid2, indexing="ij")
    Zc, Xc = np.meshgrid(*oracle.gridmp_of(grid2), indexing="ij")
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / L2[1]) * np.cos(np.pi * z / L2[0]))
    etas2, etan2 = f(Z, X), f(Zc, Xc)
    rho2 = 3300 + 40 * np.sin(2 * np.pi * X / L2[1]) * np.sin(np.pi * Z / L2[0]) + rng.uniform(-1, 1, nx2)
    # Kcont uses L / n per axis: the mean of the two others along the invariant axis makes the 3-D Kcont equal the 2-D one
    avg = 0.5 * sum((grid2[d][-1] - grid2[d][0]) / grid2[d].size for d in range(2))
    g_inv = np.linspace(0, avg * n_inv, n_inv)
    n3 = [0, 0, 0]; grid3 = [None] * 3
    n3[inv] = n_inv; grid3[inv] = g_inv
    for d in range(2):
        n3[act[d]] = nx2[d]; grid3[act[d]] = grid2[d]
    ext = lambda a: _extrude(a, inv, n_inv)
    etas, etan, rho = ext(etas2), ext(etan2), ext(rho2)
    kc2, kb2 = oracle.stokes_scaling(grid2, etas2, etan2)
    kc3, kb3 = M.scaling(grid3, etas, etan)
    assert kc3 == pytest.approx(kc2, rel=1e-13) and kb3 == pytest.approx(kb2, rel=1e-13)

    x2 = rng.standard_normal(3 * nx2[0] * nx2[1])
    X2 = x2.reshape(nx2 + [3])
    X3 = np.zeros(n3 + [4])
    X3[..., act[0]] = ext(X2[..., 0]); X3[..., act[1]] = ext(X2[..., 1]); X3[..., 3] = ext(X2[..., 2])
    X3[..., inv] = ext(rng.standard_normal(nx2))          # an invariant velocity along the invariant axis changes no other row
    y2 = oracle.stokes_apply(nx2, grid2, etas2, etan2, [1, 1, 1, 1], x2).reshape(nx2 + [3])
    r2 = oracle.stokes_rhs(nx2, rho2).reshape(nx2 + [3])
    grav = [0.0, 0.0, 0.0]; grav[act[0]] = 9.81           # the oracle's gravity is along its z
    cls2 = oracle.stokes_row_class(nx2)
    scale = np.abs(y2).max(axis=(0, 1))
    anchor2 = tuple(M.ANCHOR[a] for a in act)
    for strict in (True, False):
        y3 = M.stokes_apply(n3, grid3, etas, etan, X3.reshape(-1), strict=strict).reshape(n3 + [4])
        R3 = M.stokes_rhs(n3, grid3, etas, etan, rho, grav=grav, strict=strict).reshape(n3 + [4])
        for k in range(1, n_inv - 2):
            sl = [slice(None)] * 3; sl[inv] = k
            Y, R = y3[tuple(sl)], R3[tuple(sl)]
            for q3, q2 in ((act[0], 0), (act[1], 1), (3, 2)):
                d = np.abs(Y[..., q3] - y2[..., q2])
                if q2 == 2:
                    d[3, 2] = 0.0                         # the oracle anchors (3, 2) on every slice, the 3-D system the single cell (3, 2, 2)
                    if k == M.ANCHOR[inv]:
                        d[anchor2] = 0.0
                if not strict:                            # natural rows: the rows that are interior in the oracle as well
                    d = np.where(cls2[q2] == 1, d, 0.0)
                assert d.max() < 1e-12 * scale[q2], (strict, k, q3, d.max() / scale[q2])
            if strict:
                assert np.allclose(R[..., act[0]], r2[..., 0], rtol=1e-14, atol=0)
                assert not R[..., act[1]].any() and not R[..., inv].any() and not R[..., 3].any()
            else:
                m = cls2[0] == 1
                assert np.allclose(R[..., act[0]][m], r2[..., 0][m], rtol=1e-14, atol=0)


@pytest.mark.parametrize("inv", [2, 1, 0])
def test_heat_extrusion_reduces_to_2d_oracle(oracle, inv):
    """Heat rows under extrusion: inv = y pins k_z, k_x and the z-before-x ownership, inv = x pins k_y, the y-midpoints and
    z-before-y, inv = z pins x-before-y."""
    act = [a for a in range(3) if a != inv]
    nx2 = [9, 11]; n_inv = 6
    rng = np.random.default_rng(20 + inv)
    grid2 = [_nonuniform(nx2[0], 660e3, rng), _nonuniform(nx2[1], 800e3, rng)]
    gm2 = oracle.gridmp_of(grid2)
    g_inv = _nonuniform(n_inv, 300e3, rng)
    n3 = [0, 0, 0]; grid3 = [None] * 3
    n3[inv] = n_inv; grid3[inv] = g_inv
    for d in range(2):
        n3[act[d]] = nx2[d]; grid3[act[d]] = grid2[d]
    gm3 = _mid(grid3)
    ext = lambda a: _extrude(a, inv, n_inv)
    k2 = [rng.uniform(2, 5, nx2), rng.uniform(2, 5, nx2)]
    Cp, rho = rng.uniform(1000, 1250, nx2), rng.uniform(3200, 3400, nx2)
    H, T0 = rng.uniform(0, 1e-9, nx2) * 3300, rng.uniform(273, 1623, nx2)
    dt = 0.67 * (660e3 / (nx2[0] - 1)) ** 2 / np.max(2 * k2[0] / (rho * Cp))
    k3 = [None] * 3
    k3[act[0]], k3[act[1]], k3[inv] = ext(k2[0]), ext(k2[1]), ext(rng.uniform(2, 5, nx2))
    x2 = rng.standard_normal(nx2[0] * nx2[1])
    for bc2, bv2 in (([0, 1, 0, 1], [273.0, 0.0, 1623.0, 0.0]), ([1, 0, 1, 0], [0.02, 300.0, -0.03, 900.0]), ([0, 0, 1, 1], [1.0, 2.0, 3.0, 4.0])):
        bc3 = [1] * 6; bv3 = [7.0] * 6
        for d in range(2):
            bc3[act[d]], bc3[act[d] + 3] = bc2[d], bc2[d + 2]
            bv3[act[d]], bv3[act[d] + 3] = bv2[d], bv2[d + 2]
        y3 = M.heat_apply(n3, grid3, gm3, k3, ext(Cp), ext(rho), bc3, dt, ext(x2.reshape(nx2)).reshape(-1)).reshape(n3)
        r3 = M.heat_rhs(n3, ext(T0), ext(Cp), ext(rho), ext(H), bc3, bv3, dt).reshape(n3)
        y2 = oracle.heat_apply(nx2, grid2, gm2, k2, Cp, rho, bc2, dt, x2).reshape(nx2)
        r2 = oracle.heat_rhs(nx2, T0, Cp, rho, H, bc2, bv2, dt).reshape(nx2)
        for k in range(1, n_inv - 1):
            sl = [slice(None)] * 3; sl[inv] = k
            assert np.abs(y3[tuple(sl)] - y2).max() < 1e-12 * np.abs(y2).max()
            assert np.allclose(r3[tuple(sl)], r2, rtol=1e-14, atol=0)


# ---- axis covariance -------------------------------------------------------------------------------------------------
def test_cyclic_permutation_of_the_axes():
    """Natural rows, genuinely 3-D grid and viscosity: renaming (z, x, y) -> (x, y, z) in every input renames the output the
    same way, everywhere but on the two anchor rows (the anchor cell (3, 2, 2) is not covariant; Kcont is)."""
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 31)
    rng = np.random.default_rng(32)
    X = rng.standard_normal(n + [4])
    grav = (3.0, -4.0, 5.0)
    T = lambda a: np.transpose(a, (1, 2, 0))                # B[x, y, z] = A[z, x, y]: the new z is the old x, ...
    n_p = [n[1], n[2], n[0]]; grid_p = [grid[1], grid[2], grid[0]]
    Xp = np.stack([T(X[..., 1]), T(X[..., 2]), T(X[..., 0]), T(X[..., 3])], axis=-1)
    grav_p = (grav[1], grav[2], grav[0])
    assert M.scaling(grid_p, T(etas), T(etan)) == pytest.approx(M.scaling(grid, etas, etan), rel=1e-15)
    y = M.stokes_apply(n, grid, etas, etan, X.reshape(-1), strict=False).reshape(n + [4])
    yp = M.stokes_apply(n_p, grid_p, T(etas), T(etan), Xp.reshape(-1), strict=False).reshape(n_p + [4])
    r = M.stokes_rhs(n, grid, etas, etan, rho, grav=grav, strict=False).reshape(n + [4])
    rp = M.stokes_rhs(n_p, grid_p, T(etas), T(etan), T(rho), grav=grav_p, strict=False).reshape(n_p + [4])
    for a, ap in ((y, yp), (r, rp)):
        back = np.stack([T(a[..., 1]), T(a[..., 2]), T(a[..., 0]), T(a[..., 3])], axis=-1)
        d = np.abs(ap - back)
        d[M.ANCHOR + (3,)] = 0.0                                            # the permuted problem's anchor
        d[(M.ANCHOR[1], M.ANCHOR[2], M.ANCHOR[0], 3)] = 0.0                 # the original anchor, renamed
        for q in range(4):
            assert d[..., q].max() <= 1e-15 * max(np.abs(back[..., q]).max(), 1e-300), q
    assert np.abs(y[..., 2]).max() > 0 and np.abs(r[..., 2]).max() > 0


# ---- symmetry and null space -----------------------------------------------------------------------------------------
def test_null_space_on_interior_rows():
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 41)
    rng = np.random.default_rng(42)
    ref = np.abs(M.stokes_apply(n, grid, etas, etan, rng.standard_normal(4 * int(np.prod(n))), strict=False)).max()
    for strict in (True, False):
        rows = np.stack([M.velocity_classes(D, n, strict)[0] for D in range(3)] + [M.pressure_classes(n, strict)[0]], axis=-1)
        for q in range(4):           # rigid translation along z, x, y (tangential to four of the six walls), constant pressure
            X = np.zeros(n + [4]); X[..., q] = 1.0
            y = M.stokes_apply(n, grid, etas, etan, X.reshape(-1), strict=strict).reshape(n + [4])
            if q < 3:                # rows next to the walls the translation is normal to see the wall-normal velocity change
                ix = M._index(n)[q]
                rows_q = rows & ((ix >= 2) & (ix <= n[q] - 3))[..., None]
            else:
                rows_q = rows
            assert rows_q.any() and np.abs(y[rows_q]).max() <= 1e-13 * ref, (strict, q)


def test_assembled_blocks_symmetry():
    """Natural rows, uniform grid: the velocity block restricted to the momentum rows is symmetric to rounding, and the gradient
    is minus the transpose of the divergence once each is multiplied by its own spacing: h_D A_vp = (d_D A_pv)^T with h_D the
    distance of the two cell centres a momentum row differences the pressure over and d_D the width of the continuity row's cell
    (the rows carry -Kcont grad P and +Kcont div v)."""
    n = [5, 6, 7]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 51, uniform=True)
    A = M.assemble(lambda x: M.stokes_apply(n, grid, etas, etan, x, strict=False), n).tocsr()
    # the probe agrees with the operator on a random vector
    x = np.random.default_rng(52).standard_normal(A.shape[0])
    y = M.stokes_apply(n, grid, etas, etan, x, strict=False)
    assert np.abs(A @ x - y).max() <= 1e-13 * np.abs(y).max()
    vel = np.stack([M.velocity_classes(D, n, False)[0] for D in range(3)] + [np.zeros(n, dtype=bool)], axis=-1).reshape(-1)
    prs = np.stack([np.zeros(n, dtype=bool)] * 3 + [M.pressure_classes(n, False)[0]], axis=-1).reshape(-1)
    iv, ip = np.nonzero(vel)[0], np.nonzero(prs)[0]
    Avv = A[iv][:, iv]
    assert abs(Avv - Avv.T).max() <= 1e-13 * abs(Avv).max() and abs(Avv).max() > 0
    # the per-row spacings
    h = [L[a] / (n[a] - 1) for a in range(3)]
    comp = (np.arange(A.shape[0]) % 4)
    hv = np.array([h[c] for c in comp[iv]])                 # uniform: centre distance = cell width = h_D
    Avp = (A[iv][:, ip]).multiply(hv[:, None]).tocsr()
    Apv = A[ip][:, iv].tocsr()                              # row of a cell: entries -+ Kcont / d_D in the columns of component D
    dcol = hv
    ApvT = Apv.multiply(dcol[None, :]).T.tocsr()
    Kc = M.scaling(grid, etas, etan)[0]
    assert abs(Avp - ApvT).max() <= 1e-13 * Kc and abs(Avp).max() == pytest.approx(Kc, rel=1e-13)


# ---- manufactured solution -------------------------------------------------------------------------------------------
def _truncation(nn):
    """max |A x_exact - rhs| on the momentum rows away from the walls, for the constant-viscosity solution of
    test_hip_3d._manufactured: rho = rho0 + drho sin(kz z) cos(kx x) cos(ky y), vz = W sin cos cos, vx = U cos sin cos,
    vy = V cos cos sin, P = rho0 g z + Pm cos cos cos."""
    L = [1.0e5, 1.3e5, 0.9e5]; eta = 1e20; drho = 30.0; g = 9.81; rho0 = 3300.0
    n = [nn, nn, nn]
    grid = [np.linspace(0, L[d], nn) for d in range(3)]
    kz, kx, ky = np.pi / L[0], np.pi / L[1], np.pi / L[2]
    k2 = kz * kz + kx * kx + ky * ky
    W = drho * g * (kx * kx + ky * ky) / (eta * k2 * k2)
    Pm = -eta * k2 * kz * W / (kx * kx + ky * ky)
    U, V = kx * Pm / (eta * k2), ky * Pm / (eta * k2)
    mid = _mid(grid)
    Z, X, Y = np.meshgrid(*grid, indexing="ij")
    rho = rho0 + drho * np.sin(kz * Z) * np.cos(kx * X) * np.cos(ky * Y)
    one = np.full(n, eta)
    Kc = M.scaling(grid, one, one)[0]
    x = np.zeros(n + [4])
    Zz, Xz, Yz = np.meshgrid(grid[0], mid[1], mid[2], indexing="ij")
    x[..., 0] = W * np.sin(kz * Zz) * np.cos(kx * Xz) * np.cos(ky * Yz)
    Zx, Xx, Yx = np.meshgrid(mid[0], grid[1], mid[2], indexing="ij")
    x[..., 1] = U * np.cos(kz * Zx) * np.sin(kx * Xx) * np.cos(ky * Yx)
    Zy, Xy, Yy = np.meshgrid(mid[0], mid[1], grid[2], indexing="ij")
    x[..., 2] = V * np.cos(kz * Zy) * np.cos(kx * Xy) * np.sin(ky * Yy)
    Zc, Xc, Yc = np.meshgrid(*mid, indexing="ij")
    x[..., 3] = (rho0 * g * Zc + Pm * np.cos(kz * Zc) * np.cos(kx * Xc) * np.cos(ky * Yc)) / Kc
    res = (M.stokes_apply(n, grid, one, one, x.reshape(-1), strict=True, rounded=False)
           - M.stokes_rhs(n, grid, one, one, rho, strict=True, rounded=False)).reshape(n + [4])
    mom = max(float(np.abs(res[..., D][M.velocity_classes(D, n, True)[0]]).max()) for D in range(3))
    cont = float(np.abs(res[..., 3][M.pressure_classes(n, True)[0]]).max()) / Kc
    return mom / (drho * g), cont * L[0] / abs(W)


def test_manufactured_solution_truncation_is_second_order():
    m17, c17 = _truncation(17)
    m33, c33 = _truncation(33)
    assert m33 < m17 < 0.05 and 3.5 < m17 / m33 < 4.5, (m17, m33)
    # k_a h_a = pi / (n - 1) on every axis: the three difference quotients carry the same factor and the exact field is
    # discretely divergence-free
    assert c17 < 1e-12 and c33 < 1e-12, (c17, c33)


# ---- heat ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("kind", [M.FIXTEMP, M.FIXFLOW])
def test_heat_reproduces_constant_and_linear_fields(axis, kind):
    """A steady field (T_old = T, no heating) solves its own system: constant with insulating or matching fixed-temperature walls,
    linear along one axis with that axis's walls holding the end values or the flux k dT/dx and the four others insulating."""
    n = [6, 7, 8]; L = [1.0, 1.3, 0.9]
    rng = np.random.default_rng(60 + axis)
    grid = [_nonuniform(n[a], L[a], rng) for a in range(3)]
    mp = _mid(grid)
    kc = 3.0
    k = [np.full(n, kc)] * 3
    Cp, rho = rng.uniform(1.0, 1.25, n), rng.uniform(3.2, 3.4, n)
    H = np.zeros(n); dt = 0.01
    for slope in (0.0, 0.8):
        T = 1.0 + slope * M._along(grid[axis], axis) + np.zeros(n)
        bc = [M.FIXFLOW] * 6; bv = [0.0] * 6
        bc[axis] = bc[axis + 3] = kind
        if kind == M.FIXTEMP:
            bv[axis], bv[axis + 3] = 1.0 + slope * grid[axis][0], 1.0 + slope * grid[axis][-1]
        else:
            bv[axis] = bv[axis + 3] = kc * slope
        y = M.heat_apply(n, grid, mp, k, Cp, rho, bc, dt, T.reshape(-1))
        r = M.heat_rhs(n, T, Cp, rho, H, bc, bv, dt)
        assert np.abs(y - r).max() <= 1e-12 * np.abs(r).max(), (slope, np.abs(y - r).max())
    if kind == M.FIXTEMP:              # constant field, all six walls at its value
        T = np.full(n, 2.5)
        y = M.heat_apply(n, grid, mp, k, Cp, rho, [M.FIXTEMP] * 6, dt, T.reshape(-1))
        r = M.heat_rhs(n, T, Cp, rho, H, [M.FIXTEMP] * 6, [2.5] * 6, dt)
        assert np.abs(y - r).max() <= 1e-12 * 2.5


def test_heat_wall_ownership_z_then_x_then_y():
    n = [5, 6, 7]
    rng = np.random.default_rng(70)
    grid = [_nonuniform(n[a], 1.0, rng) for a in range(3)]
    mp = _mid(grid)
    f = lambda: rng.uniform(1, 2, n)
    bv = [10.0, 11.0, 12.0, 13.0, 14.0, 15.0]                    # z0, x0, y0, zL, xL, yL
    r = M.heat_rhs(n, f(), f(), f(), f(), [0] * 6, bv, 0.1).reshape(n)
    Z, X, Y = n[0] - 1, n[1] - 1, n[2] - 1
    expect = {(0, 2, 3): 10, (Z, 2, 3): 13, (2, 0, 3): 11, (2, X, 3): 14, (2, 2, 0): 12, (2, 2, Y): 15,        # faces
              (0, 0, 3): 10, (0, X, 3): 10, (Z, 0, 3): 13, (Z, X, 3): 13,                                      # z-x edges: z
              (0, 2, 0): 10, (Z, 2, Y): 13, (0, 2, Y): 10, (Z, 2, 0): 13,                                      # z-y edges: z
              (2, 0, 0): 11, (2, 0, Y): 11, (2, X, 0): 14, (2, X, Y): 14,                                      # x-y edges: x
              (0, 0, 0): 10, (Z, X, Y): 13, (0, X, Y): 10, (Z, 0, 0): 13}                                      # corners: z
    for node, v in expect.items():
        assert r[node] == v, node
    # the operator follows the same ownership: flux walls everywhere, the row of an edge node is its owner's flux row
    k = [f(), f(), f()]
    T = rng.standard_normal(n)
    y = M.heat_apply(n, grid, mp, k, f(), f(), [1] * 6, 0.1, T.reshape(-1)).reshape(n)
    flux0 = lambda a, node: k[a][node] * (T[tuple(v + (1 if q == a else 0) for q, v in enumerate(node))] - T[node]) / (grid[a][1] - grid[a][0])
    assert y[0, 0, 3] == pytest.approx(flux0(0, (0, 0, 3)), rel=1e-14)
    assert y[0, 2, 0] == pytest.approx(flux0(0, (0, 2, 0)), rel=1e-14)
    assert y[2, 0, 0] == pytest.approx(flux0(1, (2, 0, 0)), rel=1e-14)
    assert y[2, 2, 0] == pytest.approx(flux0(2, (2, 2, 0)), rel=1e-14)
    hi = (2, X, Y)                                               # x-y edge at the high walls: the x-wall's row
    assert y[hi] == pytest.approx(k[1][2, X - 1, Y] * (T[hi] - T[2, X - 1, Y]) / (grid[1][-1] - grid[1][-2]), rel=1e-14)


def test_direct_solve_refines_to_the_model_residual():
    n = [6, 5, 7]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 81)
    for strict in (True, False):
        ap = lambda x, rounded=True: M.stokes_apply(n, grid, etas, etan, x, strict=strict, rounded=rounded)
        A = M.assemble(ap, n)
        b = M.stokes_rhs(n, grid, etas, etan, rho, grav=(3.0, -4.0, 5.0), strict=strict)
        S = M.DirectSolver(A, ap)
        x = S.solve(b)
        assert S.residual <= 1e-12
        V = x.reshape(n + [4])
        assert np.abs(V[..., 2]).max() > 0.01 * np.abs(V[..., 0]).max()
