"""CPU checks that earn tests/stokes3_walls_model.py (the NumPy model of the 3-D Stokes rows with per-wall no-slip boundaries) its
authority: with six free-slip walls it IS tests/stokes3_model.py, it reduces to the 2-D oracle with no-slip z-walls under extrusion
along each of the three axes, its natural no-slip rows annihilate the shear of a field that is linear in the distance from the wall,
it keeps the symmetry of the velocity block, loses the tangential translations from its null space, and its advection ghosts are
the oracle's."""
import numpy as np
import pytest

import stokes3_model as M
import stokes3_walls_model as W
from test_stokes3_model import _extrude, _fields3, _nonuniform

LD = np.longdouble
N, F = W.NOSLIP, W.FREESLIP
MIXED = [N, F, N, F, N, F]                                  # every cube edge joins two kinds


def test_six_freeslip_walls_are_the_freeslip_model():
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 131)
    x = np.random.default_rng(132).standard_normal(4 * int(np.prod(n)))
    for strict in (True, False):
        ref = M.stokes_apply(n, grid, etas, etan, x, strict=strict, rounded=False)
        for bc in (None, [F] * 6):
            y = W.stokes_apply(n, grid, etas, etan, x, bc=bc, strict=strict, rounded=False)
            assert y.dtype == ref.dtype and np.array_equal(y, ref)
        assert np.array_equal(W.stokes_rhs(n, grid, etas, etan, rho, bc=[F] * 6, strict=strict, rounded=False),
                              M.stokes_rhs(n, grid, etas, etan, rho, strict=strict, rounded=False))
        assert np.array_equal(W.identity_rows(n, strict, bc=MIXED), M.identity_rows(n, strict))
        # and a no-slip wall does change rows
        assert not np.array_equal(W.stokes_apply(n, grid, etas, etan, x, bc=MIXED, strict=strict, rounded=False), ref)
    with pytest.raises(Exception, match="wall xL: kind 2"):
        W.stokes_apply(n, grid, etas, etan, x, bc=[F, F, F, F, 2, F])


@pytest.mark.parametrize("bc2", [[N, F, F, F], [F, F, N, F], [N, F, N, F]], ids=["z0", "zL", "z0zL"])
@pytest.mark.parametrize("inv", [2, 1, 0])
def test_extrusion_reduces_to_2d_oracle(oracle, inv, bc2):
    """Strict rows.  The oracle's no-slip z-walls (its x-walls are free-slip) are the walls of the FIRST active axis in 3-D:
      inv = y: the z-walls -- vx slaved along its F = z, vy along its E = z;
      inv = x: the z-walls again, with y in the role of the oracle's x -- vy slaved along E = z;
      inv = z: the x-walls, x in the role of the oracle's z and y of its x -- vy slaved along its F = x."""
    act = [a for a in range(3) if a != inv]
    nx2 = [12, 10]; L2 = [660e3, 500e3]; n_inv = 9
    rng = np.random.default_rng(110 + inv)
    grid2 = [_nonuniform(nx2[d], L2[d], rng) for d in range(2)]
    Z, X = np.meshgrid(*grid2, indexing="ij")
    Zc, Xc = np.meshgrid(*oracle.gridmp_of(grid2), indexing="ij")
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / L2[1]) * np.cos(np.pi * z / L2[0]))
    etas2, etan2 = f(Z, X), f(Zc, Xc)
    avg = 0.5 * sum((grid2[d][-1] - grid2[d][0]) / grid2[d].size for d in range(2))
    n3 = [0, 0, 0]; grid3 = [None] * 3
    n3[inv] = n_inv; grid3[inv] = np.linspace(0, avg * n_inv, n_inv)
    for d in range(2):
        n3[act[d]] = nx2[d]; grid3[act[d]] = grid2[d]
    ext = lambda a: _extrude(a, inv, n_inv)
    etas, etan = ext(etas2), ext(etan2)
    bc3 = [F] * 6
    bc3[act[0]], bc3[act[0] + 3] = bc2[0], bc2[2]
    x2 = rng.standard_normal(3 * nx2[0] * nx2[1])
    X2 = x2.reshape(nx2 + [3])
    X3 = np.zeros(n3 + [4])
    X3[..., act[0]] = ext(X2[..., 0]); X3[..., act[1]] = ext(X2[..., 1]); X3[..., 3] = ext(X2[..., 2])
    X3[..., inv] = ext(rng.standard_normal(nx2))
    y2 = oracle.stokes_apply(nx2, grid2, etas2, etan2, bc2, x2).reshape(nx2 + [3])
    free2 = oracle.stokes_apply(nx2, grid2, etas2, etan2, [F] * 4, x2).reshape(nx2 + [3])
    assert np.abs(y2 - free2).max() > 0                    # the oracle's rows do depend on the kind
    scale = np.abs(y2).max(axis=(0, 1))
    anchor2 = tuple(M.ANCHOR[a] for a in act)
    y3 = W.stokes_apply(n3, grid3, etas, etan, X3.reshape(-1), bc=bc3, strict=True).reshape(n3 + [4])
    for k in range(1, n_inv - 2):
        sl = [slice(None)] * 3; sl[inv] = k
        Y = y3[tuple(sl)]
        for q3, q2 in ((act[0], 0), (act[1], 1), (3, 2)):
            d = np.abs(Y[..., q3] - y2[..., q2])
            if q2 == 2:
                d[3, 2] = 0.0
                if k == M.ANCHOR[inv]:
                    d[anchor2] = 0.0
            assert d.max() < 1e-12 * scale[q2], (k, q3, d.max() / scale[q2])


@pytest.mark.parametrize("D", [0, 1, 2])
def test_natural_rows_linear_field_has_no_shear_at_a_noslip_wall(D):
    """v_D = s x (distance from a no-slip wall of its axis E or F), zero on the wall, constant viscosity, non-uniform grid: both edges of
    the near-wall row carry the shear stress eta s, so the row vanishes; with a free-slip wall the wall edge carries none and the row
    is eta s / (cell width)."""
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    rng = np.random.default_rng(140 + D)
    grid = [_nonuniform(n[a], L[a], rng) for a in range(3)]
    eta, s = 1e21, 3e-14
    es = np.full(n, eta); en = np.full(n, eta)
    ix = M._index(n)
    interior = M.velocity_classes(D, n, False)[0]
    for a in ((D + 1) % 3, (D + 2) % 3):
        c = grid[a].astype(LD)
        mid = np.append((c[1:] + c[:-1]) / 2, c[-1])         # v_D sits at the midpoints along a (last entry: a ghost)
        for hi in (0, 1):
            dist = (c[-1] - mid) if hi else (mid - c[0])
            X = np.zeros(n + [4], dtype=LD)
            X[..., D] = s * M._along(dist, a)
            rows = interior & (ix[a] == (n[a] - 2 if hi else 0))
            width = float(c[-1] - c[-2]) if hi else float(c[1] - c[0])
            bc = [F] * 6; bc[a + 3 * hi] = N
            y = W.stokes_apply(n, grid, es, en, X.reshape(-1), bc=bc, strict=False, rounded=False).reshape(n + [4])
            assert rows.any() and np.abs(y[..., D][rows]).max() <= 1e-15 * eta * s / width, (a, hi)
            y = W.stokes_apply(n, grid, es, en, X.reshape(-1), bc=[F] * 6, strict=False, rounded=False).reshape(n + [4])
            assert np.allclose(np.abs(y[..., D][rows]).astype(np.float64), eta * s / width, rtol=1e-12), (a, hi)


def test_velocity_block_stays_symmetric_with_mixed_walls():
    """Natural rows, uniform grid (as test_assembled_blocks_symmetry): the no-slip terms sit on the diagonal."""
    n = [5, 6, 7]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 151, uniform=True)
    ap = lambda x: W.stokes_apply(n, grid, etas, etan, x, bc=MIXED, strict=False)
    A = M.assemble(ap, n).tocsr()
    x = np.random.default_rng(152).standard_normal(A.shape[0])
    y = ap(x)
    assert np.abs(A @ x - y).max() <= 1e-13 * np.abs(y).max()
    vel = np.stack([M.velocity_classes(D, n, False)[0] for D in range(3)] + [np.zeros(n, dtype=bool)], axis=-1).reshape(-1)
    iv = np.nonzero(vel)[0]
    Avv = A[iv][:, iv]
    assert abs(Avv - Avv.T).max() <= 1e-13 * abs(Avv).max() and abs(Avv).max() > 0
    A0 = M.assemble(lambda x: M.stokes_apply(n, grid, etas, etan, x, strict=False), n).tocsr()
    dA = (A - A0).tocoo()
    assert dA.nnz > 0 and np.all(dA.row[dA.data != 0] == dA.col[dA.data != 0])


def test_tangential_translation_leaves_the_null_space_with_noslip():
    n = [6, 7, 8]; L = [1.0e5, 1.3e5, 0.9e5]
    grid, etas, etan, rho = _fields3(n, L, 161)
    rng = np.random.default_rng(162)
    ref = np.abs(M.stokes_apply(n, grid, etas, etan, rng.standard_normal(4 * int(np.prod(n))), strict=False)).max()
    for q in range(3):
        X = np.zeros(n + [4]); X[..., q] = 1.0
        ix = M._index(n)[q]
        away = ((ix >= 2) & (ix <= n[q] - 3))                # not next to the walls the translation is normal to
        # natural rows: the interior rows
        rows = M.velocity_classes(q, n, False)[0] & away
        y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=[F] * 6, strict=False).reshape(n + [4])
        assert rows.any() and np.abs(y[..., q][rows]).max() <= 1e-13 * ref
        y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=[N] * 6, strict=False).reshape(n + [4])
        assert np.abs(y[..., q][rows]).max() > 1e-3 * ref
        # strict rows: the slaved rows
        rows = M.velocity_classes(q, n, True)[1] & away
        y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=[F] * 6, strict=True).reshape(n + [4])
        assert rows.any() and not y[..., q][rows].any()
        y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=[N] * 6, strict=True).reshape(n + [4])
        assert np.all(y[..., q][rows] != 0)


@pytest.mark.parametrize("bc2", [[N, F, F, F], [F, F, N, F], [N, F, N, F], [F, N, F, F], [N, N, N, N], [F, F, F, F]],
                         ids=["z0", "zL", "z0zL", "x0", "all", "none"])
@pytest.mark.parametrize("inv", [2, 1, 0])
def test_advection_velocity_reduces_to_the_oracle(oracle, inv, bc2):
    """Ghosts of the padded centre grid under extrusion, the slices interior along the invariant axis; "z0": a no-slip z0 wall next to
    free-slip x-walls, whose passes write the z0 ghost row's two end entries."""
    act = [a for a in range(3) if a != inv]
    nx2 = [7, 9]; n_inv = 6
    rng = np.random.default_rng(170 + inv)
    grid2 = [_nonuniform(nx2[0], 660e3, rng), _nonuniform(nx2[1], 800e3, rng)]
    gm2 = oracle.gridmp_of(grid2)
    n3 = [0, 0, 0]; gm3 = [None] * 3
    n3[inv] = n_inv; gm3[inv] = (np.arange(n_inv) + 0.5) * 1e5
    for d in range(2):
        n3[act[d]] = nx2[d]; gm3[act[d]] = gm2[d]
    ext = lambda a: _extrude(a, inv, n_inv)
    v2 = [rng.standard_normal(nx2), rng.standard_normal(nx2)]
    v3 = [None] * 3
    v3[act[0]], v3[act[1]], v3[inv] = ext(v2[0]), ext(v2[1]), np.zeros(n3)
    bc3 = [F] * 6
    for d in range(2):
        bc3[act[d]], bc3[act[d] + 3] = bc2[d], bc2[d + 2]
    g2, V2 = oracle.advection_velocity(v2, gm2, nx2, bc2)
    g3, V3 = W.advection_velocity(v3, gm3, n3, bc=bc3)
    for d in range(2):
        assert np.array_equal(g3[act[d]], g2[d])
    for k in range(1, n_inv):
        sl = [slice(None)] * 3; sl[inv] = k
        for d in range(2):
            assert np.array_equal(V3[act[d]][tuple(sl)], V2[d]), (k, d)
        assert not V3[inv][tuple(sl)].any()
    if bc2 == [N, F, F, F]:
        assert not V2[1][0, 1:-1].any() and V2[1][1, 1:-1].all()      # the skipped pass leaves the z0 ghost row zero
