"""CPU checks that earn tests/stokes3_flow_model.py (the NumPy model of flow through the walls) its authority: without a flow it IS
tests/stokes3_moving_model.py, its right-hand side is linear in the flow wall by wall, plug flow solves the walls model's operator
exactly, its advection ghosts put Un on the wall, and its net flux tells a balanced corner flow from an unbalanced one.  The
pure-Python layer of pylamp3d (wall_flows, wall_fluxes, advection_velocity(wallflow=...)) is checked against it, by message where it
rejects."""
import numpy as np
import pytest

import stokes3_flow_model as Q
import stokes3_model as M
import stokes3_moving_model as V
import stokes3_walls_model as W
from test_stokes3_model import _fields3, _mid

LD = np.longdouble
N, F = W.NOSLIP, W.FREESLIP
ALL = [N] * 6
GRAV = (3.0, -4.0, 5.0)
ZERO = (0.0, 0.0, 0.0)
NX = [6, 7, 8]
LEN = [1.0e5, 1.3e5, 0.9e5]
U0 = 2e-9


def _corner(grid, u=U0, scaled=True):
    """In at z0, out at xL; the walls have unequal areas, so the outflow is scaled by the ratio of the areas."""
    Lz, Lx = grid[0][-1] - grid[0][0], grid[1][-1] - grid[1][0]
    return [u, None, None, None, u * (Lx / Lz if scaled else 1.0), None]


def test_no_flow_is_the_moving_wall_model():
    grid, etas, etan, rho = _fields3(NX, LEN, 311)
    rng = np.random.default_rng(312)
    vel = [rng.standard_normal(NX) for _ in range(3)]
    gm = _mid(grid)
    U = np.zeros((6, 3)); U[0] = (0.0, 1e-9, -2e-9)
    for bc, u in ((None, None), (ALL, U), ([N, F, N, F, N, F], U)):
        for strict in (True, False):
            ref = V.stokes_rhs(NX, grid, etas, etan, rho, grav=GRAV, bc=bc, wallvel=u, strict=strict, rounded=False)
            refs = V.stokes_rhs_scaled(NX, grid, etas, etan, rho, grav=GRAV, bc=bc, wallvel=u, strict=strict)
            for flow in (None, [None] * 6):
                r = Q.stokes_rhs(NX, grid, etas, etan, rho, grav=GRAV, bc=bc, wallvel=u, wallflow=flow, strict=strict, rounded=False)
                assert r.dtype == ref.dtype and np.array_equal(r, ref)
                assert np.array_equal(Q.stokes_rhs_scaled(NX, grid, etas, etan, rho, grav=GRAV, bc=bc, wallvel=u, wallflow=flow, strict=strict), refs)
        g0, V0 = V.advection_velocity(vel, gm, NX, bc=bc, wallvel=u)
        for flow in (None, [None] * 6):
            g1, V1 = Q.advection_velocity(vel, gm, NX, bc=bc, wallvel=u, wallflow=flow)
            for q in range(3):
                assert np.array_equal(g0[q], g1[q]) and np.array_equal(V0[q], V1[q])
                assert np.array_equal(np.signbit(V0[q]), np.signbit(V1[q]))             # (the sign of zero as well)


def test_rhs_is_linear_in_the_flow_wall_by_wall():
    grid, etas, etan, rho = _fields3(NX, LEN, 321)
    rng = np.random.default_rng(322)
    Kc = LD(M.scaling(grid, etas, etan)[0])
    per_wall = []
    for w in range(6):
        p, q = Q.AXES[w % 3]
        fl = [None] * 6
        fl[w] = rng.standard_normal((NX[p] - 1, NX[q] - 1)) * 1e-9
        per_wall.append(fl)
    part = [Q.flow_rhs(NX, fl) for fl in per_wall]
    for w, R in enumerate(part):
        a = w % 3
        assert not R[..., 3].any() and all(not R[..., c].any() for c in range(3) if c != a)
        plane = np.moveaxis(R[..., a], a, 0)
        at = 0 if w < 3 else NX[a] - 1
        assert np.array_equal(plane[at][:-1, :-1], per_wall[w][w].astype(LD))
        assert not plane[at][-1, :].any() and not plane[at][:, -1].any()               # the ghost entries beyond stay 0
        assert not np.delete(plane, at, axis=0).any()                                    # nothing off the wall plane
        neg = [None if f is None else -4.0 * f for f in per_wall[w]]                     # (a power of two: exact)
        assert np.array_equal(Q.flow_rhs(NX, neg), -4.0 * R)
    # the walls' rows are disjoint, and the whole right-hand side is gravity's and the sliding walls' plus Kcont times the flow's
    assert all(not ((part[a] != 0) & (part[b] != 0)).any() for a in range(6) for b in range(a))
    both = [per_wall[w][w] for w in range(6)]
    both = [f - Q.net_flux(grid, both)[0] / 6 / (s * _area(grid, w)) for w, (f, s) in enumerate(zip(both, (1, 1, 1, -1, -1, -1)))]
    both = [np.asarray(f, dtype=np.float64) for f in both]
    assert Q.balanced(grid, both)
    U = np.zeros((6, 3)); U[0] = (0.0, 1e-9, -2e-9)
    for strict in (True, False):
        g = V.stokes_rhs(NX, grid, etas, etan, rho, grav=GRAV, bc=ALL, wallvel=U, strict=strict, rounded=False)
        r = Q.stokes_rhs(NX, grid, etas, etan, rho, grav=GRAV, bc=ALL, wallvel=U, wallflow=both, strict=strict, rounded=False)
        assert np.array_equal(r, g + (Kc * Q.flow_rhs(NX, both)).reshape(-1))
        # the scaled entry of an identity row is Un itself
        s = Q.stokes_rhs_scaled(NX, grid, etas, etan, rho, grav=ZERO, bc=ALL, wallflow=both, strict=strict)
        assert np.array_equal(s, Q.flow_rhs(NX, both).reshape(-1).astype(np.float64))
        d = V.row_divisor(NX, grid, etas, etan, ALL, strict)
        rows = Q.flow_rhs(NX, both) != 0
        assert np.allclose(np.asarray(d, dtype=np.float64)[rows], float(Kc), rtol=1e-15, atol=0)


def _area(grid, w):
    p, q = Q.AXES[w % 3]
    return LD(grid[p][-1] - grid[p][0]) * LD(grid[q][-1] - grid[q][0])


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "natural"])
@pytest.mark.parametrize("a", [0, 1, 2], ids=["z", "x", "y"])
def test_plug_flow_is_exact(a, strict):
    """Non-uniform grid, three decades of viscosity, gravity zero, all walls free-slip, the low and the high wall of axis a carrying the
    same U: v_a = U on every v_a entry (the faces of the cells), the other components and P zero, has zero residual in the walls
    model's operator.  Bound: 1e-15 of the largest right-hand side entry, in longdouble (the terms are differences of equal numbers)."""
    grid, etas, etan, rho = _fields3(NX, LEN, 331 + a)
    flow = [None] * 6
    flow[a] = flow[a + 3] = U0
    b = Q.stokes_rhs(NX, grid, etas, etan, rho, grav=ZERO, bc=None, wallflow=flow, strict=strict, rounded=False)
    X = np.zeros(NX + [4], dtype=LD)
    p, q = Q.AXES[a]
    sl = [slice(None)] * 3
    sl[p] = slice(0, NX[p] - 1); sl[q] = slice(0, NX[q] - 1)
    X[..., a][tuple(sl)] = U0
    y = W.stokes_apply(NX, grid, etas, etan, X.reshape(-1), bc=None, strict=strict, rounded=False)
    r = np.abs(np.asarray(y, dtype=LD) - np.asarray(b, dtype=LD)).max()
    print("plug flow along %d, strict=%s: residual %.3e of %.3e" % (a, strict, float(r), float(np.abs(b).max())))
    assert np.abs(b).max() > 0 and r <= 1e-15 * np.abs(b).max()
    # and a wall left out of the right-hand side is seen
    flow[a + 3] = None
    with pytest.raises(Exception, match="net flux"):
        Q.stokes_rhs(NX, grid, etas, etan, rho, grav=ZERO, bc=None, wallflow=flow, strict=strict, rounded=False)


@pytest.mark.parametrize("kind", [F, N], ids=["freeslip", "noslip"])
def test_ghost_planes_put_un_on_the_wall(kind):
    """One wall at a time: the mean of the ghost and its neighbour is Un for the normal component (to the rounding of 2 Un - V, four
    ulps of |Un| + |V|), and for the tangential ones the neighbour's value (free-slip: copied) or the wall's U (no-slip)."""
    grid, _, _, _ = _fields3(NX, LEN, 341)
    gm = _mid(grid)
    rng = np.random.default_rng(342)
    vel = [rng.standard_normal(NX) for _ in range(3)]
    eps = np.finfo(np.float64).eps
    for w in range(6):
        a = w % 3
        p, q = Q.AXES[a]
        un = rng.standard_normal((NX[p] - 1, NX[q] - 1))
        flow = [None] * 6; flow[w] = un
        bc = [F] * 6; bc[w] = kind
        U = np.zeros((6, 3))
        if kind == N and w % 2:
            U[w] = rng.standard_normal(3); U[w, a] = 0.0                  # every other no-slip wall also slides
        _, A = Q.advection_velocity(vel, gm, NX, bc=bc, wallvel=U, wallflow=flow)
        ghost, inner = (0, 1) if w < 3 else (NX[a], NX[a] - 1)
        for c in range(3):
            Am = np.moveaxis(A[c], a, 0)
            g, i = Am[ghost][1:-1, 1:-1], Am[inner][1:-1, 1:-1]
            if c == a:
                assert np.all(np.abs(0.5 * (g + i) - un) <= 4 * eps * (np.abs(un) + np.abs(i)))
            elif kind == F:
                assert np.array_equal(g, i)
            else:
                assert np.all(np.abs(0.5 * (g + i) - U[w, c]) <= 4 * eps * (abs(U[w, c]) + np.abs(i)))
        # the rim of the plane takes the clamped entry
        Am = np.moveaxis(A[a], a, 0)
        if w == 5:                                                        # (no later pass overwrites its corners)
            assert Am[ghost][0, 0] == 2 * un[0, 0] - Am[inner][0, 0] and Am[ghost][-1, -1] == 2 * un[-1, -1] - Am[inner][-1, -1]


def test_net_flux_tells_a_balanced_corner_flow_from_an_unbalanced_one():
    grid, etas, etan, rho = _fields3(NX, LEN, 351)
    good, bad = _corner(grid), _corner(grid, scaled=False)
    phi, flux, tot = Q.net_flux(grid, good)
    assert flux[0] > 0 and flux[4] < 0 and not flux[[1, 2, 3, 5]].any()
    assert abs(phi) <= LD(1e-10) * tot and Q.balanced(grid, good)
    phi, flux, tot = Q.net_flux(grid, bad)
    assert abs(phi) > LD(1e-10) * tot and not Q.balanced(grid, bad)
    assert abs(float(phi) - U0 * LEN[2] * (LEN[1] - LEN[0])) <= 1e-12 * float(tot)
    with pytest.raises(Exception, match="net flux"):
        Q.stokes_rhs(NX, grid, etas, etan, rho, grav=ZERO, bc=ALL, wallflow=bad)
    # pylamp3d.wall_fluxes gives the same figures
    from pylamp_amd import pylamp3d as P3
    for fl in (good, bad):
        f, ph = P3.wall_fluxes(grid, fl)
        phi, flux, tot = Q.net_flux(grid, fl)
        assert np.allclose(f, np.asarray(flux, dtype=np.float64), rtol=1e-15, atol=0) and abs(ph - float(phi)) <= 1e-15 * float(tot)


def test_python_layer_matches_the_model_and_rejects_by_message():
    from pylamp_amd import pylamp3d as P3
    grid, _, _, _ = _fields3(NX, LEN, 361)
    gm = _mid(grid)
    rng = np.random.default_rng(362)
    vel = [rng.standard_normal(NX) for _ in range(3)]
    prof = rng.standard_normal((NX[0] - 1, NX[2] - 1))
    U = np.zeros((6, 3)); U[0] = (0.0, 0.5, -0.25)
    for bc, u, flow in ((None, None, [1.0, None, None, 1.0, None, None]),
                        ([N, F, F, N, F, F], None, [None, prof, None, None, prof, None]),
                        (ALL, U, [1.0, None, None, None, 0.75, None]),
                        (ALL, U, {"y0": -0.5, "zL": 2.0})):
        fl = P3.wall_flows(flow, NX)
        _, A = P3.advection_velocity(vel, gm, NX, bc, u, flow)
        _, B = Q.advection_velocity(vel, gm, NX, bc=bc, wallvel=u, wallflow=fl)
        for q in range(3):
            assert np.array_equal(A[q], B[q]) and np.array_equal(np.signbit(A[q]), np.signbit(B[q]))
    assert P3.wall_flows(None, NX) == [None] * 6
    assert P3.wall_flows([2.5] + [None] * 5, NX)[0].shape == (NX[1] - 1, NX[2] - 1)
    with pytest.raises(Exception, match=r"advection_velocity: the flow of wall xL needs the shape \(nz - 1, ny - 1\) = \(5, 7\) or a scalar \(got \(5, 6\)\)"):
        P3.advection_velocity(vel, gm, NX, None, None, [None] * 4 + [np.zeros((5, 6)), None])
    with pytest.raises(Exception, match=r"the wall flow needs six entries \[z0, x0, y0, zL, xL, yL\] \(got 3\)"):
        P3.wall_flows([None] * 3, NX)
    with pytest.raises(Exception, match=r"names a wall 'top'"):
        P3.wall_flows({"top": 1.0}, NX)
    bad = np.zeros((NX[0] - 1, NX[1] - 1)); bad[2, 3] = np.inf
    with pytest.raises(Exception, match=r"wall yL has a non-finite flow entry \[2, 3\] = inf"):
        P3.wall_flows([None] * 5 + [bad], NX)
    # Options3 knows the new name, and Simulation3 rejects a flow before it creates a context
    assert P3.Options3().bcstokesflow is None
    for kw, msg in ((dict(tracdens=8, tracdens_min=4), r"bcstokesflow: a flow through the walls needs tracs_fence_enabled = False together with marker_deletion = True"),
                    (dict(tracs_fence_enabled=False, marker_deletion=True), r"bcstokesflow: a flow through the walls needs the refill of depleted cells, tracdens >= tracdens_min > 0")):
        with pytest.raises(Exception, match=msg):
            P3.Simulation3([5, 5, 5], [1.0, 1.0, 1.0], options=P3.Options3(bcstokesflow=[1e-9, None, None, 1e-9, None, None], **kw))
