"""What makes tests/stokes3_krylov_model.py -- the NumPy model of the 3-D Krylov loop, the hydrostatic start, the deflation and the
velocity-error estimate -- trustworthy without a GPU: its hydrostatic pressure cancels the rows it is built to cancel, its deflation
weights turn the scaled continuity rows into the volume integral of the divergence, its corrected preconditioner satisfies the identity
it exists for, its recurrence residual is the true residual, and the whole loop reaches the direct solution of the assembled model
matrix.  The module also defines the cases of tests/test_hip_3d_krylov.py and records, per case, rho_model = (true velocity error) /
(reported estimate) of the model's own loop at its own stop (RHO_MODEL: the honesty check of the GPU test leans on it)."""
import numpy as np
import pytest

import stokes3_krylov_model as K
import stokes3_mg_model as G
import stokes3_model as M
import stokes3_flow_model as F
import stokes3_walls_model as W
from test_stokes3_mg_model import WALLS, fields

EPS = float(np.finfo(np.float64).eps)


def graded(n, L, ratio):
    """n coordinates from 0 to L whose cell widths grow geometrically by `ratio` from the first to the last."""
    h = float(ratio) ** np.linspace(0.0, 1.0, n - 1)
    c = np.concatenate([[0.0], np.cumsum(h)]) * (L / h.sum())
    c[-1] = L
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU comparison: viscosity over three decades (contrast 1e3), the density of test_stokes3_mg_model.fields
# ---------------------------------------------------------------------------------------------------------------------
CASES = {
    "one-level": dict(n=[6, 7, 9], walls="free", graded=False),          # no coarse level: no deflation
    "two-level": dict(n=[9, 9, 9], walls="free", graded=False),
    "aniso-mixed": dict(n=[17, 13, 21], walls="mixed", graded=False),
    "aniso-graded": dict(n=[17, 13, 21], walls="free", graded=True),     # cells 3 : 1 along z, uniform along x and y
}
_built = {}


def build_case(cid):
    if cid not in _built:
        c = dict(CASES[cid], id=cid)
        n = c["n"]
        grid, etas, etan, rho = fields(n)
        if c["graded"]:
            L = [g[-1] for g in grid]
            grid = [graded(n[0], L[0], 3.0), np.linspace(0, L[1], n[1]), np.linspace(0, L[2], n[2])]
        c.update(grid=grid, etas=etas, etan=etan, rho=rho, bc=WALLS[c["walls"]], strict=True)
        for a in list(grid) + [etas, etan, rho]:
            a.setflags(write=False)
        _built[cid] = c
    return _built[cid]


_systems = {}


def system(cid, ld):
    if (cid, ld) not in _systems:
        c = build_case(cid)
        if (cid, not ld) in _systems:
            _systems[cid, ld] = _systems[cid, not ld].other(ld)
        else:
            _systems[cid, ld] = K.System(c["grid"], c["etas"], c["etan"], c["rho"], bc=c["bc"], strict=c["strict"], ld=ld)
    return _systems[cid, ld]


# rho_model per case: measured by test_loop_reaches_the_direct_solution below, which holds the model to them
RHO_MODEL = {"two-level": 0.7405, "aniso-mixed": 0.4135, "aniso-graded": 0.3039}

_direct, _loops = {}, {}


def direct_solution(cid):
    """The solution of the assembled model matrix with the model's unscaled right-hand side (sparse LU + refinement in longdouble)."""
    if cid not in _direct:
        c = build_case(cid)
        ap = lambda x, rounded=True: W.stokes_apply(c["n"], c["grid"], c["etas"], c["etan"], x, bc=c["bc"], strict=c["strict"], rounded=rounded)
        A = M.assemble(ap, c["n"])
        rhs = F.stokes_rhs(c["n"], c["grid"], c["etas"], c["etan"], c["rho"], bc=c["bc"], strict=c["strict"])
        _direct[cid] = M.direct_solve(A, ap, rhs)
    return _direct[cid]


def velocity_error(x, ref):
    d = (np.asarray(x, dtype=np.float64) - ref).reshape(-1, 4)[:, :3]
    return float(np.linalg.norm(d) / np.linalg.norm(ref.reshape(-1, 4)[:, :3]))


def model_loop(cid):
    """The model's own solve of a case in float64: preconditioner bounds 1.1 x the converged eigenvalues, its own deflation vector."""
    if cid not in _loops:
        s = system(cid, False)
        Mfn = K.preconditioner(s, None)
        defl, Md = None, Mfn
        if len(G.level_grids(s.grid)) > 1:
            w, res = K.deflation_solve(s, Mfn)
            assert res < 0.05
            defl = (s.yAw(w), K.dot(s.vel(w), s.vel(w)))
            Md = s.M_deflated(Mfn, w)
        xh = s.hydrostatic()
        out = K.bicgstab(s, Md, s.b, xh, K.shadow(s.n).reshape(-1), ref_norm=float(s.reference_norm(xh)), defl=defl)
        out["true_error"] = velocity_error(out["x"], direct_solution(cid))
        _loops[cid] = out
    return _loops[cid]


# ---------------------------------------------------------------------------------------------------------------------
def _hash_py(i, j, k, seed):
    m = 0xFFFFFFFF
    h = ((i * 73856093) & m) ^ ((j * 19349663) & m) ^ ((k * 83492791) & m) ^ (seed & m)
    h ^= h >> 16; h = (h * 0x7feb352d) & m
    h ^= h >> 15; h = (h * 0x846ca68b) & m
    h ^= h >> 16
    return h


def test_shadow_is_the_integer_hash():
    n = [6, 7, 300]
    s = K.shadow(n)
    assert s.shape == (6, 7, 300, 4)
    assert not s[-1].any() and not s[:, -1].any() and not s[:, :, -1].any()
    for (i, j, k) in [(0, 0, 0), (1, 2, 3), (4, 5, 298), (3, 0, 257), (2, 5, 64)]:
        for c in range(4):
            assert s[i, j, k, c] == _hash_py(i, j, k, 1234 + c) * 2.0 / 2 ** 32 - 1.0
    inner = s[:-1, :-1, :-1]
    assert -1.0 <= inner.min() and inner.max() < 1.0 and abs(inner.mean()) < 0.02
    assert not np.array_equal(K.shadow(n, 99)[..., 0], s[..., 0])
    assert np.array_equal(K.shadow(n, 1235)[..., 0], s[..., 1])


@pytest.mark.parametrize("ld", [False, True])
@pytest.mark.parametrize("walls", sorted(WALLS))
@pytest.mark.parametrize("grade", [False, True])
def test_hydrostatic_start_cancels_a_layered_load(ld, walls, grade):
    """Density that varies with z only: b - A x_h vanishes on the interior z-momentum rows to rounding -- each row is
    b_z + 2 Kc rD (P_i - P_{i-1}) over the divisor, P carries the rounding of up to nz same-sign steps -- and the reference norm is 0."""
    n = [6, 7, 9]
    grid, etas, etan, _ = fields(n)
    if grade:
        grid = [graded(n[0], grid[0][-1], 3.0), grid[1], grid[2]]
    rho = 3300.0 + 200.0 * np.tanh(3 * (grid[0] / grid[0][-1] - 0.4))[:, None, None] + np.zeros(n)
    s = K.System(grid, etas, etan, rho, bc=WALLS[walls], strict=True, ld=ld)
    xh, mag = s.hydrostatic(terms=True)
    assert not s.vel(xh).any()
    res = (s.b - s.A(xh)).reshape(n + [4])
    interior = M.velocity_classes(0, n, True)[0]
    z = np.asarray(grid[0], dtype=s.dt)
    hD = np.zeros(n, dtype=s.dt); hD[1:-1] = ((z[2:] - z[:-2]) / 2)[:, None, None]
    d = np.asarray(s.divisor[..., 0], dtype=s.dt)
    terms = np.abs(s.b.reshape(n + [4])[..., 0])
    terms[1:] = terms[1:] + s.Kc * (mag[1:] + mag[:-1]) / np.where(hD[1:] > 0, hD[1:], 1) / d[1:]
    eps = float(np.finfo(s.dt).eps)
    bound = 2 * (n[0] + 4) * eps * terms + EPS * np.abs(s.b.reshape(n + [4])[..., 0])      # (b itself is rounded to float64)
    assert interior.any() and np.all(np.abs(res[..., 0])[interior] <= bound[interior])
    assert terms[interior].min() > 0 and np.abs(s.b.reshape(n + [4])[..., 0][interior]).min() > 0
    assert s.reference_norm(xh) == 0


def test_hydrostatic_reference_norm_of_a_mantle_field():
    """The 3-D mantle field of tests/test_hip_3d.py (_mantle3): lateral density contrasts leave a dynamic load; the reference norm is
    the norm of b - A x_h recomputed through the assembled matrix."""
    import scipy.sparse as sp
    n = [9, 9, 13]
    L = [660e3, 660e3, 660e3 * 12 / 8]
    grid = [np.linspace(0, L[d], n[d]) for d in range(3)]
    mid = [np.append(0.5 * (g[1:] + g[:-1]), g[-1] + 0.5 * (g[-1] - g[-2])) for g in grid]

    def field(c):
        Z, X, Y = np.meshgrid(*c, indexing="ij", sparse=True)
        return 273 + 1350 * np.clip(Z / L[0], 0, 1) + 60 * np.sin(3 * np.pi * X / L[1]) * np.sin(np.pi * Z / L[0]) * np.cos(2 * np.pi * Y / L[2])
    eta = lambda T: np.clip(1e20 * np.exp(120e3 / (8.31446 * T) - 120e3 / (8.31446 * 1623)), 1e17, 1e23)
    Tn = field(grid)
    s = K.System(grid, eta(Tn), eta(field(mid)), 3300 / (3.5e-5 * (Tn - 1623) + 1), ld=True)
    xh = s.hydrostatic()
    ref = float(s.reference_norm(xh))
    A = M.assemble(lambda x: W.stokes_apply(n, grid, s.etas, s.etan, x, strict=True), n)
    As = sp.diags(1.0 / s.divisor.reshape(-1)) @ A
    again = np.linalg.norm(s.b.astype(np.float64) - As @ xh.astype(np.float64))
    assert ref > 0 and again > 1e-3 * float(K.norm(s.b))
    assert abs(ref - again) <= 1e-10 * again
    assert ref < 0.2 * float(K.norm(s.b))               # (the hydrostatic part is most of the load)


@pytest.mark.parametrize("walls", sorted(WALLS))
@pytest.mark.parametrize("grade", [False, True])
def test_weights_turn_continuity_rows_into_the_volume_divergence(walls, grade):
    """yw . cont_rows(v) = sum over the continuity cells of volume x div v, for a random v; and the continuity rows of the model
    operator are cont_rows."""
    n = [6, 7, 9]
    grid, etas, etan, rho = fields(n)
    if grade:
        grid = [graded(n[0], grid[0][-1], 3.0), np.linspace(0, 1.1e6, n[1]), np.linspace(0, 0.9e6, n[2])]
    s = K.System(grid, etas, etan, rho, bc=WALLS[walls], strict=True, ld=True)
    v = np.asarray(np.random.default_rng(3).standard_normal(4 * int(np.prod(n))), dtype=K.LD)
    _, yw = s.deflation_vectors()
    got = K.dot(yw, s.cont_rows(v))
    X = v.reshape(n + [4])
    d = [np.diff(np.asarray(g, dtype=K.LD)) for g in grid]
    cell = (slice(0, -1),) * 3
    flux = ((X[1:, :-1, :-1, 0] - X[:-1, :-1, :-1, 0]) * d[1][None, :, None] * d[2][None, None, :]
            + (X[:-1, 1:, :-1, 1] - X[:-1, :-1, :-1, 1]) * d[0][:, None, None] * d[2][None, None, :]
            + (X[:-1, :-1, 1:, 2] - X[:-1, :-1, :-1, 2]) * d[0][:, None, None] * d[1][None, :, None])
    cont = s.cont[cell]
    want = np.sum(np.where(cont, flux, 0))
    mag = np.sum(np.abs(flux))
    assert 0 < cont.sum() < cont.size and abs(got - want) <= 1e-16 * mag
    Av = s.A(v).reshape(n + [4])[..., 3]
    X0 = X.copy(); X0[..., 3] = 0
    # (the divisor of the system is a float64 product and sum of 1 / d_a: a few float64 roundings)
    assert np.max(np.abs(np.where(s.cont, Av - s.cont_rows(v), 0))) <= 8 * EPS * np.max(np.abs(Av))
    assert np.array_equal(s.cont_rows(X0.reshape(-1)), s.cont_rows(v))


@pytest.mark.parametrize("cid", ["one-level", "aniso-mixed", "aniso-graded"])
def test_pressure_stage_maps_u_to_a_constant(cid):
    c = build_case(cid)
    s = system(cid, True)
    u, _ = s.deflation_vectors()
    zp = G.pressure_block(c["grid"], c["etan"], s.Kc, u, c["strict"], dt=K.LD)
    assert np.max(np.abs(zp[s.cont] * s.Kc - 1)) <= 4 * float(np.finfo(K.LD).eps)


@pytest.mark.parametrize("cid", ["two-level", "aniso-mixed"])
def test_corrected_preconditioner_satisfies_its_identity(cid):
    """yw . (r - A z)_cont = 0 for z = M_deflated r, to rounding, with a random w."""
    s = system(cid, True)
    rng = np.random.default_rng(8)
    r = np.asarray(rng.standard_normal(s.b.size), dtype=K.LD)
    w = np.asarray(rng.standard_normal(s.b.size), dtype=K.LD)
    Mfn = K.preconditioner(s, [2.0] * len(G.level_grids(s.grid)))
    z, coef = s.M_deflated(Mfn, w, terms=True)(r)
    _, yw = s.deflation_vectors()
    yw = yw.reshape(-1)
    res = s.prs(r) - s.prs(s.A(z))
    cont = s.cont.reshape(-1)
    mag = np.sum(np.abs(yw * s.prs(r))) + np.sum(np.abs(yw * s.cont_rows(z - coef * w).reshape(-1))) + abs(coef) * np.sum(np.abs(yw * s.cont_rows(w).reshape(-1)))
    assert abs(s.yAw(w)) > 0 and abs(coef) > 0
    assert abs(K.dot(yw[cont], res[cont])) <= 1e-12 * mag
    assert abs(K.dot(yw, s.prs(r) - s.prs(s.A(Mfn(r))))) > 1e-6 * mag          # (the uncorrected one does not)


@pytest.mark.parametrize("cid", ["one-level", "aniso-mixed"])
@pytest.mark.parametrize("m", [1, 2, 3])
def test_recurrence_residual_is_the_true_residual(cid, m):
    s = system(cid, True)
    Mfn = K.preconditioner(s, [2.0] * len(G.level_grids(s.grid)))
    xh = s.hydrostatic()
    dx, r = K.bicgstab_steps(s.A, Mfn, s.b, xh, K.shadow(s.n).reshape(-1), m)
    true = s.b - s.A(xh + dx)
    r0 = s.b - s.A(xh)
    assert K.norm(r) < K.norm(r0)
    assert K.norm(r - true) <= 1e-15 * K.norm(r0)


@pytest.mark.parametrize("cid", sorted(RHO_MODEL))
def test_loop_reaches_the_direct_solution(cid):
    """The model's loop at the solve's default tolerances against the direct solution of the assembled model matrix: converged, the
    true velocity error below 5e-8, and rho_model = true error / reported estimate as recorded in RHO_MODEL."""
    out = model_loop(cid)
    rho = out["true_error"] / out["error_estimate"]
    print("krylov3-model %-14s iterations %d checks %d |r|/|b| %.2e estimate %.3e true error %.3e rho_model %.4f"
          % (cid, out["iterations"], out["checks"], out["rel_residual"], out["error_estimate"], out["true_error"], rho))
    assert out["converged"] and 0 < out["error_estimate"] <= K.ETOL and out["checks"] < K.MAX_CHECKS
    assert out["true_error"] < 5e-8
    assert abs(rho - RHO_MODEL[cid]) <= 0.01 * RHO_MODEL[cid]
