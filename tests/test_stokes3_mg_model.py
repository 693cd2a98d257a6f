"""What makes tests/stokes3_mg_model.py -- the NumPy model of the 3-D Stokes preconditioner -- trustworthy without a GPU: its
level-0 block is the operator model that tests/test_stokes3_model.py and test_stokes3_walls_model.py tie to the 2-D oracle, its
coarse blocks are rediscretisations, its transfers and its smoother obey their defining properties, its V-cycle contracts towards
a direct solution of the same block, the whole of it preconditions the model's assembled matrix, and its pressure block inverts
the block it approximates.  The module also defines the cases of tests/test_hip_3d_mg_model.py and measures two things for each:
the model's own rounding (float64 against longdouble: FLOORS, the floor of the GPU bar) and how far twelve cold power iterations
from five random starts stay from the converged eigenvalue (the band the device's lmax is held to)."""
import copy

import numpy as np
import pytest

import stokes3_mg_model as G
import stokes3_model as M
import stokes3_walls_model as W

NOSLIP, FREESLIP = W.NOSLIP, W.FREESLIP
WALLS = {"free": [FREESLIP] * 6,
         "mixed": [NOSLIP, FREESLIP, NOSLIP, NOSLIP, FREESLIP, FREESLIP]}     # no-slip on a low and a high wall, two no-slip walls meet on z0-y0 and zL-y0
LMAX_BAND_2D = 0.15                # the band of the 2-D twin (tests/test_stokes2_mg_model.py): the model alone has to stay inside it


def nonuniform(n, L, rng):
    w = rng.uniform(0.7, 1.3, n - 1)
    g = np.concatenate([[0.0], np.cumsum(w)])
    return g * (L / g[-1])


def centres(grid):
    return [np.append((c[1:] + c[:-1]) / 2, c[-1] + (c[-1] - c[-2]) / 2) for c in grid]


def fields(n, var=0):
    """The problem of tests/test_hip_3d_model.py (_problem): cell widths U(0.7, 1.3) on all three axes, one smooth viscosity over three
    decades with a different wavenumber along every axis, sampled at the nodes and at the centres.  var shifts the phases: another
    field of the same kind, for a case whose twelve power iterations would otherwise leave the band (VISC_VAR)."""
    n = [int(v) for v in n]
    rng = np.random.default_rng(1000 + n[0] * 10007 + n[1] * 101 + n[2])
    L = [660e3, 660e3 * (n[1] - 1) / (n[0] - 1), 660e3 * (n[2] - 1) / (n[0] - 1)]
    grid = [nonuniform(n[a], L[a], rng) for a in range(3)]
    f = lambda z, x, y: 1e20 * 10 ** (1.5 * np.cos(np.pi * z / L[0] + 0.4 * var) * np.sin(2 * np.pi * x / L[1] + 0.3 + 0.3 * var)
                                      * np.cos(3 * np.pi * y / L[2] + 0.7 + 0.5 * var))
    Z, X, Y = np.meshgrid(*grid, indexing="ij", sparse=True)
    Zc, Xc, Yc = np.meshgrid(*centres(grid), indexing="ij", sparse=True)
    rho = 3300 + 40 * np.sin(np.pi * Z / L[0]) * np.sin(2 * np.pi * X / L[1]) * np.cos(np.pi * Y / L[2]) + 0 * Y
    return grid, f(Z, X, Y), f(Zc, Xc, Yc), rho


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU comparison.  Each shape is the smallest that has the path named.
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = {
    "one-level": ([6, 7, 9], {}, 1),               # coarsest-only cycle, the copy path of the preconditioner, anchor on the last cell layer
    "two-level": ([9, 9, 9], {}, 2),               # one restriction / prolongation, the coarse level 5^3 entirely rim
    "aniso": ([17, 13, 21], {}, 2),                # hierarchy stopped by one axis (6 -> 3 cells)
    "three-level": ([17, 25, 133], {}, 3),         # y-lines crossing the 64-lane tile on levels 0 and 1 (133, 67), a 34-node even coarsest axis
    "lds": ([37, 45, 131], {}, 2),                 # the marching LDS kernels and the rim above 200 000 nodes, partial tiles on all three tile axes
    "lds-bench-plan": ([37, 45, 131], {"PYLAMP_MG_NU3": "3", "PYLAMP_MG_NU3_FINE": "1"}, 2),   # V(1,1) / V(3,3): one-sweep smoothers on level 0
    "lds-nu3": ([37, 45, 131], {"PYLAMP_MG_NU3": "3"}, 2),                                      # the marching sweep with and without v_prev, c1 != 0
}
BLOCKS = {"blocks222": ([17, 17, 17], (2, 2, 2), 3),      # the same three levels as one rank
          "blocks411": ([17, 17, 17], (4, 1, 1), 2)}      # the block rule ends the hierarchy at two levels
# (nodes, walls, wall rows) -> var of fields(), where the field with var = 0 leaves the band
VISC_VAR = {}
CASES = {}


def _case(cid, shape, n, env, nlevels, walls, strict, P=(1, 1, 1)):
    var = VISC_VAR.get((tuple(n), walls, strict), 0)
    CASES[cid] = dict(id=cid, shape=shape, n=list(n), env=dict(env), nlevels=nlevels, walls=walls, bc=WALLS[walls], strict=strict,
                      P=tuple(P), var=var)


for _s, (_n, _env, _nl) in SHAPES.items():
    for _w in WALLS:
        for _strict in ((True,) if _s in ("lds-bench-plan", "lds-nu3") else (True, False)):
            _case("%s-%s-%s" % (_s, _w, "slaved" if _strict else "natural"), _s, _n, _env, _nl, _w, _strict)
for _s, (_n, _P, _nl) in BLOCKS.items():
    for _w in WALLS:
        _case("%s-%s-slaved" % (_s, _w), _s, _n, {}, _nl, _w, True, _P)

_built = {}


def build_case(cid):
    """Grid, fields and the residual of a case (cached, read-only).  r is standard normal on ALL entries: the rows without an
    equation have to be ignored."""
    if cid not in _built:
        c = dict(CASES[cid])
        grid, etas, etan, rho = fields(c["n"], c["var"])
        r = np.random.default_rng([11] + c["n"]).standard_normal(4 * int(np.prod(c["n"])))
        c.update(grid=grid, etas=etas, etan=etan, rho=rho, r=r)
        for a in grid + [etas, etan, rho, r]:
            a.setflags(write=False)
        _built[cid] = c
    return _built[cid]


def model_knobs(c):
    """The arguments of G.Precond that the case's environment and grid select, by the model's own rules."""
    return dict(nu=G.sweeps(c["n"], c["env"]), ratio=6.0, coarse_sweeps=12)


def operator_key(c):
    """Cases with the same key share their levels (their diagonals and eigenvalues)."""
    return (tuple(c["n"]), c["walls"], c["strict"], c["P"], c["var"])


_models = {}


def model(c, lmax, ld, **kw):
    """The model of a case: one object per operator and precision (the probed diagonals are kept), set to the knobs and bounds asked for."""
    key = operator_key(c) + (ld,)
    if key not in _models:
        nlev = len(G.level_grids(c["grid"], c["P"]))
        _models[key] = G.Precond(c["grid"], c["etas"], c["etan"], bc=c["bc"], strict=c["strict"], P=c["P"], lmax=[1.0] * nlev, ld=ld)
    P = copy.copy(_models[key])                 # (the levels are shared, the knobs and bounds are this caller's)
    k = dict(model_knobs(c), **kw)
    P.nu, P.ratio, P.coarse_sweeps, P.lmax = tuple(k["nu"]), k["ratio"], k["coarse_sweeps"], list(lmax)
    assert len(P.lmax) == len(P.levels)
    return P


_lam, _power, FLOORS = {}, {}, {}


def converged_lambdas(c):
    key = operator_key(c)
    if key not in _lam:
        # (3e-3 on the levels of 200 000 nodes, where an Arnoldi step takes 0.15 s: 5e-4 of the eigenvalue, against a band of 0.14)
        _lam[key] = [L.lambda_max(3e-3 if int(np.prod(L.n)) >= G.LDS_NODES else 1e-3) for L in model(c, [1.0] * c["nlevels"], False).levels]
    return _lam[key]


def power_estimates(c):
    """Per level: what twelve cold power iterations give from five random starts."""
    key = operator_key(c)
    if key not in _power:
        _power[key] = [[L.power_iteration(12, seed) for seed in range(5)] for L in model(c, [1.0] * c["nlevels"], False).levels]
    return _power[key]


def lmax_band(c):
    """The band the device's cold estimate is held to: the largest deviation of the model's own twelve-iteration estimates from the
    converged eigenvalue over the levels and the five seeds, doubled because the device starts from another vector."""
    conv = converged_lambdas(c)
    return 2.0 * max(abs(v / conv[l] - 1.0) for l, lams in enumerate(power_estimates(c)) for v in lams)


def rounding_floor(cid):
    """Per component |z64 - z_ld|_inf / |z_ld|_inf of the model itself, with lmax = 1.1 x the converged eigenvalues."""
    if cid not in FLOORS:
        c = build_case(cid)
        lm = [1.1 * v for v in converged_lambdas(c)]
        z64 = model(c, lm, False).apply(c["r"]).reshape(-1, 4)
        zld = model(c, lm, True).apply(c["r"], rounded=False).reshape(-1, 4)
        FLOORS[cid] = [float(np.max(np.abs(z64[:, q] - zld[:, q])) / np.max(np.abs(zld[:, q]))) for q in range(4)]
    return FLOORS[cid]


# ---------------------------------------------------------------------------------------------------------------------
def _rand3(n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(3)]


def _uniform(n, L=(1.0, 1.3, 0.9)):
    return [np.linspace(0, L[a], n[a]) for a in range(3)]


def _norm(v):
    return float(np.sqrt(sum(np.sum(np.asarray(a, dtype=np.float64) ** 2) for a in v)))


@pytest.mark.parametrize("walls", sorted(WALLS))
@pytest.mark.parametrize("strict", [True, False])
def test_level0_block_is_the_operator_model(walls, strict):
    """The INT rows of the level-0 block are the rows of the oracle-tied operator model applied to (v, P = 0), exactly; the probed
    diagonal is the diagonal of the model's assembled matrix; the closure leaves a field that satisfies the model's slaved rows."""
    n = [6, 7, 9]
    grid, etas, etan, _ = fields(n)
    L = G.Level(grid, etas, etan, WALLS[walls], strict, np.float64)
    V = _rand3(n, 3)
    X = np.zeros(n + [4]); X[..., 0], X[..., 1], X[..., 2] = V
    with M.working_precision(np.float64):
        Y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=WALLS[walls], strict=strict, rounded=False).reshape(n + [4])
    Yl = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=WALLS[walls], strict=strict).reshape(n + [4])
    A = M.assemble(lambda x: W.stokes_apply(n, grid, etas, etan, x, bc=WALLS[walls], strict=strict), n)
    dg = A.diagonal().reshape(n + [4])
    for D in range(3):
        interior = M.velocity_classes(D, n, strict)[0]
        assert np.array_equal(L.apply(V)[D], np.where(interior, Y[..., D], 0))
        assert np.allclose(Y[..., D], Yl[..., D], rtol=0, atol=1e-12 * np.abs(Yl[..., D]).max())     # the float64 evaluation is the same model
        assert np.all(L.diag[D][interior] < 0)
        assert np.allclose(L.diag[D][interior], dg[..., D][interior], rtol=1e-13, atol=0)
    if strict:      # a closed field satisfies the slaved rows of the matrix: A [close(v), 0] vanishes there
        C = L.close(V)
        X[..., 0], X[..., 1], X[..., 2] = C
        Yc = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=WALLS[walls], strict=True).reshape(n + [4])
        Kc = M.scaling(grid, etas, etan)[0]
        for D in range(3):
            slaved = M.velocity_classes(D, n, True)[1]
            assert slaved.any() and np.abs(Yc[..., D][slaved]).max() <= 1e-13 * Kc * np.abs(C[D]).max() / np.diff(grid[0]).min()


@pytest.mark.parametrize("walls", sorted(WALLS))
def test_coarse_levels_are_rediscretisations(walls):
    """Uniform grid, one viscosity: every coarse block is the operator model built directly on every second node with natural rows,
    and the coarsened viscosities are the constant."""
    n = [17, 9, 13]
    grid = _uniform(n)
    eta = np.full(n, 3.0e20)
    levels = G.build_levels(grid, eta, eta, WALLS[walls], True)
    assert [L.n for L in levels] == [[17, 9, 13], [9, 5, 7]] and levels[0].strict and not levels[1].strict
    C = levels[1]
    assert np.array_equal(C.etas, np.full(C.n, 3.0e20)) and np.array_equal(C.etan, np.full(C.n, 3.0e20))
    cg = [g[::2] for g in grid]
    V = _rand3(C.n, 5)
    X = np.zeros(C.n + [4]); X[..., 0], X[..., 1], X[..., 2] = V
    with M.working_precision(np.float64):
        Y = W.stokes_apply(C.n, cg, eta[::2, ::2, ::2], eta[::2, ::2, ::2], X.reshape(-1), bc=WALLS[walls], strict=False,
                           rounded=False).reshape(C.n + [4])
    for D in range(3):
        assert np.array_equal(C.apply(V)[D], np.where(M.velocity_classes(D, C.n, False)[0], Y[..., D], 0))


def test_level_rule():
    lv = lambda n, P=(1, 1, 1): [[c.size for c in g] for g in G.level_grids(_uniform(n), P)]
    assert lv([6, 7, 9]) == [[6, 7, 9]]
    assert lv([9, 9, 9]) == [[9, 9, 9], [5, 5, 5]]
    assert lv([17, 13, 21]) == [[17, 13, 21], [9, 7, 11]]                      # 6 -> 3 cells: odd
    assert lv([17, 25, 133]) == [[17, 25, 133], [9, 13, 67], [5, 7, 34]]
    assert lv([37, 45, 131]) == [[37, 45, 131], [19, 23, 66]]
    assert lv([17, 17, 17], (2, 2, 2)) == [[17, 17, 17], [9, 9, 9], [5, 5, 5]]
    assert lv([17, 17, 17], (4, 1, 1)) == [[17, 17, 17], [9, 9, 9]]            # 2 cells per block cannot be halved to 2
    assert G.sweeps([37, 45, 131]) == (2, 2) and G.sweeps([101, 101, 101]) == (1, 3)
    assert G.sweeps([37, 45, 131], {"PYLAMP_MG_NU3": "3", "PYLAMP_MG_NU3_FINE": "1"}) == (1, 3)
    assert G.sweeps([101, 101, 101], {"PYLAMP_MG_NU3": "2"}) == (2, 2) and G.sweeps([9, 9, 9], {"PYLAMP_MG_NU3": "3"}) == (3, 3)
    assert G.coarsest_sweeps([5, 5, 5]) == (12, 30.0)
    n, ratio = G.coarsest_sweeps([19, 23, 66])
    assert ratio == 0.4 * (19 * 23 * 66.0) ** (2.0 / 3.0) and n == int(np.sqrt(ratio)) and 12 < n < 150
    assert G.lds_levels(_uniform([37, 45, 131])) == [True, False] and G.lds_levels(_uniform([17, 25, 133])) == [False] * 3


def test_transfers():
    """Prolongation reproduces constants everywhere and functions linear along a component's own axis everywhere (the clamps act on
    the other two axes); restriction is P^T / 8 on the coarse rows whose stencil stays off the walls; the coarsening reproduces a
    constant viscosity exactly and a node stencil of [1 2 1]^3 / 64."""
    nf = [9, 11, 13]
    grid = _uniform(nf)
    one = np.ones(nf)
    F, C = G.build_levels(grid, one, one, None, True)
    assert C.n == [5, 6, 7]
    const = [np.full(C.n, 2.5)] * 3
    for D, p in enumerate(G.prolong(nf, C, const)):
        assert np.array_equal(p, np.full(nf, 2.5))
    lin = [np.broadcast_to(M._along(np.arange(C.n[D], dtype=float), D), C.n) for D in range(3)]
    for D, p in enumerate(G.prolong(nf, C, lin)):
        assert np.array_equal(p, np.broadcast_to(M._along(np.arange(nf[D]) / 2.0, D), nf))
    # along another axis a linear function is reproduced between the clamps: 3/4 - 1/4 of the midpoints J - 1/2 .. J + 1/2
    mid = [np.broadcast_to(M._along(np.arange(C.n[1], dtype=float) + 0.5, 1), C.n)] * 3
    p = G.prolong(nf, C, mid)[0]                                  # vz along x
    j = np.arange(nf[1])
    inside = (j >= 1) & (j <= nf[1] - 3)
    assert np.allclose(p[:, inside, :], ((j + 0.5) / 2.0)[None, inside, None], rtol=0, atol=1e-15)
    # R = P^T / 8 away from the walls, by unit vectors
    Nc, Nf = int(np.prod(C.n)), int(np.prod(nf))
    allrows = G.Level([g[::2] for g in grid], np.ones(C.n), np.ones(C.n), None, False, np.float64)
    allrows.int_ = [np.ones(C.n, dtype=bool)] * 3                 # the weights alone, without the mask of the coarse rows
    for D in range(3):
        Pm = np.zeros((Nf, Nc)); Rm = np.zeros((Nc, Nf))
        for q in range(Nc):
            e = np.zeros(Nc); e[q] = 1.0
            ec = [np.zeros(C.n)] * 3; ec[D] = e.reshape(C.n)
            Pm[:, q] = G.prolong(nf, C, ec)[D].reshape(-1)
        for q in range(Nf):
            e = np.zeros(Nf); e[q] = 1.0
            ef = [np.zeros(nf)] * 3; ef[D] = e.reshape(nf)
            Rm[:, q] = G.restrict(allrows, ef)[D].reshape(-1)
        ix = M._index(C.n)
        E, Fx = (D + 1) % 3, (D + 2) % 3
        off = (ix[D] >= 1) & (ix[D] <= C.n[D] - 2) & (ix[E] >= 1) & (ix[E] <= C.n[E] - 3) & (ix[Fx] >= 1) & (ix[Fx] <= C.n[Fx] - 3)
        rows = np.flatnonzero(off.reshape(-1))
        assert rows.size > 0
        assert np.allclose(Rm[rows], Pm.T[rows] / 8.0, rtol=0, atol=1e-15)
        assert np.allclose(Rm[rows].sum(axis=1), 1.0, rtol=0, atol=1e-15)
    # the mask: restriction gives zero on the coarse rows that are not INT
    r = G.restrict(C, _rand3(nf, 1))
    for D in range(3):
        assert np.all(r[D][~C.int_[D]] == 0) and np.all(r[D][C.int_[D]] != 0)
    # viscosity coarsening
    assert np.array_equal(G.coarsen_nodes(np.full(nf, 7.0e21)), np.full(C.n, 7.0e21))
    assert np.array_equal(G.coarsen_centres(np.full(nf, 7.0e21)), np.full(C.n, 7.0e21))
    a = np.random.default_rng(2).uniform(1, 2, nf)
    cn = G.coarsen_nodes(a)
    w = np.array([1, 2, 1]) / 4.0
    assert cn[2, 2, 3] == pytest.approx(np.einsum("i,j,k,ijk", w, w, w, a[3:6, 3:6, 5:8]), rel=1e-15)
    assert cn[0, 0, 0] == pytest.approx(np.einsum("i,j,k,ijk", w, w, w, np.pad(a, 1, mode="edge")[0:3, 0:3, 0:3]), rel=1e-15)
    cc = G.coarsen_centres(a)
    assert cc[1, 2, 3] == pytest.approx(a[2:4, 4:6, 6:8].mean(), rel=1e-15)
    assert np.array_equal(cc[-1], cc[-2]) and np.array_equal(cc[:, -1], cc[:, -2]) and np.array_equal(cc[:, :, -1], cc[:, :, -2])


@pytest.mark.parametrize("walls,strict", [("free", False), ("mixed", False)])
def test_smoothing_property(walls, strict):
    """n Chebyshev-Jacobi sweeps with f = 0 multiply an eigenvector of T = close . D^-1 A with eigenvalue lambda by p_n(lambda), the
    scaled Chebyshev polynomial of the window [lmax / ratio, lmax]:  |p_n(lambda)| <= 1 / T_n(sigma),  sigma = (ratio + 1) /
    (ratio - 1),  T_n(sigma) = cosh(n arccosh sigma), for every lambda in the window.  With the converged lmax and ratio = 6 the top
    third of the spectrum lies in the window: every such eigenvector shrinks by at least that bound, n = 1, 2, 3.  (Natural rows, the rows
    of every coarse level, with both sets of walls: with slaved rows a few eigenvalues of T are complex pairs, and the statement is
    about a real spectrum.)"""
    n = [6, 7, 9]
    grid, etas, etan, _ = fields(n)
    L = G.Level(grid, etas, etan, WALLS[walls], strict, np.float64)
    idx = [np.flatnonzero(m.reshape(-1)) for m in L.int_]
    cut = np.cumsum([0] + [i.size for i in idx])
    N = int(cut[-1])

    def unpack(x):
        V = []
        for D in range(3):
            a = np.zeros(int(np.prod(n)), dtype=x.dtype); a[idx[D]] = x[cut[D]:cut[D + 1]]
            V.append(a.reshape(n))
        return L.close(V)

    pack = lambda V: np.concatenate([V[D].reshape(-1)[idx[D]] for D in range(3)])
    T = np.stack([pack(L.jacobi(unpack(e))) for e in np.eye(N)], axis=1)
    lam, vec = np.linalg.eig(T)
    assert np.abs(lam.imag).max() <= 1e-9 * np.abs(lam).max() and lam.real.min() > 0
    lam, vec = lam.real, vec.real
    lmax = lam.max()
    assert L.lambda_max() == pytest.approx(lmax, rel=1e-4)
    ratio = 6.0
    sigma = (ratio + 1) / (ratio - 1)
    top = np.flatnonzero(lam >= 2.0 * lmax / 3.0)
    assert top.size >= 10
    zero = [np.zeros(n)] * 3
    worst = 0.0
    for nsw in (1, 2, 3):
        bound = 1.0 / np.cosh(nsw * np.arccosh(sigma))
        for k in top[:: max(1, top.size // 12)].tolist() + [int(np.argmax(lam))]:
            w = unpack(vec[:, k])
            out = L.smooth(w, zero, nsw, lmax, ratio)
            shrink = _norm(out) / _norm(w)
            worst = max(worst, shrink / bound)
            assert shrink <= bound * (1 + 1e-9), (nsw, k, lam[k], shrink, bound)
    print("smoothing %s strict=%s: largest shrink / bound %.4f over %d eigenvectors of the top third" % (walls, strict, worst, top.size))


def _velocity_block(c, P):
    """The assembled velocity block of level 0 with all its rows (INT, slaved, identity) and a refined direct solver for it."""
    n, grid, etas, etan, bc, strict = c["n"], c["grid"], c["etas"], c["etan"], c["bc"], c["strict"]
    N = int(np.prod(n))

    def apply_v(x, rounded=True):
        X = np.zeros(n + [4], dtype=np.longdouble); X[..., :3] = np.asarray(x).reshape(n + [3])
        Y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=bc, strict=strict, rounded=False).reshape(n + [4])
        return M._out(Y[..., :3].reshape(-1), rounded)
    A4 = M.assemble(lambda x: W.stokes_apply(n, grid, etas, etan, x, bc=bc, strict=strict), n)
    iv = np.sort(np.concatenate([np.arange(N) * 4 + q for q in range(3)]))
    return A4, M.DirectSolver(A4[iv][:, iv], apply_v)


def _plain_case(n, walls, strict):
    grid, etas, etan, rho = fields(n)
    return dict(n=list(n), grid=grid, etas=etas, etan=etan, rho=rho, bc=WALLS[walls], walls=walls, strict=strict, P=(1, 1, 1), var=0,
                env={}, nlevels=len(G.level_grids(grid)))


CONTRACTION = {}          # (nodes, walls, wall rows) -> measured asymptotic contraction factor per cycle


@pytest.mark.parametrize("n", [[9, 9, 9], [17, 13, 21]])
@pytest.mark.parametrize("walls,strict", [("free", True), ("mixed", True), ("mixed", False)])
def test_vcycle_contracts_towards_the_direct_solution(n, walls, strict):
    """Richardson iteration v += M_vv^-1 (f - A_vv v) with the model's V-cycle (lmax = 1.1 x converged) against the refined direct
    solution of the same block (stokes3_model.DirectSolver): the error shrinks in every one of 25 cycles; the factor of the last
    cycles is printed (DESIGN.md 6c quotes it) and stays below 0.9."""
    c = _plain_case(n, walls, strict)
    P = model(c, [1.1 * v for v in converged_lambdas(c)], False)
    L0 = P.levels[0]
    A4, solver = _velocity_block(c, P)
    f = [np.where(L0.int_[D], a, 0) for D, a in enumerate(_rand3(n, 17))]
    exact = solver.solve(np.stack(f, axis=3).reshape(-1)).reshape(n + [3])
    exact = [exact[..., D] for D in range(3)]
    assert _norm([a - b for a, b in zip(L0.close(exact), exact)]) <= 1e-10 * _norm(exact)      # the direct solution is closed
    v = [np.zeros(n)] * 3
    errs = [_norm(exact)]
    for _ in range(25):
        e = P.vcycle(0, L0.residual(v, f))
        v = [v[D] + e[D] for D in range(3)]
        errs.append(_norm([a - b for a, b in zip(v, exact)]))
    fac = np.array(errs[1:]) / np.array(errs[:-1])
    CONTRACTION[(tuple(n), walls, strict)] = float(fac[-5:].max())
    print("contraction %s %s strict=%s: first cycle %.3f, cycles 21-25 %.3f, error after 25 cycles %.1e" %
          (n, walls, strict, fac[0], fac[-5:].max(), errs[-1] / errs[0]))
    assert fac.max() < 1.0 and fac[-5:].max() < 0.9, fac


def _bicgstab(A, b, prec, rtol, maxit):
    """Right-preconditioned BiCGStab; returns (x, iterations, relative residual)."""
    x = np.zeros_like(b); r = b.copy(); rt = r.copy()
    rho = alpha = omega = 1.0
    v = np.zeros_like(b); p = np.zeros_like(b)
    bn = np.linalg.norm(b)
    for it in range(1, maxit + 1):
        rho_new = rt @ r
        beta = (rho_new / rho) * (alpha / omega)
        p = r + beta * (p - omega * v)
        y = prec(p); v = A @ y
        alpha = rho_new / (rt @ v)
        s = r - alpha * v
        z = prec(s); t = A @ z
        omega = (t @ s) / (t @ t)
        x = x + alpha * y + omega * z
        r = s - omega * t
        rho = rho_new
        if np.linalg.norm(r) <= rtol * bn:
            return x, it, float(np.linalg.norm(r) / bn)
    return x, maxit, float(np.linalg.norm(r) / bn)


ITERATIONS = {}


@pytest.mark.parametrize("n", [[9, 9, 9], [17, 13, 21]])
@pytest.mark.parametrize("walls,strict", [("free", True), ("mixed", True)])
def test_the_model_preconditions_the_assembled_matrix(n, walls, strict):
    """BiCGStab on the model's assembled 4-component matrix, row-scaled as the solver scales it (every row by the coefficient of its
    own unknown, INT momentum and symmetry rows by minus it, continuity rows by Kcont sum(1/d)), with the whole model as M: 1e-7 is
    reached; the count is printed (tests/test_hip_3d_model.py quotes 40-58 iterations of the device on [17, 13, 21])."""
    c = _plain_case(n, walls, strict)
    P = model(c, [1.1 * v for v in converged_lambdas(c)], False)
    A4, _ = _velocity_block(c, P)
    Kc = M.scaling(c["grid"], c["etas"], c["etan"])[0]
    s = A4.diagonal().reshape(n + [4]).copy()
    for D in range(3):
        s[..., D] = np.where(P.levels[0].int_[D], -s[..., D], s[..., D])
    cont, sx, sy = M.pressure_classes(n, strict)
    srd = sum(M._along(np.append(1 / np.diff(c["grid"][a]), 0.0), a) for a in range(3))
    s[..., 3] = np.where(cont, Kc * srd, np.where(sx | sy, -s[..., 3], s[..., 3]))
    assert np.all(s != 0)
    import scipy.sparse as sp
    As = sp.diags(1.0 / s.reshape(-1)) @ A4
    b = W.stokes_rhs(n, c["grid"], c["etas"], c["etan"], c["rho"], bc=c["bc"], strict=strict) / s.reshape(-1)
    x, its, res = _bicgstab(As, b, P.apply, 1e-7, 150)
    ITERATIONS[(tuple(n), walls, strict)] = its
    print("model as preconditioner %s %s strict=%s: %d iterations, residual %.1e" % (n, walls, strict, its, res))
    assert res <= 1e-7 and its <= 150, (its, res)          # (BiCGStab counts move by tens with the last digits of lmax: no tighter bound)


@pytest.mark.parametrize("strict", [True, False])
def test_pressure_block_inverts_the_block_it_approximates(strict):
    """The identity: let S^ be the pressure block of M -- the scaled identity rows (P) and symmetry rows (P_nb - P) of A [0, 0, 0, p]
    as the operator model gives them (A has no pressure-pressure coupling on the continuity rows, which are zero), and on the
    continuity rows the diagonal approximation p Kcont / (sum(1/d) eta_n).  Then S^-1 (S^ p) = p on every cell, and with r_v = 0 the
    right-hand side of the V-cycle is -A_vp p: minus the momentum rows of A [0, 0, 0, p].  One cell layer in y (5 nodes: layers 0 .. 3,
    all of them wall layers or next to one) makes every chain two hops long."""
    n = [7, 6, 5]
    grid, etas, etan, _ = fields(n)
    P = G.Precond(grid, etas, etan, bc=WALLS["mixed"], strict=strict, lmax=[1.0], ld=True)
    Kc, Kb = M.scaling(grid, etas, etan)
    p = np.random.default_rng(4).standard_normal(n)
    X = np.zeros(n + [4]); X[..., 3] = p
    Y = W.stokes_apply(n, grid, etas, etan, X.reshape(-1), bc=WALLS["mixed"], strict=strict, rounded=False).reshape(n + [4])
    cont, sx, sy = M.pressure_classes(n, strict)
    assert np.all(Y[..., 3][cont] == 0) and (not strict or (sx.any() and sy.any()))
    srd = sum(M._along(np.append(1 / np.diff(np.asarray(grid[a], dtype=np.longdouble)), 0), a) for a in range(3))
    r = np.zeros(n + [4], dtype=np.longdouble)
    r[..., 3] = np.where(cont, p * Kc / np.where(cont, srd * etan, 1), np.where(sx | sy, Y[..., 3] / Kb, Y[..., 3] / Kc))
    zp, mag = P.pressure(r, terms=True)
    assert np.abs(zp - p).max() <= 1e-17 * np.abs(p).max() * 20 and np.all(mag >= np.abs(zp) * (1 - 1e-15))
    f = P.rhs(r, zp)
    L0 = P.levels[0]
    for D in range(3):
        want = np.where(L0.int_[D], -Y[..., D], 0)
        assert np.abs(f[D] - want).max() <= 1e-17 * np.abs(want).max() * 20


def test_extrusion_gives_a_y_invariant_result():
    """A y-invariant extrusion of a 2-D problem gives a y-invariant z with z_vy = 0: uniform in y, slaved free-slip rows (the rows
    that carry an equation then have a y-invariant diagonal, which natural rows on the y-walls do not), r_vy = 0, and no pressure
    residual in the anchor's column and in the cell layers on the z- and x-walls (the symmetry rows of the y-wall edges would turn
    it into a y-dependent pressure).  One level: with a coarse level the invariance is not exact next to the y-walls, where full
    weighting reads zeros beyond the wall and the weights of the outermost coarse row add up to 7/8.  The device does the same."""
    n = [9, 9, 7]
    g3, es3, en3, _ = fields([9, 9, 9])
    grid = [g3[0], g3[1], np.linspace(0, 5e5, n[2])]
    etas = np.repeat(es3[:, :, 4:5], n[2], axis=2); etan = np.repeat(en3[:, :, 4:5], n[2], axis=2)
    r = np.repeat(np.random.default_rng(9).standard_normal((n[0], n[1], 1, 4)), n[2], axis=2)
    r[..., 2] = 0.0
    r[M.ANCHOR[0], M.ANCHOR[1], :, 3] = 0.0
    for a in (0, 1):
        for layer in (0, n[a] - 2):
            np.moveaxis(r[..., 3], a, 0)[layer] = 0.0
    P = G.Precond(grid, etas, etan, strict=True, lmax=None)
    assert len(P.levels) == 1
    z = P.apply(r.reshape(-1)).reshape(n + [4])
    assert np.abs(z[..., 2]).max() <= 1e-13 * np.abs(z[..., 0]).max()
    for q in (0, 1, 3):
        cells = z[:, :, :n[2] - 1, q]
        assert np.abs(cells).max() > 0 and np.abs(cells - cells[:, :, :1]).max() <= 1e-13 * np.abs(cells).max(), q


SMALL = [cid for cid in sorted(CASES) if int(np.prod(CASES[cid]["n"])) < G.LDS_NODES]
LARGE = [cid for cid in sorted(CASES) if CASES[cid]["shape"] == "lds"]


@pytest.mark.parametrize("cid", SMALL + LARGE)
def test_rounding_floor_and_power_iteration_of_the_gpu_cases(cid):
    """For every case of tests/test_hip_3d_mg_model.py (the two knob variants of the LDS shape share the operator of `lds`): the
    hierarchy the rules give is the one the case names; the model's own rounding (float64 against longdouble) is far below
    1e-11 / 50; twelve power iterations from five random starts stay within 15 % of the converged eigenvalue, the band of the 2-D twin."""
    c = build_case(cid)
    assert len(G.level_grids(c["grid"], c["P"])) == c["nlevels"]
    assert G.lds_levels(c["grid"], c["P"]) == [c["shape"].startswith("lds")] + [False] * (c["nlevels"] - 1)
    fl = rounding_floor(cid)
    print("floor %-28s vz %.2e vx %.2e vy %.2e p %.2e" % (cid, fl[0], fl[1], fl[2], fl[3]))
    assert max(fl) < 1e-11 / 50, fl
    conv = converged_lambdas(c)
    for l, lams in enumerate(power_estimates(c)):
        print("lambda %-28s level %d: converged %.4f, 12 iterations / converged %s" % (cid, l, conv[l], " ".join("%.3f" % (v / conv[l]) for v in lams)))
    print("band %-28s %.3f" % (cid, lmax_band(c)))
    assert lmax_band(c) <= 2 * LMAX_BAND_2D, lmax_band(c)
