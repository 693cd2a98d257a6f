"""What makes tests/stokes2_mg_model.py -- the NumPy model of the 2-D Stokes preconditioner on rectilinear grids -- trustworthy
without a GPU: its level-0 block is the oracle's matrix (pinned to the reference by the goldens), its coarse blocks are
rediscretisations, on uniform grids it reproduces oracle/proto_stokes_solver.py (which the device matches at 1e-11), its transfers
and line solves obey their defining properties, and as a preconditioner of the oracle's matrix it shows the orderings DESIGN.md
section 4 claims.  The module also defines the cases of tests/test_hip_mg_model.py and measures, for each, the model's own rounding
(float64 against longdouble): FLOORS, which sets the bar of the GPU comparison."""
import os

import numpy as np
import pytest

import stokes2_mg_model as M
from conftest import golden

ROW_TOL = 1e-13                                                  # row-wise |A||x| bar of an operator application (the suite's own)
BCS = {"ffff": [1, 1, 1, 1], "nfnf": [0, 1, 0, 1], "nfff": [0, 1, 1, 1], "ffnf": [1, 1, 0, 1]}
TSTEP, THETA = 3.0e11, 0.5                                       # oracle/gen_golden.py, the surface-stabilisation fixtures
LMAX_BAND = 0.15                                                 # the device's cold power iteration against the converged eigenvalue


def _nonuni(n, Ld, rng):
    w = rng.uniform(0.7, 1.3, n - 1); g = np.concatenate([[0.0], np.cumsum(w)]); return g * (Ld / g[-1])


def _centres(grid):
    return [np.append(0.5 * (g[1:] + g[:-1]), g[-1] + 0.5 * (g[-1] - g[-2])) for g in grid]


def visc_fields(grid, var=0):
    """Smooth over three decades plus a short-wavelength term (tests/test_hip_solve.py, the fused-levels test), and a density.
    var shifts the phases of both terms: another field of the same kind, for a case whose power iteration would otherwise leave
    the band within twelve iterations (test_rounding_floor_and_power_iteration_of_the_gpu_cases)."""
    Lz, Lx = grid[0][-1], grid[1][-1]
    f = lambda z, x: 1e20 * 10 ** (1.5 * np.sin(2 * np.pi * x / Lx + 0.4 * var) * np.cos(np.pi * z / Lz + 0.3 * var)
                                   + 0.3 * np.sin(17 * x / Lx + var) * np.sin(23 * z / Lz + 2 * var))
    Z, X = np.meshgrid(*grid, indexing="ij")
    Zc, Xc = np.meshgrid(*_centres(grid), indexing="ij")
    rho = 3300 + 40 * np.sin(2 * np.pi * X / Lx) * np.sin(np.pi * Z / Lz)
    return f(Z, X), f(Zc, Xc), rho


# ---------------------------------------------------------------------------------------------------------------------
# the cases of the GPU comparison: id -> (nodes, domain, grid kind, walls, environment, stabilisation theta or None)
# Domains are in units of 5 km x the number given; "rect": cell widths uniform random in 0.7 .. 1.3 on both axes, "graded": z graded
# 20 x geometrically, x uniform.  Each shape is the smallest at which the path named exists.
# ---------------------------------------------------------------------------------------------------------------------
KNOBS = {
    "default": {},
    "ts32": {"PYLAMP_MG_TS32": "1", "PYLAMP_MG_FUSED_MAX": "100000000"},                 # 32-node tiles on every level, level 0 included
    "staged": {"PYLAMP_MG_FUSED": "0"},                                                   # one kernel per stage, global-memory tail
    "stagedall": {"PYLAMP_MG_FUSED": "0", "PYLAMP_MG_TAIL": "0"},                         # ... down to the coarsest level
    "nu31": {"PYLAMP_MG_NU": "3,3", "PYLAMP_MG_NU0": "1,1"},                              # the bench's NS = 1 / NS = 3 tile instances
    "nu11": {"PYLAMP_MG_NU": "1,1"},
}
CASES = {}


# (nodes, grid kind, walls, line knob) -> var of visc_fields, where the field with var = 0 leaves the band on its smallest levels
VISC_VAR = {((129, 97), "rect", "nfnf", ""): 2, ((129, 129), "rect", "ffff", "2"): 3}


def _case(cid, nx, dom, kind, bc, env=None, stab=None):
    env = dict(env or {})
    var = VISC_VAR.get((tuple(nx), kind, bc, env.get("PYLAMP_MG_LINE", "")), 0)
    CASES[cid] = dict(id=cid, nx=list(nx), dom=dom, kind=kind, bc=BCS[bc], bcname=bc, env=env, stab=stab, var=var)


for _nx in ([129, 97], [73, 105]):          # two tile levels + the LDS tail at 33 x 25 | 4.5 x 6.5 tiles of 16: partial last tiles
    for _bc in ("ffff", "nfnf"):
        for _k, _env in KNOBS.items():
            _case("tiles-%dx%d-%s-%s" % (_nx[0], _nx[1], _bc, _k), _nx, (_nx[0] - 1, _nx[1] - 1), "rect", _bc, _env)
# global-memory tail with the tile kernels on: the 37 x 37 + 19 x 19 + 10 x 10 tail needs 19884 doubles of the 18600-double LDS pool
# (10 (nz+2)(nx+2) + 2 (nz+5) + 2 (nx+5) per level); every tail of at most 33 x 33 nodes fits (17896 for 33^2 ... 5^2)
_case("gmtail-73x73-nfnf", [73, 73], (72, 72), "rect", "nfnf", {"PYLAMP_MG_TAIL_NODES": "1369"})
_case("coarse-12x10-nfnf", [12, 10], (11, 9), "rect", "nfnf")                            # one level: the coarsest sweep count alone
_case("coarse-9x9-ffff", [9, 9], (8, 8), "rect", "ffff")                                 # two levels
_case("coarse-21x37-nfff", [21, 37], (20, 36), "rect", "nfff")                           # three levels, the last with odd cell counts
# line relaxation: cells 8:1
_case("lines-65x17-ffff", [65, 17], (64, 128), "rect", "ffff")                           # z-lines by themselves
_case("lines-17x65-nfnf", [17, 65], (128, 64), "rect", "nfnf")                           # x-lines by themselves
_case("lines-513x9-ffff", [513, 9], (512, 64), "rect", "ffff")                           # 9 lines per workgroup, line count no multiple
_case("lines-4097x9-ffff", [4097, 9], (4096, 64), "rect", "ffff")                        # the longest line: one per workgroup, 5 rows per thread
_case("lines-9x4097-nfnf", [9, 4097], (64, 4096), "rect", "nfnf")                        # ... for x-lines
_case("lines-129x129-z-nfnf", [129, 129], (128, 128), "rect", "nfnf", {"PYLAMP_MG_LINE": "1"})     # lines on every level; slaved rows s != 1
_case("lines-129x129-x-ffff", [129, 129], (128, 128), "rect", "ffff", {"PYLAMP_MG_LINE": "2"})
# the anisotropy rule without lines: a = 4, ratio 96, 8 sweeps -- no tile kernels
_case("aniso-129x33-ffff", [129, 33], (128, 128), "rect", "ffff", {"PYLAMP_MG_LINE": "0"})
# wall stencil of the pressure block
for _w, _env in (("auto", {}), ("off", {"PYLAMP_SCHUR_WALL": "0"}), ("on", {"PYLAMP_SCHUR_WALL": "1"})):
    _case("wall-257x33-%s" % _w, [257, 33], (256, 256), "rect", "ffff", _env)            # x-walls, 8:1
    _case("wall-33x129-%s" % _w, [33, 129], (128, 128), "rect", "ffff", _env)            # transposed, 4:1 (some cells beyond the 6:1 cap)
    _case("wall-17x129-%s" % _w, [17, 129], (128, 128), "rect", "ffff", _env)            # 8:1 higher than wide: beyond the cap everywhere
    _case("wall-graded129-%s" % _w, [129, 129], (128, 128), "graded", "ffff", _env)      # chosen cell by cell
# stabilisation-aware velocity block: every level carries szz / szx and runs staged
_case("stab-41x57-strict", [41, 57], (40, 56), "rect", "ffff", stab=THETA)
_case("stab-41x57-flipped", [41, 57], (40, 56), "rect", "ffff", stab=-THETA)

_built = {}


def build_case(cid):
    """Grid, fields and the residual of a case (cached, read-only).  r is zero on wall / slave / ghost velocity rows: inside the
    solver those rows carry no residual."""
    if cid in _built:
        return _built[cid]
    c = dict(CASES[cid])
    nx = c["nx"]
    grng = np.random.default_rng([nx[0], nx[1], 7])
    if c["kind"] == "graded":
        w = np.geomspace(1.0, 20.0, nx[0] - 1)
        grid = [np.concatenate([[0.0], np.cumsum(w)]) / w.sum() * 5e3 * c["dom"][0], np.linspace(0, 5e3 * c["dom"][1], nx[1])]
    else:
        grid = [_nonuni(nx[d], 5e3 * c["dom"][d], grng) for d in range(2)]
    etas, etan, rho = visc_fields(grid, c["var"])
    rng = np.random.default_rng([nx[0], nx[1], 11])
    r = rng.standard_normal((nx[0], nx[1], 3))
    L0 = M.Level(grid[0], grid[1], etas, etan, c["bc"], True)
    r[:, :, 0][~L0.iz] = 0.0; r[:, :, 1][~L0.ix] = 0.0
    c.update(grid=grid, etas=etas, etan=etan, rho=rho, r=r.reshape(-1))
    for a in (grid[0], grid[1], etas, etan, rho, c["r"]):
        a.setflags(write=False)
    _built[cid] = c
    return c


def model_knobs(c):
    """The arguments of M.Precond that the case's environment and grid select, by the model's own rules."""
    env, grid, nx = c["env"], c["grid"], c["nx"]
    line_knob = int(env.get("PYLAMP_MG_LINE", -1))
    smoothers = M.line_levels(grid, line_knob)
    nu, nu0, ratio = (2, 2), None, 6.0
    if "PYLAMP_MG_NU" in env or "PYLAMP_MG_NU0" in env:
        if "PYLAMP_MG_NU" in env:
            nu = tuple(int(v) for v in env["PYLAMP_MG_NU"].split(","))
        if "PYLAMP_MG_NU0" in env:
            nu0 = tuple(int(v) for v in env["PYLAMP_MG_NU0"].split(","))
    else:
        ratio, n = M.aniso_rule(grid, lines_allowed=line_knob != 0)
        if n is not None:
            nu = (n, n)
    wall = M.wall_stencil_on(grid, int(env.get("PYLAMP_SCHUR_WALL", -1)))
    kw = dict(nu=nu, nu0=nu0, ratio=ratio, smoothers=smoothers, wall=wall)
    if c["stab"] is not None:
        kw.update(rho=c["rho"], tstep=TSTEP, theta=c["stab"])
    return kw


def operator_key(c):
    """Cases with the same key share their levels (and so their eigenvalues)."""
    return (tuple(c["nx"]), c["kind"], c["bcname"], c["env"].get("PYLAMP_MG_LINE", ""), c["stab"])


_lam = {}


def converged_lambdas(c):
    """Converged lambda_max of every level's iteration matrix (cached per operator)."""
    key = operator_key(c)
    if key not in _lam:
        kw = model_knobs(c)
        P = M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=[1.0] * len(kw["smoothers"]), **kw)
        _lam[key] = [L.lambda_max(k) for L, k in zip(P.levels, P.smoothers)]
    return _lam[key]


FLOORS = {}
_power = {}


def rounding_floor(cid):
    """Per component |z64 - z_ld|_inf / |z_ld|_inf of the model itself, with lmax = 1.1 x the converged eigenvalues."""
    if cid not in FLOORS:
        c = build_case(cid)
        kw = model_knobs(c)
        lm = [1.1 * v for v in converged_lambdas(c)]
        z64 = M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=lm, **kw).apply(c["r"])
        zld = M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=lm, ld=True, **kw).apply(c["r"], rounded=False)
        Z64, ZLD = z64.reshape(-1, 3), zld.reshape(-1, 3)
        FLOORS[cid] = [float(np.max(np.abs(Z64[:, q] - ZLD[:, q])) / np.max(np.abs(ZLD[:, q]))) for q in range(3)]
    return FLOORS[cid]


# ---------------------------------------------------------------------------------------------------------------------
def _vv_block(oracle, nx, grid, etas, etan, rho, bc, **kw):
    A, _ = oracle.stokes_csr(nx, grid, etas, etan, rho, bc, **kw)
    N = nx[0] * nx[1]
    iv = np.sort(np.concatenate([np.arange(N) * 3, np.arange(N) * 3 + 1]))
    return A[iv][:, iv].tocsr()


def _rand_fields(shape, seed):
    rng = np.random.default_rng(seed)
    nx = list(shape)
    grid = [_nonuni(nx[d], 5e3 * (nx[d] - 1), rng) for d in range(2)]
    etas = 1e19 * 10 ** rng.uniform(0, 3, nx); etan = 1e19 * 10 ** rng.uniform(0, 3, nx)
    rho = 3300 + rng.uniform(-50, 50, nx)
    return nx, grid, etas, etan, rho, rng


@pytest.mark.parametrize("bc", ["ffff", "nfnf", "nfff", "ffnf"])
@pytest.mark.parametrize("shape,stab", [((13, 11), False), ((9, 14), False), ((12, 13), True)])
def test_level0_block_is_the_oracle_matrix(oracle, shape, stab, bc):
    """Level 0 on a rectilinear grid with random viscosities over three decades: on the rows that carry an equation the model's
    block times a random vector is the oracle's velocity-velocity block times it; the oracle's other rows (walls, slaved rows,
    ghosts) vanish on every vector the model's closure produces."""
    nx, grid, etas, etan, rho, rng = _rand_fields(shape, [shape[0], shape[1], 1])
    kw = dict(surfstab=True, tstep=TSTEP, theta=THETA) if stab else {}
    Avv = _vv_block(oracle, nx, grid, etas, etan, rho, BCS[bc], **kw)
    L = M.Level(grid[0], grid[1], etas, etan, BCS[bc], True, rho if stab else None, THETA * TSTEP * M.GRAV_Z if stab else 0.0)
    v = rng.standard_normal((nx[0], nx[1], 2))
    yz, yx = L.apply(v[:, :, 0], v[:, :, 1])
    ref = (Avv @ v.reshape(-1)).reshape(nx[0], nx[1], 2); bar = ROW_TOL * (abs(Avv) @ np.abs(v.reshape(-1))).reshape(nx[0], nx[1], 2)
    assert L.iz.sum() == (nx[0] - 2) * (nx[1] - 3) and L.ix.sum() == (nx[0] - 3) * (nx[1] - 2)
    assert np.all(np.abs(yz - ref[:, :, 0])[L.iz] <= bar[:, :, 0][L.iz])
    assert np.all(np.abs(yx - ref[:, :, 1])[L.ix] <= bar[:, :, 1][L.ix])
    cz, cx = L.close(v[:, :, 0], v[:, :, 1])
    vc = np.stack([cz, cx], axis=2).reshape(-1)
    res = (Avv @ vc).reshape(nx[0], nx[1], 2); bar = ROW_TOL * (abs(Avv) @ np.abs(vc)).reshape(nx[0], nx[1], 2) + 1e-300
    assert np.all(np.abs(res[:, :, 0])[~L.iz] <= bar[:, :, 0][~L.iz])
    assert np.all(np.abs(res[:, :, 1])[~L.ix] <= bar[:, :, 1][~L.ix])


@pytest.mark.parametrize("bc", ["ffff", "nfnf"])
def test_coarse_levels_are_rediscretisations(oracle, bc):
    """Levels 1 and 2 of a 33 x 41 rectilinear hierarchy: the model's block against the oracle's matrix of the coarse grid and the
    coarsened viscosities (and density: stabilised), on the rows whose stencil stays two nodes away from every wall."""
    nx, grid, etas, etan, rho, rng = _rand_fields((33, 41), [33, 41, 2])
    for stab in (False, True):
        levels = M.build_levels(grid, etas, etan, BCS[bc], rho if stab else None, THETA * TSTEP * M.GRAV_Z if stab else 0.0)
        assert [(L.nz, L.nx) for L in levels] == [(33, 41), (17, 21), (9, 11), (5, 6)]
        kw = dict(surfstab=True, tstep=TSTEP, theta=THETA) if stab else {}
        for L in levels[1:3]:
            n = [L.nz, L.nx]
            assert np.array_equal(L.z, grid[0][::(33 - 1) // (L.nz - 1)]) and np.array_equal(L.x, grid[1][::(41 - 1) // (L.nx - 1)])
            Avv = _vv_block(oracle, n, [L.z, L.x], L.etas, L.etan, L.rho if stab else np.zeros(n), BCS[bc], **kw)
            v = rng.standard_normal((n[0], n[1], 2))
            yz, yx = L.apply(v[:, :, 0], v[:, :, 1])
            ref = (Avv @ v.reshape(-1)).reshape(n[0], n[1], 2); bar = ROW_TOL * (abs(Avv) @ np.abs(v.reshape(-1))).reshape(n[0], n[1], 2)
            far = np.zeros(n, dtype=bool); far[3:n[0] - 3, 3:n[1] - 3] = True
            assert far.sum() > 0
            assert np.all(np.abs(yz - ref[:, :, 0])[far] <= bar[:, :, 0][far])
            assert np.all(np.abs(yx - ref[:, :, 1])[far] <= bar[:, :, 1][far])


def test_viscosity_coarsening_weights():
    """[1 2 1]^2 / 16 at the nodes with the edge values repeated, 2 x 2 means at the centres, last row and column copied."""
    a = np.zeros((9, 13)); a[4, 6] = 16.0; a[0, 0] = 16.0; a[3, 12] = 16.0
    c = M.coarsen_nodes(a)
    assert c.shape == (5, 7)
    assert c[2, 3] == 4 and c[1, 3] == 0 and np.array_equal(c[0:2, 0:2], [[9, 0], [0, 0]])       # corner: (1 + 2)^2 of the clamped stencil
    assert c[1, 6] == 3 and c[2, 6] == 3                                                         # odd row at the east edge: 1 x (1 + 2)
    b = np.arange(9 * 13, dtype=float).reshape(9, 13)
    m = M.coarsen_centres(b)
    assert m.shape == (5, 7) and m[1, 2] == 0.25 * (b[2, 4] + b[2, 5] + b[3, 4] + b[3, 5])
    assert np.array_equal(m[4, :6], m[3, :6]) and np.array_equal(m[:, 6], m[:, 5])
    assert np.allclose(M.coarsen_nodes(np.full((9, 13), 3.5)), 3.5, rtol=1e-15)


@pytest.mark.parametrize("name,bc", [("stokes_solve_block41", None), ("stokes_solve_tdep33x49", None), ("uniform33x25", [0, 1, 1, 1])])
def test_uniform_grids_reproduce_the_prototype(name, bc):
    """On uniform grids the model is the prototype of oracle/proto_stokes_solver.py (which the device matches at 1e-11), with the
    same lmax: the two goldens of test_preconditioner_matches_prototype and a NOSLIP-top case with the cases' viscosity field."""
    from oracle import proto_stokes_solver as PS, pylamp_oracle as O
    if bc is None:
        g = golden(name)
        nx = [int(v) for v in g["nx"]]; grid = [g["gz"], g["gx"]]; bc = [int(v) for v in g["bc"]]
        etas, etan, rho = g["etas"], g["etan"], g["rho"]
    else:
        nx = [33, 25]; grid = [np.linspace(0, 160e3, 33), np.linspace(0, 120e3, 25)]
        etas, etan, rho = visc_fields(grid)
    P = PS.Precond(nx, grid, etas, etan, rho, bc, nu=(2, 2), mode="arith")
    lm = [L.lmax for L in P.Ls]
    A, rhs = O.stokes_csr(nx, grid, etas, etan, rho, bc)
    r = np.random.default_rng(0).standard_normal(A.shape[0]) * np.abs(rhs).max()
    cls = O.stokes_row_class(nx)
    R = r.reshape(nx[0], nx[1], 3); R[:, :, 0][cls[0] != 1] = 0.0; R[:, :, 1][cls[1] != 1] = 0.0
    Q = M.Precond(nx, grid, etas, etan, bc, lmax=lm, wall=False, smoothers=[M.POINT] * len(lm))
    assert len(Q.levels) == len(P.Ls)
    z = Q.apply(r).reshape(-1, 3); zp = P.apply(r).reshape(-1, 3)
    for q in range(3):
        ratio = np.max(np.abs(z[:, q] - zp[:, q])) / np.max(np.abs(zp[:, q]))
        print("prototype %s component %d: %.2e" % (name, q, ratio))
        assert ratio <= 1e-12, (q, ratio)
    # the prototype's 15-iteration estimates (a norm ratio: not bounded by the spectral radius) lie in the band the device is held to
    for L, l in zip(Q.levels, lm):
        conv = L.lambda_max(M.POINT)
        assert (1 - LMAX_BAND) * conv <= l / 1.1 <= (1 + LMAX_BAND) * conv, (l / 1.1, conv)


def test_transfers():
    """Prolongation reproduces a constant exactly and a linear field at the interior nodes (uniform grid: the weights are the
    uniform-grid ones); restriction weights sum to 1."""
    z, x = np.linspace(0, 16, 17), np.linspace(0, 24, 25)
    e = np.ones((17, 25))
    F = M.Level(z, x, e, e, BCS["ffff"], False); C = M.Level(z[::2], x[::2], e[::2, ::2], e[::2, ::2], BCS["ffff"], False)
    one = np.ones((C.nz, C.nx))
    pz, px = M.prolong(F, C, one, one)
    assert np.array_equal(pz, np.ones((17, 25))) and np.array_equal(px, np.ones((17, 25)))
    xc_f, xc_c = x[:-1] + 0.5, x[::2][:-1] + 1.0             # vz sits at the cell centres in x, vx at those in z
    zc_f, zc_c = z[:-1] + 0.5, z[::2][:-1] + 1.0
    ez = np.zeros((C.nz, C.nx)); ez[:, :-1] = 0.3 * z[::2][:, None] - 0.7 * xc_c[None, :] + 2.0
    ex = np.zeros((C.nz, C.nx)); ex[:-1, :] = 0.3 * zc_c[:, None] - 0.7 * x[::2][None, :] + 2.0
    pz, px = M.prolong(F, C, ez, ex)
    wz = 0.3 * z[:, None] - 0.7 * xc_f[None, :] + 2.0; wx = 0.3 * zc_f[:, None] - 0.7 * x[None, :] + 2.0
    assert np.allclose(pz[:, 1:-2], wz[:, 1:-1], rtol=1e-14, atol=0)          # all but the half cell next to each x-wall
    assert np.allclose(px[1:-2, :], wx[1:-1, :], rtol=1e-14, atol=0)
    cz, cx = M.restrict(C, np.ones((17, 25)), np.ones((17, 25)))
    # (a coarse row next to a wall along its centre axis reaches one fine node beyond the wall, which is not there: 7/8)
    assert np.allclose(cz[1:-1, 1:-2], 1.0, rtol=1e-15) and np.allclose(cx[1:-2, 1:-1], 1.0, rtol=1e-15)
    assert np.allclose(cz[1:-1, 0], 0.875, rtol=1e-15) and np.allclose(cx[0, 1:-1], 0.875, rtol=1e-15)
    assert np.all(cz[~C.iz] == 0) and np.all(cx[~C.ix] == 0)
    assert abs(sum(M.W3) - 1) < 1e-16 and abs(sum(M.W4) - 1) < 1e-16
    # a single fine entry lands on the coarse rows with the weights written in the kernels
    d = np.zeros((17, 25)); d[6, 8] = 1.0
    cz, _ = M.restrict(C, d, np.zeros((17, 25)))
    assert cz[3, 4] == 0.5 * 0.375 and cz[3, 3] == 0.5 * 0.125 and cz[3, 5] == 0 and cz[2, 4] == 0 and cz.sum() == 0.5 * 0.5
    d = np.zeros((17, 25)); d[7, 9] = 1.0
    cz, _ = M.restrict(C, d, np.zeros((17, 25)))
    assert cz[3, 4] == 0.25 * 0.375 and cz[4, 4] == 0.25 * 0.375 and cz[3, 5] == 0.25 * 0.125 and cz[3, 3] == 0


@pytest.mark.parametrize("bc,finest", [("ffff", True), ("nfnf", True), ("nfnf", False)])
@pytest.mark.parametrize("kind", [M.ZLINES, M.XLINES])
def test_line_solve_and_line_sweep(kind, bc, finest):
    """17 x 9, rectilinear: T^-1 against a dense solve with the matrix assembled entry by entry from the component's own couplings;
    one line sweep with c1 = 0, c2 = 1 and f = A v* from the zero guess returns the closure of T^-1 A v* (in the device's signs:
    v = c2 T^-1 (A 0 - f) with T = -(the couplings), so the number is -T^-1 f)."""
    nx, grid, etas, etan, rho, rng = _rand_fields((17, 9), [17, 9, 3 + kind])
    L = M.Level(grid[0], grid[1], etas, etan, BCS[bc], finest)
    vs = L.close(rng.standard_normal(nx), rng.standard_normal(nx))
    fz, fx = L.apply(*vs)
    want = []
    for comp, f in ((0, fz), (1, fx)):
        m = L.iz if comp == 0 else L.ix
        dg = L.dgz if comp == 0 else L.dgx
        if comp == 0:
            nxt, prv = (L.zN, L.zS) if kind == M.ZLINES else (L.zE, L.zW)
        else:
            nxt, prv = (L.xN, L.xS) if kind == M.ZLINES else (L.xE, L.xW)
        di, dj = (1, 0) if kind == M.ZLINES else (0, 1)
        n = nx[0] * nx[1]; T = np.eye(n)
        for i in range(nx[0]):
            for j in range(nx[1]):
                if not m[i, j]:
                    continue
                k = i * nx[1] + j
                T[k, k] = dg[i, j]
                if i + di < nx[0] and j + dj < nx[1] and m[i + di, j + dj]:
                    T[k, k + di * nx[1] + dj] = -nxt[i, j]
                if i - di >= 0 and j - dj >= 0 and m[i - di, j - dj]:
                    T[k, k - di * nx[1] - dj] = -prv[i, j]
        x = np.linalg.solve(T, f.reshape(-1)).reshape(nx)
        got = L.line_solve(comp, kind, f)
        assert np.max(np.abs(got - x)) <= 1e-13 * np.max(np.abs(x)), comp
        gld = M.Level(grid[0], grid[1], etas, etan, BCS[bc], finest, dt=M.LD).line_solve(comp, kind, f.astype(M.LD))
        assert np.max(np.abs(gld - x)) <= 1e-13 * np.max(np.abs(x)), comp
        want.append(-x)
    want = L.close(*want)
    lmax = 2.0 / (1.0 + 1.0 / 6.0)                               # theta = 1: c2 = 1
    zero = np.zeros(nx)
    got = L.smooth(kind, zero, zero, fz, fx, 1, lmax, 6.0)
    for q in range(2):
        assert np.max(np.abs(got[q] - want[q])) <= 1e-13 * np.max(np.abs(want[q])), q
    if bc == "nfnf":
        assert L.s0 != 1 and L.sL != 1 and np.array_equal(got[1][0, 1:-1], L.s0 * got[1][1, 1:-1])
        assert np.array_equal(got[1][-2, 1:-1], L.sL * got[1][-3, 1:-1])


# (nodes, domain) -> cell shape a = dx / dz: either side of every gate of the wall stencil
WALL_SHAPES = [([17, 11], (1.0, 5.0)),          # a = 8
               ([17, 11], (1.6, 2.25)),         # a = 2.25: takes the x-wall stencil (gate a >= 2)
               ([17, 11], (1.6, 1.9)),          # a = 1.9: does not
               ([11, 17], (4.0, 1.6)),          # a = 1/4: z-walls
               ([11, 17], (2.25, 1.6)),         # a = 1/2.25
               ([11, 17], (5.5, 1.6)),          # a = 1/5.5: inside the 6:1 cap
               ([11, 17], (6.5, 1.6)),          # a = 1/6.5: beyond it
               ([11, 17], (8.0, 1.6))]


def test_wall_stencil_formula():
    """The pressure block against the formula of DESIGN.md section 4 written out cell by cell on uniform grids: x-walls where the
    cells are at least twice as wide as high, z-walls where they are 2 - 6 times higher than wide, the diagonal block otherwise."""
    rng = np.random.default_rng(5)
    seen = set()
    for nx, dom in WALL_SHAPES:
        grid = [np.linspace(0, dom[0], nx[0]), np.linspace(0, dom[1], nx[1])]
        a = (dom[1] / (nx[1] - 1)) / (dom[0] / (nx[0] - 1))
        which = "x" if a >= 2.0 else ("z" if 1.0 / 6.0 < a <= 0.5 else "none")
        seen.add((which, a > 1))
        en = 10 ** rng.uniform(0, 2, nx); rp = rng.standard_normal(nx)
        Kc, Kb = 0.7, 1.3
        zp = M.pressure_block(grid, en, Kc, Kb, rp, True)
        zd = M.pressure_block(grid, en, Kc, Kb, rp, False)
        cont = M.continuity_mask(*nx)
        rh = np.where(cont, rp / Kc ** 2, 0.0)
        ghost = ~cont
        for i0 in (0, nx[0] - 2):
            ghost[i0, 0] = ghost[i0, nx[1] - 2] = False
        assert ghost[M.ANCHOR] and np.allclose(zd[cont], (en * rh)[cont], rtol=1e-15) and np.allclose(zd[ghost], (rp / Kc)[ghost], rtol=1e-15)
        assert zd[0, 0] == en[0, 1] * rh[0, 1] - rp[0, 0] / Kb and zd[nx[0] - 2, nx[1] - 2] == en[nx[0] - 2, nx[1] - 3] * rh[nx[0] - 2, nx[1] - 3] - rp[nx[0] - 2, nx[1] - 2] / Kb
        want = zd.copy()
        if which == "x":
            for jw, ji in ((0, 1), (nx[1] - 2, nx[1] - 3)):
                d = lambda i: rh[i, jw] - rh[i, ji]
                ok = lambda i: 0 <= i <= nx[0] - 2 and cont[i, jw] and cont[i, ji]
                for i in range(nx[0] - 1):
                    if not ok(i):
                        continue
                    d2 = sum(d(k) - d(i) for k in (i - 1, i + 1) if ok(k))
                    want[i, jw] = en[i, jw] * (1.45 * rh[i, jw] - 0.225 * rh[i, ji] - a * a / 4 * d2)
                    want[i, ji] = en[i, ji] * (0.25 * rh[i, jw] + 0.775 * rh[i, ji])
        if which == "z":
            for iw, ii in ((0, 1), (nx[0] - 2, nx[0] - 3)):
                d = lambda j: rh[iw, j] - rh[ii, j]
                ok = lambda j: 0 <= j <= nx[1] - 2 and cont[iw, j] and cont[ii, j]
                for j in range(nx[1] - 1):
                    if not ok(j):
                        continue
                    d2 = sum(d(k) - d(j) for k in (j - 1, j + 1) if ok(k))
                    want[iw, j] = en[iw, j] * (1.45 * rh[iw, j] - 0.225 * rh[ii, j] - 1 / (4 * a * a) * d2)
                    want[ii, j] = en[ii, j] * (0.25 * rh[iw, j] + 0.775 * rh[ii, j])
        assert (which == "none") == np.array_equal(zp, zd), (a, which)
        assert np.allclose(zp, want, rtol=1e-13, atol=1e-13 * np.abs(want).max()), (a, which)
        # a pair that holds a corner cell takes no stencil (the anchor cell (3, 2) sits in no wall pair on these grids)
        if which == "x":
            assert zp[0, 1] == zd[0, 1] and zp[1, 1] != zd[1, 1]
        # a grid of fewer than 9 nodes along an axis never takes it
        small = [grid[0][:8], grid[1]] if which == "x" else [grid[0], grid[1][:8]]
        cut = (slice(0, 8), slice(None)) if which == "x" else (slice(None), slice(0, 8))
        assert np.array_equal(M.pressure_block(small, en[cut], Kc, Kb, rp[cut], True), M.pressure_block(small, en[cut], Kc, Kb, rp[cut], False))
    assert seen == {("x", True), ("none", True), ("z", False), ("none", False)}


def test_selection_rules():
    sq = lambda nz, nx: [np.linspace(0, 1, nz), np.linspace(0, 1, nx)]
    assert M.line_levels(sq(513, 33)) == [M.ZLINES] * 4 and M.line_levels(sq(33, 513)) == [M.XLINES] * 4
    assert M.line_levels(sq(129, 33)) == [M.POINT] * 4 and M.line_levels(sq(129, 129), 1) == [M.ZLINES] * 6
    assert M.line_levels(sq(8193, 513)) == [M.POINT] + [M.ZLINES] * 7          # 8193 points: too long a line
    assert M.aniso_rule(sq(129, 33)) == (96.0, 8) and M.aniso_rule(sq(129, 129)) == (6.0, None)
    assert M.aniso_rule(sq(513, 33)) == (6.0, None) and M.aniso_rule(sq(513, 33), lines_allowed=False) == (6.0 * 256, 10)
    assert M.wall_stencil_on(sq(257, 33)) and M.wall_stencil_on(sq(33, 129)) and not M.wall_stencil_on(sq(129, 129))
    assert not M.wall_stencil_on(sq(257, 33), 0) and M.wall_stencil_on(sq(129, 129), 1) and not M.wall_stencil_on(sq(8, 65))
    assert M.coarsest_sweeps(12, 10)[0] == 12 and M.coarsest_sweeps(100, 60)[0] == 48 and M.coarsest_sweeps(5, 5) == (12, 30.0)
    assert [g[0].size for g in M.level_grids(sq(21, 37))] == [21, 11, 6] and len(M.level_grids(sq(12, 10))) == 1
    assert len(M.level_grids(sq(9, 9))) == 2


class _Outer:
    """The model behind the interface of proto_stokes_solver.Scaled / bicgstab."""

    def __init__(self, oracle, P, nx, grid, etas, etan, rho, bc):
        self.P = P
        self.A, self.b = oracle.stokes_csr(nx, grid, etas, etan, rho, bc)
        self.Kc = P.Kc

    def apply(self, r):
        return self.P.apply(r)


def test_the_preconditioner_preconditions(oracle):
    """BiCGStab of the prototype on the row-scaled oracle matrix with the model as M, isoviscous, on a square: 65 x 17 nodes
    (cells 4:1) and 129 x 9 (16:1).  Asserted are the orderings DESIGN.md section 4 claims: the wall stencil needs strictly fewer
    iterations than the diagonal pressure block, and with lines the 16:1 grid reaches rtol 1e-8 within maxit."""
    from oracle import proto_stokes_solver as PS
    counts = {}
    for nx in ([65, 17], [129, 9]):
        grid = [np.linspace(0, 1, nx[0]), np.linspace(0, 1, nx[1])]
        Z, X = np.meshgrid(*grid, indexing="ij")
        eta = np.ones(nx); rho = 1.0 + 0.1 * np.exp(-((Z - 0.4) ** 2 + (X - 0.55) ** 2) / 0.02)
        bc = BCS["ffff"]
        nlev = len(M.level_grids(grid))
        for lines in (False, True):
            for wall in (False, True):
                if lines:
                    kw = dict(smoothers=[M.ZLINES] * nlev, nu=(2, 2), ratio=6.0)
                else:
                    ratio, n = M.aniso_rule(grid, lines_allowed=False)
                    kw = dict(smoothers=[M.POINT] * nlev, nu=(n, n), ratio=ratio)
                P = M.Precond(nx, grid, eta, eta, bc, wall=wall, **kw)
                S = PS.Scaled(_Outer(oracle, P, nx, grid, eta, eta, rho, bc), nx, grid)
                x, its, res = PS.bicgstab(S.A, S.b, S, rtol=1e-8, maxit=200)
                counts[(nx[0], nx[1], lines, wall)] = (its, res)
                print("model as preconditioner %dx%d lines=%d wall=%d: %d iterations, residual %.1e" % (nx[0], nx[1], lines, wall, its, res))
    for nx in ((65, 17), (129, 9)):
        for lines in (False, True):
            assert counts[nx + (lines, True)][0] < counts[nx + (lines, False)][0], (nx, lines, counts)
    for wall in (False, True):
        its, res = counts[(129, 9, True, wall)]
        assert its < 200 and res < 1e-7, counts


@pytest.mark.parametrize("cid", sorted(CASES))
def test_rounding_floor_and_power_iteration_of_the_gpu_cases(cid):
    """For every case of tests/test_hip_mg_model.py: the model's own rounding (float64 against longdouble) -- the floor the GPU bar is
    built on -- is far below 1e-11 / 50, the rules pick what the case's comment says, and twelve power iterations from five random
    starts stay within the band the device's estimate is held to."""
    c = build_case(cid)
    fl = rounding_floor(cid)
    print("floor %-28s vz %.2e vx %.2e p %.2e" % (cid, fl[0], fl[1], fl[2]))
    assert max(fl) < 1e-11 / 50, fl
    kw = model_knobs(c)
    conv = converged_lambdas(c)
    L = M.build_levels(c["grid"], c["etas"], c["etan"], c["bc"], c["rho"] if c["stab"] is not None else None,
                       (c["stab"] or 0.0) * TSTEP * M.GRAV_Z)
    key = operator_key(c)
    if key not in _power:
        _power[key] = [[lev.lambda_power(k, 12, seed) for seed in range(5)] for lev, k in zip(L, kw["smoothers"])]
    for l, lams in enumerate(_power[key]):
        print("lambda %-28s level %d smoother %2d: converged %.4f, 12 iterations / converged %s" %
              (cid, l, kw["smoothers"][l], conv[l], " ".join("%.3f" % (v / conv[l]) for v in lams)))
        for seed, lam in enumerate(lams):
            assert (1 - LMAX_BAND) * conv[l] <= lam <= (1 + LMAX_BAND) * conv[l], (l, seed, lam, conv[l])
    # what the rules pick for the named cases
    if cid.startswith("lines-65x17"):
        assert set(kw["smoothers"]) == {M.ZLINES}
    if cid.startswith("lines-17x65") or cid.startswith("lines-9x4097"):
        assert set(kw["smoothers"]) == {M.XLINES}
    if cid.startswith("aniso-"):
        assert kw["ratio"] == 96.0 and kw["nu"] == (8, 8) and set(kw["smoothers"]) == {M.POINT}
    if cid.startswith("tiles-") or cid.startswith("coarse-") or cid.startswith("gmtail-"):
        assert set(kw["smoothers"]) == {M.POINT} and kw["ratio"] == 6.0 and not kw["wall"]
    if cid.startswith("wall-"):
        assert kw["wall"] == (not cid.endswith("-off"))
