"""k_mg_tail_lds -- the V-cycle of the levels up to 33 x 33 nodes in one workgroup, every thread's rows in registers -- through
pl_stokes_precond_apply: against tests/stokes2_mg_model.py (the NumPy model, in longdouble, with the lmax the device used), against
k_mg_tail, its global-memory twin (PYLAMP_MG_FUSED=0), and by the launch counters of pl_mg_tail_launches: which of the two ran.

Shapes, each the smallest with the property named (rectilinear grids, cell widths uniform random in 0.7 .. 1.3, the viscosity field
of tests/test_stokes2_mg_model.py::visc_fields; r is zero on the velocity rows that carry no equation):
  65 x 65, ffff and nfnf   tail 33^2, 17^2, 9^2, 5^2: all 1024 threads own a node of the first level, four levels; nfnf: slave scales != 1
  65 x 49, nfnf            tail 33 x 25, 17 x 13, 9 x 7: a partial last wave, and nx - 1 = 24 is no power of two
  41 x 57, nfff            tail 21 x 29, 11 x 15, 6 x 8: the last level has odd cell counts
  9 x 9, ffff              tail 5 x 5 alone: only the coarse-sweep branch
  65 x 65, ffff, PYLAMP_MG_NU=3,3 PYLAMP_MG_NU0=1,1     three sweeps before and after, as the 2049^2 benchmark's tail runs
  65 x 65, ffff, PYLAMP_MG_NU=1,1                       no momentum term at all: the zero-guess sweep and the c1 = 0 sweep alone
Knobs are read when a context's solver is created: one fresh context per run; runs are cached and shared by the tests.

Bars: against the model, per component, |z - z_ld|_inf <= max(1e-11, 50 x floor) |z_ld|_inf (tests/test_hip_mg_model.py: floor is the
model's own float64-against-longdouble difference for the case); against the twin, per component, max|z - z_staged| < 1e-10 max|z_staged|
(tests/test_hip_solve.py::test_fused_levels_match_the_staged_path)."""
import os

import numpy as np
import pytest

import stokes2_mg_model as M
from test_stokes2_mg_model import visc_fields

pytestmark = pytest.mark.gpu

Z_TOL = 1e-11
FLOOR_FACTOR = 50.0
TWIN_TOL = 1e-10
WALLS = {"ffff": [1, 1, 1, 1], "nfnf": [0, 1, 0, 1], "nfff": [0, 1, 1, 1]}
NU31 = {"PYLAMP_MG_NU": "3,3", "PYLAMP_MG_NU0": "1,1"}
NU11 = {"PYLAMP_MG_NU": "1,1"}
STAGED = {"PYLAMP_MG_FUSED": "0"}

# id -> (nodes, walls, environment, node counts of the tail levels)
TAIL_CASES = {
    "bench-65x65-ffff": ([65, 65], "ffff", {}, [(33, 33), (17, 17), (9, 9), (5, 5)]),
    "bench-65x65-nfnf": ([65, 65], "nfnf", {}, [(33, 33), (17, 17), (9, 9), (5, 5)]),
    "wave-65x49-nfnf": ([65, 49], "nfnf", {}, [(33, 25), (17, 13), (9, 7)]),
    "odd-41x57-nfff": ([41, 57], "nfff", {}, [(21, 29), (11, 15), (6, 8)]),
    "coarsest-9x9-ffff": ([9, 9], "ffff", {}, [(5, 5)]),
    "nu31-65x65-ffff": ([65, 65], "ffff", NU31, [(33, 33), (17, 17), (9, 9), (5, 5)]),
    "nu11-65x65-ffff": ([65, 65], "ffff", NU11, [(33, 33), (17, 17), (9, 9), (5, 5)]),
}
TWIN_CASES = ("wave-65x49-nfnf", "odd-41x57-nfff")
TAIL_NU = (None, "1,2", "3,1")

_built, _runs, _floors = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _runs.clear()
    from pylamp_amd import _context
    _context.clear_contexts()


def _build(nx, walls, env=None):
    """Grid, fields, residual and the model's arguments (cached, read-only)."""
    key = (tuple(nx), walls, tuple(sorted((env or {}).items())))
    if key in _built:
        return _built[key]
    rng = np.random.default_rng([nx[0], nx[1], 7])
    grid = []
    for d in range(2):
        w = rng.uniform(0.7, 1.3, nx[d] - 1)
        g = np.concatenate([[0.0], np.cumsum(w)])
        grid.append(g * (5e3 * (nx[d] - 1) / g[-1]))
    etas, etan, rho = visc_fields(grid)
    bc = WALLS[walls]
    r = np.random.default_rng([nx[0], nx[1], 11]).standard_normal((nx[0], nx[1], 3))
    L0 = M.Level(grid[0], grid[1], etas, etan, bc, True)
    r[:, :, 0][~L0.iz] = 0.0; r[:, :, 1][~L0.ix] = 0.0
    env = dict(env or {})
    nu, nu0, ratio = (2, 2), None, 6.0
    if "PYLAMP_MG_NU" in env:
        nu = tuple(int(v) for v in env["PYLAMP_MG_NU"].split(","))
        nu0 = tuple(int(v) for v in env["PYLAMP_MG_NU0"].split(",")) if "PYLAMP_MG_NU0" in env else None
    else:
        ratio, n = M.aniso_rule(grid)
        assert n is None and ratio == 6.0                      # near-square cells: the default sweeps and window
    smoothers = M.line_levels(grid)
    assert set(smoothers) == {M.POINT}
    kw = dict(nu=nu, nu0=nu0, ratio=ratio, smoothers=smoothers, wall=M.wall_stencil_on(grid))
    c = dict(nx=list(nx), grid=grid, etas=etas, etan=etan, rho=rho, bc=bc, r=r.reshape(-1), env=env, kw=kw)
    for a in (grid[0], grid[1], etas, etan, rho, c["r"]):
        a.setflags(write=False)
    _built[key] = c
    return c


def _case(cid):
    nx, walls, env, tail = TAIL_CASES[cid]
    c = _build(nx, walls, env)
    shapes = [(z.size, x.size) for z, x in M.level_grids(c["grid"])]
    k = len(shapes) - len(tail)                                # the tail: the levels below level 0 of at most 33^2 nodes
    assert k >= 1 and shapes[k:] == tail and (k == 1 or shapes[k - 1][0] * shapes[k - 1][1] > 33 * 33), shapes
    return c


def _device(c, extra_env):
    """z = M^-1 r on a fresh context under the case's environment plus extra_env; the tail launches that one application made."""
    from pylamp_amd import pylamp_stokes as S, _context
    env = dict(c["env"]); env.update(extra_env)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        _context.clear_contexts()
        A, _ = S.makeStokesMatrix(c["nx"], c["grid"], c["etas"], c["etan"], c["rho"], c["bc"])
        before = A.mg_tail_launches()
        z = A.precond(c["r"])
        after = A.mg_tail_launches()
        nl, lm = A.mg_info()
        out = dict(z=z, nlevels=nl, lmax=lm, plan=A.mg_plan(), launches=(after[0] - before[0], after[1] - before[1]))
        del A
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        _context.clear_contexts()


def _run(cid, extra_env=None):
    key = (cid, tuple(sorted((extra_env or {}).items())))
    if key not in _runs:
        _runs[key] = _device(_case(cid), extra_env or {})
    return _runs[key]


def _floor(cid):
    """Per component |z64 - z_ld|_inf / |z_ld|_inf of the model itself, with lmax = 1.1 x the converged eigenvalues."""
    if cid not in _floors:
        c = _case(cid)
        args = (c["nx"], c["grid"], c["etas"], c["etan"], c["bc"])
        P0 = M.Precond(*args, lmax=[1.0] * len(c["kw"]["smoothers"]), **c["kw"])
        lm = [1.1 * L.lambda_max(k) for L, k in zip(P0.levels, P0.smoothers)]
        z64 = M.Precond(*args, lmax=lm, **c["kw"]).apply(c["r"]).reshape(-1, 3)
        zld = M.Precond(*args, lmax=lm, ld=True, **c["kw"]).apply(c["r"], rounded=False).reshape(-1, 3)
        _floors[cid] = [float(np.max(np.abs(z64[:, q] - zld[:, q])) / np.max(np.abs(zld[:, q]))) for q in range(3)]
    return _floors[cid]


@pytest.mark.parametrize("cid", sorted(TAIL_CASES))
def test_lds_tail_matches_the_model(cid):
    """A: z = A.precond(r) against the model in longdouble with the device's lmax; the LDS tail ran, once."""
    c = _case(cid)
    dev = _run(cid)
    kw = c["kw"]
    assert dev["nlevels"] == len(kw["smoothers"]) and dev["plan"]["nu"] == tuple(kw["nu"]), (dev["nlevels"], dev["plan"], kw)
    assert dev["plan"]["nu0"] == tuple(kw["nu0"] or kw["nu"]) and dev["plan"]["ratio"] == kw["ratio"], (dev["plan"], kw)
    assert dev["launches"] == (1, 0), dev["launches"]
    P = M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=dev["lmax"], ld=True, **kw)
    zl = P.apply(c["r"], rounded=False).reshape(-1, 3)
    Z = dev["z"].reshape(-1, 3)
    fl = _floor(cid)
    for q in range(3):
        ratio = float(np.max(np.abs(Z[:, q] - zl[:, q])) / np.max(np.abs(zl[:, q])))
        bar = max(Z_TOL, FLOOR_FACTOR * fl[q])
        print("mg-tail model %-20s component %d: %.3e (floor %.1e, bar %.1e)" % (cid, q, ratio, fl[q], bar))
        assert ratio <= bar, (q, ratio, bar)


@pytest.mark.parametrize("tail_nu", TAIL_NU, ids=lambda v: "tailnu-" + (v or "default").replace(",", ""))
@pytest.mark.parametrize("cid", TWIN_CASES)
def test_lds_tail_matches_the_global_memory_tail(cid, tail_nu):
    """B: the default against PYLAMP_MG_FUSED=0, also with tail-only sweep counts (the model has no argument for those; k_mg_tail
    honours them).  C: the LDS tail ran in the one, the global-memory tail in the other."""
    knob = {"PYLAMP_MG_TAIL_NU": tail_nu} if tail_nu else {}
    fused, staged = _run(cid, knob), _run(cid, dict(knob, **STAGED))
    assert fused["launches"] == (1, 0), fused["launches"]
    assert staged["launches"] == (0, 1), staged["launches"]
    zf, zs = fused["z"].reshape(-1, 3), staged["z"].reshape(-1, 3)
    for q in range(3):
        diff, ref = float(np.max(np.abs(zf[:, q] - zs[:, q]))), float(np.max(np.abs(zs[:, q])))
        print("mg-tail twin %-18s %-8s component %d: %.3e" % (cid, tail_nu or "default", q, diff / ref))
        assert diff < TWIN_TOL * ref, (q, diff, ref)
    if tail_nu:                                                # the knob reached both kernels: another z than without it
        assert not np.array_equal(fused["z"], _run(cid)["z"])


def test_a_tail_beyond_the_pool_runs_in_global_memory():
    """C: with PYLAMP_MG_TAIL_NODES=1369 the tail of 73 x 73 starts at 37 x 37, which the pool rule (mg_tail_lds_fits) turns away."""
    c = _build([73, 73], "nfnf")
    dev = _device(c, {"PYLAMP_MG_TAIL_NODES": "1369"})
    assert dev["launches"] == (0, 1), dev["launches"]
    assert np.all(np.isfinite(dev["z"]))


def test_lds_tail_is_deterministic():
    """D: two fresh contexts give the same bits -- no atomics, a fixed thread-to-node map."""
    cid = "bench-65x65-nfnf"
    first, second = _run(cid), _device(_case(cid), {})
    assert second["launches"] == (1, 0)
    assert np.array_equal(first["z"], second["z"])
