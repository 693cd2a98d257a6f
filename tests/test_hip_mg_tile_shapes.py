"""The 32-node instantiations of the multigrid tile kernels (k_mg_pre / k_mg_post, PYLAMP_MG_TS32=1) on shapes with several tiles per
level and partial last tiles, through pl_stokes_precond_apply: against the staged path (PYLAMP_MG_FUSED=0, all FP64), against
tests/stokes2_mg_model.py in longdouble with the device's lmax, and twice for the same bits.  A tile's set-up issues every load from
a clamped address and zeroes what does not count (mgt_fetch_* / mgt_store_*), one wave reads one spacing table, and the slave scale
is selected from values (mgt_cls_x): the shapes put tiles on the grid's rim, beyond it, and on slaved rows.

Shapes, each the smallest with the property named (rectilinear grids, cell widths uniform random in 0.7 .. 1.3, the viscosity field
of tests/test_stokes2_mg_model.py::visc_fields; r is zero on the velocity rows that carry no equation; walls ffff and nfnf, the
latter for slave scales != 1), all under PYLAMP_MG_TS32=1:
  129 x 193, NU=3,3 NU0=1,1   level 1 = 65 x 97 is 2 x 3 tiles of 32, V(3,3) as the benchmark's level 1; level 0 (4 x 6 tiles) takes the L0
                              instantiation of k_mg_pre and k_mg_post<1,32>
  131 x 99                    level 0 alone is fused (5 x 4 tiles, V(2,2)): tile counts that do not divide the level, last tiles partly
                              outside the grid
  145 x 209, NU=3,3 NU0=1,1   the same below level 0: level 1 = 73 x 105 is 3 x 4 tiles of 32, the last partial
  129 x 193, NU=1,1           NS = 1 instantiations: no momentum term
Knobs are read when a context's solver is created: one fresh context per run; runs are cached and shared by the tests.

Bars: against the model, per component, |z - z_ld|_inf <= max(1e-11, 50 x floor) |z_ld|_inf (tests/test_hip_mg_model.py: floor is
the model's own float64-against-longdouble difference for the case); against the staged path, per component,
max|z - z_staged| < 1e-10 max|z_staged| (tests/test_hip_solve.py::test_fused_levels_match_the_staged_path)."""
import os

import numpy as np
import pytest

import stokes2_mg_model as M
from test_hip_mg_tail import _build

pytestmark = pytest.mark.gpu

Z_TOL = 1e-11
FLOOR_FACTOR = 50.0
TWIN_TOL = 1e-10
TS32 = {"PYLAMP_MG_TS32": "1"}
NU31 = {"PYLAMP_MG_NU": "3,3", "PYLAMP_MG_NU0": "1,1"}
NU11 = {"PYLAMP_MG_NU": "1,1"}

# id -> (nodes, environment, node counts of levels 0 and 1)
SHAPES = {
    "nu31": ([129, 193], dict(TS32, **NU31), [(129, 193), (65, 97)]),
    "partial": ([131, 99], dict(TS32), [(131, 99), (66, 50)]),
    "partial-l1": ([145, 209], dict(TS32, **NU31), [(145, 209), (73, 105)]),
    "nu11": ([129, 193], dict(TS32, **NU11), [(129, 193), (65, 97)]),
}
CASES = [(s, w) for s in SHAPES for w in ("ffff", "nfnf")]
IDS = ["%s-%s" % c for c in CASES]

_runs, _floors = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    _runs.clear()
    from pylamp_amd import _context
    _context.clear_contexts()


def _case(shape, walls):
    nx, env, levels = SHAPES[shape]
    c = _build(nx, walls, env)
    shapes = [(z.size, x.size) for z, x in M.level_grids(c["grid"])]
    assert shapes[:2] == levels, shapes
    return c


def _device(c, env):
    """z = M^-1 r on a fresh context under env (None: the variable is unset)."""
    from pylamp_amd import pylamp_stokes as S, _context
    saved = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        _context.clear_contexts()
        A, _ = S.makeStokesMatrix(c["nx"], c["grid"], c["etas"], c["etan"], c["rho"], c["bc"])
        z = A.precond(c["r"])
        nl, lm = A.mg_info()
        out = dict(z=z, nlevels=nl, lmax=lm, plan=A.mg_plan())
        del A
        return out
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        _context.clear_contexts()


def _run(shape, walls, form):
    """form: "tiles" (the case's environment), "staged" (plus PYLAMP_MG_FUSED=0 PYLAMP_L0_MIXED=0, the twin of
    test_fused_levels_match_the_staged_path: a staged level 0 may otherwise store in FP32)."""
    key = (shape, walls, form)
    if key not in _runs:
        c = _case(shape, walls)
        off = "0" if form == "staged" else None
        _runs[key] = _device(c, dict(c["env"], PYLAMP_MG_FUSED=off, PYLAMP_L0_MIXED=off))
    return _runs[key]


def _floor(shape, walls):
    """Per component |z64 - z_ld|_inf / |z_ld|_inf of the model itself, with lmax = 1.1 x the converged eigenvalues."""
    key = (tuple(SHAPES[shape][0]), tuple(sorted(SHAPES[shape][1].items())), walls)
    if key not in _floors:
        c = _case(shape, walls)
        args = (c["nx"], c["grid"], c["etas"], c["etan"], c["bc"])
        P0 = M.Precond(*args, lmax=[1.0] * len(c["kw"]["smoothers"]), **c["kw"])
        lm = [1.1 * L.lambda_max(k) for L, k in zip(P0.levels, P0.smoothers)]
        z64 = M.Precond(*args, lmax=lm, **c["kw"]).apply(c["r"]).reshape(-1, 3)
        zld = M.Precond(*args, lmax=lm, ld=True, **c["kw"]).apply(c["r"], rounded=False).reshape(-1, 3)
        _floors[key] = [float(np.max(np.abs(z64[:, q] - zld[:, q])) / np.max(np.abs(zld[:, q]))) for q in range(3)]
    return _floors[key]


@pytest.mark.parametrize("shape,walls", CASES, ids=IDS)
def test_tiles32_match_the_staged_path(shape, walls):
    """Every multigrid stage as a kernel of its own computes the same to 1e-10 of the largest entry."""
    zf, zs = _run(shape, walls, "tiles")["z"].reshape(-1, 3), _run(shape, walls, "staged")["z"].reshape(-1, 3)
    for q in range(3):
        diff, ref = float(np.max(np.abs(zf[:, q] - zs[:, q]))), float(np.max(np.abs(zs[:, q])))
        print("mg-tiles32 staged %-18s component %d: %.3e" % (shape + "-" + walls, q, diff / ref))
        assert diff < TWIN_TOL * ref, (q, diff, ref)


@pytest.mark.parametrize("shape,walls", CASES, ids=IDS)
def test_tiles32_match_the_model(shape, walls):
    """Against the model in longdouble with the device's lmax."""
    c = _case(shape, walls)
    dev = _run(shape, walls, "tiles")
    kw = c["kw"]
    assert dev["nlevels"] == len(kw["smoothers"]) and dev["plan"]["nu"] == tuple(kw["nu"]), (dev["nlevels"], dev["plan"], kw)
    assert dev["plan"]["nu0"] == tuple(kw["nu0"] or kw["nu"]) and dev["plan"]["ratio"] == kw["ratio"], (dev["plan"], kw)
    P = M.Precond(c["nx"], c["grid"], c["etas"], c["etan"], c["bc"], lmax=dev["lmax"], ld=True, **kw)
    zl = P.apply(c["r"], rounded=False).reshape(-1, 3)
    Z = dev["z"].reshape(-1, 3)
    fl = _floor(shape, walls)
    for q in range(3):
        ratio = float(np.max(np.abs(Z[:, q] - zl[:, q])) / np.max(np.abs(zl[:, q])))
        bar = max(Z_TOL, FLOOR_FACTOR * fl[q])
        print("mg-tiles32 model %-18s component %d: %.3e (floor %.1e, bar %.1e)" % (shape + "-" + walls, q, ratio, fl[q], bar))
        assert ratio <= bar, (q, ratio, bar)


def test_tiles32_are_deterministic():
    """Two fresh contexts give the same bits -- no atomics, a fixed thread-to-node map."""
    first = _run("partial-l1", "nfnf", "tiles")
    c = _case("partial-l1", "nfnf")
    second = _device(c, dict(c["env"], PYLAMP_MG_FUSED=None, PYLAMP_L0_MIXED=None))
    assert np.array_equal(first["z"], second["z"])
