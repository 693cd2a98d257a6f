"""pl3_stokes_precond_apply against tests/stokes3_mg_model.py, the NumPy model of the 3-D Stokes preconditioner: z = M^-1 r of the
device, component by component, against the model evaluated in longdouble with the lmax the device used -- k3_stage1 with its
symmetry chains, k3_dinv / k3_cheb0 / k3_cheb, the marching LDS kernels k3_sweep_m<0> / <1> with their rim threads, k3_resid,
k3_restrict, k3_prolong_add, k3_coarsen, k3_close, the Chebyshev recurrences and the level and sweep rules, on one rank and on blocks.

The cases (tests/test_stokes3_mg_model.py, CASES) name the smallest shape at which each path exists; grids are non-uniform in all
three axes, the viscosity spans three decades, r is standard normal on ALL entries.  Knobs are read when a context is created: one
fresh context per case.

Bars.  Plan: levels, sweeps, ratio, coarsest sweeps and LDS flags equal what the model's rules give.  lmax: lmax / 1.1 of every level
within the band of the model's converged eigenvalue that the model's own twelve-iteration estimates need, doubled
(test_stokes3_mg_model.lmax_band: 0.13 ... 0.25, the model alone stays inside the 2-D twin's 0.15).  Pressure, row by row:
|z_p - z_p,model| <= 1e-13 x sum |terms|, no lmax involved.  Every component: |z - z_ld|_inf <= max(1e-11, 50 x floor) |z_ld|_inf --
1e-11 is the bar of the 2-D twin, floor the model's own rounding (float64 against longdouble, per case), 50 the allowance for the
kernels' summation order and FMA contraction.  Every test prints the ratios it saw; the largest per check is printed when the module
is done (DESIGN.md section 6c quotes them).

Not covered.  The switches PYLAMP_3D_LDS and PYLAMP_3D_BAND are function-static and cannot be flipped inside one process: the model,
not a per-node twin, is the reference for the LDS kernels.  A coarse level on the LDS kernels needs >= 1.6 M nodes on level 0; the
`lds` cases with natural rows run the marching kernels on the operator that coarse levels use.  The deflation correction and the
Krylov loop are untouched (the entry point applies the preconditioner without the deflation correction)."""
import os

import numpy as np
import pytest

import stokes3_mg_model as G
from test_stokes3_mg_model import CASES, build_case, converged_lambdas, lmax_band, model, model_knobs, rounding_floor

pytestmark = pytest.mark.gpu

Z_TOL = 1e-11
FLOOR_FACTOR = 50.0
P_ROW_TOL = 1e-13
LMAX_SAFETY = 1.1
COMP = ["vz", "vx", "vy", "P"]

_margins = {}


def _note(check, what, value):
    print("mg3-model %-10s %-44s %.3e" % (check, what, value))
    _margins[check] = max(_margins.get(check, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for check in sorted(_margins):
        print("\nlargest ratio %-10s %.3e" % (check, _margins[check]), end="")
    print()
    _margins.clear()


class _environment:
    def __init__(self, env):
        self.env = dict(env)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        return False


def _operator(P3, c, ctx):
    A, _ = P3.makeStokesMatrix(c["n"], c["grid"], c["etas"], c["etan"], c["rho"], bc=c["bc"], ctx=ctx, strict_reference=c["strict"])
    return A


def _applied(A, r):
    z = A.precond(r)
    nl, lm = A.mg_info()
    return dict(z=z, nlevels=nl, lmax=lm, plan=A.mg_plan())


def _device_apply(c, extra=None):
    """z = M^-1 r on a fresh context (fresh contexts of a block layout) under the case's environment, and what that application
    used; one entry per rank."""
    from pylamp_amd import pylamp3d as P3
    with _environment(c["env"]):
        if c["P"] == (1, 1, 1):
            ctx = P3.Context3(c["n"], c["grid"])
            try:
                A = _operator(P3, c, ctx)
                out = _applied(A, c["r"])
                if extra:
                    extra(P3, A, out)
                return [out]
            finally:
                ctx.close()
        vc = P3.VirtualCluster3(c["n"], c["grid"], *c["P"])
        try:
            return vc.all(lambda ctx, rank: _applied(_operator(P3, c, ctx), c["r"]), timeout=300)
        finally:
            vc.close()


def _check_plan(c, dev):
    """The device chose what the model's rules choose from the grid and the knobs."""
    kw = model_knobs(c)
    plan = dev["plan"]
    assert dev["nlevels"] == c["nlevels"] == len(G.level_grids(c["grid"], c["P"])), (dev["nlevels"], c["nlevels"])
    assert (plan["nu_fine"], plan["nu"]) == tuple(kw["nu"]), (plan, kw)
    assert plan["ratio"] == kw["ratio"], (plan, kw)
    coarsest = [g.size for g in G.level_grids(c["grid"], c["P"])[-1]]
    n, ratio = G.coarsest_sweeps(coarsest, kw["coarse_sweeps"])
    assert plan["coarse_sweeps"] == n and plan["coarse_ratio"] == pytest.approx(ratio, rel=1e-14), (plan, n, ratio)
    assert plan["lds"] == G.lds_levels(c["grid"], c["P"]), (plan, G.lds_levels(c["grid"], c["P"]))


def _check_lmax(c, dev):
    conv, band = converged_lambdas(c), lmax_band(c)
    for l, (lm, cv) in enumerate(zip(dev["lmax"], conv)):
        ratio = lm / LMAX_SAFETY / cv
        _note("lmax", "%s level %d (band %.3f)" % (c["id"], l, band), abs(ratio - 1.0))
        assert 1 - band <= ratio <= 1 + band, (l, lm, cv, band)


def _check_pressure(c, P, z, what=""):
    """z_p row by row: closed form, no lmax."""
    n = c["n"]
    zp, mag = P.pressure(c["r"], terms=True)
    got = z.reshape(n + [4])[..., 3]
    err = np.abs(got - zp).astype(np.float64); bar = (P_ROW_TOL * mag).astype(np.float64)
    assert np.all(bar[:n[0] - 1, :n[1] - 1, :n[2] - 1] > 0)
    worst = float(np.max(err[bar > 0] / bar[bar > 0]))
    _note("pressure", c["id"] + what, worst * P_ROW_TOL)
    assert np.all(err <= bar), (worst, np.argwhere(err > bar)[:5])


def _check_z(c, P, z, what=""):
    fl = rounding_floor(c["id"])
    zl = P.apply(c["r"], rounded=False).reshape(-1, 4)
    Z = z.reshape(-1, 4)
    bad = []
    for q in range(4):
        d = np.abs(Z[:, q] - zl[:, q])
        ratio = float(d.max() / np.max(np.abs(zl[:, q])))
        bar = max(Z_TOL, FLOOR_FACTOR * fl[q])
        _note("z", "%s%s %s (floor %.1e)" % (c["id"], what, COMP[q], fl[q]), ratio)
        if not ratio <= bar:
            bad.append((COMP[q], ratio, bar, tuple(int(v) for v in np.unravel_index(int(np.argmax(d)), c["n"]))))
    assert not bad, "component, ratio, bar, node (i, j, k) of the largest error: %s" % bad


def _check_against_model(c, dev, what=""):
    P = model(c, dev["lmax"], True)
    _check_pressure(c, P, dev["z"], what)
    _check_z(c, P, dev["z"], what)


ONE_RANK = [cid for cid in sorted(CASES) if CASES[cid]["P"] == (1, 1, 1)]
BLOCKED = [cid for cid in sorted(CASES) if CASES[cid]["P"] != (1, 1, 1)]


@pytest.mark.parametrize("cid", ONE_RANK)
def test_preconditioner_matches_the_model(cid):
    c = build_case(cid)
    dev = _device_apply(c)[0]
    _check_plan(c, dev)
    _check_lmax(c, dev)
    _check_against_model(c, dev)


@pytest.mark.parametrize("cid", BLOCKED)
def test_preconditioner_on_blocks_matches_the_model(cid):
    """[17, 17, 17] on 2 x 2 x 2 blocks (the three levels of one rank) and on 4 x 1 x 1 (two: the model gets the layout): the halo
    exchanges inside the V-cycle.  Every rank's z is compared; the ranks hold the same hierarchy, and on 2 x 2 x 2 two fresh
    clusters agree bitwise."""
    c = build_case(cid)
    devs = _device_apply(c)
    assert len(devs) == int(np.prod(c["P"]))
    for rank, dev in enumerate(devs):
        assert dev["lmax"] == devs[0]["lmax"] and dev["plan"] == devs[0]["plan"] and dev["nlevels"] == devs[0]["nlevels"]
        _check_plan(c, dev)
        if rank == 0:
            _check_lmax(c, dev)
            _check_against_model(c, dev)
        else:
            assert np.array_equal(dev["z"], devs[0]["z"]), "rank %d holds another z than rank 0" % rank
    if c["P"] == (2, 2, 2):
        again = _device_apply(c)
        for rank, dev in enumerate(again):
            assert dev["lmax"] == devs[0]["lmax"] and np.array_equal(dev["z"], devs[0]["z"]), "second cluster, rank %d" % rank


def test_two_fresh_contexts_agree_bitwise():
    """The marching LDS kernels, their rim and the reductions of the power iteration are deterministic."""
    c = build_case("lds-mixed-slaved")
    a, b = _device_apply(c)[0], _device_apply(c)[0]
    assert a["lmax"] == b["lmax"]
    assert np.array_equal(a["z"], b["z"])


@pytest.mark.parametrize("cid", ["aniso-mixed-slaved", "three-level-free-natural"])
def test_later_applications_match_the_model_with_their_own_lmax(cid):
    """A second application on the same context (warm power iteration: another lmax) and one after a solve each match the model with
    the lmax that application reports; the pressure component does not depend on lmax and is bit for bit the same."""
    c = build_case(cid)
    later = []

    def more(P3, A, out):
        later.append(("second", _applied(A, c["r"])))
        P3.solve(A)
        assert A.last_stats["converged"] == 1
        later.append(("after-solve", _applied(A, c["r"])))
    dev = _device_apply(c, more)[0]
    _check_plan(c, dev)
    _check_against_model(c, dev)
    zp = dev["z"].reshape(-1, 4)[:, 3]
    for what, d in later:
        _check_plan(c, d)
        assert np.array_equal(d["z"].reshape(-1, 4)[:, 3], zp), what
        conv = converged_lambdas(c)
        for l, lm in enumerate(d["lmax"]):          # a warm estimate has iterated further: it stays in the band of the cold one
            assert abs(lm / LMAX_SAFETY / conv[l] - 1.0) <= lmax_band(c), (what, l, lm, conv[l])
        _check_against_model(c, d, " " + what)
