"""The marker kernels the resident step launches on a RECTILINEAR grid, pinned stage by stage.

On a non-uniform grid pl_step.hip selects other kernels than the ones tests/test_hip_mic_resident.py and test_hip_scatter_split.py pin:
    tracer -> grid     k_scatter_binned<NF, false> over the cell-sorted tracers with coordinate tables (mic_axis_locate):
                       <0,false> with nf = 6 (heat on), <2,false> and <1,false> + count accumulator (heat off), <1,false> for the
                       three staggered sets and the subgrid diffusion; 8 x 32-cell tiles with an (8+2) x (32+2) LDS window, run
                       sums in registers cut at PL_RUN_MAX = 8, global atomics for contributions outside the window
    temperature        k_gather<false,0> on a ring / pitch plane, k_subgrid_part1, k_scatter_binned<1,false>, k_gather, k_subgrid_part2
    advection + sort   k_rk4<false> (search on the padded centre grid), k_cell_count with the node coordinates, full sort
Simulation.scatter_fields / temp_to_tracers / advect run exactly those stage functions.  Expected values: the oracle under
rect_search(), which tests/test_mic2_rect_model.py pins to a plain per-tracer statement of the rule.  Inputs: tests/mic2_rect_cases.py
(graded grids, per-cell populations with runs of 1, 7, 8, 9, 17 and 300 tracers, empty cells, tracers on lines and beyond the walls).

Bounds: those of test_hip_mic_resident.py -- maxrel < 1e-12 for the arithmetic fields, pointrel < ETA_TOL for the geometric
viscosities, NaN masks identical -- and, for RK4, of test_hip_parity.py::test_mic_rectilinear_vs_oracle (positions 1e-12,
velocities 1e-9).  No bound is widened.  Every case first asserts that more than half of its tracers lie in another cell than
the regular-grid formula gives: a kernel that ignored the coordinate tables could not pass.  Observed on an MI355X over all
cases: arithmetic fields <= 1.9e-15, etas / etan <= 9.3e-14, temperature <= 2.0e-16, RK4 positions 2.1e-16, velocities 1.9e-15.
The kernels add with atomics in no fixed order, so no run-to-run bit equality is asked for.
"""
import numpy as np
import pytest

import mic2_rect_cases as K
import test_hip_mic_resident as R
from conftest import maxrel, pointrel

pytestmark = pytest.mark.gpu

ETA_TOL = R.ETA_TOL
NODES = (("rho", R.TR_RH0, 5), ("etas", R.TR_ET0, 6), ("cp", R.TR_HCP, 5), ("f_T", R.TR_TMP, 5), ("H", R.TR_IHT, 5), ("mat", R.TR_MAT, 5))
_REF = {}


def _expected(oracle, nx, grid, X, F, heat=True):
    """The step's scatters by the oracle on the four graded target sets (R._targets builds the regular ones)."""
    tg = K.targets(grid)
    with oracle.rect_search():
        if not heat:
            ref = dict(zip(("rho", "etas"), oracle.trac2grid(X, F[:, [R.TR_RH0, R.TR_ET0]], tg["nodes"], nx, [5, 6])))
            ref["etan"], = oracle.trac2grid(X, F[:, [R.TR_ET0]], tg["centres"], nx, [2])      # unweighted geometric mean
            return ref
        ref = dict(zip([h[0] for h in NODES], oracle.trac2grid(X, F[:, [h[1] for h in NODES]], tg["nodes"], nx, [h[2] for h in NODES])))
        ref["etan"], = oracle.trac2grid(X, F[:, [R.TR_ET0]], tg["centres"], nx, [6])
        ref["kz"], = oracle.trac2grid(X, F[:, [R.TR_HCD]], tg["zmid"], nx, [5])
        ref["kx"], = oracle.trac2grid(X, F[:, [R.TR_HCD]], tg["xmid"], nx, [5])
    return ref


def _expected_of(oracle, name, heat=True):
    """... of a named case, computed once."""
    if (name, heat) not in _REF:
        nx, L, grid, X, F = K.case(name)
        _REF[(name, heat)] = _expected(oracle, nx, grid, X, F, heat)
    return _REF[(name, heat)]


def _within(name, a, b):
    err = pointrel(a, b) if name in ("etas", "etan") else maxrel(a, b)        # (both assert identical NaN masks)
    print("   %-5s %.3e  (%d NaN nodes)" % (name, err, int(np.isnan(b).sum())))
    return err < (ETA_TOL if name in ("etas", "etan") else 1e-12)


def _check(got, ref):
    assert set(got) == set(ref)
    bad = [k for k in got if not _within(k, got[k], ref[k])]
    assert not bad, bad


def _graded(grid, X):
    share = K.share_off_regular(grid, X)
    print("   %d tracers, %.2f of them in another cell than floor((n-1) x / L) gives" % (X.shape[0], share))
    assert share > 0.5


def _scatter(nx, L, grid, X, F, **kw):
    sim = R._sim(nx, L, X, F, grid=grid, **kw)
    try:
        return sim.scatter_fields(), sim.census()
    finally:
        sim.close()


@pytest.mark.parametrize("name", ["19x39", "11x69", "5x5"])
def test_scatter_heat_on(oracle, name):
    """k_scatter_binned<0,false> (nf = 6) on the nodes and <1,false> on the three staggered sets: all nine fields."""
    nx, L, grid, X, F = K.case(name)
    _graded(grid, X)
    ref = _expected_of(oracle, name)
    if name == "19x39":
        assert all(np.isnan(r).any() for r in ref.values())               # the empty cells reach all four target sets
    got, cen = _scatter(nx, L, grid, X, F)
    _check(got, ref)
    assert np.array_equal(cen, K.census_of(grid, X))


@pytest.mark.parametrize("name", ["19x39", "5x5"])
def test_scatter_heat_off(oracle, name):
    """<2,false> on the nodes, and <1,false> with the COUNT accumulator: the centre viscosity of the advect-only branch is the
    UNWEIGHTED geometric mean (scheme 2, pylamp2.py:316-319)."""
    nx, L, grid, X, F = K.case(name)
    _graded(grid, X)
    got, _ = _scatter(nx, L, grid, X, F, do_heatdiff=False)
    _check(got, _expected_of(oracle, name, heat=False))


def test_scatter_tracers_on_lines(oracle):
    """Tracers exactly on node lines (tile rims included), on centre lines -- the node lines of the staggered sets --, on the
    walls z = 0, x = 0 and on z = L, x = L (last cell, a = 1): the sort's search and the scatter's own search must agree on
    the cell, for every target set; the census is the search-cell count."""
    nx, L, grid, X, F = K.case("lines")
    _graded(grid, X)
    on = sum(int(np.isin(X[:, d], np.concatenate([grid[d], K.targets(grid)["centres"][d]])).sum()) for d in range(2))
    assert on >= 60
    got, cen = _scatter(nx, L, grid, X, F)
    _check(got, _expected_of(oracle, "lines"))
    assert np.array_equal(cen, K.census_of(grid, X))


def test_scatter_tracers_beyond_the_walls(oracle):
    """About 300 tracers up to 2.5 end-cell widths outside, every side and the corners: the sort clamps them into the wall
    cells, their contributions leave the LDS window (global-atomic fallback) or the grid, and the oracle extends the grid
    with the end spacing."""
    nx, L, grid, X, F = K.case("outside")
    _graded(grid, X)
    out = (X[:, 0] < 0) | (X[:, 0] > L[0]) | (X[:, 1] < 0) | (X[:, 1] > L[1])
    assert out.sum() >= 250
    got, _ = _scatter(nx, L, grid, X, F)
    _check(got, _expected_of(oracle, "outside"))


def test_first_temperature_gather(oracle):
    """first = True (it == 1, pylamp2.py:445): k_gather<false,0> reading a ring / pitch plane with global indices; a tracer on
    z = L is outside for the gather, and the step interpolates with stopOnError."""
    nx, L, grid, X, F = K.case("lines-inside")
    _graded(grid, X)
    T = 1500 + 300 * np.random.default_rng(5).standard_normal(nx)
    with oracle.rect_search():
        exp = oracle.grid2trac(X, grid, [T], nx, stop_on_error=True)[:, 0]
    sim = R._sim(nx, L, X, F, grid=grid)
    try:
        got = sim.temp_to_tracers(T, 1.0, first=True)
    finally:
        sim.close()
    err = maxrel(got, exp)
    print("   T %.3e" % err)
    assert err < 1e-12
    X1 = np.concatenate([X, [[L[0], 0.37 * L[1]]]])
    F1 = K.tracer_fields(X1, {R.TR_RH0: 1.0, R.TR_ET0: 1.0})
    with oracle.rect_search():
        with pytest.raises(Exception, match="stopOnError"):
            oracle.grid2trac(X1, grid, [T], nx, stop_on_error=True)
    sim = R._sim(nx, L, X1, F1, grid=grid)
    try:
        with pytest.raises(Exception, match="stopOnError"):
            sim.temp_to_tracers(T, 1.0, first=True)
    finally:
        sim.close()


@pytest.mark.parametrize("subgrid", [True, False])
def test_temperature_update_with_subgrid_diffusion(oracle, subgrid):
    """first = False: k_gather<false,0> of newtemp - f_T, k_subgrid_part1, k_scatter_binned<1,false> of the subgrid change,
    the second gather and k_subgrid_part2 (pylamp2.py:453-480); dx in the diffusion time scale stays L / (n - 1)
    (pylamp2.py:87), on the device as in R._subgrid_expected."""
    nx, L, grid, X, F = K.case("19x39-full")
    _graded(grid, X)
    F = F.copy()
    sim = R._sim(nx, L, X, F, grid=grid, do_subgrid_heatdiff=subgrid)
    try:
        f_T = sim.scatter_fields()["f_T"]
        assert not np.isnan(f_T).any()
        F[:, R.TR_RHO] = F[:, R.TR_RH0]                               # what the property update left on the device
        Z, Xg = np.meshgrid(*grid, indexing="ij")
        newtemp = f_T + 15 * np.sin(3 * np.pi * Xg / L[1]) * np.sin(2 * np.pi * Z / L[0])
        tstep = 0.3 * (L[0] / (nx[0] - 1)) ** 2 * 3300 * 1250 / 4.0     # a diffusive step: exp(-dt/dt0) well inside (0, 1)
        got = sim.temp_to_tracers(newtemp, tstep, first=False)
    finally:
        sim.close()
    with oracle.rect_search():
        exp = R._subgrid_expected(oracle, X, F, grid, nx, L, f_T, newtemp, tstep, subgrid)
    err = maxrel(got, exp)
    print("   T %.3e  (largest change %.1f K)" % (err, np.abs(exp - F[:, R.TR_TMP]).max()))
    assert np.abs(exp - F[:, R.TR_TMP]).max() > 1.0
    assert err < 1e-12


@pytest.mark.parametrize("fence", [False, True])
def test_rk4_and_full_sort(oracle, fence):
    """k_rk4<false> through velocities on the padded centre grid with a step of 1.5 of the smallest cell (stages near the walls
    leave the grid), then the search-based full sort: census, row identity, and a second scatter on the moved set."""
    nx, L, grid, X, F = K.case("19x39")
    _graded(grid, X)
    gp = K.padded_centres(grid)
    Vz, Vx, dt = K.velocities(grid, np.random.default_rng(6))
    with oracle.rect_search():
        v0, x0 = oracle.rk4(X, gp, [Vz, Vx], nx, dt)
    left = (x0[:, 0] <= 0) | (x0[:, 0] >= L[0]) | (x0[:, 1] <= 0) | (x0[:, 1] >= L[1])
    assert left.sum() >= 5
    if fence:
        x0, _, v0, n_removed = oracle.fence_and_delete(x0.copy(), F.copy(), v0, L, True)
        assert n_removed == 0
    sim = R._sim(nx, L, X, F, grid=grid)
    try:
        assert np.array_equal(sim.grid[0], grid[0]) and np.array_equal(sim.grid[1], grid[1])
        v, x = sim.advect(Vz, Vx, dt, fence=fence)
        ex, ev = maxrel(x, x0), maxrel(v, v0)
        print("   %d tracers beyond a wall; x %.3e v %.3e" % (left.sum(), ex, ev))
        assert ex < 1e-12 and ev < 1e-9
        assert np.array_equal(sim.census(), K.census_of(grid, x))
        X1, F1 = sim.tracers()
        assert np.array_equal(X1, x) and np.array_equal(F1, F)            # the uploaded rows, every column but the position bit-equal
        got = sim.scatter_fields()
    finally:
        sim.close()
    _check(got, _expected(oracle, nx, grid, X1, F1))
