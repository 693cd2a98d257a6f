"""The fused scatter with the target sets of a strip divided over the waves of a workgroup (pl_mic_cells.hip: sc_split_sets).

    k_scatter_cells<6,1,true,IND,SPLIT>   heat step: nodes | centres | z-mid + x-mid faces, three waves per strip
    k_scatter_cells<2,2,false,false,3>    heat off:  nodes | centres, two waves
    k_scatter_cells<1,0,false,false,0>    subgrid diffusion: one set, one wave (the same source with another table)

Every case goes through Simulation.scatter_fields() and checks, with the bounds of test_hip_mic_resident.py,
  * the oracle's trac2grid on the four staggered target grids (maxrel < 1e-12; etas / etan pointrel < ETA_TOL; NaN masks identical),
  * PYLAMP_SC_SPLIT unset against PYLAMP_SC_SPLIT=0 (one wave, all sets): the same bits in all fields,
  * two consecutive calls: the same bits,
  * PYLAMP_SCATTER=0, the independent one-set-per-pass kernels, within the same bounds.
Shapes: the smallest that reach every path of the work division (see the cases).
"""
import os

import numpy as np
import pytest

import test_hip_mic_resident as R
from conftest import golden, maxrel, pointrel

pytestmark = pytest.mark.gpu

ETA_TOL = R.ETA_TOL
HEAT = (("rho", R.TR_RH0, 5), ("etas", R.TR_ET0, 6), ("cp", R.TR_HCP, 5), ("f_T", R.TR_TMP, 5), ("H", R.TR_IHT, 5), ("mat", R.TR_MAT, 5))


def _cells(nx, L, counts, rng):
    """counts[i, j] tracers, uniform strictly inside cell (i, j)."""
    ci, cj = np.nonzero(counts)
    rep = counts[ci, cj]
    i = np.repeat(ci, rep); j = np.repeat(cj, rep)
    h = [L[0] / (nx[0] - 1), L[1] / (nx[1] - 1)]
    X = np.stack([(i + rng.uniform(0.01, 0.99, i.size)) * h[0], (j + rng.uniform(0.01, 0.99, j.size)) * h[1]], axis=1)
    return X[rng.permutation(X.shape[0])]


def _columns(X, L, rng):
    n = X.shape[0]
    return {R.TR_RH0: rng.uniform(3200, 3400, n), R.TR_ET0: 10 ** rng.uniform(19, 22, n), R.TR_HCP: rng.uniform(1000, 1300, n),
            R.TR_HCD: rng.uniform(2, 5, n), R.TR_TMP: 273 + 1350 * X[:, 0] / L[0] + rng.uniform(-30, 30, n),
            R.TR_IHT: 1e-11 * rng.uniform(0.5, 2, n), R.TR_MAT: np.round(rng.uniform(0, 3, n))}


def _expected(oracle, nx, L, X, F, heat=True):
    tg = R._targets(oracle, nx, L)
    if not heat:
        ref = dict(zip(("rho", "etas"), oracle.trac2grid(X, F[:, [R.TR_RH0, R.TR_ET0]], tg["nodes"], nx, [5, 6])))
        ref["etan"], = oracle.trac2grid(X, F[:, [R.TR_ET0]], tg["centres"], nx, [2])       # unweighted geometric mean
        return ref
    ref = dict(zip([h[0] for h in HEAT], oracle.trac2grid(X, F[:, [h[1] for h in HEAT]], tg["nodes"], nx, [h[2] for h in HEAT])))
    ref["etan"], = oracle.trac2grid(X, F[:, [R.TR_ET0]], tg["centres"], nx, [6])
    ref["kz"], = oracle.trac2grid(X, F[:, [R.TR_HCD]], tg["zmid"], nx, [5])
    ref["kx"], = oracle.trac2grid(X, F[:, [R.TR_HCD]], tg["xmid"], nx, [5])
    return ref


def _with_env(name, value, fn):
    os.environ[name] = value
    try:
        return fn()
    finally:
        del os.environ[name]


def _within(name, a, b):
    err = pointrel(a, b) if name in ("etas", "etan") else maxrel(a, b)
    print("   %-5s %.3e" % (name, err))
    return err < (ETA_TOL if name in ("etas", "etan") else 1e-12)


def _ndiff(a, b):
    return int(np.sum(~((a == b) | (np.isnan(a) & np.isnan(b)))))


def _scatter_all(sim):
    """(split, split again, one wave, one-set-per-pass kernels)"""
    assert "PYLAMP_SC_SPLIT" not in os.environ and "PYLAMP_SCATTER" not in os.environ
    got = sim.scatter_fields(); again = sim.scatter_fields()
    one = _with_env("PYLAMP_SC_SPLIT", "0", sim.scatter_fields)
    return got, again, one


def _check(got, again, one, old, ref):
    assert set(got) == set(ref)
    for k in got:
        assert _within(k, got[k], ref[k]), "oracle: " + k
        assert _within(k, got[k], old[k]), "one-set-per-pass kernels: " + k
    for k in got:
        print("   %-5s split/one wave differ at %d nodes, run to run at %d" % (k, _ndiff(got[k], one[k]), _ndiff(got[k], again[k])))
    for k in got:
        assert np.array_equal(got[k], one[k], equal_nan=True), "split != one wave: " + k
        assert np.array_equal(got[k], again[k], equal_nan=True), "run to run: " + k


def _case(oracle, nx, L, X, cols, heat=True):
    F = R._tracers(X, cols)
    sim = R._sim(nx, L, X, F, **({} if heat else {"do_heatdiff": False}))
    try:
        got, again, one = _scatter_all(sim)
        old = _with_env("PYLAMP_SCATTER", "0", sim.scatter_fields)
    finally:
        sim.close()
    _check(got, again, one, old, _expected(oracle, nx, L, X, F, heat))
    return got


NX35, L35 = [35, 31], [680e3, 600e3]


@pytest.fixture(scope="module")
def strips():
    """34 x 30 cells: row strips of 32 and 2 rows, column strips of 14, 14 and 2 columns -- first, middle and last strips both ways,
    the ring row and column, the closing column, rows owned by one strip and visited by two; ~16 tracers per cell, ~5 % of the
    cells empty."""
    rng = np.random.default_rng(3531)
    counts = np.where(rng.random((34, 30)) < 0.05, 0, rng.integers(14, 19, (34, 30)))
    X = _cells(NX35, L35, counts, rng)
    cols = _columns(X, L35, rng)
    X.setflags(write=False)
    return X, cols


def test_strip_geometry(oracle, strips):
    X, cols = strips
    got = _case(oracle, NX35, L35, X, cols)
    assert all(np.isfinite(v).sum() > 0.9 * v.size for v in got.values())


def test_multi_window_rows(oracle):
    """5 x 30 cells: a row at 26 per cell (364 per strip row > SC_CAP = 320), one at 50 per cell (three windows), one cell with
    400 tracers of its own (a cell that spans windows), 8 per cell elsewhere: the barriers inside the window loop."""
    nx, L = [6, 31], [100e3, 600e3]
    rng = np.random.default_rng(631)
    counts = np.full((5, 30), 8)
    counts[1, :] = 26; counts[2, :] = 50; counts[3, 17] = 400
    X = _cells(nx, L, counts, rng)
    _case(oracle, nx, L, X, _columns(X, L, rng))


def test_one_partial_strip(oracle):
    """One strip that is partial both ways, every cell populated: 4 x 4 cells (pl_create takes no grid below 5 x 5 nodes)."""
    nx, L = [5, 5], [80e3, 80e3]
    rng = np.random.default_rng(45)
    X = _cells(nx, L, np.full((4, 4), 16), rng)
    _case(oracle, nx, L, X, _columns(X, L, rng))


def test_misplaced_outside_fixture(oracle):
    """Markers beyond the walls leave their sort cell: exactly one wave lists each, and k_scatter_cells_listed adds all sets of the
    349 listed markers (of 900) in a fixed order -- the same bits from call to call and from either work division."""
    g = golden("trac2grid")
    nx = [int(v) for v in g["nx"]]; L = [float(v) for v in g["L"]]
    X = g["outside_tr_x"]
    _case(oracle, nx, L, X, _columns(X, L, np.random.default_rng(1114)))


def test_misplaced_beyond_the_ordered_kernel(oracle):
    """More listed markers than k_scatter_cells_listed takes (SC_SLOW_DET = 2048): k_scatter_cells_slow adds them with atomics in
    no fixed order, so this case checks values only -- the oracle and the one-set-per-pass kernels, with the usual bounds."""
    g = golden("trac2grid")
    nx = [int(v) for v in g["nx"]]; L = [float(v) for v in g["L"]]
    rng = np.random.default_rng(2049)
    inside = _cells(nx, L, np.full((nx[0] - 1, nx[1] - 1), 12), rng)
    beyond = np.stack([rng.uniform(-0.3, 1.3, 6000) * L[0], rng.uniform(-0.3, 1.3, 6000) * L[1]], axis=1)
    beyond = beyond[(beyond[:, 0] < 0) | (beyond[:, 0] > L[0]) | (beyond[:, 1] < 0) | (beyond[:, 1] > L[1])]
    assert beyond.shape[0] > 2048 + 200
    X = np.concatenate([inside, beyond])
    F = R._tracers(X, _columns(X, L, rng))
    sim = R._sim(nx, L, X, F)
    try:
        got = sim.scatter_fields()
        old = _with_env("PYLAMP_SCATTER", "0", sim.scatter_fields)
    finally:
        sim.close()
    ref = _expected(oracle, nx, L, X, F)
    for k in got:
        assert _within(k, got[k], ref[k]), "oracle: " + k
        assert _within(k, got[k], old[k]), "one-set-per-pass kernels: " + k


def test_misplaced_on_cell_boundaries(oracle, strips):
    """Tracers exactly on node lines of the 35 x 31 grid, strip rims included: a tracer listed twice or by no wave shows up
    against the oracle."""
    X0, cols0 = strips
    gz = np.linspace(0, L35[0], NX35[0]); gx = np.linspace(0, L35[1], NX35[1])
    hz, hx = gz[1], gx[1]
    extra = np.array([[gz[5], 3.3 * hx], [gz[32], 14.5 * hx], [7.2 * hz, gx[14]], [31.5 * hz, gx[28]], [gz[32], gx[14]], [gz[1], gx[1]],
                      [gz[33], gx[29]], [0.0, 9.4 * hx], [12.6 * hz, 0.0], [gz[16], gx[15]]])
    X = np.concatenate([X0, extra])
    rng = np.random.default_rng(9)
    ecols = _columns(extra, L35, rng)
    _case(oracle, NX35, L35, X, {k: np.concatenate([cols0[k], ecols[k]]) for k in cols0})


def test_epoch_layout(oracle, strips):
    """k_scatter_cells<6,1,true,true,*>: after a sort that is not followed by a download the constant columns are read through the
    slot index; the indices travel one row ahead through LDS, staged by the whole workgroup."""
    X, cols = strips
    nx, L = NX35, L35
    sim = R._sim(nx, L, X, R._tracers(X, cols))
    try:
        h = [L[0] / (nx[0] - 1), L[1] / (nx[1] - 1)]
        gz = np.concatenate([[-0.5 * h[0]], 0.5 * (sim.grid[0][1:] + sim.grid[0][:-1]), [L[0] + 0.5 * h[0]]])
        gx = np.concatenate([[-0.5 * h[1]], 0.5 * (sim.grid[1][1:] + sim.grid[1][:-1]), [L[1] + 0.5 * h[1]]])
        Zp, Xp = np.meshgrid(gz, gx, indexing="ij")
        Vz = 1e-9 * np.sin(np.pi * Zp / L[0]) * np.cos(3 * np.pi * Xp / L[1]); Vx = -1e-9 / 3 * np.cos(np.pi * Zp / L[0]) * np.sin(3 * np.pi * Xp / L[1])
        sim.advect(Vz, Vx, 0.6 * h[0] / 1e-9, fence=True, download=False)
        assert sim.layout()[0] == 1
        got, again, one = _scatter_all(sim)
        assert sim.layout()[0] == 1
        old = _with_env("PYLAMP_SCATTER", "0", sim.scatter_fields)
        X1, F1 = sim.tracers()
    finally:
        sim.close()
    _check(got, again, one, old, _expected(oracle, nx, L, X1, F1))


def test_heat_off_two_waves(oracle, strips):
    """k_scatter_cells<2,2,false,false,3>: nodes | centres; etan is the UNWEIGHTED geometric mean (scheme 2)."""
    X, cols = strips
    _case(oracle, NX35, L35, X, cols, heat=False)


def test_subgrid_scatter_one_wave(oracle, strips):
    """k_scatter_cells<1,0,false,false,0> between the two gathers of the subgrid diffusion: the shared source still serves the
    one-wave instantiation."""
    X, cols = strips
    nx, L = NX35, L35
    # (every node needs a value for the gather back: fill the empty cells of the shared set)
    rng = np.random.default_rng(77)
    Xf = np.concatenate([X, _cells(nx, L, np.full((34, 30), 1), rng)])
    cf = _columns(Xf, L, rng)
    F = R._tracers(Xf, cf)
    sim = R._sim(nx, L, Xf, F, do_subgrid_heatdiff=True)
    try:
        fields = sim.scatter_fields()
        F[:, R.TR_RHO] = F[:, R.TR_RH0]
        grid = [np.linspace(0, L[0], nx[0]), np.linspace(0, L[1], nx[1])]
        Z, Xg = np.meshgrid(*grid, indexing="ij")
        newtemp = fields["f_T"] + 15 * np.sin(3 * np.pi * Xg / L[1]) * np.sin(2 * np.pi * Z / L[0])
        tstep = 0.3 * (L[0] / (nx[0] - 1)) ** 2 * 3300 * 1250 / 4.0
        got = sim.temp_to_tracers(newtemp, tstep, first=False)
    finally:
        sim.close()
    exp = R._subgrid_expected(oracle, Xf, F, grid, nx, L, fields["f_T"], newtemp, tstep, True)
    err = maxrel(got, exp)
    print("   subgrid %.3e" % err)
    assert err < 1e-11
