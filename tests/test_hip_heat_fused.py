"""The heat solve's Chebyshev sweeps several per launch (k_heat_cheb_fused, one rank) against one sweep per launch
(PYLAMP_HEAT_FUSE=0): the same arithmetic per node in another kernel, so the same sweep counts and solutions equal to
8 eps max|x| ("same arithmetic, other kernel"; bitwise is the aim).

The fused kernel works on tiles of 64 x 32 nodes whose inner (64 - 2K) x (32 - 2K) nodes are written, K <= KMAX = 5 sweeps per
launch: a column band of 54 and a row chunk of 22 interior nodes at K = 5 (56 x 24 at K = 4, 58 x 26 at K = 3, 60 x 28 at K = 2,
the launches that take the 4, 3 or 2 sweeps left over)."""
import ctypes as C
import itertools

import numpy as np
import pytest

from conftest import golden, relerr

pytestmark = pytest.mark.gpu
VEL_TOL = 1e-6
KMAX, BAND, CHUNK = 5, 54, 22
EPS = np.finfo(np.float64).eps
FIXTEMP, FIXFLOW = 0, 1


def _fused_launches(ctx):
    """k_heat_cheb_fused launches on the context so far: the sign that the kernel under test ran at all"""
    n = C.c_longlong(-1)
    ctx.check(ctx.lib.pl_heat_fused_launches(ctx.handle(), C.byref(n)))
    return n.value


def _solve_both(monkeypatch, nx, args, **kw):
    """{mode: (x, stats + fused_launches, A x - rhs, rhs)} for PYLAMP_HEAT_FUSE=0 and unset, a fresh context each."""
    from pylamp_amd import pylamp_diff as D, _context
    out = {}
    for mode in ("0", None):
        if mode is None:
            monkeypatch.delenv("PYLAMP_HEAT_FUSE", raising=False)
        else:
            monkeypatch.setenv("PYLAMP_HEAT_FUSE", mode)
        _context.clear_contexts()
        A, rhs = D.makeDiffusionMatrix(nx, *args)
        x = D.solve(A, rhs, **kw)
        out[mode] = (x.copy(), dict(A.last_stats, fused_launches=_fused_launches(A._ctx)), A @ x - rhs, rhs)
        del A
    _context.clear_contexts()
    return out


def _same(out):
    (x0, s0, _, _), (x1, s1, _, _) = out["0"], out[None]
    print("iterations", s0["iterations"], s1["iterations"], "max diff", np.max(np.abs(x1 - x0)), "bound", 8 * EPS * np.max(np.abs(x0)),
          "bitwise", np.array_equal(x0, x1))
    assert s0["iterations"] == s1["iterations"], (s0, s1)
    assert s0["converged"] == s1["converged"], (s0, s1)
    # the two modes are two kernels: none of the fused launches with the knob at 0, some without it (a lone sweep has none)
    assert s0["fused_launches"] == 0 and (s1["fused_launches"] > 0 or s1["iterations"] < 2), (s0, s1)
    assert np.max(np.abs(x1 - x0)) <= 8 * EPS * np.max(np.abs(x0))


def test_fixtures_have_both_wall_kinds():
    kinds = set()
    for tag in ("a0", "b1", "c0"):
        kinds |= set(int(b) for b in golden("heat_" + tag)["bc"])
    assert kinds == {FIXTEMP, FIXFLOW}


@pytest.mark.parametrize("tag", ["a0", "b1", "c0"])
def test_fused_sweeps_on_fixtures(tag, monkeypatch):
    g = golden("heat_" + tag)
    nx = [int(v) for v in g["nx"]]
    args = ([g["gz"], g["gx"]], [g["gmz"], g["gmx"]], g["T"], [g["kz"], g["kx"]], g["Cp"], g["rho"], g["H"], list(g["bc"]),
            list(g["bcvalue"]), float(g["tstep"]))
    out = _solve_both(monkeypatch, nx, args)
    for mode in out:
        assert out[mode][1]["converged"] == 1, (mode, out[mode][1])
    _same(out)
    assert relerr(out[None][0].reshape(nx), g["sol"].reshape(nx)) < VEL_TOL


def _graded(n, L, rng):
    """n node coordinates from 0 to L, cell widths varying by a factor ~3 (graded towards one end, jittered)"""
    w = np.linspace(1.0, 3.0, n - 1) * rng.uniform(0.9, 1.1, n - 1)
    x = np.concatenate([[0.0], np.cumsum(w)])
    x *= L / x[-1]
    x[-1] = L
    return x


def _synthetic(nx, bc, seed):
    """variable k, rho, cp and heat production on a rectilinear grid graded in both axes; a time step that keeps the Gershgorin
    radius of D^-1 A_red below 0.97 (the Chebyshev branch) with a few dozen sweeps"""
    rng = np.random.default_rng(seed)
    L = [660e3, 820e3]
    grid = [_graded(nx[0], L[0], rng), _graded(nx[1], L[1], rng)]
    gridmp = []
    for gc in grid:
        m = (gc[1:] + gc[:-1]) / 2
        gridmp.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    shp = tuple(nx)
    T = 273.0 + 1350.0 * (grid[0][:, None] / L[0]) + rng.uniform(-20, 20, shp)
    kz = rng.uniform(2.0, 5.0, shp); kx = rng.uniform(2.0, 5.0, shp)
    cp = rng.uniform(1000.0, 1400.0, shp); rho = rng.uniform(2800.0, 3400.0, shp)
    H = rng.uniform(0.0, 3e-6, shp)
    hmin = min(np.min(np.diff(grid[0])), np.min(np.diff(grid[1])))
    tstep = 0.5 * hmin ** 2 * 2800.0 * 1000.0 / 5.0
    bcvalue = [(273.0 if b == FIXTEMP else 0.0) for b in bc]
    if bc[2] == FIXTEMP:
        bcvalue[2] = 1623.0
    return (grid, gridmp, T, [kz, kx], cp, rho, H, list(bc), bcvalue, tstep)


SHAPES = [
    ([5, 6], [0, 1, 0, 1]),                                        # smaller than any halo
    ([33, 41], [0, 1, 0, 1]),
    ([2 * CHUNK + 1 + 2, 2 * BAND + 1 + 2], [0, 1, 0, 1]),         # one interior node more than two chunks x two bands
    ([2 * CHUNK - 1 + 2, 2 * BAND - 1 + 2], [1, 0, 0, 1]),         # one fewer; FIXFLOW on a z-wall and an x-wall
]


@pytest.mark.parametrize("nx,bc", SHAPES)
def test_fused_sweeps_on_graded_grids(nx, bc, monkeypatch):
    out = _solve_both(monkeypatch, nx, _synthetic(nx, bc, 7))
    for mode in out:
        assert out[mode][1]["converged"] == 1, (mode, out[mode][1])
    _same(out)
    x, st, res, rhs = out[None]
    print("fused residual", np.linalg.norm(res) / np.linalg.norm(rhs), st)
    assert np.linalg.norm(res) <= 1e-9 * np.linalg.norm(rhs)


@pytest.mark.parametrize("maxit", [1, 2, 3, KMAX - 1, KMAX, KMAX + 1, KMAX + 3, 2 * KMAX + 1])
def test_sweep_counts_off_the_launch_size(maxit, monkeypatch):
    """maxit caps a round's sweeps: rounds of 1, 2, 3, K - 1, K, K + 1, K + 3 and 2 K + 1 sweeps take every combination of fused
    launches, a shorter fused launch of every length and a single sweep; not converged, and still the same iterate in both modes"""
    nx = [33, 41]
    out = _solve_both(monkeypatch, nx, _synthetic(nx, [0, 1, 0, 1], 11), maxit=maxit)
    assert out[None][1]["iterations"] == maxit, out[None][1]
    assert out[None][1]["fused_launches"] == maxit // KMAX + (1 if maxit % KMAX >= 2 else 0), out[None][1]
    _same(out)


@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("off", [1, -1])
def test_shorter_launches_at_their_own_tile_edges(K, off, monkeypatch):
    """a launch of K < KMAX sweeps writes a band of 64 - 2K columns and a chunk of 32 - 2K rows per tile: one round of K sweeps
    (maxit = K: ONE such launch) on grids with one interior node more / fewer than two chunks x two bands of that geometry"""
    band, chunk = 64 - 2 * K, 32 - 2 * K
    nx = [2 * chunk + off + 2, 2 * band + off + 2]
    out = _solve_both(monkeypatch, nx, _synthetic(nx, [0, 1, 0, 1] if off > 0 else [1, 0, 0, 1], 13 + K), maxit=K)
    assert out[None][1]["iterations"] == K and out[None][1]["fused_launches"] == 1, out[None][1]
    _same(out)


NBASE = 4           # baseline runs D is taken from


def _run12(mp, fused):
    from pylamp_amd import driver, _context
    if fused:
        mp.delenv("PYLAMP_HEAT_FUSE", raising=False)
    else:
        mp.setenv("PYLAMP_HEAT_FUSE", "0")
    _context.clear_contexts()
    nx = [65, 65]; L = [660e3, 660e3]
    tr_x, tr_f = driver.mantle_tracers(nx, L, 16, np.random.default_rng(3))
    sim = driver.Simulation(nx, L, tr_x, tr_f, driver.Options())
    reps = [sim.step() for _ in range(12)]
    out = {"ntrac": [r["ntrac"] for r in reps], "limiter": [r["limiter"] for r in reps],
           "heat_its": [r["heat"]["iterations"] for r in reps], "stokes_its": [r["stokes"]["iterations"] for r in reps],
           "fields": {n: sim.field(n) for n in ("temp", "velz", "velx", "pres")}, "tr_x": sim.tracers()[0],
           "fused_launches": _fused_launches(sim.ctx)}
    sim.close()
    _context.clear_contexts()
    return out


def _d_rule(base, b, what):
    """the protocol of profiles/step_host_refactor_equal.json: D = the largest pairwise difference among the baseline runs; the run
    under test equals one of them bit for bit where D = 0 and lies within 2 D of each otherwise"""
    D = max(float(np.max(np.abs(p - q))) for p, q in itertools.combinations(base, 2))
    d = [float(np.max(np.abs(b - p))) for p in base]
    print(what, "D", D, "diffs", d, "scale", float(np.max(np.abs(base[0]))))
    if D == 0.0:
        assert any(np.array_equal(b, p) for p in base), what
    else:
        assert max(d) <= 2 * D, (what, D, d)


def test_twelve_steps_fused_against_single_sweeps():
    """12 time steps at 65^2 nodes, 16 markers per node, PYLAMP_HEAT_FUSE unset against 0: the fused kernel inside pl_step (warm
    start, the step's coefficient planes, repeated solves on one context, no synchronisation behind the stage).  Marker counts,
    limiter and heat iteration counts equal, Stokes iterations within one per step, fields and tracer positions by the D-rule.
    The Stokes solve does not repeat itself bit for bit, and D from TWO baseline runs is too noisy an estimate of its spread (a
    third run of the SAME code lay outside 2 D in one draw of three: pressure 2.96e-20 against 2.88e-20), so D is the largest
    pairwise difference among NBASE = 4 baseline runs; the bound itself stays 2 D."""
    mp = pytest.MonkeyPatch()
    try:
        base = [_run12(mp, False) for _ in range(NBASE)]
        e = _run12(mp, True)
    finally:
        mp.undo()
    a = base[0]
    print("stokes its", a["stokes_its"], e["stokes_its"], "heat its", a["heat_its"], e["heat_its"], "fused launches", e["fused_launches"])
    assert e["fused_launches"] >= 12 and all(b["fused_launches"] == 0 for b in base)
    for k in ("ntrac", "limiter", "heat_its"):
        assert all(b[k] == e[k] for b in base), k
    assert all(abs(p - q) <= 1 for b in base for p, q in zip(b["stokes_its"], e["stokes_its"]))
    for n in a["fields"]:
        _d_rule([b["fields"][n] for b in base], e["fields"][n], n)
    _d_rule([b["tr_x"] for b in base], e["tr_x"], "tracer positions")

