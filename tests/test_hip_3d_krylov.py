"""The 3-D Stokes Krylov loop, its deflation and its error estimate against tests/stokes3_krylov_model.py:
what lies in pl_3d.hip between the preconditioner and the numbers a solve hands back, kernel by kernel and then as a loop.

a. k3_dots / k3_dots_own / k3_dots11 with r3_block (pl_reduce3.h) and sum_partials3, k3_axpby, k3_p_update, k3_xr_update, k3_xrp_update and
   k3_random, one launch each through pl3_krylov_probe.  Sums against longdouble sums: |got - want| <= 5 (trips + 10 + 1024) eps
   sum |terms|, trips = ceil(n / (1024 x 256)) -- the longest accumulation chain (per-thread trips, six shuffle steps, four wave sums,
   1024 partials on the host), the 5 of the 2-D twin's SUM_TOL.  Updates element by element: 4 eps sum |terms of the element|.
b. the hydrostatic start and its reference norm (k3_hydro / k3_hydro_add / k3_shift, hydrostatic_start3), on one rank and on blocks.
c. the first three iterations of pl3_stokes_solve, fused and unfused, against the model's recurrence with the device's lmax and w.
d. the deflation: k3_defl_setup, the vector w, the correction at the end of stokes_M3 and the reuse rule of deflation_setup3.
e. the reported error estimate: the formula, and its honesty against a direct solution.
f. the ring and padding entries of the 14 work vectors stay exactly zero (after every solve of c and e, and on an LDS-sized grid);
   on blocks, where the rings hold the neighbours' values, the ring sum is the sum of those planes (the positive control).
g. the estimate between the true-residual checks, fused and unfused, with its parts, late in the iteration.

Bars of c - e: max(1e-11, 50 x floor) as tests/test_hip_3d_mg_model.py, floor the model's float64 result against its longdouble one.
Every test prints the ratios it saw; the largest per check is printed when the module is done (DESIGN.md section 6c quotes them).
One fresh context per case: ctx->etol is sticky and the knobs are read per solve."""
import os

import numpy as np
import pytest

import stokes3_flow_model as F
import stokes3_krylov_model as K
import stokes3_mg_model as G
from test_stokes3_krylov_model import RHO_MODEL, build_case, direct_solution, graded, system, velocity_error
from test_stokes3_mg_model import WALLS, fields

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
SUM_FACTOR, UPDATE_TOL = 5.0, 4.0
BLOCKS, THREADS = 1024, 256
Z_TOL, FLOOR_FACTOR = 1e-11, 50.0
COMP = ["vz", "vx", "vy", "P"]
_margins = {}


def _note(check, what, value):
    print("krylov3 %-12s %-52s %.3e" % (check, what, value))
    _margins[check] = max(_margins.get(check, 0.0), float(value))


@pytest.fixture(scope="module", autouse=True)
def _module_state():
    yield
    for check in sorted(_margins):
        print("\nlargest ratio %-12s %.3e" % (check, _margins[check]), end="")
    print()
    _margins.clear()


class _environment:
    def __init__(self, env):
        self.env = dict(env)

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in self.env}
        for k, v in self.env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


# ---------------------------------------------------------------------------------------------------------------------
# a. reduction and update kernels
# ---------------------------------------------------------------------------------------------------------------------
def vol(n, P=(1, 1, 1)):
    """Elements per array of the largest block: y stride = (16 + ny + 1) rounded up to 16, times (nx + 2)(nz + 2)."""
    b = [(n[a] - 1) // P[a] + 1 for a in range(3)]
    return (b[0] + 2) * (b[1] + 2) * (((16 + b[2] + 1 + 15) // 16) * 16)


def _second_trip_cube():
    n = 8
    while 4 * vol([n, n, n]) <= BLOCKS * THREADS:
        n += 1
    return [n, n, n]


CUBE = _second_trip_cube()                  # the smallest cube on which only some threads take a second trip
assert BLOCKS * THREADS < 4 * vol(CUBE) < 2 * BLOCKS * THREADS and CUBE == [32, 32, 32]
LINE = [6, 6, 517]                          # on 1 x 1 x 2 blocks: 258 and 259 nodes along y, the second kk trip of k3_dots_own
SHAPES = {"tiny": [6, 7, 9], "cube": CUBE, "line": LINE}
assert 4 * vol(SHAPES["tiny"]) < BLOCKS * THREADS / 2          # most of the 1024 workgroups get no element


def sum_tol(n):
    trips = -(-4 * vol(n) // (BLOCKS * THREADS))
    return SUM_FACTOR * (trips + 10 + BLOCKS) * EPS


def _ldot(a, b):
    """(sum a b, sum |a b|) in longdouble."""
    p = np.asarray(a, dtype=LD) * np.asarray(b, dtype=LD)
    return np.sum(p), np.sum(np.abs(p))


_operands = {}


def operands(shape, kind):
    """Ten vectors (nz, nx, ny, 4).  spread: mixed sign, magnitudes over six decades.  cancel: s is then shifted along t and rt so that
    t.s and rt.s are about 1e-6 of sum |terms|."""
    if (shape, kind) not in _operands:
        n = SHAPES[shape]
        rng = np.random.default_rng([5, int(kind == "cancel")] + n)
        v = {k: rng.standard_normal(n + [4]) * 10.0 ** rng.uniform(-3, 3, n + [4]) for k in ("t", "s", "rt", "x", "dx", "y", "z", "r", "p", "v")}
        if kind == "cancel":
            t, s, rt = [np.asarray(v[k], dtype=LD) for k in ("t", "s", "rt")]
            target = 1e-6 * np.array([np.sum(np.abs(t * s)), np.sum(np.abs(rt * s))], dtype=np.float64)
            m = np.array([[np.sum(t * t), np.sum(t * rt)], [np.sum(rt * t), np.sum(rt * rt)]], dtype=np.float64)
            c = np.linalg.solve(m, np.array([np.sum(t * s), np.sum(rt * s)], dtype=np.float64) - target)
            v["s"] = (s - LD(c[0]) * t - LD(c[1]) * rt).astype(np.float64)
            for a in ("t", "rt"):
                d, mag = _ldot(v[a], v["s"])
                assert 1e-8 * mag < abs(d) < 1e-4 * mag, (a, float(d), float(mag))
        v["yw"] = rng.uniform(0.5, 2.0, n) * 10.0 ** rng.uniform(-2, 2, n)
        for a in v.values():
            a.setflags(write=False)
        _operands[shape, kind] = v
    return _operands[shape, kind]


def _probe_operator(P3, n, ctx):
    one = np.ones(n)
    A, _ = P3.makeStokesMatrix(n, [np.linspace(0, 1, v) for v in n], one, one, one, ctx=ctx)
    return A


class _one_rank:
    def __init__(self, n):
        from pylamp_amd import pylamp3d as P3
        self.P3 = P3
        self.ctx = P3.Context3(n, [np.linspace(0, 1, v) for v in n])
        self.n = n

    def __enter__(self):
        return self.P3, _probe_operator(self.P3, self.n, self.ctx)

    def __exit__(self, *exc):
        self.ctx.close()
        return False


def _check_sums(what, n, got, pairs):
    tol = sum_tol(n)
    for q, (a, b) in enumerate(pairs):
        want, mag = _ldot(a, b)
        err = abs(LD(got[q]) - want)
        _note("sum", "%s [%d]" % (what, q), float(err / mag) / tol if mag > 0 else 0.0)
        assert err <= tol * mag, (what, q, float(got[q]), float(want), float(err / mag) if mag > 0 else err, tol)


def _dot_pairs(v, nd):
    a = [v["t"], v["t"], v["rt"], v["rt"], v["s"]][:nd]
    b = [v["s"], v["t"], v["s"], v["t"], v["s"]][:nd]
    return a, b


@pytest.mark.parametrize("kind", ["spread", "cancel"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dots_match_longdouble_sums(shape, kind):
    """k3_dots with 1 ... 5 products, r3_block and sum_partials3."""
    n, v = SHAPES[shape], operands(shape, kind)
    with _one_rank(n) as (P3, A):
        for nd in range(1, 6):
            a, b = _dot_pairs(v, nd)
            sums, _ = A.krylov_probe(P3.PROBE_DOTS, a + [None] * (5 - nd) + b, scalars=[nd])
            assert np.all(np.isnan(sums[nd:]))
            _check_sums("%s %s dots nd=%d" % (shape, kind, nd), n, sums, list(zip(a, b)))
        assert A.ring_sum() == 0.0


@pytest.mark.parametrize("kind", ["spread", "cancel"])
def test_dots_on_blocks_count_every_node_once(kind):
    """[6, 6, 517] on 1 x 1 x 2 virtual ranks: blocks of 258 and 259 nodes along y, so k3_dots_own takes its second kk trip; the rings
    hold the neighbour's values and must not be counted.  Same bound as one rank, and the two agree within it."""
    from pylamp_amd import pylamp3d as P3
    n, v = LINE, operands("line", kind)
    a, b = _dot_pairs(v, 5)
    grid = [np.linspace(0, 1, k) for k in n]
    vc = P3.VirtualCluster3(n, grid, 1, 1, 2)
    try:
        def run(ctx, rank):
            first, count = (C_int3(), C_int3())
            ctx.check(ctx.lib.pl3_local_block(ctx.handle(), first, count))
            A = _probe_operator(P3, n, ctx)
            return list(count), A.krylov_probe(P3.PROBE_DOTS, a + b, scalars=[5])[0]
        out = vc.all(run, timeout=300)
    finally:
        vc.close()
    assert sorted(c[2] for c, _ in out) == [258, 259]
    with _one_rank(n) as (P3, A):
        one = A.krylov_probe(P3.PROBE_DOTS, a + b, scalars=[5])[0]
    for rank, (_, sums) in enumerate(out):
        assert np.array_equal(sums[:5], out[0][1][:5]), "rank %d holds other sums than rank 0" % rank
    _check_sums("line %s blocks" % kind, n, out[0][1], list(zip(a, b)))
    _check_sums("line %s one rank" % kind, n, one, list(zip(a, b)))
    for q in range(5):
        assert abs(out[0][1][q] - one[q]) <= sum_tol(n) * float(_ldot(a[q], b[q])[1])          # (the same bound, between the two)


def C_int3():
    import ctypes
    return (ctypes.c_int * 3)()


def _want11(v, x, dx, yw):
    """The 11 sums as (a, b) pairs of arrays."""
    t, s, rt = v["t"], v["s"], v["rt"]
    zero = np.zeros(1)
    pairs = [(t, s), (t, t), (rt, s), (rt, t), (s, s), (t[..., 3], s[..., 3]), (t[..., 3], t[..., 3]), (s[..., 3], s[..., 3])]
    if x is None:
        pairs.append((zero, zero))
    else:
        X = x[..., :3] if (dx is None or dx is x) else x[..., :3] + dx[..., :3]        # (float64, as the kernel forms x + dx)
        pairs.append((X, X))
    pairs += [(zero, zero), (zero, zero)] if yw is None else [(yw, s[..., 3]), (yw, t[..., 3])]
    return pairs


@pytest.mark.parametrize("kind", ["spread", "cancel"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_dots11_matches_longdouble_sums(shape, kind):
    """k3_dots11 + sum_partials3 with every combination of x / dx / yw present or NULL, and dx the vector x itself."""
    n, v = SHAPES[shape], operands(shape, kind)
    with _one_rank(n) as (P3, A):
        for x in (None, v["x"]):
            for dx in (None, "alias", v["dx"]):
                for yw in (None, v["yw"]):
                    d = x if isinstance(dx, str) else dx
                    sums, _ = A.krylov_probe(P3.PROBE_DOTS11, [v["t"], v["s"], v["rt"], x, d], yw=yw)
                    what = "%s %s dots11 x=%d dx=%s yw=%d" % (shape, kind, x is not None, "alias" if d is x and d is not None else d is not None, yw is not None)
                    _check_sums(what, n, sums, _want11(v, x, d, yw))
                    if x is None:
                        assert sums[8] == 0.0
                    if yw is None:
                        assert sums[9] == 0.0 and sums[10] == 0.0
        assert A.ring_sum() == 0.0


def test_dots11_partition():
    """Values planted in one array at a time: sums 5 - 7 and 9 - 10 see the pressure array only, sum 8 the velocity arrays only -- a
    partition that is off by a whole array fails here.  Then one value in the first and in the last OWNED node of each array, (0, 0, 0)
    and (nz - 1, nx - 1, ny - 1): the ends of what an upload can reach.  The raw entries 0 and vol - 1 of a device array are ring and
    padding entries, which no upload writes and which stay zero (the ring test below); a partition that is off by ONE ENTRY
    (`e >= np` against `e > np`) moves only such an entry and cannot be seen through the probe."""
    n = SHAPES["tiny"]
    rng = np.random.default_rng(21)
    yw = rng.uniform(0.5, 2.0, n)
    first, last = (0, 0, 0), (n[0] - 1, n[1] - 1, n[2] - 1)
    with _one_rank(n) as (P3, A):
        for c in range(4):
            for where in ("all", first, last):
                t, s, rt, x = [np.zeros(n + [4]) for _ in range(4)]
                for a in (t, s, rt, x):
                    if where == "all":
                        a[..., c] = rng.uniform(0.5, 2.0, n)
                    else:
                        a[where + (c,)] = rng.uniform(0.5, 2.0)
                sums, _ = A.krylov_probe(P3.PROBE_DOTS11, [t, s, rt, x, x], yw=yw)
                v = dict(t=t, s=s, rt=rt)
                _check_sums("partition array %d %s" % (c, where), n, sums, _want11(v, x, x, yw))
                assert np.all(sums[:5] > 0)
                if c == 3:
                    assert np.all(sums[5:8] > 0) and sums[8] == 0.0 and np.all(sums[9:] > 0)
                else:
                    assert np.all(sums[5:8] == 0.0) and sums[8] > 0 and np.all(sums[9:] == 0.0)


def _check_update(what, got, want, mag):
    err = np.abs(np.asarray(got, dtype=LD).reshape(want.shape) - want)
    bar = UPDATE_TOL * EPS * mag
    ok = bar > 0
    _note("update", what, float(np.max(err[ok] / bar[ok])))
    assert np.all(err <= bar), (what, float(np.max(err[ok] / bar[ok])))


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_update_kernels_element_by_element(shape):
    n, v = SHAPES[shape], operands(shape, "spread")
    L = {k: np.asarray(a, dtype=LD) for k, a in v.items()}
    al, om, be = 0.37, -1.9, 2.3e-2
    with _one_rank(n) as (P3, A):
        _, o = A.krylov_probe(P3.PROBE_AXPBY, [v["x"], v["z"]], scalars=[al, om], fetch=[2])
        _check_update(shape + " axpby", o[2], al * L["x"] + om * L["z"], np.abs(al * L["x"]) + np.abs(om * L["z"]))
        _, o = A.krylov_probe(P3.PROBE_AXPBY, [v["x"], v["x"]], scalars=[1.0, 0.0], fetch=[2])
        assert np.array_equal(o[2].reshape(n + [4]), v["x"])                  # (the copy y = 1 x + 0 x of the loop)
        _, o = A.krylov_probe(P3.PROBE_P, [v["p"], v["r"], v["v"]], scalars=[be, om], fetch=[0])
        p_new = L["r"] + be * (L["p"] - om * L["v"])
        p_mag = np.abs(L["r"]) + abs(be) * (np.abs(L["p"]) + np.abs(om * L["v"]))
        _check_update(shape + " p_update", o[0], p_new, p_mag)
        x_new, x_mag = L["x"] + al * L["y"] + om * L["z"], np.abs(L["x"]) + np.abs(al * L["y"]) + np.abs(om * L["z"])
        r_new, r_mag = L["s"] - om * L["t"], np.abs(L["s"]) + np.abs(om * L["t"])
        _, o = A.krylov_probe(P3.PROBE_XR, [v[k] for k in ("x", "y", "z", "r", "s", "t")], scalars=[al, om], fetch=[0, 3])
        _check_update(shape + " xr_update x", o[0], x_new, x_mag)
        _check_update(shape + " xr_update r", o[3], r_new, r_mag)
        _, o = A.krylov_probe(P3.PROBE_XRP, [v[k] for k in ("x", "y", "z", "r", "s", "t", "p", "v")], scalars=[al, om, be], fetch=[0, 3, 6])
        _check_update(shape + " xrp_update x", o[0], x_new, x_mag)
        _check_update(shape + " xrp_update r", o[3], r_new, r_mag)
        _check_update(shape + " xrp_update p", o[6], r_new + be * (L["p"] - om * L["v"]), r_mag + abs(be) * (np.abs(L["p"]) + np.abs(om * L["v"])))
        assert A.ring_sum() == 0.0


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_shadow_residual_is_bit_equal(shape):
    n = SHAPES[shape]
    with _one_rank(n) as (P3, A):
        for seed in (K.SHADOW_SEED, 7):
            _, o = A.krylov_probe(P3.PROBE_RANDOM, [], scalars=[seed], fetch=[0])
            assert np.array_equal(o[0].reshape(n + [4]), K.shadow(n, seed)), seed


# ---------------------------------------------------------------------------------------------------------------------
# b. hydrostatic start
# ---------------------------------------------------------------------------------------------------------------------
def _hydro_problem(n, grade, walls, kind):
    grid, etas, etan, rho = fields(n)
    L = [g[-1] for g in grid]
    grid = [graded(n[0], L[0], 3.0) if grade else np.linspace(0, L[0], n[0]), np.linspace(0, L[1], n[1]), np.linspace(0, L[2], n[2])]
    grav, flow = None, None
    if kind == "layered":
        rho = 3300.0 + 200.0 * np.tanh(3 * (grid[0] / L[0] - 0.4))[:, None, None] + np.zeros(n)
    elif kind == "nogravity":
        grav = (0.0, 0.0, 0.0)
    elif kind == "flow":
        flow = [1e-9, None, None, 1e-9, None, None]          # in through z0, out through zL
        assert F.balanced(grid, flow)
    return dict(n=n, grid=grid, etas=etas, etan=etan, rho=rho, bc=WALLS[walls], grav=grav, flow=flow, kind=kind)


def _hydro_device(P3, p, ctx):
    A, _ = P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], bc=p["bc"], grav=p["grav"], ctx=ctx, wallflow=p["flow"])
    return A.hydrostatic()


def _check_hydro(what, p, xh, ref):
    n = p["n"]
    if "model" not in p:
        p["model"] = K.System(p["grid"], p["etas"], p["etan"], p["rho"], bc=p["bc"], grav=p["grav"], wallflow=p["flow"], ld=True)
    s = p["model"]
    want = s.hydrostatic()
    X = xh.reshape(n + [4])
    assert not X[..., :3].any(), what
    Pw = want.reshape(n + [4])[..., 3]
    pmax = float(np.max(np.abs(Pw)))
    err = float(np.max(np.abs(np.asarray(X[..., 3], dtype=LD) - Pw)))
    if p["kind"] == "nogravity":
        assert pmax == 0.0 and err == 0.0 and ref == 0.0, what
        return
    _note("hydro P", what, err / (4 * n[0] * EPS * pmax))
    assert err <= 4 * n[0] * EPS * pmax, (what, err / pmax)
    rw = float(s.reference_norm(want))
    if p["kind"] == "layered":
        assert rw == 0.0 and ref == 0.0, (what, ref)
    else:
        assert rw > 0 and ref > 0
        _note("hydro ref", what, abs(ref - rw) / rw / 1e-12)
        assert abs(ref - rw) <= 1e-12 * rw, (what, ref, rw)


HYDRO = [(n, g, w, "mantle") for n in ([6, 7, 9], [17, 13, 21]) for g in (False, True) for w in ("free", "mixed")] + \
        [([17, 13, 21], True, "mixed", "flow"), ([6, 7, 9], False, "free", "nogravity"), ([17, 13, 21], True, "mixed", "layered"),
         ([6, 7, 9], False, "free", "layered")]


@pytest.mark.parametrize("n,grade,walls,kind", HYDRO)
def test_hydrostatic_start_matches_the_model(n, grade, walls, kind):
    from pylamp_amd import pylamp3d as P3
    p = _hydro_problem(n, grade, walls, kind)
    ctx = P3.Context3(n, p["grid"])
    try:
        xh, ref = _hydro_device(P3, p, ctx)
    finally:
        ctx.close()
    _check_hydro("%s %s %s %s" % (n, "graded" if grade else "uniform", walls, kind), p, xh, ref)


@pytest.mark.parametrize("layout", [(2, 1, 1), (2, 2, 2)])
@pytest.mark.parametrize("kind", ["mantle", "layered"])
def test_hydrostatic_start_on_blocks(layout, kind):
    """k3_hydro per block, the column totals of the blocks above (k3_hydro_add) and the anchor value from the rank that owns it."""
    from pylamp_amd import pylamp3d as P3
    p = _hydro_problem([17, 17, 17], True, "mixed", kind)
    vc = P3.VirtualCluster3(p["n"], p["grid"], *layout)
    try:
        out = vc.all(lambda ctx, rank: _hydro_device(P3, p, ctx), timeout=300)
    finally:
        vc.close()
    assert len(out) == int(np.prod(layout))
    for rank, (xh, ref) in enumerate(out):
        _check_hydro("blocks %s %s rank %d" % (layout, kind, rank), p, xh, ref)


# ---------------------------------------------------------------------------------------------------------------------
# c. the first iterations, d. the deflation, e. the estimate
# ---------------------------------------------------------------------------------------------------------------------
def _device_solve(cid, maxit=None, env=None, after=None, start=False):
    """One solve of the case on a fresh context (maxit None: the default) under the environment, and what the device holds afterwards.
    after(P3, ctx, A) may go on with the same context; start=True adds the device's start vector x_h."""
    from pylamp_amd import pylamp3d as P3
    c = build_case(cid)
    ctx = P3.Context3(c["n"], c["grid"])
    try:
        A, _ = P3.makeStokesMatrix(c["n"], c["grid"], c["etas"], c["etan"], c["rho"], bc=c["bc"], ctx=ctx, strict_reference=c["strict"])
        with _environment(env or {}):
            x = P3.solve(A) if maxit is None else P3.solve(A, maxit=maxit)
        out = _state(P3, A, x)
        if start:
            out["xh"] = A.hydrostatic()[0]           # (last: it writes work vectors, u's among them)
        if after:
            after(P3, ctx, A)
    finally:
        ctx.close()
    return out


def _state(P3, A, x):
    return dict(x=x, stats=dict(A.last_stats), dx=A.work_vector(P3.WORK_DX), r=A.work_vector(P3.WORK_R), s=A.work_vector(P3.WORK_S),
                rt=A.work_vector(P3.WORK_RT), b=A.work_vector(P3.WORK_B), w=A.work_vector(P3.WORK_W), lmax=A.mg_info()[1],
                defl=A.defl_info(), ring=A.ring_sum())


def _model_M(s, dev):
    """The model's preconditioner for a system in its precision: the device's lmax, and the deflation correction with the device's w
    where the device's solve deflated."""
    Mfn = K.preconditioner(s, dev["lmax"])
    return s.M_deflated(Mfn, dev["w"]) if dev["defl"]["active"] else Mfn


def _bars(a64, ald):
    """Per component: max(1e-11, 50 x floor), floor = |a64 - a_ld|_inf / |a_ld|_inf."""
    a64, ald = a64.reshape(-1, 4), ald.reshape(-1, 4)
    return [max(Z_TOL, FLOOR_FACTOR * float(np.max(np.abs(a64[:, q] - ald[:, q])) / np.max(np.abs(ald[:, q])))) for q in range(4)]


def _check_components(check, what, got, ald, bars):
    got, ald = np.asarray(got).reshape(-1, 4), ald.reshape(-1, 4)
    bad = []
    for q in range(4):
        ratio = float(np.max(np.abs(got[:, q] - ald[:, q])) / np.max(np.abs(ald[:, q])))
        _note(check, "%s %s (bar %.1e)" % (what, COMP[q], bars[q]), ratio)
        if not ratio <= bars[q]:
            bad.append((COMP[q], ratio, bars[q]))
    assert not bad, (what, bad)


@pytest.mark.parametrize("cid", ["one-level", "two-level", "aniso-mixed"])
def test_first_iterations_match_the_recurrence(cid):
    """pl3_stokes_solve(rhs = NULL, maxit = m), m = 1, 2, 3, fused (PYLAMP_3D_FUSED unset) and unfused (= 0): dx and r against the
    model's recurrence in longdouble, rel_residual against |b - A (x_h + dx)| / ref of the model, and fused against unfused."""
    runs = [(m, {"PYLAMP_3D_FUSED": f}) for m in (1, 2, 3) for f in (None, "0")]
    devs = [_device_solve(cid, m, env) for m, env in runs]
    sl, s64 = system(cid, True), system(cid, False)
    d0 = devs[0]
    nlev = len(G.level_grids(sl.grid))
    assert len(d0["lmax"]) == nlev and d0["defl"]["active"] == (nlev > 1)
    assert np.array_equal(d0["rt"].reshape(sl.n + [4]), K.shadow(sl.n))
    assert float(np.max(np.abs(d0["b"] - sl.b))) <= 4 * EPS * float(np.max(np.abs(sl.b)))
    for d in devs:
        assert d["lmax"] == d0["lmax"] and np.array_equal(d["w"], d0["w"])
        assert all(d["defl"][k] == d0["defl"][k] for k in ("valid", "active", "q", "inner_iterations", "inner_residual", "yAw", "wvel2", "checks"))
        assert d["ring"] == 0.0
    rt = K.shadow(sl.n).reshape(-1)
    xh_l, xh_64 = sl.hydrostatic(), s64.hydrostatic()
    ref = sl.reference_norm(xh_l)
    tr_l = K.bicgstab_steps(sl.A, _model_M(sl, d0), sl.b, xh_l, rt, 3, trace=True)
    tr_64 = K.bicgstab_steps(s64.A, _model_M(s64, d0), s64.b, xh_64, rt, 3, trace=True)
    for k, (m, env) in enumerate(runs):
        d, what = devs[k], "%s m=%d %s" % (cid, m, "unfused" if env["PYLAMP_3D_FUSED"] else "fused")
        assert d["stats"]["iterations"] == m, what
        (dxl, rl), (dx64, r64) = tr_l[m - 1], tr_64[m - 1]
        bdx, br = _bars(dx64, dxl), _bars(r64, rl)
        _check_components("iter dx", what, d["dx"], dxl, bdx)
        _check_components("iter r", what, d["r"], rl, br)
        rel = float(K.norm(sl.b - sl.A(xh_l + dxl)) / ref)
        _note("iter rel", what, abs(d["stats"]["rel_residual"] - rel) / rel / max(br))
        assert abs(d["stats"]["rel_residual"] - rel) <= max(br) * rel, (what, d["stats"]["rel_residual"], rel)
        if k % 2:
            f = devs[k - 1]
            _check_components("fused", what + " against fused dx", d["dx"], np.asarray(f["dx"], dtype=LD), bdx)
            _check_components("fused", what + " against fused r", d["r"], np.asarray(f["r"], dtype=LD), br)


@pytest.mark.parametrize("cid", ["two-level", "aniso-mixed"])
def test_deflation(cid):
    """k3_defl_setup, the vector w of the inner solve, the correction at the end of stokes_M3, and the reuse rule: a second solve with
    unchanged coefficients keeps w as it is, a third after a change of the viscosity still deflates correctly."""
    c = build_case(cid)
    sl, s64 = system(cid, True), system(cid, False)
    n = sl.n
    r = np.random.default_rng([13] + n).standard_normal(sl.b.size)
    got = {}

    def more(P3, ctx, A):
        got["info"] = A.defl_info(vectors=True)
        got["z"] = A.precond_deflated(r)
        got["lmax"] = A.mg_info()[1]
        P3.solve(A)
        got["second"] = A.defl_info()
        got["w2"] = A.work_vector(P3.WORK_W)
        Z, X, Y = np.meshgrid(*[g / g[-1] for g in c["grid"]], indexing="ij")
        f = 1 + 0.3 * np.sin(2 * np.pi * Z) * np.sin(2 * np.pi * X) * np.sin(2 * np.pi * Y)
        A3, _ = P3.makeStokesMatrix(n, c["grid"], c["etas"] * f, c["etan"] * f, c["rho"], bc=c["bc"], ctx=ctx, strict_reference=c["strict"])
        P3.solve(A3)
        got["third"] = A3.defl_info()
        got["third_stats"] = dict(A3.last_stats)
        got["z3"] = A3.precond_deflated(r)
    dev = _device_solve(cid, after=more)
    info = got["info"]
    assert info["valid"] and info["active"] and info["q"] == -1.0 and info["inner_iterations"] > 0 and dev["stats"]["converged"] == 1
    # k3_defl_setup
    u, yw = sl.deflation_vectors()
    for name, a, b in (("u", info["u"], u), ("yw", info["yw"], yw)):
        rel = np.abs(np.asarray(a, dtype=LD) - b)
        _note("defl " + name, cid, float(np.max(rel[b != 0] / np.abs(b[b != 0]))) / (8 * EPS))
        assert np.all(rel <= 8 * EPS * np.abs(b)) and np.array_equal(a != 0, sl.cont), name
    # the vector w
    w = np.asarray(dev["w"], dtype=LD)
    uv = sl.u_vector()
    res = float(K.norm(uv - sl.A(w)) / K.norm(uv))
    _note("defl w", cid + " |u - A w| / |u| against the device's", abs(res - info["inner_residual"]) / res / 1e-10)
    assert res < 0.05 and abs(res - info["inner_residual"]) <= 1e-10 * res, (res, info["inner_residual"])
    yAw, wvel2 = float(sl.yAw(w)), float(K.dot(sl.vel(w), sl.vel(w)))
    yAw_mag = float(np.sum(np.abs(yw * sl.cont_rows(w))))          # (both are sums of the reduction kernels: their bound)
    assert abs(info["yAw"] - yAw) <= 2 * sum_tol(n) * yAw_mag and abs(info["wvel2"] - wvel2) <= sum_tol(n) * wvel2, (info, yAw, wvel2)
    # the corrected preconditioner
    dz = dict(dev, lmax=got["lmax"])
    zl, z64 = _model_M(sl, dz)(r), _model_M(s64, dz)(r)
    _check_components("defl z", cid, got["z"], zl, _bars(z64, zl))
    ywf = yw.reshape(-1)
    for name, z in (("first", got["z"]), ("third", got["z3"])):
        cz = sl.cont_rows(np.asarray(z, dtype=LD)).reshape(-1)
        mag = float(np.sum(np.abs(ywf * r.reshape(-1, 4)[:, 3])) + np.sum(np.abs(ywf * cz)))
        val = float(abs(K.dot(ywf, np.asarray(r.reshape(-1, 4)[:, 3], dtype=LD) - cz)))
        _note("defl ident", "%s %s solve" % (cid, name), val / mag / 1e-12)
        assert val <= 1e-12 * mag, (name, val, mag)
    # reuse
    sec = got["second"]
    assert sec["valid"] and sec["active"] and sec["inner_iterations"] == 0 and np.array_equal(got["w2"], dev["w"])
    assert sec["q"] < 0.1 and abs(sec["q"] - info["inner_residual"]) <= 1e-12 * info["inner_residual"], (sec, info)
    assert got["third"]["valid"] and got["third"]["active"] and got["third"]["q"] >= 0 and got["third_stats"]["converged"] == 1, got["third"]


@pytest.mark.parametrize("cid", sorted(RHO_MODEL))
def test_error_estimate_is_the_formula_and_honest(cid):
    """A converged solve at the default tolerances against the direct solution of the model matrix: the reported estimate is the
    model's formula at the device's final x (when fewer than 6 checks were taken), and the true velocity error is at most
    max(1, 2 rho_model) times it (rho_model: what the model's own loop achieves, tests/test_stokes3_krylov_model.py).
    The final iterate is the device's x_h + dx before the sum is rounded to float64, its residual (b - A x_h) - A dx with the device's
    b: at |s| ~ 1e-10 |b| one rounding of x_h + dx or of b moves the residual, and with it the estimate, by 1e-6 and more."""
    dev = _device_solve(cid, start=True)
    st = dev["stats"]
    sl, s64 = system(cid, True), system(cid, False)
    assert st["converged"] == 1 and dev["ring"] == 0.0
    err = velocity_error(dev["x"], direct_solution(cid))
    ratio = err / st["error_estimate"]
    _note("est honest", "%s true error %.3e estimate %.3e rho_model %.4f: ratio" % (cid, err, st["error_estimate"], RHO_MODEL[cid]), ratio)
    checks = dev["defl"]["checks"]
    assert 1 <= checks <= 6
    if checks < 6:
        est = []
        for s in (sl, s64):
            xh, dx, b = [np.asarray(dev[k], dtype=s.dt) for k in ("xh", "dx", "b")]
            x = xh + dx
            res = (b - s.A(xh)) - s.A(dx)
            d = (dev["defl"]["yAw"], dev["defl"]["wvel2"]) if dev["defl"]["active"] else ()
            est.append(float(s.estimate(res, _model_M(s, dev)(res), x, *d)))
        bar = max(1e-6, FLOOR_FACTOR * abs(est[1] - est[0]) / est[0])
        _note("est formula", "%s (bar %.1e, %d checks)" % (cid, bar, checks), abs(st["error_estimate"] - est[0]) / est[0])
        assert abs(st["error_estimate"] - est[0]) <= bar * est[0], (st["error_estimate"], est)
    assert err < 5e-8, err
    assert err <= max(1.0, 2 * RHO_MODEL[cid]) * st["error_estimate"], (err, st["error_estimate"], RHO_MODEL[cid])


REC_TOL = 1e-6


@pytest.mark.parametrize("cid", ["one-level", "two-level", "aniso-mixed"])
def test_estimate_between_the_checks(cid):
    """est_rec3 and what bicgstab3 feeds it, late in the iteration: the fused branch forms |r|^2 and |r_cont|^2 of r = s - omega t from
    the sums of k3_dots11 (s.s - 2 omega t.s + omega^2 t.t, once over the vector and once over the pressure array), |x_vel|^2 of the
    iterate BEFORE the update and the anchor part from yw.s_p - omega yw.t_p; the unfused branch takes dots of r and of the updated
    iterate.  A converged solve gives N; fresh contexts then stop at maxit = N - 3 (and N - 4 for the iterate before), fused and
    unfused, and report the last estimate with its parts (pl3_stokes_defl_info).  Each part and the estimate against the model's
    formula on the device's own r (K_R) and dx, in longdouble, with the a_mom the device reports (1 before the first check).
    Bar 1e-6 relative: every sum is good to sum_tol = 5 (trips + 10 + 1024) eps sum |terms| = 1.2e-12 sum |terms|, and
    |s - omega t|^2 loses (s.s + 2 |omega| |t.s| + omega^2 t.t) / |r|^2 <= 4 s.s / |r|^2 on top (omega minimises |s - omega t|): 1e-6
    allows s.s / |r|^2 up to 2e5, a residual that falls 450-fold inside the second half of one iteration.  The anchor part is held to
    1e-6 of the same expression with sum |yw r_p| in place of yw . r_p: the deflation keeps yw . r_cont near zero (1e-8 of sum |terms|
    here), so the sum is nearly all cancellation and a relative bar on its value would test rounding.  For the same reason this solve
    says little about the combination yw.s_p - omega yw.t_p; the two sums themselves are pinned with real data by the k3_dots11 probe
    above.  Fused against unfused: the same estimate up to the 10 %
    that |x_vel| of the iterate before the update is allowed to differ by (the comment in bicgstab3)."""
    full = _device_solve(cid)
    N = full["stats"]["iterations"]
    assert full["stats"]["converged"] == 1 and N > 8
    m = N - 3
    fused = _device_solve(cid, m, {"PYLAMP_3D_FUSED": None}, start=True)
    before = _device_solve(cid, m - 1, {"PYLAMP_3D_FUSED": None})
    unfused = _device_solve(cid, m, {"PYLAMP_3D_FUSED": "0"})
    sl = system(cid, True)
    yw = sl.deflation_vectors()[1].reshape(-1)
    n_amp = max(sl.n)
    got = {}
    for name, d, dx_for_x in (("fused", fused, before["dx"]), ("unfused", unfused, unfused["dx"])):
        info = d["defl"]
        assert d["stats"]["iterations"] == m and info["rec_iteration"] == m and info["checks"] == 0 and info["rec_a_mom"] == 1.0, (name, info)
        a_mom = LD(info["rec_a_mom"])
        assert d["ring"] == 0.0
        r = np.asarray(d["r"], dtype=LD)
        x = np.asarray(fused["xh"], dtype=LD) + np.asarray(dx_for_x, dtype=LD)
        rr, rc, xx = K.dot(r, r), K.dot(sl.prs(r), sl.prs(r)), K.dot(sl.vel(x), sl.vel(x))
        ap = abs(K.dot(yw, sl.prs(r)) / info["yAw"]) * np.sqrt(info["wvel2"] / xx) if info["active"] else LD(0)
        ap_mag = np.sum(np.abs(yw * sl.prs(r))) / abs(info["yAw"]) * np.sqrt(info["wvel2"] / xx) if info["active"] else LD(0)
        want = (n_amp * np.sqrt(rc) + a_mom * np.sqrt(rr - rc)) / np.sqrt(xx) + ap
        for part, g, w in (("rr", info["rec_rr"], rr), ("rc", info["rec_rc"], rc), ("xx", info["rec_xx"], xx), ("anchor", info["rec_anchor"], ap),
                           ("estimate", info["rec"], want)):
            if part == "anchor" and not info["active"]:
                assert g == 0.0
                continue
            ratio = float(abs(LD(g) - w) / (ap_mag if part == "anchor" else w))
            _note("rec " + part, "%s %s m=%d" % (cid, name, m), ratio / REC_TOL)
            assert ratio <= REC_TOL, (cid, name, part, g, float(w))
        assert 0 < info["rec"] and (info["active"] == (len(G.level_grids(sl.grid)) > 1))
        got[name] = info["rec"]
    ratio = abs(got["fused"] / got["unfused"] - 1.0)
    _note("rec fused", "%s fused against unfused m=%d" % (cid, m), ratio / 0.1)
    assert ratio <= 0.1, got


def test_ring_sum_sees_the_rings():
    """The positive control of the ring tests: on 1 x 1 x 2 blocks of [6, 6, 517] an upload fills the ring plane of each block with the
    neighbour's nodes (global k = 258 on rank 0, 257 on rank 1), and k3_axpby, a flat kernel, writes y = 1 x + 0 z = x there as well:
    the ring sum of a rank is 2 sum |x| + sum |z| over its plane, nothing else (fresh contexts: the other work vectors are zero)."""
    from pylamp_amd import pylamp3d as P3
    n, v = LINE, operands("line", "spread")
    vc = P3.VirtualCluster3(n, [np.linspace(0, 1, k) for k in n], 1, 1, 2)
    try:
        def run(ctx, rank):
            A = _probe_operator(P3, n, ctx)
            A.krylov_probe(P3.PROBE_AXPBY, [v["x"], v["z"]], scalars=[1.0, 0.0])
            return A.ring_sum()
        out = vc.all(run, timeout=300)
    finally:
        vc.close()
    for rank, plane in enumerate((258, 257)):
        want = 2 * np.sum(np.abs(np.asarray(v["x"][:, :, plane], dtype=LD))) + np.sum(np.abs(np.asarray(v["z"][:, :, plane], dtype=LD)))
        _note("ring sum", "rank %d" % rank, float(abs(out[rank] - want) / want) / sum_tol(n))
        assert want > 0 and abs(out[rank] - want) <= sum_tol(n) * want, (rank, out[rank], float(want))


def test_ring_stays_zero_under_the_marching_kernels():
    """[37, 45, 131]: level 0 runs the marching LDS kernels and their rim.  After a converged solve the ring and padding entries of the
    14 work vectors are exactly zero -- what the flat reductions of one rank rely on."""
    from pylamp_amd import pylamp3d as P3
    n = [37, 45, 131]
    grid, etas, etan, rho = fields(n)
    ctx = P3.Context3(n, grid)
    try:
        A, _ = P3.makeStokesMatrix(n, grid, etas, etan, rho, bc=WALLS["mixed"], ctx=ctx)
        P3.solve(A)
        assert A.last_stats["converged"] == 1 and A.mg_plan()["lds"][0]
        assert A.ring_sum() == 0.0
    finally:
        ctx.close()
