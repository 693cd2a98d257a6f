"""Inflow material of the 3-D refill on the GPU (pl3_mic_set_inflow, k_m3_inject<true>; Options3.bcinflow, set_inflow_material)
against the NumPy model tests/mic3_inflow_model.py, whose inputs tests/test_mic3_inflow_model.py checks on the CPU.

Bounds.  Everything is exact.  The refill cases run on grids whose spacings are powers of two (tests/mic3_inflow_cases.py says why),
so positions, fields and stored velocities are compared bit for bit with the model; the Simulation3 runs compare staged with
resident bit for bit and the marked set with what the rule predicts from the counter-based uniforms.

The crowded shape is [5, 5, 5] nodes: the smallest node set pl3_create accepts (5 per axis), with tracdens 140 / 70."""
import ctypes as C
import functools

import numpy as np
import pytest

import mic3_inflow_cases as K
import mic3_refill_model as R

pytestmark = pytest.mark.gpu

ZERO = (0.0, 0.0, 0.0)
FREE = dict(tracs_fence_enabled=False, marker_deletion=True)


def _refill_on_gpu(shape, graded, unique, material, flow, then=None):
    """One pl3_resident_refill of the case's tracers; `then`: called with the simulation before the refill.  Returns
    (x, f, v, counters, inflow_count)."""
    from pylamp_amd import pylamp3d as P3
    nx, dens, dmin = K.SHAPES[shape]
    grid = K.grid_of(shape, graded)
    tr_x, tr_f = K.tracers_of(shape, graded)
    opt = P3.Options3(tracdens=dens, tracdens_min=dmin, inject_seed=K.SEED, inject_unique_ids=unique, marker_search=graded,
                      bcstokesflow=flow, bcinflow=material, **FREE)
    sim = P3.Simulation3(nx, [g[-1] for g in grid], tr_x, tr_f, opt, grid=grid if graded else None)
    try:
        assert all(np.array_equal(a, b) for a, b in zip(sim.grid, grid))
        if then:
            then(sim)
        got = sim.refill(it=K.IT)
        x, f = sim.tracers()
        return x, f, sim.tracer_velocity(), got, sim.ctx.inflow_count()
    finally:
        sim.close()


@functools.lru_cache(maxsize=None)
def _never(shape, graded, unique):
    return _refill_on_gpu(shape, graded, unique, None, K.flow_of(shape))


def _same_state(a, b):
    return all(np.array_equal(p, q, equal_nan=True) for p, q in zip(a[:3], b[:3]))


@pytest.mark.parametrize("unique", [False, True], ids=["reference_ids", "unique_ids"])
@pytest.mark.parametrize("graded", [False, True], ids=["regular", "graded_search"])
@pytest.mark.parametrize("shape", list(K.SHAPES))
def test_refill_matches_model_bitwise(shape, graded, unique):
    """pl3_resident_refill with materials on z0, x0, xL (inflow), zL (outflow) and yL (no flow) against the model: x, f, v bit for bit
    and the inflow count."""
    x, f, v, got, count = _refill_on_gpu(shape, graded, unique, K.material_of(shape), K.flow_of(shape))
    rx, rf, rv, info = K.model(shape, graded, unique)
    print("%s %s: %d tracers, %d injected into %d cells (%d empty), %d inflow tracers" % (
        shape, "graded" if graded else "regular", rx.shape[0], info["ninjected"], info["nrefilled"], info["nempty"], info["ninflow"]))
    want = dict(ninjected=info["ninjected"], nrefilled=info["nrefilled"], nempty=info["nempty"], mincount=info["mincount"], nremoved=0,
                ninflow=info["ninflow"])
    assert got == want and info["ninflow"] > 0
    assert count == (info["ninflow"], info["ninflow"])
    assert x.shape == rx.shape
    assert np.array_equal(x, rx, equal_nan=True)
    assert np.array_equal(f, rf, equal_nan=True)
    assert np.array_equal(v, rv, equal_nan=True)
    # positions, IDs and counts are those of the run without a material: the rule is an overlay on the field values of new tracers
    nx_, nf, nv, ngot, ncount = _never(shape, graded, unique)
    assert np.array_equal(x, nx_) and np.array_equal(v, nv) and np.array_equal(f[:, K.TR_ID], nf[:, K.TR_ID])
    assert np.array_equal(f[~info["inflow"]], nf[~info["inflow"]], equal_nan=True)
    assert ngot == {k: want[k] for k in want if k != "ninflow"} and ncount == (0, 0)


def test_set_then_clear_and_two_runs():
    """A material that was set and cleared again leaves the refill bit for bit what a context that never had one gives, and the count at
    zero; so does a material on a wall without flow alone, which runs k_m3_inject<true> with a rule that never fires (on a general
    grid as well, where the positions are no exact sums); two identical runs with a material agree bit for bit."""
    from pylamp_amd import pylamp3d as P3
    shape = "small"
    mat, flow = K.material_of(shape), K.flow_of(shape)

    def clear(sim):
        assert sim.ctx.inflow_material()[0] is not None
        sim.set_inflow_material(None)
        assert sim.ctx.inflow_material() == [None] * 6

    never = _never(shape, False, False)
    cleared = _refill_on_gpu(shape, False, False, mat, flow, then=clear)
    assert _same_state(cleared, never) and cleared[3] == never[3] and "ninflow" not in cleared[3] and cleared[4] == (0, 0)
    idle = _refill_on_gpu(shape, False, False, [None] * 5 + [mat[5]], flow)
    assert _same_state(idle, never) and idle[3] == dict(never[3], ninflow=0) and idle[4] == (0, 0)
    runs = [_refill_on_gpu(shape, True, True, mat, flow) for _ in range(2)]
    assert _same_state(*runs) and runs[0][3] == runs[1][3] and runs[0][3]["ninflow"] > 0
    # a general grid: spacings that are no powers of two
    nx, L = [6, 5, 7], [1.0e5, 1.2e5, 0.8e5]
    rng = np.random.default_rng(3)
    tr_x = rng.random((400, 3)) * np.array(L) * 0.999 + 5e-4 * np.array(L)
    tr_f = rng.uniform(1.0, 2.0, (400, K.NF)); tr_f[:, K.TR_ID] = np.arange(400)
    out = []
    for material in (None, [None] * 5 + [{K.TR_ALP: 7.0}], [{K.TR_MAT: 2.0}] + [None] * 5):
        sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(tracdens=8, tracdens_min=4, bcinflow=material, **FREE,
                                                            bcstokesflow=[1e-9, None, None, 1e-9, None, None]))
        c = sim.refill(it=2)
        out.append((*sim.tracers(), sim.tracer_velocity(), c))
        sim.close()
    assert out[0][3]["ninjected"] > 100
    assert _same_state(out[1], out[0]) and out[1][3] == dict(out[0][3], ninflow=0)
    assert np.array_equal(out[2][0], out[0][0]) and np.array_equal(out[2][1][:, K.TR_ID], out[0][1][:, K.TR_ID]) and out[2][3]["ninflow"] > 0
    assert ((out[2][1][:, K.TR_MAT] == 2.0).sum()) == out[2][3]["ninflow"]


# ---- Simulation3: the plug flow of tests/test_hip_3d_flow.py ---------------------------------------------------------------------
SIM_NX = [17, 17, 17]
SIM_L = [100e3, 100e3, 100e3]
SIM_U = 1e-9
SIM_MOD = 0.3
PLUG = [SIM_U, None, None, SIM_U, None, None]
TR_HCP = 5


def _sim_tracers(heat):
    """8 tracers per cell, each at its own height (k + 0.5) / 8 of the cell, on a 2 x 2 lattice in x, y; uniform properties.  With
    steps of 0.3 cells the cells along z0 hold 6 tracers after the first step and 3 after the second, at 0.6625, 0.7875 and 0.9125 of
    the cell, which the refill (tracdens_min = 4) tops up with 5 new ones."""
    m = [v - 1 for v in SIM_NX]
    dz, dx, dy = (SIM_L[a] / m[a] for a in range(3))
    ci, cj, ck, k = np.meshgrid(np.arange(m[0]), np.arange(m[1]), np.arange(m[2]), np.arange(8), indexing="ij")
    tr_x = np.stack([(ci + (k + 0.5) / 8) * dz, (cj + 0.25 + 0.5 * (k & 1)) * dx, (ck + 0.25 + 0.5 * ((k >> 1) & 1)) * dy], axis=-1).reshape(-1, 3)
    tr_f = np.zeros((tr_x.shape[0], K.NF))
    tr_f[:, K.TR_ID] = np.arange(tr_x.shape[0])[::-1]      # (new IDs count from the largest one left: the outflow must not take it)
    tr_f[:, K.TR_RH0] = 3300.0; tr_f[:, 0] = 3300.0; tr_f[:, K.TR_MAT] = 1; tr_f[:, 10] = 1e19; tr_f[:, K.TR_ETA] = 1e19
    if heat:
        tr_f[:, K.TR_TMP] = 273.0 + 1350.0 * tr_x[:, 0] / SIM_L[0]; tr_f[:, K.TR_HCD] = 4.0; tr_f[:, TR_HCP] = 1250.0
    return tr_x, tr_f


@functools.lru_cache(maxsize=None)
def _run(resident, plan, heat=False):
    """One step per entry of `plan`: "none" (no material), "mat" or "heatmat" (a material on z0).  The first is Options3.bcinflow, the
    later ones are set with set_inflow_material before their step.  Cached: nobody writes to the result."""
    from pylamp_amd import pylamp3d as P3
    mats = {"none": None, "mat": [{K.TR_MAT: 2, K.TR_TMP: 1500.0, K.TR_RH0: 3200.0}] + [None] * 5,
            "heatmat": [{K.TR_MAT: 2, K.TR_TMP: 1500.0}] + [None] * 5}
    tr_x, tr_f = _sim_tracers(heat)
    opt = P3.Options3(do_heatdiff=heat, tdep_rho=False, tdep_eta=False, resident=resident, grav=ZERO, tracdens=8, tracdens_min=4,
                      inject_unique_ids=True, tstep_modifier=SIM_MOD, rk4_classic=True, bcstokesflow=PLUG, bcinflow=mats[plan[0]], **FREE)
    sim = P3.Simulation3(SIM_NX, SIM_L, tr_x, tr_f, opt)
    out = []
    names = ("rho", "etas", "etan", "velz", "velx", "vely", "pres") + (("temp", "T") if heat else ())
    try:
        for it, name in enumerate(plan):
            if it > 0:
                sim.set_inflow_material(mats[name])
            rep = sim.step()
            assert rep["stokes"]["converged"] == 1, rep
            x, f = sim.tracers()
            out.append(dict(rep=rep, x=x, f=f, v=sim.tracer_velocity(), fields={k: sim.field(k).copy() for k in names}, n0=tr_x.shape[0]))
    finally:
        sim.close()
    return out


def _same(a, b):
    for it, (s, r) in enumerate(zip(a, b)):
        for k in ("iterations", "converged", "rel_residual", "error_estimate"):
            assert s["rep"]["stokes"][k] == r["rep"]["stokes"][k], (it, k)
        for k in ("tstep", "ntrac", "ninjected", "nrefilled", "nempty", "nremoved"):
            assert s["rep"][k] == r["rep"][k], (it, k)
        assert s["rep"].get("ninflow") == r["rep"].get("ninflow"), it
        for k in s["fields"]:
            assert np.array_equal(s["fields"][k], r["fields"][k]), (it, k)
        for k in ("x", "f", "v"):
            assert np.array_equal(s[k], r[k], equal_nan=True), (it, k)


def _predicted_inflow(it):
    """How many of the 5 new tracers of each of the 256 cells along z0 get a wall-axis uniform below 0.6625, from the generator of
    the refill (tests/mic3_refill_model.inj_uniform) with the step counter `it`; and how close any comes to 0.6625."""
    u = np.array([[R.inj_uniform(12345, c, q, 3 * it) for q in range(5)] for c in range(256)])
    return int((u < 0.6625).sum()), float(np.abs(u - 0.6625).min())


def test_simulation3_plug_flow_marks_what_enters():
    """Two steps of plug flow with bcinflow on z0 = {TR_MAT: 2, TR_TMP: 1500, TR_RH0: 3200}: staged and resident agree bit for bit; step
    1 refills nothing; after step 2 the new tracers below the lowest resident (0.6625 dz) carry the material, all three columns
    together, nobody else does, and ninflow counts them."""
    staged = _run(False, ("mat", "mat"))
    resident = _run(True, ("mat", "mat"))
    _same(staged, resident)
    dz = SIM_L[0] / (SIM_NX[0] - 1)
    assert staged[0]["rep"]["ninjected"] == 0 and staged[0]["rep"]["ninflow"] == 0 and (staged[0]["f"][:, K.TR_MAT] == 1).all()
    s = staged[1]
    rep, x, f = s["rep"], s["x"], s["f"]
    assert rep["nrefilled"] == 256 and rep["ninjected"] == 1280 and rep["nempty"] == 0
    new = f[:, K.TR_ID] >= s["n0"]
    assert new.sum() == 1280 and (x[new, 0] < dz).all()
    res = ~new & (x[:, 0] < dz)
    assert res.sum() == 3 * 256 and np.abs(x[res, 0].min() - 0.6625 * dz) <= 1e-5 * dz
    want, margin = _predicted_inflow(2)
    assert margin > 1e-4 and np.abs(x[new, 0] - 0.6625 * dz).min() > 1e-4 * dz
    marked = f[:, K.TR_MAT] == 2
    print("step 2: %d of 1280 new tracers below 0.6625 dz carry the material (predicted %d), nearest to the threshold %.3g" % (marked.sum(), want, margin))
    assert np.array_equal(marked, new & (x[:, 0] < 0.6625 * dz))
    assert (f[~marked, K.TR_MAT] == 1).all()
    assert np.array_equal(marked, f[:, K.TR_TMP] == 1500.0) and np.array_equal(marked, f[:, K.TR_RH0] == 3200.0)
    assert (f[~marked, K.TR_RH0] == 3300.0).all() and (f[~marked, K.TR_TMP] == 0.0).all()
    assert rep["ninflow"] == marked.sum() == want and 800 < want < 900


def test_set_inflow_material_between_steps_starts_and_stops_the_marking():
    never = _run(False, ("none", "none"))
    started = _run(False, ("none", "mat"))
    stopped = _run(False, ("mat", "none"))
    marked = _run(False, ("mat", "mat"))
    assert all("ninflow" not in s["rep"] for s in never) and (never[1]["f"][:, K.TR_MAT] == 1).all() and never[1]["rep"]["ninjected"] == 1280
    _same(started[:1], never[:1])
    assert "ninflow" not in started[0]["rep"] and started[1]["rep"]["ninflow"] == marked[1]["rep"]["ninflow"] > 0
    _same(started[1:], marked[1:])
    assert stopped[0]["rep"]["ninflow"] == 0 and "ninflow" not in stopped[1]["rep"]
    for k in ("x", "f", "v"):
        assert np.array_equal(stopped[1][k], never[1][k], equal_nan=True), k


def test_inflow_with_heat_diffusion_staged_and_resident():
    """do_heatdiff = True with finite TR_TMP, TR_HCD, TR_HCP on the tracers and a material that prescribes TR_TMP: staged and resident bit
    for bit, both solves converge, no NaN in any field; the prescribed temperature is a tracer temperature like any other."""
    staged = _run(False, ("heatmat", "heatmat"), heat=True)
    resident = _run(True, ("heatmat", "heatmat"), heat=True)
    _same(staged, resident)
    for s in staged:
        assert s["rep"]["heat"]["converged"] == 1, s["rep"]
        for k, a in s["fields"].items():
            assert not np.isnan(a).any(), k
    f = staged[1]["f"]
    marked = f[:, K.TR_MAT] == 2
    assert staged[1]["rep"]["ninflow"] == marked.sum() > 0 and (f[marked, K.TR_TMP] == 1500.0).all() and np.isfinite(f).all()
    assert (f[~marked, K.TR_TMP] != 1500.0).all()


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_rejections_by_message():
    from pylamp_amd import pylamp3d as P3, _lib
    nx = [5, 6, 7]
    grid = [np.linspace(0, 1.0 + a, nx[a]) for a in range(3)]
    ctx = P3.Context3(nx, grid)
    lib = ctx.lib
    plane = np.ascontiguousarray(np.full((2, 5, 6), 3.0))

    def err(rc):
        assert rc != 0
        return lib.pl3_last_error(ctx.handle()).decode()

    def same(a, b):
        return all((p is None) == (q is None) and (p is None or (sorted(p) == sorted(q) and all(np.array_equal(p[c], q[c]) for c in p)))
                   for p, q in zip(a, b))

    try:
        assert ctx.inflow_material() == [None] * 6 and ctx.inflow_count() == (0, 0)
        good = [{P3.TR_MAT: 2.0, P3.TR_TMP: np.arange(30.0).reshape(5, 6)}, None, None, None, {P3.TR_RHO: 3000.0}, None]
        ctx.set_inflow_material(good)
        held = ctx.inflow_material()
        assert sorted(held[0]) == [P3.TR_TMP, P3.TR_MAT] and np.array_equal(held[0][P3.TR_TMP], good[0][P3.TR_TMP]) and (held[0][P3.TR_MAT] == 2.0).all()
        assert held[4][P3.TR_RHO].shape == (4, 6) and (held[4][P3.TR_RHO] == 3000.0).all() and held[1] is None
        out = (C.c_int64 * 2)()
        assert lib.pl3_mic_set_inflow(None, 0, 1, _lib.dptr(plane)) != 0 and b"NULL context" in lib.pl3_last_error(None)
        assert lib.pl3_mic_get_inflow(None, 0, None, None) != 0 and b"NULL context" in lib.pl3_last_error(None)
        assert lib.pl3_mic_inflow_count(None, out) != 0 and b"NULL context" in lib.pl3_last_error(None)
        for wall in (-1, 6):
            assert ("pl3_mic_set_inflow: wall %d is not one of 0 ... 5" % wall) in err(lib.pl3_mic_set_inflow(ctx.handle(), wall, 1, _lib.dptr(plane)))
            assert ("pl3_mic_get_inflow: wall %d is not one of 0 ... 5" % wall) in err(lib.pl3_mic_get_inflow(ctx.handle(), wall, None, None))
        msg = err(lib.pl3_mic_set_inflow(ctx.handle(), 0, (1 << 12) | 1, _lib.dptr(plane)))
        assert "pl3_mic_set_inflow" in msg and "wall z0" in msg and "bit 12" in msg and "TR__ID" in msg
        msg = err(lib.pl3_mic_set_inflow(ctx.handle(), 3, 1 << 14, _lib.dptr(plane)))
        assert "wall zL" in msg and "bit 14" in msg and "TR__ID" not in msg
        msg = err(lib.pl3_mic_set_inflow(ctx.handle(), 1, 3, None))
        assert "pl3_mic_set_inflow: wall x0 names columns but values is NULL" in msg
        bad = plane.copy(); bad[1, 2, 3] = np.nan
        msg = err(lib.pl3_mic_set_inflow(ctx.handle(), 0, (1 << 3) | (1 << 8), _lib.dptr(bad)))
        assert "pl3_mic_set_inflow: wall z0, column 8 has a non-finite value at index 15 = nan" in msg
        assert "NULL argument" in err(lib.pl3_mic_inflow_count(ctx.handle(), None))
        for bad_m, text in (([None] * 5, r"Context3.set_inflow_material: the inflow material needs six entries"),
                            ([None, {P3.TR__ID: 1.0}, None, None, None, None], r"of wall x0 names TR__ID"),
                            ([{P3.TR_MAT: 5.0}, {99: 1.0}, None, None, None, None], r"of wall x0 names an unknown column 99"),
                            ([{P3.TR_MAT: 5.0}, {P3.TR_MAT: np.zeros((3, 3))}, None, None, None, None], r"column 8 of the inflow material of wall x0 needs the shape \(nz - 1, ny - 1\) = \(4, 6\)"),
                            ([{P3.TR_MAT: 5.0}, None, None, None, None, {P3.TR_MAT: np.inf}], r"wall yL has a non-finite value \[0, 0\] = inf")):
            with pytest.raises(Exception, match=text):
                ctx.set_inflow_material(bad_m)
        assert same(ctx.inflow_material(), held)              # the rejected calls changed nothing
        # the state survives the Stokes settings; clearing one wall leaves the others
        ctx.set_stokes_walls([0] * 6)
        ctx.set_wall_flow([1e-9, None, None, 1e-9, None, None])
        ctx.set_wall_flow(None)
        assert same(ctx.inflow_material(), held)
        ctx.check(lib.pl3_mic_set_inflow(ctx.handle(), 0, 0, None))
        assert same(ctx.inflow_material(), [None] + held[1:])
    finally:
        ctx.close()
    vc = P3.VirtualCluster3([9, 9, 9], [np.linspace(0, 1, 9)] * 3, 2, 1, 1)
    try:
        c2 = vc.ctxs[0]
        one = np.ones((8, 8))
        assert c2.lib.pl3_mic_set_inflow(c2.handle(), 0, 1, _lib.dptr(one)) != 0
        msg = c2.lib.pl3_last_error(c2.handle())
        assert b"one rank" in msg and b"pl3_mic_set_inflow" in msg
    finally:
        vc.close()
    with pytest.raises(Exception, match=r"Simulation3: Options3.bcinflow: the inflow material of wall z0 names TR__ID"):
        P3.Simulation3(nx, [1.0, 2.0, 3.0], options=P3.Options3(bcinflow=[{P3.TR__ID: 1}, None, None, None, None, None]))
    # a material on a wall that carries no flow is accepted
    sim = P3.Simulation3(nx, [1.0, 2.0, 3.0], options=P3.Options3(bcinflow=[None, None, {P3.TR_MAT: 4}, None, None, None]))
    try:
        assert sim.ctx.inflow_material()[2] is not None and sim.ctx.wall_flow() == [None] * 6
    finally:
        sim.close()
