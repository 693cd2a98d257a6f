"""Lifetime of the wall planes on the device, through Context3, for the two settings that keep six optional planes in one buffer: the
through-flow of the Stokes walls (planes over faces) and the profiles of the heat walls (planes over nodes, NaN where another wall owns
the node).  nx = (5, 6, 7) on the graded grid of tests/test_hip_3d_model.py: every plane has another shape.

One sequence per setting: set a subset A, set another subset B, a rejected call, clear, set A again (the buffer is allocated anew),
and the operator's right-hand side against a fresh context's -- with the copies that pl3_transfer_stats counts per call:
a set with at least one plane is one copy of all six planes' bytes, a set that clears is none, a get is one copy per wall that is asked
for and has a plane."""
import ctypes as C

import numpy as np
import pytest

from test_hip_3d_model import WALLS, _heat_problem, _problem

gpu = pytest.mark.gpu
N = (5, 6, 7)
FACES = [(5, 6), (4, 6), (4, 5)] * 2
NODES = [(6, 7), (5, 7), (5, 6)] * 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same_planes(got, want):
    assert [g is None for g in got] == [w is None for w in want], ([g is None for g in got], [w is None for w in want])
    for g, w in zip(got, want):
        assert g is None or (g.shape == w.shape and np.array_equal(_bits(g), _bits(w)))


def _copies(ctx):
    """(copies, bytes) since the last call, both size classes together."""
    v = (C.c_int64 * 4)()
    ctx.check(ctx.lib.pl3_transfer_stats(ctx.handle(), v, 1))
    return int(v[0]) + int(v[2]), int(v[1]) + int(v[3])


def _flow_planes(seed, axes):
    """The same random plane on the low and the high wall of each of the axes: what enters leaves, so the net flux vanishes."""
    rng = np.random.default_rng(seed)
    out = [None] * 6
    for a in axes:
        out[a] = rng.uniform(-1e-9, 1e-9, FACES[a])
        out[a + 3] = out[a].copy()
    return out


def _heat_planes(seed, walls):
    """Random planes with NaN at every node another wall owns (z-walls own their edges, then x-walls, then y-walls)."""
    rng = np.random.default_rng(seed)
    out = [None] * 6
    for w in walls:
        v = rng.uniform(300, 1500, NODES[w])
        if w % 3 >= 1:
            v[0, :] = v[-1, :] = np.nan
        if w % 3 == 2:
            v[:, 0] = v[:, -1] = np.nan
        out[w] = v
    return out


def _stokes_rhs(P3, ctx, flow):
    p = _problem(N)
    return P3.makeStokesMatrix(p["n"], p["grid"], p["etas"], p["etan"], p["rho"], grav=(3.0, -4.0, 5.0), ctx=ctx, wallflow=flow)[1]


def _heat_rhs(P3, ctx, values):
    h = _heat_problem(N)
    bc, bv = WALLS["mixed"]
    return P3.makeDiffusionMatrix(h["n"], h["grid"], h["mid"], h["T0"], h["k"], h["Cp"], h["rho"], h["H"], bc, bv, h["dt"], ctx=ctx,
                                  wallvalues=values)[1]


SETTINGS = {
    # setter and getter of Context3, the library's setter, planes A and B, the walls of one bad call and its message, shapes, rhs
    "flow": dict(set="set_wall_flow", get="wall_flow", entry="pl3_stokes_set_wall_flow", A=_flow_planes(1, (0, 1)), B=_flow_planes(2, (1, 2)),
                 bad=(2, (3, 4), np.inf, b"pl3_stokes_set_wall_flow: wall y0 has a non-finite flow entry [3, 4] = inf"), shapes=FACES,
                 rhs=_stokes_rhs),
    "heat": dict(set="set_heat_wall_values", get="heat_wall_values", entry="pl3_heat_set_wall_values", A=_heat_planes(3, (0, 1, 5)),
                 B=_heat_planes(4, (1, 2, 3)), bad=(2, (3, 4), np.inf, b"pl3_heat_set_wall_values: wall y0 has a non-finite entry [3, 4] = inf"),
                 shapes=NODES, rhs=_heat_rhs),
}


@gpu
@pytest.mark.parametrize("what", sorted(SETTINGS))
def test_planes_through_set_replace_reject_clear_and_set_again(what):
    from pylamp_amd import pylamp3d as P3, _lib
    s = SETTINGS[what]
    p = _problem(N)
    all_bytes = 8 * sum(int(np.prod(shp)) for shp in s["shapes"])
    plane_bytes = lambda planes: 8 * sum(v.size for v in planes if v is not None)
    count = lambda planes: sum(v is not None for v in planes)
    ctx = P3.Context3(p["n"], p["grid"])
    try:
        setter, getter = getattr(ctx, s["set"]), getattr(ctx, s["get"])
        _copies(ctx)
        assert getter() == [None] * 6 and _copies(ctx) == (0, 0)
        for planes in (s["A"], s["B"]):               # the walls of A outside B come back as None
            setter(planes)
            assert _copies(ctx) == (1, all_bytes)
            _same_planes(getter(), planes)
            assert _copies(ctx) == (count(planes), plane_bytes(planes))
        # one non-finite entry, handed to the library without the Python validator: rejected, mask and planes as before
        w, (i, j), v, message = s["bad"]
        bad = [None if a is None else a.copy() for a in s["B"]]
        bad[w][i, j] = v
        if what == "flow":
            bad[w + 3][i, j] = v
        ptr = (_lib.c_double_p * 6)(*[None if a is None else _lib.dptr(a) for a in bad])
        assert getattr(ctx.lib, s["entry"])(ctx.handle(), ptr) != 0
        assert ctx.lib.pl3_last_error(ctx.handle()) == message
        assert _copies(ctx) == (0, 0)
        _same_planes(getter(), s["B"])
        _copies(ctx)
        # clear, and set A again into a new buffer
        setter(None)
        assert _copies(ctx) == (0, 0)
        assert getter() == [None] * 6 and _copies(ctx) == (0, 0)
        setter([None] * 6)                             # (clearing what is clear)
        assert getter() == [None] * 6 and _copies(ctx) == (0, 0)
        setter(s["A"])
        assert _copies(ctx) == (1, all_bytes)
        _same_planes(getter(), s["A"])
        rhs = s["rhs"](P3, ctx, None)                  # None: the planes of the context as they are
        _same_planes(getter(), s["A"])
    finally:
        ctx.close()
    fresh = P3.Context3(p["n"], p["grid"])
    try:
        want = s["rhs"](P3, fresh, s["A"])
        plain = s["rhs"](P3, fresh, [None] * 6)
    finally:
        fresh.close()
    assert not np.isnan(rhs).any()
    assert np.array_equal(_bits(rhs), _bits(want))
    assert not np.array_equal(rhs, plain)              # (the planes do enter the right-hand side)
