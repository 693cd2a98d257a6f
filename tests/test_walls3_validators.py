"""The three validators of the per-wall planes of pylamp3d -- wall_flows (faces), wall_heat_values (nodes, ownership of the edges)
and wall_materials (faces, several columns per wall) -- pinned call by call: the exact message of every rejection and the exact
result of every accepted input.  nx = (5, 6, 7): the three extents differ, so a swapped axis cannot pass.  The planes are
(n_p - 1, n_q - 1) over faces and (n_p, n_q) over nodes, p < q the two other axes of the wall in z, x, y order:

    wall     faces    nodes
    z0, zL   (5, 6)   (6, 7)
    x0, xL   (4, 6)   (5, 7)
    y0, yL   (4, 5)   (5, 6)

No GPU and no library: the functions are NumPy only."""
import numpy as np
import pytest

from pylamp_amd import pylamp3d as P3

NX = (5, 6, 7)
FACES = [(5, 6), (4, 6), (4, 5)] * 2
NODES = [(6, 7), (5, 7), (5, 6)] * 2
SIX = "[z0, x0, y0, zL, xL, yL]"
WALLS = "z0, x0, y0, zL, xL, yL"


def _six(**by_name):
    return [by_name.get(k) for k in P3.WALL_NAMES]


def _arr(shape, **entries):
    """zeros(shape) with entries like i2j3=np.nan set."""
    a = np.zeros(shape)
    for k, v in entries.items():
        i, j = k[1:].split("j")
        a[int(i), int(j)] = v
    return a


def _ramp(shape, start=0.0):
    return start + np.arange(float(np.prod(shape))).reshape(shape)


def _assert_plane(got, want):
    assert isinstance(got, np.ndarray) and got.dtype == np.float64 and got.flags["C_CONTIGUOUS"]
    assert got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _assert_planes(got, want):
    assert isinstance(got, list) and len(got) == 6
    for g, w in zip(got, want):
        if w is None:
            assert g is None
        else:
            _assert_plane(g, np.asarray(w, dtype=np.float64))


# ---- rejections: (function, argument, who or None for the default, the whole message) -----------------------------------
ERRORS = {
    # wall_flows
    "flow-unknown-wall": ("wall_flows", {"top": 1.0}, None,
                          "3-D Stokes: the wall flow names a wall 'top' (the walls are %s)" % WALLS),
    "flow-unknown-wall-who": ("wall_flows", {"zL": 1.0, "Z0": 1.0}, "who",
                              "who: the wall flow names a wall 'Z0' (the walls are %s)" % WALLS),
    "flow-count-5": ("wall_flows", [None] * 5, None, "3-D Stokes: the wall flow needs six entries %s (got 5)" % SIX),
    "flow-count-7": ("wall_flows", (1.0,) * 7, "who", "who: the wall flow needs six entries %s (got 7)" % SIX),
    "flow-count-0": ("wall_flows", [], None, "3-D Stokes: the wall flow needs six entries %s (got 0)" % SIX),
    "flow-no-array": ("wall_flows", {"zL": "fast"}, None,
                      "3-D Stokes: the flow of wall zL needs the shape (nx - 1, ny - 1) = (5, 6) or a scalar (got an object that is no array)"),
    "flow-ragged": ("wall_flows", {"x0": [[1.0, 2.0], [3.0]]}, None,
                    "3-D Stokes: the flow of wall x0 needs the shape (nz - 1, ny - 1) = (4, 6) or a scalar (got an object that is no array)"),
    "flow-shape-z": ("wall_flows", {"z0": np.zeros((6, 5))}, None,
                     "3-D Stokes: the flow of wall z0 needs the shape (nx - 1, ny - 1) = (5, 6) or a scalar (got (6, 5))"),
    "flow-shape-x": ("wall_flows", {"xL": np.zeros((6, 4))}, None,
                     "3-D Stokes: the flow of wall xL needs the shape (nz - 1, ny - 1) = (4, 6) or a scalar (got (6, 4))"),
    "flow-shape-y": ("wall_flows", {"y0": np.zeros((5, 4))}, "who",
                     "who: the flow of wall y0 needs the shape (nz - 1, nx - 1) = (4, 5) or a scalar (got (5, 4))"),
    "flow-shape-nodes": ("wall_flows", {"yL": np.zeros((5, 6))}, None,
                         "3-D Stokes: the flow of wall yL needs the shape (nz - 1, nx - 1) = (4, 5) or a scalar (got (5, 6))"),
    "flow-shape-1d": ("wall_flows", {"zL": np.zeros(30)}, None,
                      "3-D Stokes: the flow of wall zL needs the shape (nx - 1, ny - 1) = (5, 6) or a scalar (got (30,))"),
    "flow-nan": ("wall_flows", {"x0": _arr((4, 6), i2j3=np.nan, i3j1=np.inf)}, None,
                 "3-D Stokes: wall x0 has a non-finite flow entry [2, 3] = nan"),
    "flow-inf": ("wall_flows", {"yL": _arr((4, 5), i3j4=-np.inf)}, "who", "who: wall yL has a non-finite flow entry [3, 4] = -inf"),
    "flow-nan-edge": ("wall_flows", {"xL": _arr((4, 6), i0j0=np.nan)}, None, "3-D Stokes: wall xL has a non-finite flow entry [0, 0] = nan"),
    "flow-nan-scalar": ("wall_flows", {"z0": np.nan}, None, "3-D Stokes: wall z0 has a non-finite flow entry [0, 0] = nan"),
    "flow-first-wall-wins": ("wall_flows", _six(z0=_arr((5, 6), i4j5=np.inf), x0=np.zeros((6, 4))), None,
                             "3-D Stokes: wall z0 has a non-finite flow entry [4, 5] = inf"),
    # wall_heat_values
    "heat-unknown-wall": ("wall_heat_values", {"top": 1.0}, None,
                          "3-D heat: the heat wall values name a wall 'top' (the walls are %s)" % WALLS),
    "heat-count-5": ("wall_heat_values", [None] * 5, None, "3-D heat: the heat wall values need six entries %s (got 5)" % SIX),
    "heat-count-7": ("wall_heat_values", (1.0,) * 7, "who", "who: the heat wall values need six entries %s (got 7)" % SIX),
    "heat-no-sequence": ("wall_heat_values", 3.0, None, "3-D heat: the heat wall values need six entries %s (got float)" % SIX),
    "heat-no-array": ("wall_heat_values", {"zL": "hot"}, None,
                      "3-D heat: the values of heat wall zL need the shape (nx, ny) = (6, 7) or a scalar (got an object that is no array)"),
    "heat-shape-z": ("wall_heat_values", {"z0": np.zeros((7, 6))}, None,
                     "3-D heat: the values of heat wall z0 need the shape (nx, ny) = (6, 7) or a scalar (got (7, 6))"),
    "heat-shape-x": ("wall_heat_values", {"xL": np.zeros((7, 5))}, None,
                     "3-D heat: the values of heat wall xL need the shape (nz, ny) = (5, 7) or a scalar (got (7, 5))"),
    "heat-shape-y": ("wall_heat_values", {"y0": np.zeros((6, 5))}, "who",
                     "who: the values of heat wall y0 need the shape (nz, nx) = (5, 6) or a scalar (got (6, 5))"),
    "heat-shape-faces": ("wall_heat_values", {"yL": np.zeros((4, 5))}, None,
                         "3-D heat: the values of heat wall yL need the shape (nz, nx) = (5, 6) or a scalar (got (4, 5))"),
    "heat-nan-z-corner": ("wall_heat_values", {"z0": _arr((6, 7), i0j0=np.nan)}, None,
                          "3-D heat: heat wall z0 has a non-finite entry [0, 0] = nan"),               # a z-wall owns all of its nodes
    "heat-nan-x-yedge": ("wall_heat_values", {"xL": _arr((5, 7), i0j3=np.nan, i2j0=np.inf, i3j6=np.nan)}, None,
                         "3-D heat: heat wall xL has a non-finite entry [2, 0] = inf"),               # an x-wall owns its y-edges, not rows 0, 4
    "heat-nan-y-interior": ("wall_heat_values", {"y0": _arr((5, 6), i0j2=np.nan, i3j0=np.nan, i3j1=-np.inf)}, "who",
                            "who: heat wall y0 has a non-finite entry [3, 1] = -inf"),                  # a y-wall owns neither
    "heat-nan-scalar-z": ("wall_heat_values", {"zL": np.inf}, None, "3-D heat: heat wall zL has a non-finite entry [0, 0] = inf"),
    "heat-nan-scalar-y": ("wall_heat_values", {"yL": np.nan}, None, "3-D heat: heat wall yL has a non-finite entry [1, 1] = nan"),
    # wall_materials
    "mat-dict": ("wall_materials", {"z0": {3: 1.0}}, None,
                 "3-D markers: the inflow material needs six entries %s, each None or a dict (got dict)" % SIX),
    "mat-empty-dict-as-six": ("wall_materials", {}, "who", "who: the inflow material needs six entries %s, each None or a dict (got dict)" % SIX),
    "mat-no-sequence": ("wall_materials", 3.0, None,
                        "3-D markers: the inflow material needs six entries %s, each None or a dict (got float)" % SIX),
    "mat-count-5": ("wall_materials", [None] * 5, None, "3-D markers: the inflow material needs six entries %s (got 5)" % SIX),
    "mat-count-7": ("wall_materials", ({},) * 7, "who", "who: the inflow material needs six entries %s (got 7)" % SIX),
    "mat-no-dict": ("wall_materials", _six(x0=1600.0), None,
                    "3-D markers: the inflow material of wall x0 needs a dict {column: value} or None (got float)"),
    "mat-no-dict-array": ("wall_materials", _six(yL=np.zeros((4, 5))), "who",
                          "who: the inflow material of wall yL needs a dict {column: value} or None (got ndarray)"),
    "mat-id": ("wall_materials", _six(z0={3: 1.0, 12: 7.0}), None,
               "3-D markers: the inflow material of wall z0 names TR__ID: the IDs are handed out by the refill and cannot be prescribed"),
    "mat-column-13": ("wall_materials", _six(xL={13: 1.0}), None,
                      "3-D markers: the inflow material of wall xL names an unknown column 13 (the tracer columns are the TR_* constants 0 ... 11)"),
    "mat-column-negative": ("wall_materials", _six(y0={-1: 1.0}), None,
                            "3-D markers: the inflow material of wall y0 names an unknown column -1 (the tracer columns are the TR_* constants 0 ... 11)"),
    "mat-column-str": ("wall_materials", _six(zL={"rho": 1.0}), "who",
                       "who: the inflow material of wall zL names an unknown column 'rho' (the tracer columns are the TR_* constants 0 ... 11)"),
    "mat-column-float": ("wall_materials", _six(zL={3.0: 1.0}), None,
                         "3-D markers: the inflow material of wall zL names an unknown column 3.0 (the tracer columns are the TR_* constants 0 ... 11)"),
    "mat-column-bool": ("wall_materials", _six(z0={True: 1.0}), None,
                        "3-D markers: the inflow material of wall z0 names an unknown column True (the tracer columns are the TR_* constants 0 ... 11)"),
    "mat-no-array": ("wall_materials", _six(zL={3: "hot"}), None,
                     "3-D markers: column 3 of the inflow material of wall zL needs the shape (nx - 1, ny - 1) = (5, 6) or a scalar (got an object that is no array)"),
    "mat-shape-z": ("wall_materials", _six(z0={0: 1.0, 3: np.zeros((6, 5))}), None,
                    "3-D markers: column 3 of the inflow material of wall z0 needs the shape (nx - 1, ny - 1) = (5, 6) or a scalar (got (6, 5))"),
    "mat-shape-x": ("wall_materials", _six(xL={np.int64(5): np.zeros((6, 4))}), None,
                    "3-D markers: column 5 of the inflow material of wall xL needs the shape (nz - 1, ny - 1) = (4, 6) or a scalar (got (6, 4))"),
    "mat-shape-y": ("wall_materials", _six(y0={11: np.zeros((5, 4))}), "who",
                    "who: column 11 of the inflow material of wall y0 needs the shape (nz - 1, nx - 1) = (4, 5) or a scalar (got (5, 4))"),
    "mat-shape-stacked": ("wall_materials", _six(yL={1: np.zeros((2, 4, 5))}), None,
                          "3-D markers: column 1 of the inflow material of wall yL needs the shape (nz - 1, nx - 1) = (4, 5) or a scalar (got (2, 4, 5))"),
    "mat-nan": ("wall_materials", _six(x0={3: 1.0, 0: _arr((4, 6), i1j5=np.nan, i2j0=np.inf)}), None,
                "3-D markers: column 0 of the inflow material of wall x0 has a non-finite value [1, 5] = nan"),
    "mat-inf-scalar": ("wall_materials", _six(yL={7: -np.inf}), "who",
                       "who: column 7 of the inflow material of wall yL has a non-finite value [0, 0] = -inf"),
    "mat-dict-order-wins": ("wall_materials", _six(z0={5: np.nan, 12: 1.0}), None,            # columns are checked in the dict's order
                            "3-D markers: column 5 of the inflow material of wall z0 has a non-finite value [0, 0] = nan"),
}


@pytest.mark.parametrize("case", sorted(ERRORS))
def test_rejection_message(case):
    fn, arg, who, message = ERRORS[case]
    with pytest.raises(Exception) as e:
        getattr(P3, fn)(arg, NX) if who is None else getattr(P3, fn)(arg, NX, who)
    assert type(e.value) is Exception
    assert str(e.value) == message


# ---- accepted inputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fn", ["wall_flows", "wall_heat_values", "wall_materials"])
def test_none_and_six_none(fn):
    f = getattr(P3, fn)
    assert f(None, NX) == [None] * 6
    assert f([None] * 6, NX) == [None] * 6
    assert f((None,) * 6, NX, "who") == [None] * 6


@pytest.mark.parametrize("fn, shapes", [("wall_flows", FACES), ("wall_heat_values", NODES)])
def test_planes_scalars_and_the_dict_by_name(fn, shapes):
    f = getattr(P3, fn)
    full = [_ramp(s, 100.0 * w) for w, s in enumerate(shapes)]
    _assert_planes(f(full, NX), full)
    _assert_planes(f(tuple(full), NX, "who"), full)
    _assert_planes(f(dict(zip(P3.WALL_NAMES, full)), NX), full)
    _assert_planes(f({}, NX), [None] * 6)
    # scalars are broadcast: Python and NumPy numbers, 0-d arrays, bools, numbers in a string (what np.array(..., float64) takes)
    got = f([1.5, None, np.float32(0.25), 2, np.array(-3.0), True], NX)
    _assert_planes(got, [np.full(shapes[0], 1.5), None, np.full(shapes[2], 0.25), np.full(shapes[3], 2.0), np.full(shapes[4], -3.0),
                         np.full(shapes[5], 1.0)])
    _assert_planes(f({"xL": "2.5"}, NX), [None, None, None, None, np.full(shapes[4], 2.5), None])
    # a dict by name in any order, with None for a wall
    got = f({"yL": full[5], "z0": 7, "x0": None}, NX)
    _assert_planes(got, [np.full(shapes[0], 7.0), None, None, None, None, full[5]])
    # nested lists, integers, a transposed (Fortran-ordered) view and a strided slice come back as contiguous float64 copies
    ints = np.arange(np.prod(shapes[1])).reshape(shapes[1])
    fview = np.asfortranarray(full[2])
    wide = _ramp((shapes[3][0], 2 * shapes[3][1]))
    got = f([full[0].tolist(), ints, fview, wide[:, ::2], None, None], NX)
    _assert_planes(got, [full[0], ints.astype(np.float64), full[2], np.ascontiguousarray(wide[:, ::2]), None, None])
    # the result never aliases the input
    src = full[4].copy()
    got = f({"xL": src}, NX)
    got[4][0, 0] = -1.0
    assert src[0, 0] == full[4][0, 0]


def test_flows_take_any_iterable_of_six():
    full = [_ramp(s) for s in FACES]
    _assert_planes(P3.wall_flows(iter(full), NX), full)
    _assert_planes(P3.wall_flows(np.zeros(6), NX), [np.zeros(s) for s in FACES])


def test_heat_entries_another_wall_owns_are_not_checked():
    """z-walls own their edges, then x-walls, then y-walls: rows 0 and nz - 1 of an x- or y-wall's plane, also columns 0 and nx - 1 of
    a y-wall's, are never read; NaN there is accepted and kept."""
    x = _ramp((5, 7)); x[0, :] = np.nan; x[4, :] = np.inf
    y = _ramp((5, 6)); y[0, :] = np.nan; y[4, :] = np.nan; y[:, 0] = -np.inf; y[:, 5] = np.nan
    got = P3.wall_heat_values({"x0": x, "xL": x, "y0": y, "yL": y}, NX)
    _assert_planes(got, [None, x, y, None, x, y])
    assert np.isnan(got[1][0]).all() and np.isinf(got[4][4]).all() and np.isnan(got[5][:, 5]).all()
    # the same entries on the flow's planes (all of them are read) are rejected
    with pytest.raises(Exception, match=r"wall x0 has a non-finite flow entry \[0, 0\] = nan"):
        P3.wall_flows({"x0": x[:4, :6]}, NX)


def test_material_columns_are_stacked_in_ascending_order():
    a3, a0, a11 = _ramp((4, 6), 300.0), _ramp((4, 6)), _ramp((4, 6), 1100.0)
    got = P3.wall_materials(_six(x0={3: a3, 11: a11, 0: a0}, zL={5: 2, np.int32(1): 0.5}, y0={}, yL={7: _ramp((4, 5)).tolist()}), NX, "who")
    assert [g is None for g in got] == [True, False, True, False, True, False]
    mask, planes = got[1]
    assert mask == (1 << 0) | (1 << 3) | (1 << 11) and type(mask) is int
    _assert_plane(planes, np.stack([a0, a3, a11]))
    mask, planes = got[3]
    assert mask == (1 << 1) | (1 << 5)
    _assert_plane(planes, np.stack([np.full((5, 6), 0.5), np.full((5, 6), 2.0)]))
    mask, planes = got[5]
    assert mask == 1 << 7
    _assert_plane(planes, _ramp((4, 5))[None])
    assert P3.wall_materials([{}] * 6, NX) == [None] * 6
    assert P3.TR__ID == 12
