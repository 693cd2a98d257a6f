"""The inflow material of the 3-D refill on the CPU: the option and its normalisation (pylamp3d.wall_materials), the NumPy model
tests/mic3_inflow_model.py against the plain refill model, and the inputs of the GPU cases (tests/mic3_inflow_cases.py): they must
reach every branch of the rule that include/pylamp_hip.h states at pl3_mic_set_inflow."""
import functools

import numpy as np
import pytest

import mic3_inflow_cases as K
import mic3_inflow_model as I
import mic3_refill_model as R
import mic3_rect_model as S

CASES = [(shape, graded) for shape in K.SHAPES for graded in (False, True)]


@functools.lru_cache(maxsize=None)
def _model(shape, graded, unique=False):
    return K.model(shape, graded, unique)


def test_options3_takes_bcinflow():
    from pylamp_amd import pylamp3d as P3
    assert P3.Options3().bcinflow is None
    m = [{P3.TR_MAT: 2}, None, None, None, None, None]
    assert P3.Options3(bcinflow=m).bcinflow is m


def test_wall_materials_normalises_scalars_and_planes():
    from pylamp_amd import pylamp3d as P3
    from pylamp_amd.pylamp_const import TR_MRK, TR_RH0
    nx = [5, 6, 7]
    assert P3.wall_materials(None, nx) == [None] * 6
    plane = np.arange(4.0 * 6).reshape(4, 6)
    out = P3.wall_materials([{P3.TR_TMP: 1500, P3.TR_MAT: 2.0}, {TR_RH0: plane, TR_MRK: 5}, None, {}, None, {P3.TR_RHO: np.float32(3)}], nx)
    assert out[2] is None and out[3] is None and out[4] is None
    mask, a = out[0]
    assert mask == (1 << P3.TR_TMP) | (1 << P3.TR_MAT) and a.shape == (2, 5, 6) and a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    assert (a[0] == 1500.0).all() and (a[1] == 2.0).all()                   # ascending column order: TR_TMP = 3 before TR_MAT = 8
    mask, a = out[1]
    assert mask == (1 << TR_MRK) | (1 << TR_RH0) and a.shape == (2, 4, 6)
    assert (a[0] == 5.0).all() and np.array_equal(a[1], plane)
    mask, a = out[5]
    assert mask == 1 and a.shape == (1, 4, 5) and (a == 3.0).all()


def test_wall_materials_rejects_by_name():
    from pylamp_amd import pylamp3d as P3
    nx = [5, 6, 7]
    who = "somebody"
    with pytest.raises(Exception, match=r"somebody: the inflow material needs six entries \[z0, x0, y0, zL, xL, yL\] \(got 5\)"):
        P3.wall_materials([None] * 5, nx, who)
    with pytest.raises(Exception, match=r"somebody: the inflow material needs six entries .* \(got dict\)"):
        P3.wall_materials({P3.TR_MAT: 2}, nx, who)
    with pytest.raises(Exception, match=r"somebody: the inflow material of wall x0 needs a dict \{column: value\} or None \(got float\)"):
        P3.wall_materials([None, 3.0, None, None, None, None], nx, who)
    with pytest.raises(Exception, match=r"somebody: column 3 of the inflow material of wall y0 needs the shape \(nz - 1, nx - 1\) = \(4, 5\) or a scalar \(got \(5, 4\)\)"):
        P3.wall_materials([None, None, {P3.TR_TMP: np.zeros((5, 4))}, None, None, None], nx, who)
    with pytest.raises(Exception, match=r"somebody: the inflow material of wall zL names TR__ID: the IDs are handed out by the refill"):
        P3.wall_materials([None, None, None, {P3.TR__ID: 1.0}, None, None], nx, who)
    for key in (13, -1, "TR_MAT", 2.5):
        with pytest.raises(Exception, match=r"somebody: the inflow material of wall z0 names an unknown column .* \(the tracer columns are the TR_\* constants 0 \.\.\. 11\)"):
            P3.wall_materials([{key: 1.0}, None, None, None, None, None], nx, who)
    bad = np.ones((5, 6)); bad[2, 3] = np.inf
    with pytest.raises(Exception, match=r"somebody: column 8 of the inflow material of wall z0 has a non-finite value \[2, 3\] = inf"):
        P3.wall_materials([{P3.TR_MAT: bad}, None, None, None, None, None], nx, who)
    with pytest.raises(Exception, match=r"column 0 of the inflow material of wall xL has a non-finite value \[0, 0\] = nan"):
        P3.wall_materials([None, None, None, None, {P3.TR_RHO: np.nan}, None], nx, who)


@pytest.mark.parametrize("shape,graded", CASES)
def test_without_a_material_the_model_is_the_refill_model(shape, graded):
    x, f = K.tracers_of(shape, graded)
    _, dens, dmin = K.SHAPES[shape]
    base = (S.refill if graded else R.refill)(x, f, K.grid_of(shape, graded), dens, dmin, K.SEED, K.IT)
    for material, flow in ((None, "default"), ([None] * 6, "default"), ("default", None)):
        got = K.model(shape, graded, False, material=material, flow=flow)
        for a, b in zip(got[:3], base[:3]):
            assert np.array_equal(a, b, equal_nan=True)
        assert got[3]["ninflow"] == 0 and not got[3]["inflow"].any()
        for k in ("ninjected", "nrefilled", "nempty", "mincount"):
            assert got[3][k] == base[3][k]


@pytest.mark.parametrize("shape,graded", CASES)
def test_the_gpu_cases_reach_every_branch(shape, graded):
    """(i) an inflow tracer, (ii) a new tracer of an inflow cell that keeps the mean because a resident is nearer the wall, (iii) an
    emptied inflow cell, (iv) an edge cell that qualifies for two walls, (v) a refilled cell on a material wall whose face has outward
    flow, (vi) a refilled cell on a material wall without any flow -- and, in the crowded shape, an inflow cell whose residents and
    deficit both exceed 64.  The positions of the model are exact sums on these grids (one rounding), and no new tracer ties dmin."""
    x, f, v, info = _model(shape, graded)
    nx, dens, dmin = K.SHAPES[shape]
    new, cell, infl = info["new"], info["cell"], info["inflow"]
    wall = dict(zip(info["cells"].tolist(), info["wall"].tolist()))
    why = dict(zip(info["cells"].tolist(), info["why"]))
    in_cell = np.array([wall.get(int(c), -1) >= 0 for c in cell])
    res = np.bincount(cell[~new], minlength=int(np.prod([n - 1 for n in nx])))
    assert infl.any() and info["ninflow"] == infl.sum() and not infl[~new].any() and in_cell[infl].all()           # (i)
    assert (new & in_cell & ~infl).any()                                                                              # (ii)
    empty = [c for c in wall if wall[c] >= 0 and res[c] == 0]
    assert empty and all(infl[(cell == c) & new].all() and ((cell == c) & new).sum() == dens for c in empty)          # (iii)
    assert any(y.count("in") >= 2 for y in why.values())                                                              # (iv)
    assert any("outward" in y for y in why.values())                                                                  # (v)
    assert any("noflow" in y for y in why.values())                                                                   # (vi)
    assert set(info["wall"].tolist()) >= {-1, 0, 1, 4} and not {2, 3, 5} & set(info["wall"].tolist())
    # an inflow cell of x0 and one of xL: the profile decides, and the planes of x0 give every cell its own value
    mrk = f[infl & np.isin(cell, [c for c in wall if wall[c] == 1]), K.TR_MRK]
    assert np.unique(mrk).size > 1
    # the prescribed columns are finite in the emptied inflow cells, the others are 0/0
    for c in empty:
        rows = (cell == c) & new
        cols = [int(k) for k in K.material_of(shape)[wall[c]]]
        rest = [q for q in range(K.NF) if q not in cols and q != K.TR_ID]
        assert np.isfinite(f[rows][:, cols]).all() and np.isnan(f[rows][:, rest]).all()
    if shape == "crowded":
        assert any(wall[c] >= 0 and 64 < res[c] < dmin and dens - res[c] > 64 for c in wall)
    # no new tracer of an inflow cell sits within 2^-20 of a cell width of dmin: an ulp cannot flip the decision
    grid = K.grid_of(shape, graded)
    dm = dict(zip(info["cells"].tolist(), info["dmin"].tolist()))
    for c in wall:
        if wall[c] < 0 or not np.isfinite(dm[c]):
            continue
        a = wall[c] % 3
        rows = (cell == c) & new
        s = x[rows, a] - grid[a][0] if wall[c] < 3 else grid[a][-1] - x[rows, a]
        assert np.abs(s - dm[c]).min() > 2.0 ** -20 * 2.0 ** 11


def test_the_id_rule_does_not_change_the_inflow_set():
    a = _model("small", False, False)
    b = _model("small", False, True)
    assert np.array_equal(a[3]["inflow"], b[3]["inflow"]) and np.array_equal(a[0], b[0])
    cols = [q for q in range(K.NF) if q != K.TR_ID]
    assert np.array_equal(a[1][:, cols], b[1][:, cols], equal_nan=True) and not np.array_equal(a[1][:, K.TR_ID], b[1][:, K.TR_ID])
