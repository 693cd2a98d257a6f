"""Inputs of the inflow-material tests (plain helper module, no fixtures, no project code): shared by tests/test_mic3_inflow_model.py,
which checks on the CPU that they reach every branch of the rule, and tests/test_hip_mic3_inflow.py, which runs them on the GPU.

Grids.  Every spacing is a power of two, on the regular grid (one power) and on the graded one (1 : 2 : 4 and back).  A new tracer
sits at g + u h; with h a power of two u h is exact, so the kernel's fused multiply-add and NumPy's multiply-then-add round the same
sum once and the positions can be compared bit for bit (on a general grid they differ by an ulp, tests/test_hip_mic3_refill.py).
The graded spacings are no multiple of a regular grid's, so the regular-grid cell formula would put tracers into other cells than
the search does.

Shapes.  [6, 5, 7] with tracdens 8 / 4: odd sizes, every wall layer distinct.  [5, 5, 5] with tracdens 140 / 70: the smallest node
set a context accepts, with cells whose residents (65 .. 69) and deficit (71 .. 75) both exceed one 64-lane wave.
"""
import numpy as np

import mic3_inflow_model as I

NF, TR_ID = 13, 12
TR_ETA, TR_MRK, TR_TMP, TR_HCD, TR_RH0, TR_ALP, TR_MAT = 1, 2, 3, 4, 6, 7, 8
SHAPES = {"small": ([6, 5, 7], 8, 4), "crowded": ([5, 5, 5], 140, 70)}
SEED, IT = 777, 5
U = 2.0 ** -30                                                # m/s


def grid_of(shape, graded):
    nx = SHAPES[shape][0]
    out = []
    for n in nx:
        if graded:
            up = [1.0, 2.0, 4.0]
            h = (up + up[::-1])[:n - 1] if n - 1 > 3 else up[:n - 1]
            h = np.array(h) * 2.0 ** 11
        else:
            h = np.full(n - 1, 2.0 ** 12)
        out.append(np.concatenate([[0.0], np.cumsum(h)]))
    return out


def flow_of(shape):
    """z0 and zL the same uniform U: in at z0, out at zL.  x0 and xL share one profile over (z, y) that takes both signs and is never
    0, so x0 takes inflow where it is positive and xL where it is negative; the fluxes of each pair cancel exactly on any grid."""
    nx = SHAPES[shape][0]
    i, j = np.meshgrid(np.arange(nx[0] - 1), np.arange(nx[2] - 1), indexing="ij")
    prof = U * np.where((i + j) % 2 == 0, 1.0, -1.0) * (1.0 + 0.25 * i + 0.125 * j)
    return [U, prof, None, U, prof.copy(), None]


def material_of(shape):
    """Different column sets per wall; x0 with planes that vary over the wall, the others scalars.  zL is outflow and yL has no flow:
    their materials never fire."""
    nx = SHAPES[shape][0]
    i, j = np.meshgrid(np.arange(nx[0] - 1), np.arange(nx[2] - 1), indexing="ij")
    return [{TR_MAT: 2.0, TR_TMP: 1500.0},
            {TR_RH0: 3000.0 + 10.0 * i + j, TR_MRK: 100.0 + i * (nx[2] - 1) + j},
            None,
            {TR_HCD: 9.0},
            {TR_ETA: 1e21, TR_MAT: 3.0, TR_TMP: 300.0},
            {TR_ALP: 7.0}]


def planes_of(shape, material):
    """{column: plane} per wall, scalars broadcast: the form the model takes."""
    nx = SHAPES[shape][0]
    out = []
    for w, m in enumerate(material):
        if m is None:
            out.append(None)
            continue
        p, q = I.AXES[w % 3]
        out.append({c: np.broadcast_to(np.asarray(v, dtype=np.float64), (nx[p] - 1, nx[q] - 1)) for c, v in m.items()})
    return out


def flow_planes(shape, flow):
    nx = SHAPES[shape][0]
    return [None if f is None else np.broadcast_to(np.asarray(f, dtype=np.float64), (nx[I.AXES[w % 3][0]] - 1, nx[I.AXES[w % 3][1]] - 1))
            for w, f in enumerate(flow)]


def tracers_of(shape, graded):
    """Per cell a seeded count from 0 to tracdens, zeros included, uniform inside the cell (never on a face); the crowded shape
    also gets cells with 65 .. 69 residents on the inflow walls.  Positive values in every column, IDs a permutation from 100."""
    nx, dens, dmin = SHAPES[shape]
    grid = grid_of(shape, graded)
    rng = np.random.default_rng(31 + len(shape) + (7 if graded else 0))
    nc = [n - 1 for n in nx]
    cnt = rng.integers(0, dens + 1, nc)
    cnt[0, 1, 2] = 0; cnt[1, 0, 1] = 0; cnt[2, nc[1] - 1, 1] = 0          # emptied cells on z0, on x0 (profile > 0) and on xL (< 0)
    cnt[2, 0, 0] = 1; cnt[1, 0, 0] = 2                                    # x0 once more where it flows in, and where it flows out
    if shape == "crowded":
        cnt[0, 2, 1] = 67; cnt[0, 0, 0] = 65; cnt[1, nc[1] - 1, 0] = 69   # z0; the edge z0 / x0; xL where the profile is negative
    xs = []
    for c in np.ndindex(*nc):
        u = 2.0 ** -10 + (1.0 - 2.0 ** -9) * rng.random((int(cnt[c]), 3))
        xs.append(np.stack([grid[d][c[d]] + u[:, d] * (grid[d][c[d] + 1] - grid[d][c[d]]) for d in range(3)], 1))
    x = np.concatenate(xs)
    x = x[rng.permutation(x.shape[0])]
    f = rng.uniform(1.0, 2.0, (x.shape[0], NF)) * 10.0 ** rng.integers(0, 20, NF)
    f[:, TR_ID] = rng.permutation(x.shape[0]) + 100.0
    return x, f


def model(shape, graded, unique, material="default", flow="default"):
    x, f = tracers_of(shape, graded)
    _, dens, dmin = SHAPES[shape]
    mat = material_of(shape) if material == "default" else material
    fl = flow_of(shape) if flow == "default" else flow
    return I.refill(x, f, grid_of(shape, graded), dens, dmin, SEED, IT, unique_ids=unique,
                    material=None if mat is None else planes_of(shape, mat), flow=None if fl is None else flow_planes(shape, fl), search=graded)
