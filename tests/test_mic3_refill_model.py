"""CPU checks of the 3-D census + refill: the new names exist, Simulation3 accepts the injection options, and the NumPy model the
GPU kernels are compared with (tests/mic3_refill_model.py) is the reference's rule: it equals oracle.inject exactly on a grid with
one cell layer along y and reproduces it layer by layer on a replicated set."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mic3_refill_model as R

NF, TR_ID = 13, 12


def test_header_bindings_and_module_expose_the_refill_names():
    txt = open(os.path.join(ROOT, "include", "pylamp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from pylamp_amd import _lib, pylamp3d as P3
    for n in ("pl3_resident_refill", "pl3_resident_advect"):
        assert re.search(r"\b%s\s*\(" % n, txt), "not declared: " + n
        assert n in _lib.SIGNATURES, "not bound: " + n
        assert hasattr(_lib.load(), n), "not exported: " + n
    assert re.search(r"\bpl3_resident_rk4\s*\(", txt)                  # keeps its place
    for n in ("refill", "advect"):
        assert callable(getattr(P3.Simulation3, n))
    o = P3.Options3()
    assert o.inject_seed == 12345 and o.inject_unique_ids is False and o.tracdens == 0 and o.tracdens_min == 0


def test_simulation3_accepts_the_injection_options():
    import torch
    from pylamp_amd import pylamp3d as P3
    nx, L = [5, 5, 5], [1.0, 1.0, 1.0]
    for kw in (dict(tracdens_min=3), dict(tracdens=4, tracdens_min=5), dict(tracdens=-1), dict(tracdens=2, tracdens_min=-1)):
        with pytest.raises(Exception, match="injection"):
            P3.Simulation3(nx, L, options=P3.Options3(**kw))
    try:
        sim = P3.Simulation3(nx, L, options=P3.Options3(tracdens=8, tracdens_min=4))
    except Exception as e:                 # without a GPU the constructor goes on to the context and fails there
        assert not torch.cuda.is_available(), e
        assert "injection" not in str(e), e
        assert re.search("no HIP device|no CPU fallback", str(e)), e
    else:
        sim.close()


def test_generator_is_a_uniform_of_its_counters_only():
    u = np.array([[R.inj_uniform(12345, c, q, 7) for q in range(40)] for c in range(50)])
    assert (u >= 0).all() and (u < 1).all() and np.unique(u).size == u.size
    assert abs(u.mean() - 0.5) < 0.03                                  # 2000 draws: sigma = 0.0065
    assert R.inj_uniform(12345, 3, 4, 7) == u[3, 4] and R.inj_uniform(12346, 3, 4, 7) != u[3, 4]
    assert R.inj_uniform(1, 0xFFFFFFFF, 0, 0) == R.inj_uniform(1, -1, 0, 0)       # a + 1 wraps at 2^32


def _thinned_2d(rng, nx2, L2, n, dens_lo=0.0):
    """n tracers, uniformly random, with the corner z < 0.4 Lz, x < 0.4 Lx thinned and two cells emptied; positive fields."""
    p = rng.random((n, 2)) * np.array(L2) * 0.999998 + 1e-6 * np.array(L2)
    corner = (p[:, 0] < 0.4 * L2[0]) & (p[:, 1] < 0.4 * L2[1])
    keep = ~corner | (rng.random(n) < 0.35)
    hz, hx = L2[0] / (nx2[0] - 1), L2[1] / (nx2[1] - 1)
    for ci, cj in ((1, 1), (5, 7)):
        keep &= ~((np.floor(p[:, 0] / hz) == ci) & (np.floor(p[:, 1] / hx) == cj))
    p = p[keep]
    f = rng.uniform(1.0, 2.0, (p.shape[0], NF)) * 10.0 ** rng.integers(0, 20, NF)
    f[:, TR_ID] = rng.permutation(p.shape[0]) + 100.0
    return p, f


def test_model_equals_the_2d_oracle_on_one_cell_layer(oracle):
    """ny = 2: the 3-D cell number is the 2-D one.  The oracle's rand(m, 2) for the next deficient cell is fed from the model's
    generator; positions (z, x), IDs and fields of the new rows must then be EQUAL, the NaN rows of the empty cells included."""
    rng = np.random.default_rng(11)
    nx2 = [9, 11]; L2 = [660e3, 820e3]
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    p2, f2 = _thinned_2d(rng, nx2, L2, 520)
    n = p2.shape[0]
    g3 = g2 + [np.array([0.0, 50e3])]
    p3 = np.insert(p2, 2, rng.uniform(1e3, 49e3, n), axis=1)
    seed, it, dens, dmin = 777, 4, 9, 5
    x, f, v, info = R.refill(p3, f2, g3, dens, dmin, seed, it)
    cells = list(info["cells"]); calls = []

    def rand(m, dim):
        c = cells[len(calls)]; calls.append(c)
        return np.array([[R.inj_uniform(seed, c, q, 3 * it + d) for d in range(dim)] for q in range(m)]).reshape(m, dim)
    ox, of, oinfo = oracle.inject(p2.copy(), f2.copy(), g2, nx2, L2, dens, dmin, rand=rand)
    assert np.array_equal(oinfo["cells"], info["cells"]) and np.array_equal(oinfo["n_missing"], info["need"])
    assert oinfo["n_injected"] == info["ninjected"] > 100 and info["nrefilled"] >= 10 and info["nempty"] >= 2
    new = info["new"]
    assert new.sum() == info["ninjected"] and x.shape[0] == n + info["ninjected"]
    assert np.array_equal(x[new][:, :2], ox[n:])                       # same cells in the same order, same ordinals
    assert np.array_equal(f[new], of[n:], equal_nan=True)
    assert np.isnan(f[new]).any() and not np.isnan(f[new][:, TR_ID]).any()
    assert (x[new][:, 2] >= 0).all() and (x[new][:, 2] < 50e3).all() and not v[new].any()
    # residents: the caller's tracers, stably sorted by cell
    assert np.array_equal(np.sort(f[~new][:, TR_ID]), np.sort(f2[:, TR_ID]))
    c_res = info["cell"][~new]
    assert (np.diff(info["cell"]) >= 0).all() and np.array_equal(info["census"].ravel(), np.bincount(info["cell"], minlength=80))
    o = np.argsort(R.cells_of(p3, g3)[0], kind="stable")
    assert np.array_equal(x[~new], p3[o]) and np.array_equal(c_res, R.cells_of(p3, g3)[0][o])
    # unique IDs: max + 1, + 2, ... in the order of the new rows
    _, fu, _, _ = R.refill(p3, f2, g3, dens, dmin, seed, it, unique_ids=True)
    assert np.array_equal(fu[new][:, TR_ID], f2[:, TR_ID].max() + 1 + np.arange(info["ninjected"]))
    # nothing to do
    x0, f0, _, i0 = R.refill(p3, f2, g3, dens, 0, seed, it)
    assert i0["ninjected"] == 0 and np.array_equal(x0, p3[o]) and np.array_equal(f0, f2[o])


def test_model_reproduces_the_2d_oracle_layer_by_layer_on_a_replicated_set(oracle):
    """A 2-D set copied r times into each of four y layers, densities multiplied by r: every layer has the oracle's deficient
    cells, r times its deficits and its means.  Bound: the means are the same positive values summed in another order and
    number -- fewer than T = r tracdens summands, each sum off by at most (k - 1) 2^-53 relative, plus the divisions: 2 T 2^-52
    covers both sides."""
    rng = np.random.default_rng(12)
    nx2 = [9, 11]; L2 = [660e3, 820e3]; r = 3; ncy = 4
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    p2, f2 = _thinned_2d(rng, nx2, L2, 520)
    n = p2.shape[0]
    g3 = g2 + [np.linspace(0, 200e3, ncy + 1)]
    ys = (np.repeat(np.arange(ncy), r) + rng.uniform(0.1, 0.9, ncy * r)) * 50e3
    p3 = np.concatenate([np.insert(p2, 2, y, axis=1) for y in ys])
    f3 = np.tile(f2, (ncy * r, 1)); f3[:, TR_ID] = np.arange(f3.shape[0])
    dens, dmin = 9, 5
    x, f, v, info = R.refill(p3, f3, g3, r * dens, r * dmin, 5, 1)
    _, of, oinfo = oracle.inject(p2.copy(), f2.copy(), g2, nx2, L2, dens, dmin, rand=lambda m, d: np.zeros((m, d)))
    omean = {c: of[n + int(np.sum(oinfo["n_missing"][:q]))] for q, c in enumerate(oinfo["cells"])}
    assert info["ninjected"] == ncy * r * oinfo["n_injected"] and info["nrefilled"] == ncy * len(oinfo["cells"])
    bound = 2 * (r * dens) * 2.0 ** -52
    worst = 0.0
    cols = [q for q in range(NF) if q != TR_ID]
    for k in range(ncy):
        mine = info["cells"] % ncy == k
        assert np.array_equal(info["cells"][mine] // ncy, oinfo["cells"])
        assert np.array_equal(info["need"][mine], r * oinfo["n_missing"])
        rows = np.where(info["new"] & (info["cell"] % ncy == k))[0]
        for t in rows:
            a, b = f[t, cols], omean[info["cell"][t] // ncy][cols]
            assert np.array_equal(np.isnan(a), np.isnan(b))
            if not np.isnan(b).any():
                worst = max(worst, float(np.max(np.abs(a - b) / np.abs(b))))
    print("replicated means: worst relative difference %.3g (bound %.3g)" % (worst, bound))
    assert worst <= bound
