"""CPU checks of the 3-D fence-off deletion: the new names exist, Simulation3 accepts exactly one combination of the two options,
and the NumPy model the GPU is compared with (tests/mic3_delete_model.py) is the reference's rule: on a grid with one cell layer
along y its survivors and counts are those of oracle.fence_and_delete with the fence off."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import mic3_delete_model as D
import mic3_refill_model as R

NF, TR_ID = 13, 12


def test_header_bindings_and_module_expose_the_deletion_names():
    txt = open(os.path.join(ROOT, "include", "pylamp_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from pylamp_amd import _lib, pylamp3d as P3
    for n in ("pl3_mic_set_deletion", "pl3_mic_get_deletion", "pl3_tracers_removed"):
        assert re.search(r"\b%s\s*\(" % n, code), "not declared: " + n
        assert n in _lib.SIGNATURES, "not bound: " + n
        assert hasattr(_lib.load(), n), "not exported: " + n
    assert "fence == 0 on a context without pl3_mic_set_deletion" in re.sub(r"\s*\n \*\s*", " ", txt)
    assert [f for f, _ in _lib.Step3Report._fields_][-2:] == ["ms_total", "nremoved"]
    for n in ("set_marker_deletion", "marker_deletion", "tracers_removed"):
        assert callable(getattr(P3.Context3, n))
    assert P3.Options3().marker_deletion is False and P3.Options3(marker_deletion=True).marker_deletion is True


def test_simulation3_takes_the_two_switches_together_or_not_at_all():
    """Both rejections are raised before a context is made: no GPU is needed."""
    from pylamp_amd import pylamp3d as P3
    nx, L = [5, 5, 5], [1.0, 1.0, 1.0]
    with pytest.raises(Exception, match=r"fence-off.*marker_deletion = True$"):
        P3.Simulation3(nx, L, options=P3.Options3(tracs_fence_enabled=False))
    with pytest.raises(Exception, match=r"marker_deletion = True needs tracs_fence_enabled = False"):
        P3.Simulation3(nx, L, options=P3.Options3(marker_deletion=True))


def test_outside_is_the_rule_of_the_header():
    L = [2.0, 3.0, 5.0]
    x = np.array([[1.0, 1.0, 1.0], [0.0, 1.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, np.nextafter(5.0, 0.0)], [np.nextafter(0.0, 1.0), 1.0, 1.0],
                  [np.nan, 1.0, 1.0], [np.nan, -1.0, 1.0], [1.0, 1.0, 5.5], [-1e-300, 1.0, 1.0], [1.0, np.inf, 1.0]])
    assert D.outside(x, L).tolist() == [False, True, True, False, False, False, True, True, True, True]


def test_model_equals_the_2d_oracle_deletion_on_one_cell_layer(oracle):
    """ny = 2 and every y inside the layer: the 3-D rule is the 2-D one.  Tracers sit inside, beyond each of the four walls and
    exactly on them; the survivors (compared by their full rows), the number removed and the census must be EQUAL."""
    rng = np.random.default_rng(31)
    nx2 = [9, 11]; L2 = [660e3, 820e3]
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    n = 900
    p2 = (rng.random((n, 2)) * 1.2 - 0.1) * np.array(L2)                 # a tenth of the box beyond every wall
    p2[:6] = [[0.0, 1e5], [L2[0], 1e5], [1e5, 0.0], [1e5, L2[1]], [np.nextafter(L2[0], 0), 1e5], [np.nextafter(0.0, 1.0), 1e5]]
    f2 = rng.uniform(1.0, 2.0, (n, NF)); f2[:, TR_ID] = rng.permutation(n) + 100.0
    v2 = rng.standard_normal((n, 2))
    g3 = g2 + [np.array([0.0, 50e3])]
    p3 = np.insert(p2, 2, rng.uniform(1e3, 49e3, n), axis=1)
    v3 = np.insert(v2, 2, rng.standard_normal(n), axis=1)
    ox, of, ov, nout = oracle.fence_and_delete(p2.copy(), f2.copy(), v2.copy(), L2, fence_enabled=False)
    x, f, v, info, kept = D.sort_delete_refill(p3, f2, g3, tr_v=v3)
    assert 100 < nout == info["nremoved"] == n - x.shape[0] and kept[4] and kept[5] and not kept[:4].any()
    assert np.array_equal(f2[kept], of) and np.array_equal(p2[kept], ox) and np.array_equal(v2[kept], ov)
    # the survivors, stably sorted by cell, every row whole
    o = np.argsort(R.cells_of(p3[kept], g3)[0], kind="stable")
    assert np.array_equal(x, p3[kept][o]) and np.array_equal(f, f2[kept][o]) and np.array_equal(v, v3[kept][o])
    assert info["ninjected"] == 0 and not info["new"].any()
    _, _, cnt = oracle.census(ox, nx2, L2)
    assert np.array_equal(info["census"].ravel(), cnt) and cnt.sum() == n - nout


def test_the_refill_of_a_deleting_sort_sees_the_survivors(oracle):
    """Deletion, then the oracle's census + refill on what is left, against the model's one call: same deficient cells, same
    deficits, and the IDs number from the largest ID among the survivors -- the holder of the largest ID of all leaves."""
    rng = np.random.default_rng(32)
    nx2 = [7, 6]; L2 = [6.0, 5.0]
    g2 = [np.linspace(0, L2[0], nx2[0]), np.linspace(0, L2[1], nx2[1])]
    n = 200
    p2 = (rng.random((n, 2)) * 1.1 - 0.05) * np.array(L2)
    f2 = rng.uniform(1.0, 2.0, (n, NF)); f2[:, TR_ID] = rng.permutation(n).astype(float)
    p2[np.argmax(f2[:, TR_ID])] = [-0.5, 2.5]
    g3 = g2 + [np.array([0.0, 1.0])]
    p3 = np.insert(p2, 2, rng.uniform(0.1, 0.9, n), axis=1)
    seed, it, dens, dmin = 5, 2, 9, 5                                    # (fewer than 8 residents: NumPy's mean sums them one after the other too)
    x, f, v, info, kept = D.sort_delete_refill(p3, f2, g3, dens, dmin, seed, it)
    ox, of, _, nout = oracle.fence_and_delete(p2.copy(), f2.copy(), np.zeros((n, 2)), L2, fence_enabled=False)
    cells = list(info["cells"]); calls = []

    def rand(m, dim):
        c = cells[len(calls)]; calls.append(c)
        return np.array([[R.inj_uniform(seed, c, q, 3 * it + d) for d in range(dim)] for q in range(m)]).reshape(m, dim)
    ix, if_, iinfo = oracle.inject(ox.copy(), of.copy(), g2, nx2, L2, dens, dmin, rand=rand)
    assert nout == info["nremoved"] > 10 and iinfo["n_injected"] == info["ninjected"] > 0
    assert np.array_equal(iinfo["cells"], info["cells"]) and np.array_equal(iinfo["n_missing"], info["need"])
    new = info["new"]
    assert np.array_equal(f[new], if_[ox.shape[0]:], equal_nan=True) and np.array_equal(x[new][:, :2], ix[ox.shape[0]:])
    assert f[new][:, TR_ID].min() == f2[kept][:, TR_ID].max() < f2[:, TR_ID].max()
