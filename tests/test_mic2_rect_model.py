"""CPU: the oracle's rect_search mode (np.searchsorted, np.add.at; "defined here") against the plain per-tracer statement of the
rectilinear rule in tests/mic2_rect_model.py (bisect, math.fsum), on the inputs of the GPU stage tests
(tests/mic2_rect_cases.py): trac2grid schemes 5, 6, 2 on the four target sets, grid2trac LINEAR and VELDIV, RK4.

Bounds.  The model's node sums are exactly rounded; the oracle adds the same float64 terms one after the other.  For m terms of
one sign the naive sum is off by at most (m - 1) eps relative, so a weighted mean acc / wsum is within 2 (m + 1) eps of the
model's, relative (all tracer columns here are >= 0), and exp(S / W) within that times max |ln eta| (51 here).  m is the largest
number of contributions any node receives, taken from the model.  Tracers beyond an end add the rounding of their in-cell
coordinate: the oracle builds the extended nodes one by one (c - h, (c - h) - h ...), the rule takes c + f h; each differs from
the exact node by a few eps |c|, i.e. a few eps |c| / h in the weight, and a weight error dw moves a mean by at most dw times the
spread of the values over the mean (< 1 for the arithmetic columns, < 7 in ln eta).  The gathers have no long sums: a few
roundings per term, bounds of 64 eps of the largest value.
"""
import numpy as np
import pytest

from conftest import maxrel, pointrel
import mic2_rect_cases as K
import mic2_rect_model as M

EPS = 2.0 ** -52
# (result name, tracer column, scheme, target set)
HEAT = (("rho", K.TR_RH0, 5, "nodes"), ("etas", K.TR_ET0, 6, "nodes"), ("cp", K.TR_HCP, 5, "nodes"), ("f_T", K.TR_TMP, 5, "nodes"),
        ("H", K.TR_IHT, 5, "nodes"), ("mat", K.TR_MAT, 5, "nodes"), ("etan", K.TR_ET0, 6, "centres"), ("etan2", K.TR_ET0, 2, "centres"),
        ("kz", K.TR_HCD, 5, "zmid"), ("kx", K.TR_HCD, 5, "xmid"))


def _scatter_bounds(grid, X, m):
    far = max(float(np.abs(X[:, d]).max()) / float(np.diff(grid[d]).min()) for d in range(2))
    outside = any((X[:, d] < 0).any() or (X[:, d] > grid[d][-1]).any() for d in range(2))
    arith = 2 * (m + 1) * EPS + (16 * EPS * far if outside else 0.0)
    geom = 2 * (m + 1) * EPS * 51.0 + (16 * EPS * far * 7.0 if outside else 0.0)
    return arith, geom


@pytest.mark.parametrize("name", ["19x39", "11x69", "5x5", "lines", "outside"])
def test_oracle_trac2grid_equals_the_plain_model(oracle, name):
    nx, L, grid, X, F = K.case(name)
    tg = K.targets(grid)
    assert K.share_off_regular(grid, X) > 0.5
    worst = {}
    for tname, tgrid in tg.items():
        sel = [h for h in HEAT if h[3] == tname]
        cols = [h[1] for h in sel]; sch = [h[2] for h in sel]
        with oracle.rect_search():
            ref = oracle.trac2grid(X, F[:, cols], tgrid, nx, sch)
        mod, count = M.trac2grid(X, F[:, cols], tgrid, sch)
        arith, geom = _scatter_bounds(grid, X, int(count.max()))
        for h, r, q in zip(sel, ref, mod):
            err = pointrel(r, q) if h[2] & 2 else maxrel(r, q)          # (both require identical NaN masks)
            worst[h[0]] = (err, geom if h[2] & 2 else arith)
            if name != "11x69" and name != "5x5":
                assert np.isnan(q).any(), h[0]                          # the holes of the population reach every target set
    print("  ".join("%s %.1e/%.1e" % (k, e, b) for k, (e, b) in worst.items()))
    for k, (e, b) in worst.items():
        assert e <= b, (k, e, b)


def test_last_coordinate_rule_with_tracers_beyond_it(oracle):
    """A marker exactly on the last coordinate belongs to the last cell (a = 1) also when other markers lie beyond that
    coordinate -- visible in the UNWEIGHTED schemes, which count the marker at the two nodes of its cell."""
    nx, L, grid, X, _ = K.case("5x5")
    rng = np.random.default_rng(3)
    extra = np.concatenate([K.outside_tracers(grid, rng, 64),
                            [(L[0], 0.3 * L[1]), (0.4 * L[0], L[1]), (L[0], L[1]), (L[0], grid[1][2]), (0.0, L[1])]])
    X, F = K.with_extra(X, L, extra, rng)
    cols = [K.TR_RH0, K.TR_ET0, K.TR_HCD, K.TR_ET0]; sch = [5, 6, 1, 2]
    with oracle.rect_search():
        ref = oracle.trac2grid(X, F[:, cols], grid, nx, sch)
    mod, count = M.trac2grid(X, F[:, cols], grid, sch)
    arith, geom = _scatter_bounds(grid, X, int(count.max()))
    for s, r, q in zip(sch, ref, mod):
        err = pointrel(r, q) if s & 2 else maxrel(r, q)
        print("scheme %d: %.2e" % (s, err))
        assert err <= (geom if s & 2 else arith), s


@pytest.mark.parametrize("name", ["lines", "outside"])
def test_oracle_grid2trac_equals_the_plain_model(oracle, name):
    nx, L, grid, X, F = K.case(name)
    rng = np.random.default_rng(5)
    T = 1500 + 300 * rng.standard_normal(nx)
    with oracle.rect_search():
        ref = oracle.grid2trac(X, grid, [T], nx, defval=-7.0)
    mod, n_out = M.grid2trac_linear(X, grid, [T], defval=-7.0)
    assert n_out == int((ref[:, 0] == -7.0).sum()) and n_out >= (11 if name == "lines" else 250)
    assert np.array_equal(ref[:, 0] == -7.0, mod[:, 0] == -7.0)
    assert maxrel(ref, mod) < 64 * EPS
    # stopOnError: raised exactly when a tracer is outside (at or beyond the last coordinate included)
    with oracle.rect_search():
        with pytest.raises(Exception, match="stopOnError"):
            oracle.grid2trac(X, grid, [T], nx, stop_on_error=True)
        Xi = K.case("lines-inside")[3]
        assert M.grid2trac_linear(Xi, grid, [T])[1] == 0
        oracle.grid2trac(Xi, grid, [T], nx, stop_on_error=True)
    # VELDIV on the padded centre grid; tracers inside it and outside it apart (outside: vz extrapolated from cell (0, 0), large)
    gp = K.padded_centres(grid)
    Vz, Vx, _ = K.velocities(grid, rng)
    with oracle.rect_search():
        ref = oracle.grid2trac(X, gp, [Vz, Vx], [nx[0] + 1, nx[1] + 1], defval=0, method=oracle.M_VELDIV)
    mod = M.grid2trac_veldiv(X, gp, [Vz, Vx], defval=0.0)
    ins = np.all([(X[:, d] >= gp[d][0]) & (X[:, d] < gp[d][-1]) for d in range(2)], axis=0)
    assert ins.sum() > 10000 and (name == "lines" or (~ins).sum() > 50)
    for part in (ins, ~ins):
        if part.any():
            assert maxrel(ref[part], mod[part]) < 64 * EPS


@pytest.mark.parametrize("name", ["19x39", "5x5"])
def test_oracle_rk4_equals_the_plain_model(oracle, name):
    nx, L, grid, X, F = K.case(name)
    gp = K.padded_centres(grid)
    Vz, Vx, dt = K.velocities(grid, np.random.default_rng(6))
    with oracle.rect_search():
        v0, x0 = oracle.rk4(X, gp, [Vz, Vx], nx, dt)
    v1, x1 = M.rk4(X, gp, [Vz, Vx], dt)
    left = (x0[:, 0] <= 0) | (x0[:, 0] >= L[0]) | (x0[:, 1] <= 0) | (x0[:, 1] >= L[1])
    print("%d of %d tracers end beyond a wall; x %.2e v %.2e" % (left.sum(), X.shape[0], maxrel(x0, x1), maxrel(v0, v1)))
    assert left.sum() >= 5
    # positions: |x| <= L, a handful of roundings per stage; velocities (x_new - x) / dt: the cancellation leaves eps L / (dt |v|)
    assert maxrel(x0, x1) < 64 * EPS
    assert maxrel(v0, v1) < 64 * EPS * max(L) / (dt * np.abs(v1).max())
