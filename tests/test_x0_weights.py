"""The weights of the extrapolated Stokes start (pylamp_amd/csrc/pl_x0.h), on the CPU.

The time step cannot show a wrong weight -- the stopping rule of the solve is the same whatever the start, only the iteration
count moves -- so the header is compiled into a small program of its own with the host C++ compiler and checked here:
the weights reproduce polynomials up to the fitted degree (moment conditions), and the special cases hold by value.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pylamp_amd", "csrc")
X0_HIST = 5
NHIST = 300                    # seeded step histories per (order, keep)
BOUND = 1e-8                   # moment error relative to 1 + sum |L_i tau_i^a|

# one case per input line: n_prev keep order wx d[0..5]  ->  nh l0 l[0..4]
MAIN = r"""
#include "pl_x0.h"
#include <cstdio>
int main() {
    int n_prev, keep, order; double wx, d[X0_HIST + 1];
    while (std::scanf("%d %d %d %lf %lf %lf %lf %lf %lf %lf", &n_prev, &keep, &order, &wx, &d[0], &d[1], &d[2], &d[3], &d[4], &d[5]) == 10) {
        const X0Weights w = pl_x0_weights(d, n_prev, keep, order, wx);
        std::printf("%d %.17g %.17g %.17g %.17g %.17g %.17g\n", w.nh, w.l0, w.l[0], w.l[1], w.l[2], w.l[3], w.l[4]);
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def weights(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++") if c and shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("x0")
    src, exe = str(d / "x0_main.cpp"), str(d / "x0_main")
    open(src, "w").write(MAIN)
    subprocess.check_call([cxx, "-std=c++17", "-O2", "-I", CSRC, src, "-o", exe])

    def run(cases):
        """cases: (n_prev, keep, order, wx, d[6]) -> list of (nh, l0, l[5])"""
        text = "".join("%d %d %d %.17g %s\n" % (c[0], c[1], c[2], c[3], " ".join("%.17g" % v for v in c[4])) for c in cases)
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
        res = [(int(t[0]), float(t[1]), np.array([float(v) for v in t[2:]])) for t in (ln.split() for ln in out if ln)]
        assert len(res) == len(cases)
        return res
    return run


def histories(rng, n):
    """full histories d[0..5]: consecutive ratios in [0.25, 4] (log-uniform), d[0] <= 2 d[1]"""
    d = np.empty((n, X0_HIST + 1))
    d[:, 1] = 10.0 ** rng.uniform(-3.0, 15.0, n)                         # model time steps of any magnitude
    d[:, 0] = d[:, 1] * 2.0 ** rng.uniform(-2.0, 1.0, n)
    for k in range(2, X0_HIST + 1):
        d[:, k] = d[:, k - 1] * 4.0 ** rng.uniform(-1.0, 1.0, n)
    r = d[:, :-1] / d[:, 1:]
    assert np.all(r >= 0.25) and np.all(r <= 4.0) and np.all(d[:, 0] <= 2.0 * d[:, 1])
    return d


def test_weights_reproduce_polynomials(weights):
    rng = np.random.default_rng(20240)
    cases = []
    for order in (1, 2, 3):
        for keep in range(order, X0_HIST + 1):
            d = histories(rng, NHIST)
            wx = np.where(rng.random(NHIST) < 0.5, 1.0, rng.uniform(0.25, 1.0, NHIST))     # the default and a shortened target
            cases += [(keep, keep, order, wx[i], d[i]) for i in range(NHIST)]
    worst = 0.0
    for (n_prev, keep, order, wx, d), (nh, l0, l) in zip(cases, weights(cases)):
        assert nh == keep, "a full history is used in full"
        L = np.concatenate([[l0], l[:nh]])
        tau = np.concatenate([[0.0], -np.cumsum(d[1:nh + 1]) / d[0]])
        deg = min(order, nh)                                # (one older solution: the linear formula, wx d0 / d1 <= 2 is not capped)
        for a in range(deg + 1):
            terms = L * tau ** a
            err = abs(terms.sum() - wx ** a) / (1.0 + np.abs(terms).sum())
            worst = max(worst, err)
            assert err <= BOUND, (order, keep, a, err, list(d), wx, list(L))
    print("worst moment error %.3g over %d histories" % (worst, len(cases)))


def test_special_cases_by_value(weights):
    cases = [
        (1, 1, 1, 1.0, [3.0, 2.0, 0, 0, 0, 0]),              # 0: one older solution: (1 + w, -w), w = wx d0 / d1
        (1, 3, 2, 0.5, [3.0, 2.0, 5.0, 5.0, 0, 0]),          # 1: ... whatever keep and order say
        (1, 1, 1, 1.0, [5.0, 2.0, 0, 0, 0, 0]),              # 2: w capped at 2
        (3, 3, 2, 1.0, [5.0, 2.0, 2.0, 2.0, 0, 0]),          # 3: the step more than doubled: linear formula, capped
        (3, 3, 2, 0.5, [4.5, 2.0, 2.0, 2.0, 0, 0]),          # 4: ... not capped
        (4, 4, 2, 1.0, [1.0, 1.0, 1.0, 0.0, 1.0, 0]),        # 5: d[3] is not positive: solutions 1, 2 remain
        (4, 4, 2, 1.0, [1.0, 1.0, -1.0, 1.0, 1.0, 0]),       # 6: d[2] is not positive: solution 1 remains
        (4, 4, 2, 1.0, [1.0, 0.0, 1.0, 1.0, 1.0, 0]),        # 7: d[1] is not positive: none
        (4, 4, 2, 1.0, [float("nan"), 1.0, 1.0, 1.0, 1.0, 0]),   # 8: d[0] is not a number: none
        (0, 3, 2, 1.0, [1.0, 1.0, 1.0, 1.0, 0, 0]),          # 9: no history
        (5, 2, 2, 1.0, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),      # 10: equal steps, quadratic through 3 solutions: 3, -3, 1
        (5, 1, 1, 1.0, [1.0, 1.0, 1.0, 1.0, 1.0, 1.0]),      # 11: keep limits the history
    ]
    r = weights(cases)

    def check(k, nh, l0, l):
        assert r[k][0] == nh, (k, r[k])
        np.testing.assert_allclose(r[k][1], l0, rtol=1e-13, atol=0, err_msg=str(k))
        np.testing.assert_allclose(r[k][2], np.concatenate([l, np.zeros(X0_HIST - len(l))]), rtol=1e-13, atol=1e-13, err_msg=str(k))
    check(0, 1, 2.5, [-1.5])
    check(1, 1, 1.75, [-0.75])
    check(2, 1, 3.0, [-2.0])
    check(3, 1, 3.0, [-2.0])
    check(4, 1, 1.0 + 0.5 * 4.5 / 2.0, [-0.5 * 4.5 / 2.0])
    check(5, 2, 3.0, [-3.0, 1.0])
    check(6, 1, 2.0, [-1.0])
    check(7, 0, 1.0, [])
    check(8, 0, 1.0, [])
    check(9, 0, 1.0, [])
    check(10, 2, 3.0, [-3.0, 1.0])
    check(11, 1, 2.0, [-1.0])
