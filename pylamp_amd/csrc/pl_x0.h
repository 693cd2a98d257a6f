// Weights of the extrapolated initial guess of the Stokes solve (pl_step.hip: stokes_start).  Host only -- no HIP types, no
// environment -- so that a plain C++ program can test it (tests/test_x0_weights.py): the step's outputs cannot show a wrong
// weight, only the iteration count depends on it.
#pragma once
#include <algorithm>
#include <cmath>
constexpr int X0_HIST = 5;                     // older Stokes solutions kept at most for the extrapolated initial guess
struct X0Weights { int nh; double l0, l[X0_HIST]; };      // x <- l0 x + sum_{k < nh} l[k] h[k]; h[k]: the older solutions, newest first
// Weights of the polynomial of degree `order` fitted (least squares when more than order + 1 solutions are kept, else
// interpolating) to the solutions at model times 0, -d[1], -d[1]-d[2], ... and evaluated at +wx d[0].  d[0..X0_HIST]: the last
// time steps (newest first; d[0] leads to the solution sought), n_prev: older solutions held, keep: used at most.  A time step
// that more than doubled (or a missing history) falls back to the linear formula with its weight capped at 2.
inline X0Weights pl_x0_weights(const double* d, int n_prev, int keep, int order, double wx) {
    int np = std::min(keep, n_prev);                   // older solutions used
    for (int k = 0; k <= np; k++) if (!(d[k] > 0.0)) np = std::min(np, std::max(0, k - 1));
    if (np >= 2 && d[0] > 2.0 * d[1]) np = 1;
    X0Weights w{};
    w.nh = np; w.l0 = 1.0;
    if (np == 1) {
        const double c = std::min(2.0, wx * d[0] / d[1]);
        w.l0 = 1.0 + c; w.l[0] = -c;
    } else if (np >= 2) {
        const int deg = std::min(order, np), m = np + 1;
        double tau[X0_HIST + 1] = {}, G[4][5] = {};              // times in units of d[0]; normal equations (V^T V) c = t
        for (int k = 1; k <= np; k++) tau[k] = tau[k - 1] - d[k] / d[0];
        for (int a2 = 0; a2 <= deg; a2++) {
            for (int b2 = 0; b2 <= deg; b2++) for (int i = 0; i < m; i++) G[a2][b2] += std::pow(tau[i], a2 + b2);
            G[a2][deg + 1] = std::pow(wx, a2);
        }
        bool ok = true;
        for (int c = 0; c <= deg && ok; c++) {                    // Gauss-Jordan with partial pivoting on the (deg+1) system
            int pv = c;
            for (int r = c + 1; r <= deg; r++) if (std::fabs(G[r][c]) > std::fabs(G[pv][c])) pv = r;
            if (!(std::fabs(G[pv][c]) > 1e-300)) { ok = false; break; }
            for (int k = 0; k <= deg + 1; k++) std::swap(G[c][k], G[pv][k]);
            for (int r = 0; r <= deg; r++) if (r != c) {
                const double f = G[r][c] / G[c][c];
                for (int k = c; k <= deg + 1; k++) G[r][k] -= f * G[c][k];
            }
        }
        if (ok) {
            double L[X0_HIST + 1];
            for (int i = 0; i < m; i++) {
                L[i] = 0.0;
                for (int a2 = 0; a2 <= deg; a2++) L[i] += std::pow(tau[i], a2) * G[a2][deg + 1] / G[a2][a2];
            }
            w.l0 = L[0];
            for (int k = 0; k < np; k++) w.l[k] = L[k + 1];
        } else w.nh = 0;
    }
    return w;
}
