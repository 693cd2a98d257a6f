// Matrix-free staggered-grid Stokes operator  y = A x  and its right-hand side.
//
// Replaces the lil_matrix assembly of pylamp_stokes.makeStokesMatrix
// (pylamp_stokes.py:104-563).  Rows are classified from the GLOBAL node index inside the
// kernel (ghost / wall / tangential-slave / corner / anchor / interior); nothing per-row
// is stored.  Unknowns live in three SoA planes (vz | vx | P) with a one-node ring.
//
// Bound: HBM.  Algorithmic traffic per node and apply: x 24 B + etas 8 + etan 8 + y 24
// = 64 B.
#include "pl_internal.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <limits>

#define TB(tab, k) (tab)[(k) + PL_TOFF]

// ---------------------------------------------------------------------------------------------------
// Two-columns-per-lane variant: every plane row is read with 16-byte (double2) loads, the j-1 / j+1
// neighbours come from the adjacent lanes (ds_bpermute), only the two edge lanes issue an extra
// 8-byte load.  Why: with 8-byte loads the texture-address unit was busy 84 % of the kernel time
// (PMC TA_TA_BUSY, profiles/r01_pmc_stalls.csv): the L1 path serves 4 lanes per cycle whatever the
// width, so double2 halves the address cycles per byte and there are 14 instead of 34 loads per wave.
// A wave covers 128 columns of one row; rows/columns outside the block are never dereferenced past
// the ring (planes carry a ring row above/below and >= 1 pad column each side).
// all values one node needs, as scalars
struct StokesVals {
    double vz_c, vz_w, vz_e, vz_n, vz_s, vz_nw;      // n = row i+1, s = row i-1, nw = (i+1, j-1)
    double vx_c, vx_w, vx_e, vx_n, vx_s, vx_se;      // se = (i-1, j+1)
    double p_c, p_w, p_e, p_s;
    double en_c, en_w, en_s;
    double es_c, es_e, es_n;
    double rdx_j, rdx_m, rDx_j, rDx_p;
};

// The memory-only twin of this kernel runs in 58 us against 80 us (2049^2): the arithmetic is NOT free.  The
// row scales of the scaled operator are therefore a template switch (the plain operator performs no division
// at all) and use v_rcp_f64 + one Newton step (pl_rcp, 2.2e-15) instead of the ~15-instruction IEEE division sequence.
template <bool SCALED>
__device__ inline void stokes_node_vals(const PlStokesOp& op, int i, int j, int c, const StokesVals& q,
                                        const double* __restrict__ x, double& oz, double& ox, double& op_) {
    const PlGeom& g = op.g;
    const int nz = g.nz, nx = g.nx, p = g.pitch;
    const double Kc = op.Kc;
    const double iKc = op.iKc;
    double sz = iKc, sx = iKc, sp = iKc;
    double yz;
    if (j == nx - 1 || i == 0 || i == nz - 1) yz = Kc * q.vz_c;
    else if (j == 0) yz = Kc * (q.vz_c - q.vz_e);
    else if (j == nx - 2) yz = Kc * (q.vz_c - q.vz_w);
    else {
        // factored so that the row-only products are shared by the lane's two columns and each viscosity is
        // multiplied once (the arithmetic of this kernel is ~1/3 of its run time: FP64 issues at half rate)
        const double rdz_i = TB(g.rdz, i), rdz_m = TB(g.rdz, i - 1), rDz_i = TB(g.rDz, i);
        const double Az = 4.0 * rdz_i * rDz_i, Azm = 4.0 * rdz_m * rDz_i, Pz = 2.0 * Kc * rDz_i;     // row constants
        const double k2 = 2.0 * q.rdx_j;                                                              // column constant
        const double tE = q.es_e * k2, tW = q.es_c * k2;
        const double cN = q.en_c * Az, cS = q.en_s * Azm, cE = tE * q.rDx_p, cW = tW * q.rDx_j;
        const double xE = tE * rDz_i, xW = tW * rDz_i;
        yz = cN * (q.vz_n - q.vz_c) - cS * (q.vz_c - q.vz_s) + cE * (q.vz_e - q.vz_c) - cW * (q.vz_c - q.vz_w) +
             xE * (q.vx_e - q.vx_se) - xW * (q.vx_c - q.vx_s) - Pz * (q.p_c - q.p_s);
        if (SCALED) sz = pl_rcp(cN + cS + cE + cW);
        if (op.surfstab) {
            const double* __restrict__ r = op.rho;
            yz += op.ss * op.gz * 0.5 * ((r[c + 1] + r[c + p + 1] - r[c - 1] - r[c + p - 1]) * q.rDx_j * q.vx_c +
                                         (r[c + p] + r[c + p + 1] - r[c - p] - r[c - p + 1]) * rDz_i * q.vz_c);
        }
    }
    double yx;
    if (i == nz - 1 || j == 0 || j == nx - 1) yx = Kc * q.vx_c;
    else if (i == 0) {
        if (op.bc_z0 == PL_BC_FREESLIP) yx = Kc * (q.vx_c - q.vx_n);
        else yx = Kc * ((-TB(g.rDz, 1) - TB(g.rdz, 0)) * q.vx_c + TB(g.rDz, 1) * q.vx_n);
    } else if (i == nz - 2) {
        if (op.bc_zL == PL_BC_FREESLIP) yx = Kc * (q.vx_c - q.vx_s);
        else yx = Kc * ((TB(g.rDz, nz - 2) + TB(g.rdz, nz - 2)) * q.vx_c - TB(g.rDz, nz - 2) * q.vx_s);
    } else {
        const double rdz_i = TB(g.rdz, i), rDz_i = TB(g.rDz, i), rDz_p = TB(g.rDz, i + 1);
        const double r2 = 2.0 * rdz_i, twoKc = 2.0 * Kc;                                             // row constants
        const double B4 = 4.0 * q.rDx_j;                                                              // column constants
        const double Bx = B4 * q.rdx_j, Bxm = B4 * q.rdx_m, Px = twoKc * q.rDx_j;
        const double uN = q.es_n * r2, uS = q.es_c * r2;
        const double cE = q.en_c * Bx, cW = q.en_w * Bxm, cN = uN * rDz_p, cS = uS * rDz_i;
        const double zN = uN * q.rDx_j, zS = uS * q.rDx_j;
        yx = cE * (q.vx_e - q.vx_c) - cW * (q.vx_c - q.vx_w) + cN * (q.vx_n - q.vx_c) - cS * (q.vx_c - q.vx_s) +
             zN * (q.vz_n - q.vz_nw) - zS * (q.vz_c - q.vz_w) - Px * (q.p_c - q.p_w);
        if (SCALED) sx = pl_rcp(cE + cW + cN + cS);
        if (op.surfstab && op.gx != 0.0) {
            const double* __restrict__ r = op.rho;
            yx += op.ss * op.gx * 0.5 * ((r[c + 1] + r[c + p + 1] - r[c - 1] - r[c + p - 1]) * q.rDx_j * q.vx_c +
                                         (r[c + p] + r[c + p + 1] - r[c - p] - r[c - p + 1]) * rDz_i * q.vz_c);
        }
    }
    double yp;
    if (i == nz - 1 || j == nx - 1 || (i == op.anchor_i && j == op.anchor_j)) yp = Kc * q.p_c;
    else if ((i == 0 || i == nz - 2) && j == 0) { yp = op.Kb * (q.p_e - q.p_c); if (SCALED) sp = pl_rcp(op.Kb); }
    else if ((i == 0 || i == nz - 2) && j == nx - 2) { yp = op.Kb * (q.p_w - q.p_c); if (SCALED) sp = pl_rcp(op.Kb); }
    else {
        yp = Kc * ((q.vx_e - q.vx_c) * q.rdx_j + (q.vz_n - q.vz_c) * TB(g.rdz, i));
        if (SCALED) sp = iKc * pl_rcp(q.rdx_j + TB(g.rdz, i));
    }
    (void)x;
    oz = SCALED ? yz * sz : yz; ox = SCALED ? yx * sx : yx; op_ = SCALED ? yp * sp : yp;
}

// Straight-line twin of stokes_node_vals for a node whose three rows are all of the interior class
// (1 <= i <= nz-3, 1 <= j <= nx-3, not the anchor, no stabilisation): no classification, no exec-mask regions.
struct StokesRowK { double Az, Azm, Pz, rDz_i, rDz_p, r2, twoKc, rdz_i, Kc, iKc; };
template <bool SCALED>
__device__ inline void stokes_interior_vals(const StokesRowK& k, const StokesVals& q, double& oz, double& ox, double& op_) {
    const double dzn = q.vz_n - q.vz_c, dxe = q.vx_e - q.vx_c;
    const double k2 = 2.0 * q.rdx_j;
    const double tE = q.es_e * k2, tW = q.es_c * k2;
    const double cN = q.en_c * k.Az, cS = q.en_s * k.Azm, cE = tE * q.rDx_p, cW = tW * q.rDx_j;
    const double yz = cN * dzn - cS * (q.vz_c - q.vz_s) + cE * (q.vz_e - q.vz_c) - cW * (q.vz_c - q.vz_w) +
                      (tE * k.rDz_i) * (q.vx_e - q.vx_se) - (tW * k.rDz_i) * (q.vx_c - q.vx_s) - k.Pz * (q.p_c - q.p_s);
    const double B4 = 4.0 * q.rDx_j;
    const double uN = q.es_n * k.r2, uS = q.es_c * k.r2;
    const double dE = q.en_c * (B4 * q.rdx_j), dW = q.en_w * (B4 * q.rdx_m), dN = uN * k.rDz_p, dS = uS * k.rDz_i;
    const double yx = dE * dxe - dW * (q.vx_c - q.vx_w) + dN * (q.vx_n - q.vx_c) - dS * (q.vx_c - q.vx_s) +
                      (uN * q.rDx_j) * (q.vz_n - q.vz_nw) - (uS * q.rDx_j) * (q.vz_c - q.vz_w) -
                      (k.twoKc * q.rDx_j) * (q.p_c - q.p_w);
    const double yp = k.Kc * (dxe * q.rdx_j + dzn * k.rdz_i);
    if (SCALED) {
        oz = yz * pl_rcp(cN + cS + cE + cW);
        ox = yx * pl_rcp(dE + dW + dN + dS);
        op_ = yp * (k.iKc * pl_rcp(q.rdx_j + k.rdz_i));
    } else { oz = yz; ox = yx; op_ = yp; }
}

// Both columns of one lane from the twelve loaded rows, then the (double2) stores.
struct StokesRows { Row2 vz_s, vz_i, vz_n, vx_s, vx_i, vx_n, p_s, p_i, en_s, en_i, es_i, es_n, t_rdx, t_rDx; };
// MODE (PlApplyMode) != 0: the lane's contributions to the epilogue sums are ADDED to acc[] (see PlApplyArgs)
template <bool SCALED, int MODE>
__device__ inline void stokes_compute_store(const PlStokesOp& op, const StokesRows& R, int i, int jw, int lj0, int c,
                                            const double* __restrict__ x, double* __restrict__ y, const PlApplyArgs& a,
                                            double (&acc)[PL_EPI_NSUM]) {
    const PlGeom& g = op.g;
    const double* __restrict__ add = a.add;
    const double* __restrict__ coef = a.coef;
    const Row2 &vz_s = R.vz_s, &vz_i = R.vz_i, &vz_n = R.vz_n, &vx_s = R.vx_s, &vx_i = R.vx_i, &vx_n = R.vx_n;
    const Row2 &p_s = R.p_s, &p_i = R.p_i, &en_s = R.en_s, &en_i = R.en_i, &es_i = R.es_i, &es_n = R.es_n;
    const double rdx_a = R.t_rdx.v.x, rdx_b = R.t_rdx.v.y, rdx_m = R.t_rdx.w;
    const double rDx_a = R.t_rDx.v.x, rDx_b = R.t_rDx.v.y, rDx_pp = R.t_rDx.e;
    const int j0 = g.gj0 + lj0;
    StokesVals q;
    double oz[2], ox[2], opv[2];
    const bool colB = (lj0 + 1) < g.lnx;
    // wave-uniform: every node of this wave is of the interior class in all three equations
    const bool fast = !op.surfstab && i >= 1 && i <= g.nz - 3 && jw >= 1 && jw + 127 <= g.nx - 3 &&
                      !(i == op.anchor_i && op.anchor_j >= jw && op.anchor_j < jw + 128);
    StokesRowK rk;
    if (fast) {
        const double rdz_i = TB(g.rdz, i), rdz_m = TB(g.rdz, i - 1), rDz_i = TB(g.rDz, i);
        rk.Az = 4.0 * rdz_i * rDz_i; rk.Azm = 4.0 * rdz_m * rDz_i; rk.Pz = 2.0 * op.Kc * rDz_i; rk.rDz_i = rDz_i;
        rk.rDz_p = TB(g.rDz, i + 1); rk.r2 = 2.0 * rdz_i; rk.twoKc = 2.0 * op.Kc; rk.rdz_i = rdz_i; rk.Kc = op.Kc; rk.iKc = op.iKc;
    }
    // column A (lj0)
    q.vz_c = vz_i.v.x; q.vz_w = vz_i.w; q.vz_e = vz_i.v.y; q.vz_n = vz_n.v.x; q.vz_s = vz_s.v.x; q.vz_nw = vz_n.w;
    q.vx_c = vx_i.v.x; q.vx_w = vx_i.w; q.vx_e = vx_i.v.y; q.vx_n = vx_n.v.x; q.vx_s = vx_s.v.x; q.vx_se = vx_s.v.y;
    q.p_c = p_i.v.x; q.p_w = p_i.w; q.p_e = p_i.v.y; q.p_s = p_s.v.x;
    q.en_c = en_i.v.x; q.en_w = en_i.w; q.en_s = en_s.v.x;
    q.es_c = es_i.v.x; q.es_e = es_i.v.y; q.es_n = es_n.v.x;
    q.rdx_j = rdx_a; q.rdx_m = rdx_m; q.rDx_j = rDx_a; q.rDx_p = rDx_b;
    if (fast) stokes_interior_vals<SCALED>(rk, q, oz[0], ox[0], opv[0]);
    else stokes_node_vals<SCALED>(op, i, j0, c, q, x, oz[0], ox[0], opv[0]);
    // column B (lj0 + 1)
    q.vz_c = vz_i.v.y; q.vz_w = vz_i.v.x; q.vz_e = vz_i.e; q.vz_n = vz_n.v.y; q.vz_s = vz_s.v.y; q.vz_nw = vz_n.v.x;
    q.vx_c = vx_i.v.y; q.vx_w = vx_i.v.x; q.vx_e = vx_i.e; q.vx_n = vx_n.v.y; q.vx_s = vx_s.v.y; q.vx_se = vx_s.e;
    q.p_c = p_i.v.y; q.p_w = p_i.v.x; q.p_e = p_i.e; q.p_s = p_s.v.y;
    q.en_c = en_i.v.y; q.en_w = en_i.v.x; q.en_s = en_s.v.y;
    q.es_c = es_i.v.y; q.es_e = es_i.e; q.es_n = es_n.v.y;
    q.rdx_j = rdx_b; q.rdx_m = rdx_a; q.rDx_j = rDx_b; q.rDx_p = rDx_pp;
    if (fast) stokes_interior_vals<SCALED>(rk, q, oz[1], ox[1], opv[1]);
    else if (colB) stokes_node_vals<SCALED>(op, i, j0 + 1, c + 1, q, x, oz[1], ox[1], opv[1]);
    if (add) {                                              // wave-uniform: y = A x + coef[0] * add (pl_solver.hip, deflation)
        const double cf = coef[0];
        const long long P = g.plane;
        if (colB) {
            const double2 az = *reinterpret_cast<const double2*>(add + c), ax = *reinterpret_cast<const double2*>(add + c + P),
                          ap = *reinterpret_cast<const double2*>(add + c + 2 * P);
            oz[0] += cf * az.x; oz[1] += cf * az.y; ox[0] += cf * ax.x; ox[1] += cf * ax.y; opv[0] += cf * ap.x; opv[1] += cf * ap.y;
        } else { oz[0] += cf * add[c]; ox[0] += cf * add[c + P]; opv[0] += cf * add[c + 2 * P]; }
    }
    if (!colB) { oz[1] = 0.0; ox[1] = 0.0; opv[1] = 0.0; }     // (the epilogue sums run over both columns)
    // a lane's two values of one plane of a vector (the second one 0 beyond the row)
    auto ld2 = [&](const double* __restrict__ v, int q) {
        const double* __restrict__ ptr = v + c + q * g.plane;
        return colB ? *reinterpret_cast<const double2*>(ptr) : make_double2(ptr[0], 0.0);
    };
    if (MODE == PL_EPI_DOT1) {
        const double2 rz = ld2(a.a1, 0), rx = ld2(a.a1, 1), rp = ld2(a.a1, 2);
        acc[0] += rz.x * oz[0] + rz.y * oz[1] + rx.x * ox[0] + rx.y * ox[1] + rp.x * opv[0] + rp.y * opv[1];
    }
    if (MODE == PL_EPI_DOT5) {
        const double2 sz = ld2(a.a1, 0), sx = ld2(a.a1, 1), sp = ld2(a.a1, 2);
        const double2 rz = ld2(a.a2, 0), rx = ld2(a.a2, 1), rp = ld2(a.a2, 2);
        const double ts_c = opv[0] * sp.x + opv[1] * sp.y, tt_c = opv[0] * opv[0] + opv[1] * opv[1], ss_c = sp.x * sp.x + sp.y * sp.y;
        acc[0] += oz[0] * sz.x + oz[1] * sz.y + ox[0] * sx.x + ox[1] * sx.y + ts_c;
        acc[1] += oz[0] * oz[0] + oz[1] * oz[1] + ox[0] * ox[0] + ox[1] * ox[1] + tt_c;
        acc[2] += rz.x * sz.x + rz.y * sz.y + rx.x * sx.x + rx.y * sx.y + rp.x * sp.x + rp.y * sp.y;
        acc[3] += rz.x * oz[0] + rz.y * oz[1] + rx.x * ox[0] + rx.y * ox[1] + rp.x * opv[0] + rp.y * opv[1];
        acc[4] += sz.x * sz.x + sz.y * sz.y + sx.x * sx.x + sx.y * sx.y + ss_c;
        if (a.cont) { acc[5] += ts_c; acc[6] += tt_c; acc[7] += ss_c; }
    }
    if (MODE == PL_EPI_RESID) {
        const double2 bz = ld2(a.a1, 0), bx = ld2(a.a1, 1), bp = ld2(a.a1, 2);
        if (a.y2) {                                         // A x itself is kept too
            double* __restrict__ y2 = a.y2;
            if (colB) {
                *reinterpret_cast<double2*>(y2 + c) = make_double2(oz[0], oz[1]);
                *reinterpret_cast<double2*>(y2 + c + g.plane) = make_double2(ox[0], ox[1]);
                *reinterpret_cast<double2*>(y2 + c + 2 * g.plane) = make_double2(opv[0], opv[1]);
            } else { y2[c] = oz[0]; y2[c + g.plane] = ox[0]; y2[c + 2 * g.plane] = opv[0]; }
        }
        oz[0] = bz.x - oz[0]; oz[1] = bz.y - oz[1]; ox[0] = bx.x - ox[0]; ox[1] = bx.y - ox[1]; opv[0] = bp.x - opv[0]; opv[1] = bp.y - opv[1];
        const double rr_c = opv[0] * opv[0] + opv[1] * opv[1];
        acc[PL_RS_RR] += oz[0] * oz[0] + oz[1] * oz[1] + ox[0] * ox[0] + ox[1] * ox[1] + rr_c;
        acc[PL_RS_RR_C] += rr_c;
        acc[PL_RS_BB] += bz.x * bz.x + bz.y * bz.y + bx.x * bx.x + bx.y * bx.y + bp.x * bp.x + bp.y * bp.y;
        if (a.want_xx) {
            double2 uz = make_double2(vz_i.v.x, colB ? vz_i.v.y : 0.0), ux = make_double2(vx_i.v.x, colB ? vx_i.v.y : 0.0);
            if (a.a2) { const double2 wz = ld2(a.a2, 0), wx = ld2(a.a2, 1); uz.x += wz.x; uz.y += wz.y; ux.x += wx.x; ux.y += wx.y; }
            acc[PL_RS_XX] += uz.x * uz.x + uz.y * uz.y + ux.x * ux.x + ux.y * ux.y;
        }
        if (a.want_ysum) {                                  // y . r over the continuity rows (k_defl_ysum, pl_solver.hip)
            const int nz = g.nz, nx = g.nx;
            const double hz = (i < nz - 1) ? 1.0 / TB(g.rdz, i) : 0.0;
            const bool zwall = (i == 0 || i == nz - 2);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int j = j0 + k;
                const bool is_cont = !(i >= nz - 1 || j >= nx - 1 || (i == op.anchor_i && j == op.anchor_j)) && !(zwall && (j == 0 || j == nx - 2));
                if (is_cont && (k == 0 || colB)) acc[PL_RS_YR] += (hz + 1.0 / (k ? rdx_b : rdx_a)) * opv[k];
            }
        }
    }
    if (colB) {
        *reinterpret_cast<double2*>(y + c) = make_double2(oz[0], oz[1]);
        *reinterpret_cast<double2*>(y + c + g.plane) = make_double2(ox[0], ox[1]);
        *reinterpret_cast<double2*>(y + c + 2 * g.plane) = make_double2(opv[0], opv[1]);
    } else {
        y[c] = oz[0]; y[c + g.plane] = ox[0]; y[c + 2 * g.plane] = opv[0];
    }
}

// Sum of acc[q] over the wave for all eight q in 10 exchanges instead of 48: every step halves both the lanes a value is spread
// over and the values a lane carries (lane bits 5, 4, 3 select the half that is kept), three plain steps finish.  On return
// lane L holds the wave's sum of value L >> 3.  The order of the additions is fixed by the lane numbers: deterministic.
__device__ inline double wave_sum8(const double (&a)[PL_EPI_NSUM], int lane) {
    double b[4], d[2];
    const bool h5 = lane & 32, h4 = lane & 16, h3 = lane & 8;
#pragma unroll
    for (int q = 0; q < 4; q++) { const double keep = h5 ? a[q + 4] : a[q], send = h5 ? a[q] : a[q + 4]; b[q] = keep + __shfl_xor(send, 32, 64); }
#pragma unroll
    for (int q = 0; q < 2; q++) { const double keep = h4 ? b[q + 2] : b[q], send = h4 ? b[q] : b[q + 2]; d[q] = keep + __shfl_xor(send, 16, 64); }
    double e = (h3 ? d[1] : d[0]) + __shfl_xor(h3 ? d[0] : d[1], 8, 64);
    e += __shfl_xor(e, 4, 64); e += __shfl_xor(e, 2, 64); e += __shfl_xor(e, 1, 64);
    return e;
}

// MODE 0 returns early for the rows beyond the block and the lanes beyond the row; with an epilogue these fall through with zero
// contributions, because the whole workgroup meets in the reduction: wave exchange, ROWS x 8 doubles of LDS, one store of the
// workgroup's partial sums (no atomics: the second stage adds them in a fixed order).  The epilogue kernels are held to 4 waves per
// SIMD (128 VGPRs; the compiler takes 140 by itself, and DOT5 then runs in 131 instead of 118 us at 2049^2); MODE 0 is left alone.
template <int ROWS, bool SCALED, int MODE>
__global__ __launch_bounds__(64 * ROWS, MODE != 0 ? 4 : 1) void k_stokes_apply_v2(PlStokesOp op, const double* __restrict__ x,
                                                               double* __restrict__ y, PlApplyArgs a) {
    const PlGeom& g = op.g;
    const int lane = threadIdx.x;
    const int lj0 = (blockIdx.x * 64 + lane) * 2;          // this lane's two columns: lj0, lj0+1
    const int li = blockIdx.y * ROWS + threadIdx.y;
    double acc[PL_EPI_NSUM] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (MODE == PL_EPI_NONE && li >= g.lnz) return;         // wave-uniform
    if (li < g.lnz) {
    const bool active = lj0 < g.lnx;                        // lanes beyond the row take part in shuffles only
    const bool has_right = (lj0 + 2) < g.lnx;               // the lane to the right holds real columns
    const int p = g.pitch;
    const int c = (li + PL_RING) * p + PL_PADL + lj0;             // element offset of column A (16-B aligned)
    const double* __restrict__ vz = x;
    const double* __restrict__ vx = x + g.plane;
    const double* __restrict__ P = x + 2 * g.plane;
    const double* __restrict__ es = op.etas;
    const double* __restrict__ en = op.etan;
#define ROW(ptr, dr, w, e) load_row2((ptr) + (long long)c - lj0 + (long long)(dr) * p, lj0, active, w, e, lane, has_right)
    const Row2 vz_s = ROW(vz, -1, false, false), vz_i = ROW(vz, 0, true, true), vz_n = ROW(vz, 1, true, false);
    const Row2 vx_s = ROW(vx, -1, false, true), vx_i = ROW(vx, 0, true, true), vx_n = ROW(vx, 1, false, false);
    const Row2 p_s = ROW(P, -1, false, false), p_i = ROW(P, 0, true, true);
    const Row2 en_s = ROW(en, -1, false, false), en_i = ROW(en, 0, true, false);
    const Row2 es_i = ROW(es, 0, false, true), es_n = ROW(es, 1, false, false);
#undef ROW
    // x tables: pair at (j, j+1) plus the two outer neighbours (tables are padded by PL_TOFF entries)
    const Row2 t_rdx = load_row2(g.rdx + PL_TOFF + g.gj0, lj0, active, true, false, lane, has_right);
    const Row2 t_rDx = load_row2(g.rDx + PL_TOFF + g.gj0, lj0, active, false, true, lane, has_right);
    if (MODE == PL_EPI_NONE && !active) return;
    if (active) {
        const int i = g.gi0 + li;
        StokesRows R{vz_s, vz_i, vz_n, vx_s, vx_i, vx_n, p_s, p_i, en_s, en_i, es_i, es_n, t_rdx, t_rDx};
        stokes_compute_store<SCALED, MODE>(op, R, i, g.gj0 + blockIdx.x * 128, lj0, c, x, y, a, acc);
    }
    }
    if (MODE != PL_EPI_NONE) {
        __shared__ double sh[ROWS][PL_EPI_NSUM];
        const int blk = blockIdx.y * gridDim.x + blockIdx.x;
        if (MODE == PL_EPI_DOT1) {
            double s = acc[0];
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) sh[threadIdx.y][0] = s;
            __syncthreads();
            if (threadIdx.y == 0 && lane < 2) {
                double t = 0.0;
                for (int w = 0; w < ROWS; w++) t += sh[w][0];
                a.part[2 * (long long)blk + lane] = lane == 0 ? t : 0.0;
            }
        } else {
            const double s = wave_sum8(acc, lane);
            if ((lane & 7) == 0) sh[threadIdx.y][lane >> 3] = s;
            __syncthreads();
            if (threadIdx.y == 0 && lane < PL_EPI_NSUM) {
                double t = 0.0;
                for (int w = 0; w < ROWS; w++) t += sh[w][lane];
                a.part[PL_EPI_NSUM * (long long)blk + lane] = t;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_stokes_rhs(PlStokesOp op, double* __restrict__ rhs) {
    const PlGeom& g = op.g;
    const int lj = blockIdx.x * 64 + threadIdx.x, li = blockIdx.y * 4 + threadIdx.y;
    if (lj >= g.lnx || li >= g.lnz) return;
    const int i = g.gi0 + li, j = g.gj0 + lj, nz = g.nz, nx = g.nx, p = g.pitch;
    const long long c = pl_idx(g, li, lj);
    const double* __restrict__ r = op.rho;
    double bz = 0.0, bx = 0.0;
    if (i >= 1 && i <= nz - 2 && j >= 1 && j <= nx - 3) bz = -0.5 * (r[c] + r[c + 1]) * op.gz;
    if (i >= 1 && i <= nz - 3 && j >= 1 && j <= nx - 2) bx = -0.5 * (r[c] + r[c + p]) * op.gx;
    rhs[c] = bz; rhs[c + g.plane] = bx; rhs[c + 2 * g.plane] = 0.0;
}

static dim3 grid2d(const PlGeom& g) { return dim3((g.lnx + 63) / 64, (g.lnz + 3) / 4); }

// The row-block height of a launch: 16 on large grids, 4 otherwise (PYLAMP_APPLY_ROWS: 2, 4, 8 or 16 for every plain launch;
// the epilogue modes exist for the two heights in use, 4 and 16)
int pl_apply_rows(const PlGeom& g, int mode, int rows) {
    static const int rows_knob = [] { const char* e = getenv("PYLAMP_APPLY_ROWS"); return e ? atoi(e) : 0; }();
    if (!rows) rows = rows_knob ? rows_knob : ((long long)g.lnz * g.lnx >= 8000000LL ? 16 : 4);
    if (mode != PL_EPI_NONE) return rows >= 16 ? 16 : 4;
    return (rows == 16 || rows == 8 || rows == 2) ? rows : 4;
}

// a.add != NULL: y = A x + a.coef[0] * a.add; a.mode: the reductions of PlApplyArgs
void pl_launch_stokes_apply(pl_ctx* ctx, const PlStokesOp& op, const double* x, double* y, const PlApplyArgs& a) {
    // Variants measured on MI355X at 2049^2: 8-byte loads 84 us; double2 81 us; + register row
    // marching (R = 8/16) 99/104 us; XCD-aware block remap, plane-stride padding: no effect; a memory-only twin
    // (same loads and stores, no arithmetic) 58 us -> the arithmetic was exposed: no divisions in the plain
    // operator 76 us, factored coefficients 73 us, branch-free interior path 64 us.  Sharing the rows of a
    // 4- or 8-row tile through LDS (5 instead of 12 global row loads per wave) is SLOWER (68 us): the L1 re-reads
    // were never the limit, the barrier is one.  Round 3: two output rows per wave (17 instead of 24 row loads per pair of rows, 162 VGPRs):
    // 69 vs 68 us at 2049^2, 298 vs 290 us at 4097^2 -- the re-reads are not what the kernel waits for.  Removed.
    // (The scalar one-column-per-lane kernel of round 1 is gone: the vectorised one is pinned directly against the reference's
    // explicit matrices on five grids, tests/test_hip_parity.py.)  double2 accesses need even plane strides and an even first
    // column: the pitch is a multiple of 16 and block columns start at even multiples (pl_set_comm_2d enforces even block widths).
    const int gx = (op.g.lnx + 127) / 128;
    const int rows = pl_apply_rows(op.g, a.mode, a.rows);
#define PL_APPLY_LAUNCH(ROWS, MODE)                                                                                     \
    do {                                                                                                                \
        if (op.scaled) hipLaunchKernelGGL((k_stokes_apply_v2<ROWS, true, MODE>), dim3(gx, (op.g.lnz + ROWS - 1) / ROWS), dim3(64, ROWS), 0, ctx->stream, op, x, y, a);  \
        else hipLaunchKernelGGL((k_stokes_apply_v2<ROWS, false, MODE>), dim3(gx, (op.g.lnz + ROWS - 1) / ROWS), dim3(64, ROWS), 0, ctx->stream, op, x, y, a);           \
    } while (0)
#define PL_APPLY_MODE(MODE) do { if (rows == 16) PL_APPLY_LAUNCH(16, MODE); else PL_APPLY_LAUNCH(4, MODE); } while (0)
    switch (a.mode) {
    case PL_EPI_DOT1: PL_APPLY_MODE(PL_EPI_DOT1); break;
    case PL_EPI_DOT5: PL_APPLY_MODE(PL_EPI_DOT5); break;
    case PL_EPI_RESID: PL_APPLY_MODE(PL_EPI_RESID); break;
    default:
        if (rows == 16) PL_APPLY_LAUNCH(16, PL_EPI_NONE);
        else if (rows == 8) PL_APPLY_LAUNCH(8, PL_EPI_NONE);
        else if (rows == 2) PL_APPLY_LAUNCH(2, PL_EPI_NONE);
        else PL_APPLY_LAUNCH(4, PL_EPI_NONE);
    }
#undef PL_APPLY_MODE
#undef PL_APPLY_LAUNCH
}

void pl_launch_stokes_rhs(pl_ctx* ctx, const PlStokesOp& op, double* rhs) {
    hipLaunchKernelGGL(k_stokes_rhs, grid2d(op.g), dim3(64, 4), 0, ctx->stream, op, rhs);
}

// np.min semantics: NaN if any NaN
static double np_min(const double* a, size_t n) {
    double m = std::numeric_limits<double>::infinity();
    bool nan = false;
    for (size_t k = 0; k < n; k++) { if (a[k] != a[k]) nan = true; else if (a[k] < m) m = a[k]; }
    return nan ? std::numeric_limits<double>::quiet_NaN() : m;
}

// pylamp_stokes.py:116-122; python's min(a, b) returns a unless b < a
void pl_stokes_scaling_host(const PlGeomHost& gh, double minetas, double minetan, double* Kc, double* Kb) {
    double mineta = (minetan < minetas) ? minetan : minetas;
    int nz = (int)gh.zc.size(), nx = (int)gh.xc.size();
    double avgdx = (gh.xc[nx - 1] - gh.xc[0]) / nx;
    double avgdz = (gh.zc[nz - 1] - gh.zc[0]) / nz;
    *Kc = 2.0 * mineta / (avgdx + avgdz);
    *Kb = 4.0 * mineta / ((avgdx + avgdz) * (avgdx + avgdz));
}

int pl_stokes_check_bc(pl_ctx* ctx, const int bc[4]) {
    // Only the wall types that give a non-singular system in the reference are offered
    // (SURVEY.md 8 a2.3): z-walls NOSLIP or FREESLIP, x-walls FREESLIP.
    for (int w = 0; w < 4; w += 2)
        if (bc[w] != PL_BC_NOSLIP && bc[w] != PL_BC_FREESLIP)
            return pl_fail(ctx, "stokes: z-wall boundary condition must be NOSLIP or FREESLIP");
    for (int w = 1; w < 4; w += 2)
        if (bc[w] != PL_BC_FREESLIP)
            return pl_fail(ctx, "stokes: x-wall boundary condition must be FREESLIP");
    return 0;
}

void pl_stokes_fill_op(pl_ctx* ctx, double* etas, double* etan, double* rho, const int bc[4], int surfstab,
                       double tstep, double theta, double Kc, double Kb) {
    PlStokesOp& op = ctx->sop;
    op.g = ctx->geom.d;
    op.etas = etas; op.etan = etan; op.rho = rho;
    op.Kc = Kc; op.Kb = Kb; op.iKc = 1.0 / Kc;
    op.bc_z0 = bc[0]; op.bc_zL = bc[2];
    op.surfstab = surfstab ? 1 : 0; op.ss = theta * tstep;
    op.anchor_i = 3; op.anchor_j = 2;
    op.gz = 9.81; op.gx = 0.0;                     // pylamp_const.py:21
    op.scaled = 0;
    ctx->sop_ready = true;
}

extern "C" int pl_stokes_set_coeffs(pl_ctx* ctx, const double* etas, const double* etan, const double* rho,
                                    const int bc[4], int surfstab, double tstep, double theta) {
    if (!etas || !etan || !rho || !bc) return pl_fail(ctx, "pl_stokes_set_coeffs: NULL argument");
    PL_TRY(pl_stokes_check_bc(ctx, bc));
    if (surfstab && !(tstep == tstep)) return pl_fail(ctx, "surface stabilization needs predetermined tstep");
    PL_HIP(ctx, hipSetDevice(ctx->device));
    const PlGeom& g = ctx->geom.d;
    size_t pb = (size_t)g.plane * sizeof(double);
    double *d_es, *d_en, *d_rho;
    PL_TRY(pl_buf(ctx, "etas", pb, &d_es)); PL_TRY(pl_buf(ctx, "etan", pb, &d_en)); PL_TRY(pl_buf(ctx, "rho", pb, &d_rho));
    PL_TRY(pl_plane_upload(ctx, g, etas, d_es));
    PL_TRY(pl_plane_upload(ctx, g, etan, d_en));
    PL_TRY(pl_plane_upload(ctx, g, rho, d_rho));
    size_t n = (size_t)ctx->nz * ctx->nx;
    double Kc, Kb;
    pl_stokes_scaling_host(ctx->geom, np_min(etas, n), np_min(etan, n), &Kc, &Kb);
    pl_stokes_fill_op(ctx, d_es, d_en, d_rho, bc, surfstab, tstep, theta, Kc, Kb);
    {   // viscosity contrast over the values the operator reads (etan: the physical cells)
        double lo = std::numeric_limits<double>::infinity(), hi = 0.0;
        for (int i = 0; i < ctx->nz; i++)
            for (int j = 0; j < ctx->nx; j++) {
                const double a = etas[(size_t)i * ctx->nx + j];
                if (a > 0.0) { lo = std::min(lo, a); hi = std::max(hi, a); }
                if (i < ctx->nz - 1 && j < ctx->nx - 1) { const double b = etan[(size_t)i * ctx->nx + j]; if (b > 0.0) { lo = std::min(lo, b); hi = std::max(hi, b); } }
            }
        ctx->visc_contrast = (hi > 0.0 && lo > 0.0 && std::isfinite(hi / lo)) ? hi / lo : 1.0;
    }
    return 0;
}

extern "C" int pl_stokes_get_scaling(pl_ctx* ctx, double* kcont, double* kbond) {
    if (!ctx->sop_ready) return pl_fail(ctx, "stokes operator not set");
    if (kcont) *kcont = ctx->sop.Kc;
    if (kbond) *kbond = ctx->sop.Kb;
    return 0;
}

extern "C" int pl_stokes_apply(pl_ctx* ctx, const double* x, double* y) {
    if (!ctx->sop_ready) return pl_fail(ctx, "stokes operator not set");
    PL_HIP(ctx, hipSetDevice(ctx->device));
    const PlGeom& g = ctx->geom.d;
    size_t vb = (size_t)3 * g.plane * sizeof(double);
    double *dx, *dy;
    PL_TRY(pl_buf(ctx, "api_x", vb, &dx)); PL_TRY(pl_buf(ctx, "api_y", vb, &dy));
    PL_TRY(pl_vec3_upload(ctx, g, x, dx));
    PL_TRY(pl_halo(ctx, g, dx, 3, g.plane));
    pl_launch_stokes_apply(ctx, ctx->sop, dx, dy);
    PL_HIP(ctx, hipGetLastError());
    PL_TRY(pl_vec3_download(ctx, g, dy, y));
    return 0;
}

extern "C" int pl_stokes_rhs(pl_ctx* ctx, double* rhs) {
    if (!ctx->sop_ready) return pl_fail(ctx, "stokes operator not set");
    PL_HIP(ctx, hipSetDevice(ctx->device));
    const PlGeom& g = ctx->geom.d;
    double* dy;
    PL_TRY(pl_buf(ctx, "api_y", (size_t)3 * g.plane * sizeof(double), &dy));
    pl_launch_stokes_rhs(ctx, ctx->sop, dy);
    PL_HIP(ctx, hipGetLastError());
    PL_TRY(pl_vec3_download(ctx, g, dy, rhs));
    return 0;
}

__global__ void k_fill_pseudo(double* __restrict__ v, long long n, unsigned seed) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < n; k += (long long)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)(k * 2654435761u) ^ seed;
        h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
        v[k] = (double)h * (2.0 / 4294967296.0) - 1.0;
    }
}

static int apply_bench(pl_ctx* ctx, int scaled, int reps, double* avg_ms) {
    if (!ctx->sop_ready) return pl_fail(ctx, "stokes operator not set");
    if (reps < 1) reps = 1;
    PL_HIP(ctx, hipSetDevice(ctx->device));
    const PlGeom& g = ctx->geom.d;
    size_t vb = (size_t)3 * g.plane * sizeof(double);
    double *dx, *dy;
    PL_TRY(pl_buf(ctx, "api_x", vb, &dx)); PL_TRY(pl_buf(ctx, "api_y", vb, &dy));
    hipLaunchKernelGGL(k_fill_pseudo, dim3(2048), dim3(256), 0, ctx->stream, dx, 3 * g.plane, 12345u);
    PlStokesOp op = ctx->sop; op.scaled = scaled ? 1 : 0;
    pl_launch_stokes_apply(ctx, op, dx, dy);      // warm-up
    PL_TRY(pl_timer_start(ctx));
    for (int r = 0; r < reps; r++) pl_launch_stokes_apply(ctx, op, dx, dy);
    double ms = 0;
    PL_TRY(pl_timer_stop_ms(ctx, &ms));
    PL_HIP(ctx, hipGetLastError());
    if (avg_ms) *avg_ms = ms / reps;
    return 0;
}
extern "C" int pl_stokes_apply_bench(pl_ctx* ctx, int reps, double* avg_ms) { return apply_bench(ctx, 0, reps, avg_ms); }
// the row-scaled variant y = D_r A x, the one the Krylov solver launches
extern "C" int pl_stokes_apply_scaled_bench(pl_ctx* ctx, int reps, double* avg_ms) { return apply_bench(ctx, 1, reps, avg_ms); }

// Stream triad a = b + s c on three arrays of n doubles (24 n bytes per launch, 16 B per lane): the measured HBM rate of
// this box, against which the roofline fractions are reported next to the datasheet peak.
__global__ __launch_bounds__(256) void k_triad(long long n2, double2* __restrict__ a, const double2* __restrict__ b,
                                               const double2* __restrict__ c, double s) {
    long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    for (; k < n2; k += (long long)gridDim.x * blockDim.x) {
        const double2 u = b[k], v = c[k];
        a[k] = make_double2(u.x + s * v.x, u.y + s * v.y);
    }
}
extern "C" int pl_stream_triad_bench(pl_ctx* ctx, int64_t n, int reps, double* avg_ms) {
    if (n < 1024 || reps < 1) return pl_fail(ctx, "pl_stream_triad_bench: bad argument");
    PL_HIP(ctx, hipSetDevice(ctx->device));
    n &= ~(int64_t)1;
    double* buf;
    PL_TRY(pl_buf(ctx, "triad", (size_t)3 * n * sizeof(double), &buf, false));
    hipLaunchKernelGGL(k_fill_pseudo, dim3(2048), dim3(256), 0, ctx->stream, buf, 3 * n, 777u);
    // one double2 per thread measured fastest on MI355X (tools/triad_sweep.py: 6.07 TB/s at 3 x 1 GiB against 4.6 TB/s with 8192
    // grid-striding blocks)
    unsigned nblk = (unsigned)std::min<long long>((n / 2 + 255) / 256, 1 << 20);
    if (const char* e = getenv("PYLAMP_TRIAD_BLOCKS")) { long v = atol(e); if (v >= 64 && v <= (1 << 22)) nblk = (unsigned)v; }
    auto launch = [&]() {
        hipLaunchKernelGGL(k_triad, dim3(nblk), dim3(256), 0, ctx->stream, (long long)(n / 2), (double2*)buf, (const double2*)(buf + n),
                           (const double2*)(buf + 2 * n), 0.5);
    };
    launch();
    PL_TRY(pl_timer_start(ctx));
    for (int r = 0; r < reps; r++) launch();
    double ms = 0;
    PL_TRY(pl_timer_stop_ms(ctx, &ms));
    PL_HIP(ctx, hipGetLastError());
    if (avg_ms) *avg_ms = ms / reps;
    return 0;
}
