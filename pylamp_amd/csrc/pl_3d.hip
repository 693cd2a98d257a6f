// 3-D staggered Stokes + heat (BASELINE config 5).  PARITY UNPINNED: the reference implements 2-D only
// (pylamp_const.py:6 "DIM = 2  # 2 or 3, currently only 2 implemented"; pylamp_stokes.py:30-35 prints
// "NOT IMPLEMENTED" for dim != 2).  What it does fix is the intent: axis order z, x, y (pylamp_const.py:9-13), arrays
// (nz, nx, ny), pressure as equation IP = DIM = 3, DOF order iz*nx*ny*4 + ix*ny*4 + iy*4 + ieq (pylamp_stokes.py:24).
// This file extends the 2-D rows of pylamp_stokes.py:376-518 and pylamp_diff.py:157-179 dimension by dimension
//  so that a y-invariant extrusion of a 2-D problem reproduces the 2-D operator and solution on every
// y-slice (tests/test_hip_3d.py), and is otherwise validated by manufactured solutions and true residuals.
//
// Staggering: vz at (z_i, x_j+1/2, y_k+1/2), vx at (z_i+1/2, x_j, y_k+1/2), vy at (z_i+1/2, x_j+1/2, y_k), P and the
// normal viscosity eta_n at cell centres, the shear viscosity eta_s ONCE at the nodes (z_i, x_j, y_k) and averaged on
// the fly onto the edge a term needs (the 80 B/node layout of SURVEY 8d: x 32 + y 32 + eta_n 8 + eta_s 8).
// One velocity component's row is the same expression under a cyclic permutation of the axes: the kernels are
// templated on the component.  Solver: the 2-D design (pl_solver.hip) in 3-D -- row-scaled BiCGStab, block-triangular
// preconditioner [[A_vv, A_vp],[0, S^]] with one geometric-multigrid V-cycle (Chebyshev-Jacobi smoothing, rediscretised
// coarse operators with natural wall rows, arithmetic viscosity coarsening) for A_vv.  One GPU per problem.
#include "pl_internal.h"
#include "pl_mic3.h"
#include "pl_reduce3.h"
#include "pl_step3.h"
#include "pl_walls3.h"
#include "pl_x0.h"
#include <algorithm>
#include <cmath>

#define P3_PAD 16                    // left padding of a y-line: node k = 0 is 128-B aligned
// Coefficient tables are read through the constant address space: with a wave-uniform index (the z and x axes: blockIdx.z and the
// readfirstlane'd row of the workgroup, K3_PROLOGUE) the load is a scalar one (s_load, scalar cache) instead of 64 identical lanes
// of a vector load.  The tables are written by the host before any kernel that reads them.
typedef const double __attribute__((address_space(4))) * pl_ctab;
#define TB(tab, k) (((pl_ctab)(tab))[(k) + PL_TOFF])

struct G3 {
    int n[3];                        // nodes of THIS RANK's block along z, x, y (the whole grid on one rank)
    int gn[3];                       // global node counts nz, nx, ny
    int o[3];                        // global index of local node (0, 0, 0)
    long long s[3];                  // element strides of z, x, y
    long long vol;                   // elements per scalar array (incl. one ring of nodes in z and x, padding in y)
    const double* rd[3];             // 1/(c[i+1]-c[i])      per axis, zero padded, GLOBAL index + PL_TOFF
    const double* rD[3];             // 1/(c[i+1]-c[i-1])
};
__host__ __device__ inline long long i3(const G3& g, int i, int j, int k) {
    return (long long)(i + 1) * g.s[0] + (long long)(j + 1) * g.s[1] + (k + P3_PAD);
}

struct Op3 {
    G3 g;
    const double* es; const double* en; const double* rho;
    double Kc, Kb, iKc;
    int slave;                       // 1: the reference's slaved outermost in-domain tangential rows (finest level); 0: natural rows
    int noslip;                      // bit w of [z0, x0, y0, zL, xL, yL]: that wall is no-slip (0: every wall free-slip)
    double grav[3];
    int anchor[3];
};

enum { C3_ZERO = 0, C3_INT = 1, C3_SLAVE = 2 };

// class of the row of velocity component D at node idx; slaves get the offset to their (interior) master
template <int D> __device__ inline int cls3(const Op3& op, const int* idx, long long& moff) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const int* n = op.g.gn;
    moff = 0;
    if (idx[D] <= 0 || idx[D] >= n[D] - 1 || idx[E] >= n[E] - 1 || idx[F] >= n[F] - 1) return C3_ZERO;
    if (op.slave) {
        if (idx[E] == 0) moff += op.g.s[E]; else if (idx[E] == n[E] - 2) moff -= op.g.s[E];
        if (idx[F] == 0) moff += op.g.s[F]; else if (idx[F] == n[F] - 2) moff -= op.g.s[F];
        if (moff != 0) return C3_SLAVE;
    }
    return C3_INT;
}

// ---- no-slip walls (include/pylamp_hip.h).  Every row they change lies on the layers 0 and n - 2 of a tangential axis:
// the per-node kernels and k3_rim evaluate them, the marching kernels never do.  The mask is a kernel argument and the table entries a
// wall reads have fixed indices (0, 1, n - 2): scalar.  In the K3_PROLOGUE kernels the layer tests along z and x are wave-uniform as
// well; in k3_rim a thread's node comes from its own index, so there the layer tests are per lane (the rim is ~4 % of the nodes).
template <int A> __device__ inline bool nos3(const Op3& op, int hi) { return (op.noslip >> (A + 3 * hi)) & 1; }
// a row slaved along axis A at its low / high wall is Kc (sd v + sn v_nb): free-slip 1, -1; no-slip the reference's extrapolation row
// (pylamp_stokes.py:165-166,204-205): v extrapolated linearly to the wall is zero
template <int A> __device__ inline void slave_coef3(const Op3& op, int hi, double& sd, double& sn) {
    const int m = hi ? op.g.gn[A] - 2 : 1;
    const double rD = TB(op.g.rD[A], m), rd = TB(op.g.rd[A], hi ? m : 0);
    sd = hi ? rD + rd : -(rD + rd); sn = hi ? -rD : rD;
}
// v / v_nb of that row
template <int A> __device__ inline double gam3(const Op3& op, int hi) {
    if (!nos3<A>(op, hi)) return 1.0;
    double sd, sn;
    slave_coef3<A>(op, hi, sd, sn);
    return -sn / sd;
}
// v_slave / v_master along the chain of a C3_SLAVE row (E, then F): the closure of the smoother, the transfers and k3_close
template <int D> __device__ inline double fac3(const Op3& op, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    if (!op.noslip) return 1.0;
    double f = 1.0;
    if (idx[E] == 0) f = gam3<E>(op, 0); else if (idx[E] == op.g.gn[E] - 2) f = gam3<E>(op, 1);
    if (idx[F] == 0) f *= gam3<F>(op, 0); else if (idx[F] == op.g.gn[F] - 2) f *= gam3<F>(op, 1);
    return f;
}
// the slaved row itself at the low / high wall of A (unb: the inward neighbour); scaled: divided by Kc sd
template <int A> __device__ inline double slave_row3(const Op3& op, int hi, double u0, double unb, bool scaled) {
    if (!nos3<A>(op, hi)) { const double y = u0 - unb; return scaled ? y : op.Kc * y; }
    double sd, sn;
    slave_coef3<A>(op, hi, sd, sn);
    return scaled ? u0 + (sn / sd) * unb : op.Kc * (sd * u0 + sn * unb);
}
// 1 / (Kc sd) of component D's C3_SLAVE row: its row scale
template <int D> __device__ inline double slave_scale3(const Op3& op, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    if (!op.noslip) return op.iKc;
    double sd = 1.0, sn;
    if (idx[E] == 0) { if (nos3<E>(op, 0)) slave_coef3<E>(op, 0, sd, sn); }
    else if (idx[E] == op.g.gn[E] - 2) { if (nos3<E>(op, 1)) slave_coef3<E>(op, 1, sd, sn); }
    else if (idx[F] == 0) { if (nos3<F>(op, 0)) slave_coef3<F>(op, 0, sd, sn); }
    else if (nos3<F>(op, 1)) slave_coef3<F>(op, 1, sd, sn);
    return op.iKc / sd;
}
// natural rows: the coefficient of -v_D that a no-slip wall of axis A adds to the row at layer ia (0 elsewhere and on free-slip walls):
// the dv_D/dx_A half of the shear stress on the wall edge, one-sided against v_D = 0 on the wall, eta (2 rd v) rd; em / ep: the
// viscosities of the row's lower / upper edge along A
template <int A> __device__ inline double wall_coef3(const Op3& op, int ia, double em, double ep) {
    if (!op.noslip) return 0.0;
    if (ia == 0 && nos3<A>(op, 0)) { const double rd = TB(op.g.rd[A], 0); return 2.0 * em * rd * rd; }
    if (ia == op.g.gn[A] - 2 && nos3<A>(op, 1)) { const double rd = TB(op.g.rd[A], ia); return 2.0 * ep * rd * rd; }
    return 0.0;
}

// (A_vv v)_D without the pressure term and the sum `dg` of the four..six own-component coefficients at element c.
// Zero-padded tables make the mirror terms of natural wall rows vanish (rD[0] = rD[n-1] = 0).
template <int D> __device__ inline void row3(const Op3& op, const double* const* __restrict__ v, long long c, const int* idx,
                                              double& Av, double& dg) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const G3& g = op.g;
    const long long sd = g.s[D], se = g.s[E], sf = g.s[F];
    const double* __restrict__ u = v[D];
    const double* __restrict__ es = op.es;
    const double rd_d = TB(g.rd[D], idx[D]), rd_dm = TB(g.rd[D], idx[D] - 1), rD_d = TB(g.rD[D], idx[D]);
    const double u0 = u[c];
    const double cN = 4.0 * op.en[c] * rd_d * rD_d, cS = 4.0 * op.en[c - sd] * rd_dm * rD_d;
    double a = cN * (u[c + sd] - u0) - cS * (u0 - u[c - sd]);
    double d = cN + cS;
    {   // tangential axis E: the edge viscosities are node values averaged along F
        const double rd_e = TB(g.rd[E], idx[E]), rD_e = TB(g.rD[E], idx[E]), rD_ep = TB(g.rD[E], idx[E] + 1);
        const double ep = 0.5 * (es[c + se] + es[c + se + sf]), em = 0.5 * (es[c] + es[c + sf]);
        const double cE = 2.0 * ep * rD_ep * rd_e, cW = 2.0 * em * rD_e * rd_e;
        const double* __restrict__ w = v[E];
        a += cE * (u[c + se] - u0) - cW * (u0 - u[c - se]) + (2.0 * ep * rD_d * rd_e) * (w[c + se] - w[c + se - sd]) -
             (2.0 * em * rD_d * rd_e) * (w[c] - w[c - sd]);
        d += cE + cW;
        const double cw = wall_coef3<E>(op, idx[E], em, ep);
        if (cw != 0.0) { a -= cw * u0; d += cw; }
    }
    {   // tangential axis F: averaged along E
        const double rd_f = TB(g.rd[F], idx[F]), rD_f = TB(g.rD[F], idx[F]), rD_fp = TB(g.rD[F], idx[F] + 1);
        const double ep = 0.5 * (es[c + sf] + es[c + sf + se]), em = 0.5 * (es[c] + es[c + se]);
        const double cE = 2.0 * ep * rD_fp * rd_f, cW = 2.0 * em * rD_f * rd_f;
        const double* __restrict__ w = v[F];
        a += cE * (u[c + sf] - u0) - cW * (u0 - u[c - sf]) + (2.0 * ep * rD_d * rd_f) * (w[c + sf] - w[c + sf - sd]) -
             (2.0 * em * rD_d * rd_f) * (w[c] - w[c - sd]);
        d += cE + cW;
        const double cw = wall_coef3<F>(op, idx[F], em, ep);
        if (cw != 0.0) { a -= cw * u0; d += cw; }
    }
    Av = a; dg = d;
}
// diagonal sum only
template <int D> __device__ inline double diag3(const Op3& op, long long c, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const G3& g = op.g;
    const long long sd = g.s[D], se = g.s[E], sf = g.s[F];
    const double* __restrict__ es = op.es;
    const double rD_d = TB(g.rD[D], idx[D]);
    double d = 4.0 * op.en[c] * TB(g.rd[D], idx[D]) * rD_d + 4.0 * op.en[c - sd] * TB(g.rd[D], idx[D] - 1) * rD_d;
    const double rd_e = TB(g.rd[E], idx[E]), rd_f = TB(g.rd[F], idx[F]);
    d += (es[c + se] + es[c + se + sf]) * TB(g.rD[E], idx[E] + 1) * rd_e + (es[c] + es[c + sf]) * TB(g.rD[E], idx[E]) * rd_e;
    d += (es[c + sf] + es[c + sf + se]) * TB(g.rD[F], idx[F] + 1) * rd_f + (es[c] + es[c + se]) * TB(g.rD[F], idx[F]) * rd_f;
    if (op.noslip) {
        d += wall_coef3<E>(op, idx[E], 0.5 * (es[c] + es[c + sf]), 0.5 * (es[c + se] + es[c + se + sf]));
        d += wall_coef3<F>(op, idx[F], 0.5 * (es[c] + es[c + se]), 0.5 * (es[c + sf] + es[c + sf + se]));
    }
    return d;
}

// li, lj, lk: node of this rank's block; i, j, k (= idx): its GLOBAL index -- row classes and spacing tables are global
#define K3_PROLOGUE(g)                                                                          \
    const int lk = blockIdx.x * 64 + threadIdx.x, lj = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + threadIdx.y), li = blockIdx.z; \
    if (lk >= (g).n[2] || lj >= (g).n[1]) return;                                               \
    const long long c = i3((g), li, lj, lk);                                                    \
    const int k = lk + (g).o[2], j = __builtin_amdgcn_readfirstlane(lj + (g).o[1]), i = li + (g).o[0]; \
    const int idx[3] = {i, j, k};                                                               \
    (void)idx;
static dim3 grid3(const G3& g) { return dim3((g.n[2] + 63) / 64, (g.n[1] + 3) / 4, g.n[0]); }
// (Tried: z-marching -- a workgroup owns a 64 x 4 tile in (y, x) and walks 32 planes so that the planes i-1, i, i+1 it needs
// are the ones it has just touched.  Measured at 257^3 on MI355X: apply 1.44 ms against 0.93 ms with one plane per workgroup
// -- the kernel is bound by the latency of its ~70 dependent 8-byte loads per node, not by HBM traffic, and marching cuts the
// parallelism that hides it.  Removed.)

// ---- full Stokes operator --------------------------------------------------------------------------------------
struct V4 { const double* p[4]; };
struct W4 { double* p[4]; };
struct V3 { const double* p[3]; };
struct W3 { double* p[3]; };

// pressure row class: 0 ghost/anchor (Kc P), 1 continuity, 2 symmetry with the neighbour at offset moff (Kb (P_nb - P))
__device__ inline int cls3_p(const Op3& op, const int* idx, long long& moff) {
    const int* n = op.g.gn;
    moff = 0;
    if (idx[0] >= n[0] - 1 || idx[1] >= n[1] - 1 || idx[2] >= n[2] - 1) return 0;
    if (idx[0] == op.anchor[0] && idx[1] == op.anchor[1] && idx[2] == op.anchor[2]) return 0;
    // with natural wall rows every pressure cell appears in a momentum row: no symmetry rows
    if (!op.slave) return 1;
    const bool bz = idx[0] == 0 || idx[0] == n[0] - 2, bx = idx[1] == 0 || idx[1] == n[1] - 2, by = idx[2] == 0 || idx[2] == n[2] - 2;
    if (bz && bx) { moff = idx[1] == 0 ? op.g.s[1] : -op.g.s[1]; return 2; }            // the 2-D corner rule (pylamp_stokes.py:358-369)
    if (by && (bz || bx)) { moff = idx[2] == 0 ? op.g.s[2] : -op.g.s[2]; return 2; }     // remaining cube edges: inward along y
    return 1;
}

template <int D> __device__ inline double apply_vel3(const Op3& op, const double* const* v, const double* __restrict__ P, long long c,
                                                     const int* idx, bool scaled) {
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    const double u0 = v[D][c];
    if (cl == C3_ZERO) return scaled ? u0 : op.Kc * u0;
    if (cl == C3_SLAVE) {
        // the matrix row couples to the neighbour along the FIRST boundary axis (E before F), pylamp_stokes.py:170-175
        constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
        const int* n = op.g.gn;
        if (idx[E] == 0) return slave_row3<E>(op, 0, u0, v[D][c + op.g.s[E]], scaled);
        if (idx[E] == n[E] - 2) return slave_row3<E>(op, 1, u0, v[D][c - op.g.s[E]], scaled);
        if (idx[F] == 0) return slave_row3<F>(op, 0, u0, v[D][c + op.g.s[F]], scaled);
        return slave_row3<F>(op, 1, u0, v[D][c - op.g.s[F]], scaled);
    }
    double Av, dg;
    row3<D>(op, v, c, idx, Av, dg);
    Av -= 2.0 * op.Kc * TB(op.g.rD[D], idx[D]) * (P[c] - P[c - op.g.s[D]]);
    return scaled ? Av * pl_rcp(dg) : Av;
}

// rim_only != 0: only the nodes with a wall / slaved / symmetry row are evaluated (all four rows of such a node); the interior rows are
// k3_apply_m's
template <bool SCALED> __global__ __launch_bounds__(256) void k3_apply(Op3 op, V4 x, W4 y, int rim_only) {
    K3_PROLOGUE(op.g)
    if (rim_only) {
        long long m_;
        if (cls3<0>(op, idx, m_) == C3_INT && cls3<1>(op, idx, m_) == C3_INT && cls3<2>(op, idx, m_) == C3_INT && cls3_p(op, idx, m_) == 1) return;
    }
    const double* v[3] = {x.p[0], x.p[1], x.p[2]};
    const double* __restrict__ P = x.p[3];
    y.p[0][c] = apply_vel3<0>(op, v, P, c, idx, SCALED);
    y.p[1][c] = apply_vel3<1>(op, v, P, c, idx, SCALED);
    y.p[2][c] = apply_vel3<2>(op, v, P, c, idx, SCALED);
    long long moff;
    const int cl = cls3_p(op, idx, moff);
    double yp;
    if (cl == 0) yp = SCALED ? P[c] : op.Kc * P[c];
    else if (cl == 2) yp = SCALED ? (P[c + moff] - P[c]) : op.Kb * (P[c + moff] - P[c]);
    else {
        const G3& g = op.g;
        const double rz = TB(g.rd[0], i), rx = TB(g.rd[1], j), ry = TB(g.rd[2], k);
        const double div = (v[0][c + g.s[0]] - v[0][c]) * rz + (v[1][c + g.s[1]] - v[1][c]) * rx + (v[2][c + g.s[2]] - v[2][c]) * ry;
        yp = SCALED ? div * pl_rcp(rz + rx + ry) : op.Kc * div;
    }
    y.p[3][c] = yp;
}

// rhs (pylamp_stokes.py:429,490 extended: density averaged onto the face), optionally row-scaled like k3_apply<true>
// ---- moving no-slip walls (pl3_stokes_set_wall_velocity; include/pylamp_hip.h).  The terms are affine: they touch the
// right-hand side only, so the velocities travel as an argument of k3_rhs alone and Op3 stays as it is.  Wall and component of an entry
// are template constants, the side follows from a layer test on a global index (wave-uniform along z and x): scalar reads of the kernel
// arguments.  moving == 0 skips all of it.
template <int A, int D> __device__ inline double wall_vel3(const Pl3WallVel& mv, int hi) { return hi ? mv.u[3 * (A + 3) + D] : mv.u[3 * A + D]; }
// right-hand side of the row of v_D slaved along A at its low / high wall: unscaled -+Kc rd U_D ("v_D extrapolated linearly to the wall is
// U_D"); scaled (divided by Kc sd) (1 - gamma) U_D
template <int A, int D> __device__ inline double slave_rhs3(const Op3& op, const Pl3WallVel& mv, int hi, bool scaled) {
    if (!((mv.moving >> (A + 3 * hi)) & 1)) return 0.0;
    const double U = wall_vel3<A, D>(mv, hi);
    const double rd = TB(op.g.rd[A], hi ? op.g.gn[A] - 2 : 0);
    if (!scaled) return hi ? op.Kc * rd * U : -(op.Kc * rd * U);
    double sd, sn;
    slave_coef3<A>(op, hi, sd, sn);
    return (hi ? rd : -rd) / sd * U;
}
// natural rows: the constant part of the wall-edge shear 2 eta rd^2 (v_D - U_D) of a moving wall of axis A, on the left-hand side
template <int A, int D> __device__ inline double wall_rhs3(const Op3& op, const Pl3WallVel& mv, int ia, double em, double ep) {
    const int hi = ia == 0 ? 0 : 1;
    if ((ia != 0 && ia != op.g.gn[A] - 2) || !((mv.moving >> (A + 3 * hi)) & 1)) return 0.0;
    return wall_coef3<A>(op, ia, em, ep) * wall_vel3<A, D>(mv, hi);
}
// ---- flow through walls (pl3_stokes_set_wall_flow; include/pylamp_hip.h).  Affine as well: the identity row of a wall-normal
// velocity v_D on the wall plane of D (global index 0 or n_D - 1, and at most n - 2 along the two other axes) gains Un -- unscaled Kc Un --
// read from the wall's plane by the global face indices, so that every block of a decomposition reads the same six planes.  The planes
// travel as an argument of k3_rhs alone; mask == 0 skips all of it.  The test on idx[D] is wave-uniform for D = z, x.
template <int D> __device__ inline double flow_rhs3(const Op3& op, const Pl3WallFlow& fl, const int* idx, bool scaled) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3, P = E < F ? E : F, Q = E < F ? F : E;
    const int* n = op.g.gn;
    const int hi = idx[D] == 0 ? 0 : 1;
    if ((idx[D] != 0 && idx[D] != n[D] - 1) || !((fl.mask >> (D + 3 * hi)) & 1)) return 0.0;
    if (idx[P] > n[P] - 2 || idx[Q] > n[Q] - 2) return 0.0;                   // the ghost entries beyond stay 0
    const double un = fl.un[D + 3 * hi][(long long)idx[P] * (n[Q] - 1) + idx[Q]];
    return scaled ? un : op.Kc * un;
}
template <int D> __device__ inline double rhs_vel3(const Op3& op, const Pl3WallVel& mv, const Pl3WallFlow& fl, long long c, const int* idx, bool scaled) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    if (fl.mask != 0 && cl == C3_ZERO) return flow_rhs3<D>(op, fl, idx, scaled);
    if (mv.moving != 0 && cl == C3_SLAVE) {                 // the wall of the first boundary axis (E before F) supplies U
        const int* n = op.g.gn;
        if (idx[E] == 0) return slave_rhs3<E, D>(op, mv, 0, scaled);
        if (idx[E] == n[E] - 2) return slave_rhs3<E, D>(op, mv, 1, scaled);
        if (idx[F] == 0) return slave_rhs3<F, D>(op, mv, 0, scaled);
        return slave_rhs3<F, D>(op, mv, 1, scaled);
    }
    const bool walls = mv.moving != 0 && !op.slave;          // (with slaved rows no interior row lies on a wall layer)
    if (cl != C3_INT || (op.grav[D] == 0.0 && !walls)) return 0.0;
    const long long se = op.g.s[E], sf = op.g.s[F];
    double b = 0.0;
    if (op.grav[D] != 0.0) {
        const double* r = op.rho;
        b = -0.25 * ((r[c] + r[c + se]) + (r[c + sf] + r[c + se + sf])) * op.grav[D];
    }
    if (walls) {                                             // on a cube edge both walls contribute
        const double* __restrict__ es = op.es;
        b -= wall_rhs3<E, D>(op, mv, idx[E], 0.5 * (es[c] + es[c + sf]), 0.5 * (es[c + se] + es[c + se + sf]));
        b -= wall_rhs3<F, D>(op, mv, idx[F], 0.5 * (es[c] + es[c + se]), 0.5 * (es[c + sf] + es[c + sf + se]));
    }
    return scaled ? b / diag3<D>(op, c, idx) : b;
}
__global__ __launch_bounds__(256) void k3_rhs(Op3 op, W4 b, int scaled, Pl3WallVel mv, Pl3WallFlow fl) {
    K3_PROLOGUE(op.g)
    b.p[0][c] = rhs_vel3<0>(op, mv, fl, c, idx, scaled);
    b.p[1][c] = rhs_vel3<1>(op, mv, fl, c, idx, scaled);
    b.p[2][c] = rhs_vel3<2>(op, mv, fl, c, idx, scaled);
    b.p[3][c] = 0.0;
}
// b *= D_r (a user-supplied right-hand side)
template <int D> __device__ inline double scale_vel3(const Op3& op, long long c, const int* idx) {
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    return cl == C3_INT ? 1.0 / diag3<D>(op, c, idx) : (cl == C3_SLAVE ? slave_scale3<D>(op, idx) : op.iKc);
}
__global__ __launch_bounds__(256) void k3_scale_rows(Op3 op, W4 b) {
    K3_PROLOGUE(op.g)
    long long moff;
    b.p[0][c] *= scale_vel3<0>(op, c, idx);
    b.p[1][c] *= scale_vel3<1>(op, c, idx);
    b.p[2][c] *= scale_vel3<2>(op, c, idx);
    const int cl = cls3_p(op, idx, moff);
    const G3& g = op.g;
    b.p[3][c] *= cl == 0 ? op.iKc : (cl == 2 ? 1.0 / op.Kb : op.iKc / (TB(g.rd[0], i) + TB(g.rd[1], j) + TB(g.rd[2], k)));
}

// ---- preconditioner pieces ---------------------------------------------------------------------------------------
// z_p = S^-1 r_p from the SCALED residual (continuity rows: r eta_n / Kc^2 -> rs (sum rd) eta_n / Kc; ghost / anchor: rs;
// symmetry rows: P = P_nb - rs)
__device__ inline double prec_p3(const Op3& op, const double* __restrict__ rp, long long c, const int* idx) {
    long long moff;
    const int cl = cls3_p(op, idx, moff);
    const G3& g = op.g;
    if (cl == 0) return rp[c];
    if (cl == 1) return rp[c] * (TB(g.rd[0], idx[0]) + TB(g.rd[1], idx[1]) + TB(g.rd[2], idx[2])) * op.en[c] * op.iKc;
    // symmetry: value of the neighbour (one or two steps of the chain end on a continuity cell) minus the own residual
    int id2[3] = {idx[0], idx[1], idx[2]};
    long long c2 = c; double acc = 0.0;
    for (int hop = 0; hop < 3; hop++) {
        long long m2;
        const int cl2 = cls3_p(op, id2, m2);
        if (cl2 != 2) break;
        acc -= rp[c2];
        const int ax = (m2 == op.g.s[1] || m2 == -op.g.s[1]) ? 1 : 2;
        id2[ax] += (m2 > 0) ? 1 : -1; c2 += m2;
    }
    long long m3;
    const int cl3 = cls3_p(op, id2, m3);
    const double base = cl3 == 1 ? rp[c2] * (TB(g.rd[0], id2[0]) + TB(g.rd[1], id2[1]) + TB(g.rd[2], id2[2])) * op.en[c2] * op.iKc : rp[c2];
    return base + acc;
}
template <int D> __device__ inline double stage1_vel3(const Op3& op, const double* __restrict__ rs, const double* __restrict__ rp, long long c,
                                                      const int* idx, double zp_c) {
    long long moff;
    if (cls3<D>(op, idx, moff) != C3_INT) return 0.0;
    int idm[3] = {idx[0], idx[1], idx[2]}; idm[D] -= 1;
    return rs[c] * diag3<D>(op, c, idx) + 2.0 * op.Kc * TB(op.g.rD[D], idx[D]) * (zp_c - prec_p3(op, rp, c - op.g.s[D], idm));
}
// z_p = S^-1 r_p and f = r_v - A_vp z_p on the interior momentum rows (unscaled), 0 elsewhere
__global__ __launch_bounds__(256) void k3_stage1(Op3 op, V4 rs, double* __restrict__ zp, W3 f) {
    K3_PROLOGUE(op.g)
    const double z0 = prec_p3(op, rs.p[3], c, idx);
    zp[c] = z0;
    f.p[0][c] = stage1_vel3<0>(op, rs.p[0], rs.p[3], c, idx, z0);
    f.p[1][c] = stage1_vel3<1>(op, rs.p[1], rs.p[3], c, idx, z0);
    f.p[2][c] = stage1_vel3<2>(op, rs.p[2], rs.p[3], c, idx, z0);
}

// one Chebyshev-Jacobi sweep  v_next = v + c1 (v - v_prev) + c2 D^-1 (f - A v)  with the constraint rows closed in the same
// pass (a slave evaluates its master's update).  zero != 0: v = 0 is implied and not read.
template <int D> __device__ inline double cheb3(const Op3& op, const double* const* v, const double* __restrict__ vprev,
                                                const double* __restrict__ f, double c1, double c2, long long c, const int* idx, int zero) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    if (cl == C3_ZERO) return 0.0;
    const long long cm = c + moff;
    int im[3] = {idx[0], idx[1], idx[2]};
    if (cl == C3_SLAVE) {
        if (idx[E] == 0) im[E] = 1; else if (idx[E] == op.g.gn[E] - 2) im[E] = op.g.gn[E] - 3;
        if (idx[F] == 0) im[F] = 1; else if (idx[F] == op.g.gn[F] - 2) im[F] = op.g.gn[F] - 3;
    }
    // (a slave of a no-slip wall is its master's update times v_slave / v_master)
    const bool chain = cl == C3_SLAVE && op.noslip != 0;
    if (zero) { const double r = (-c2 * f[cm]) * pl_rcp(diag3<D>(op, cm, im)); return chain ? fac3<D>(op, idx) * r : r; }
    double Av, dg;
    row3<D>(op, v, cm, im, Av, dg);
    const double v0 = v[D][cm];
    const double mom = (c1 != 0.0) ? c1 * (v0 - (vprev ? vprev[cm] : 0.0)) : 0.0;
    const double r = v0 + mom + (c2 * (Av - f[cm])) * pl_rcp(dg);                        // D = -dg
    return chain ? fac3<D>(op, idx) * r : r;
}
// rim_only != 0: only the nodes with a wall or slaved row (all three rows of such a node); the interior rows are k3_sweep_m's
__device__ inline bool k3_all_interior(const Op3& op, const int* idx) {
    long long m_;
    return cls3<0>(op, idx, m_) == C3_INT && cls3<1>(op, idx, m_) == C3_INT && cls3<2>(op, idx, m_) == C3_INT;
}
__global__ __launch_bounds__(256) void k3_cheb(Op3 op, V3 vcur, V3 vprev, V3 f, W3 vnext, double c1, double c2, int zero, int rim_only) {
    K3_PROLOGUE(op.g)
    if (rim_only && k3_all_interior(op, idx)) return;
    const double* v[3] = {vcur.p[0], vcur.p[1], vcur.p[2]};
    vnext.p[0][c] = cheb3<0>(op, v, vprev.p[0], f.p[0], c1, c2, c, idx, zero);
    vnext.p[1][c] = cheb3<1>(op, v, vprev.p[1], f.p[1], c1, c2, c, idx, zero);
    vnext.p[2][c] = cheb3<2>(op, v, vprev.p[2], f.p[2], c1, c2, c, idx, zero);
}
// 1 / diag of the three velocity rows (interior rows; 0 elsewhere), once per set of coefficients: the first sweep of every smoothing
// sequence starts from the zero guess, v1 = -c2 f / diag, and used to rebuild the diagonal from ~30 viscosity loads per node
__global__ __launch_bounds__(256) void k3_dinv(Op3 op, W3 dinv) {
    K3_PROLOGUE(op.g)
    long long moff;
    dinv.p[0][c] = cls3<0>(op, idx, moff) == C3_INT ? pl_rcp(diag3<0>(op, c, idx)) : 0.0;
    dinv.p[1][c] = cls3<1>(op, idx, moff) == C3_INT ? pl_rcp(diag3<1>(op, c, idx)) : 0.0;
    dinv.p[2][c] = cls3<2>(op, idx, moff) == C3_INT ? pl_rcp(diag3<2>(op, c, idx)) : 0.0;
}
template <int D> __device__ inline double cheb0_3(const Op3& op, int cl, const int* idx, double r) {
    return (cl == C3_SLAVE && op.noslip != 0) ? fac3<D>(op, idx) * r : r;
}
// v1 = -c2 f / diag at the row's master (a slave evaluates its master's update: the same numbers as k3_cheb with zero != 0)
__global__ __launch_bounds__(256) void k3_cheb0(Op3 op, V3 f, V3 dinv, W3 vnext, double c2) {
    K3_PROLOGUE(op.g)
    long long moff;
    int cl = cls3<0>(op, idx, moff);
    vnext.p[0][c] = cl == C3_ZERO ? 0.0 : cheb0_3<0>(op, cl, idx, (-c2 * f.p[0][c + moff]) * dinv.p[0][c + moff]);
    cl = cls3<1>(op, idx, moff);
    vnext.p[1][c] = cl == C3_ZERO ? 0.0 : cheb0_3<1>(op, cl, idx, (-c2 * f.p[1][c + moff]) * dinv.p[1][c + moff]);
    cl = cls3<2>(op, idx, moff);
    vnext.p[2][c] = cl == C3_ZERO ? 0.0 : cheb0_3<2>(op, cl, idx, (-c2 * f.p[2][c + moff]) * dinv.p[2][c + moff]);
}
// mode 0: r = f - A v on interior rows (0 elsewhere); mode 1: y = D^-1 A v with closure (power iteration)
template <int D> __device__ inline double resid3(const Op3& op, const double* const* v, const double* __restrict__ f, long long c,
                                                 const int* idx, int mode) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    if (cl == C3_ZERO || (mode == 0 && cl != C3_INT)) return 0.0;
    const long long cm = c + moff;
    int im[3] = {idx[0], idx[1], idx[2]};
    if (cl == C3_SLAVE) {
        if (idx[E] == 0) im[E] = 1; else if (idx[E] == op.g.gn[E] - 2) im[E] = op.g.gn[E] - 3;
        if (idx[F] == 0) im[F] = 1; else if (idx[F] == op.g.gn[F] - 2) im[F] = op.g.gn[F] - 3;
    }
    double Av, dg;
    row3<D>(op, v, cm, im, Av, dg);
    if (mode == 0) return f[c] - Av;
    const double r = Av * pl_rcp(dg);
    return (cl == C3_SLAVE && op.noslip != 0) ? fac3<D>(op, idx) * r : r;
}
__global__ __launch_bounds__(256) void k3_resid(Op3 op, V3 vv, V3 f, W3 r, int mode, int rim_only) {
    K3_PROLOGUE(op.g)
    if (rim_only && k3_all_interior(op, idx)) return;
    const double* v[3] = {vv.p[0], vv.p[1], vv.p[2]};
    r.p[0][c] = resid3<0>(op, v, f.p[0], c, idx, mode);
    r.p[1][c] = resid3<1>(op, v, f.p[1], c, idx, mode);
    r.p[2][c] = resid3<2>(op, v, f.p[2], c, idx, mode);
}

// ---- LDS-tiled variants of the three heavy stencil kernels (round 4) ------------------------------------------------------------------------
// Counters (tools/pmc_passes.sh, profiles/r04_3d257_pmc.csv) say what binds the per-node kernels above: not HBM (the XCD-banded
// workgroup order cut k3_apply's traffic from 2.46x to 1.07x of the algorithmic bytes and made it 9 % SLOWER), not the branches (a
// branch-free rewrite with 114 registers: 29 % slower), but the NUMBER of 8-byte gather instructions -- 68 ... 129 per node, ~22 cycles
// of the CU's texture path each, whether they hit or not (time = 100 us + 11 us x loads per node over k3_cont_rows / k3_heat_apply /
// k3_apply).  Here a workgroup loads its 4 x 64 tile of the planes i-1, i, i+1 with a one-node rim ONCE, coalesced (23 ... 28 loads per
// thread instead of 88 ... 129), and evaluates the rows from LDS (ds_read: a quarter of the cycles of a gather).  Same thread <-> node
// mapping, same row functions (row3 / diag3 on an Op3 whose strides and viscosity pointers are the window's); the rare slaved rows (their
// master's stencil can leave the window) and symmetry rows take the global-memory path.  PYLAMP_3D_LDS=0 keeps the per-node kernels.
#define K3T_SR 68                        // row pitch of the window: 66 columns (k-1 .. k+64) padded
#define K3T_SP (6 * K3T_SR)              // plane pitch: 6 rows (j-1 .. j+4)
#define K3T_N (3 * K3T_SP)               // one array: 3 planes
// ---- z-marching variant: the workgroup keeps its tile and walks K3M_ZC planes --------------------------------------------------------------
// The window's three planes live in a ring of LDS slots; per step ONE new plane of every array is fetched (2 elements per thread and
// array, requested BEFORE the step's arithmetic and written behind it: the latency is hidden even at two workgroups per CU), i.e.
// ~12 loads per node instead of 28 (tile-at-a-time) or 88 (per-node kernel).  The rows are row3's expressions on (plane slot, in-plane
// index) pairs.
#define K3M_ZC 32
struct K3Ring { int o[3]; };                         // LDS offsets of the planes i-1, i, i+1
template <int D, int dD, int dE, int dF> __device__ inline double k3r_at(const double* __restrict__ A, const K3Ring& r, int q) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    constexpr int dz = (D == 0 ? dD : 0) + (E == 0 ? dE : 0) + (F == 0 ? dF : 0);
    constexpr int dx = (D == 1 ? dD : 0) + (E == 1 ? dE : 0) + (F == 1 ? dF : 0);
    constexpr int dy = (D == 2 ? dD : 0) + (E == 2 ? dE : 0) + (F == 2 ? dF : 0);
    return A[r.o[1 + dz] + q + dx * K3T_SR + dy];
}
// row3 on the ring (same expressions, same order)
// the spacing-table entries a node's rows use, per axis a: 1/(c[i+1]-c[i]), the same one node lower, 1/(c[i+1]-c[i-1]), the same one node
// higher.  The marching kernel loads the x and y entries ONCE per thread and the z entries once per plane (scalar loads share the LDS
// counter: one inside the row evaluation drains the LDS pipeline each time)
struct K3Tab { double rd[3], rdm[3], rD[3], rDp[3]; };
template <int D> __device__ inline void row3r(const K3Tab& tb, const double* const* __restrict__ V, const double* __restrict__ ES, const double* __restrict__ EN,
                                               const K3Ring& r, const K3Ring& rs, const K3Ring& rn, int q, double& Av, double& dg) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const double* __restrict__ u = V[D];
    const double rd_d = tb.rd[D], rd_dm = tb.rdm[D], rD_d = tb.rD[D];
    const double u0 = k3r_at<D, 0, 0, 0>(u, r, q);
    const double cN = 4.0 * k3r_at<D, 0, 0, 0>(EN, rn, q) * rd_d * rD_d, cS = 4.0 * k3r_at<D, -1, 0, 0>(EN, rn, q) * rd_dm * rD_d;
    double a = cN * (k3r_at<D, 1, 0, 0>(u, r, q) - u0) - cS * (u0 - k3r_at<D, -1, 0, 0>(u, r, q));
    double d = cN + cS;
    {
        const double rd_e = tb.rd[E], rD_e = tb.rD[E], rD_ep = tb.rDp[E];
        const double ep = 0.5 * (k3r_at<D, 0, 1, 0>(ES, rs, q) + k3r_at<D, 0, 1, 1>(ES, rs, q)), em = 0.5 * (k3r_at<D, 0, 0, 0>(ES, rs, q) + k3r_at<D, 0, 0, 1>(ES, rs, q));
        const double cE = 2.0 * ep * rD_ep * rd_e, cW = 2.0 * em * rD_e * rd_e;
        const double* __restrict__ w = V[E];
        a += cE * (k3r_at<D, 0, 1, 0>(u, r, q) - u0) - cW * (u0 - k3r_at<D, 0, -1, 0>(u, r, q)) +
             (2.0 * ep * rD_d * rd_e) * (k3r_at<D, 0, 1, 0>(w, r, q) - k3r_at<D, -1, 1, 0>(w, r, q)) -
             (2.0 * em * rD_d * rd_e) * (k3r_at<D, 0, 0, 0>(w, r, q) - k3r_at<D, -1, 0, 0>(w, r, q));
        d += cE + cW;
    }
    {
        const double rd_f = tb.rd[F], rD_f = tb.rD[F], rD_fp = tb.rDp[F];
        const double ep = 0.5 * (k3r_at<D, 0, 0, 1>(ES, rs, q) + k3r_at<D, 0, 1, 1>(ES, rs, q)), em = 0.5 * (k3r_at<D, 0, 0, 0>(ES, rs, q) + k3r_at<D, 0, 1, 0>(ES, rs, q));
        const double cE = 2.0 * ep * rD_fp * rd_f, cW = 2.0 * em * rD_f * rd_f;
        const double* __restrict__ w = V[F];
        a += cE * (k3r_at<D, 0, 0, 1>(u, r, q) - u0) - cW * (u0 - k3r_at<D, 0, 0, -1>(u, r, q)) +
             (2.0 * ep * rD_d * rd_f) * (k3r_at<D, 0, 0, 1>(w, r, q) - k3r_at<D, -1, 0, 1>(w, r, q)) -
             (2.0 * em * rD_d * rd_f) * (k3r_at<D, 0, 0, 0>(w, r, q) - k3r_at<D, -1, 0, 0>(w, r, q));
        d += cE + cW;
    }
    Av = a; dg = d;
}
// this thread's (up to 2) elements of one plane slab (6 rows x 66 columns): global offset within the plane li = 0, LDS offset, validity
// (addresses beyond the block's ring are clamped into it: every thread loads unconditionally -- a predicated load per array and element
//  was a basic block of its own with a branch, 24 per plane -- and what lands in those window entries is never read: the rows the
//  marching kernels evaluate are strictly inside the domain.  has2: this thread also carries one of the elements 256..395.)
struct K3PSlots { long long go[2]; int lo[2]; bool has2; };
__device__ inline K3PSlots k3m_slots(const G3& g, int lj0, int lk0) {
    K3PSlots q;
    const int tid = threadIdx.y * 64 + threadIdx.x;
    q.has2 = tid + 256 < 396;
#pragma unroll
    for (int u = 0; u < 2; u++) {
        const int e = min(tid + 256 * u, 395), r = e / 66, c = e % 66;
        const int lj = min(lj0 + r - 1, g.n[1]), lk = min(lk0 + c - 1, g.n[2]);
        q.go[u] = i3(g, 0, lj, lk);
        q.lo[u] = r * K3T_SR + c;
    }
    return q;
}
// strictly inside the domain in the two in-plane axes / in z: all four rows of such a node are interior rows (cls3 == C3_INT, cls3_p == 1
// but for the anchor cell, which k3_rim rewrites behind the marching kernel)
__device__ inline bool k3m_inside(const G3& g, int ax, int l) { const int gi = l + g.o[ax]; return l < g.n[ax] && gi >= 1 && gi <= g.gn[ax] - 3; }
// ---- the rim of the marching kernels: every node with a wall, slaved, ghost or symmetry row lies on one of the nine planes
// index in {0, n - 2, n - 1} of an axis (global indices), plus the pressure anchor.  One thread per rim node (~600 000 of 17 M at 257^3;
// a full-grid pass that only classifies took 169 us per launch): ALL rows of the node by the per-node row functions.
struct RimArgs { Op3 op; V4 x; W4 y; V3 vprev; V3 f; double c1, c2; int what, scaled; };       // what: 0 apply, 1 Chebyshev sweep, 2 residual
__device__ inline long long k3_rim_count(const G3& g) { return 3LL * g.n[1] * g.n[2] + 3LL * g.n[0] * g.n[2] + 3LL * g.n[0] * g.n[1] + 1; }
// (the marching kernels run this in workgroups of their own BEHIND the tiles -- the rim fills the tail of the launch instead of
//  a 35 us launch of its own; the anchor cell, strictly inside the domain, is a pressure row only: the tiles leave it alone)
__device__ __forceinline__ void k3_rim_body(const RimArgs& a, long long t) {
    const G3& g = a.op.g;
    const long long N[3] = {3LL * g.n[1] * g.n[2], 3LL * g.n[0] * g.n[2], 3LL * g.n[0] * g.n[1]};
    bool anchor_only = false;
    int l[3];
    auto rimpos = [&](int ax, int which) { const int gi = which == 0 ? 0 : g.gn[ax] - 3 + which; return gi - g.o[ax]; };      // 0, n-2, n-1 -> local
    auto on_rim = [&](int ax, int li) { const int gi = li + g.o[ax]; return gi == 0 || gi >= g.gn[ax] - 2; };
    if (t < N[0]) {                                         // z slabs: (which, j, k)
        const int w = (int)(t / ((long long)g.n[1] * g.n[2])); const long long r = t % ((long long)g.n[1] * g.n[2]);
        l[0] = rimpos(0, w); l[1] = (int)(r / g.n[2]); l[2] = (int)(r % g.n[2]);
    } else if ((t -= N[0]) < N[1]) {                        // x slabs: (which, i, k), without the z slabs' nodes
        const int w = (int)(t / ((long long)g.n[0] * g.n[2])); const long long r = t % ((long long)g.n[0] * g.n[2]);
        l[1] = rimpos(1, w); l[0] = (int)(r / g.n[2]); l[2] = (int)(r % g.n[2]);
        if (on_rim(0, l[0])) return;
    } else if ((t -= N[1]) < N[2]) {                        // y slabs: (which, i, j), without the others'
        const int w = (int)(t / ((long long)g.n[0] * g.n[1])); const long long r = t % ((long long)g.n[0] * g.n[1]);
        l[2] = rimpos(2, w); l[0] = (int)(r / g.n[1]); l[1] = (int)(r % g.n[1]);
        if (on_rim(0, l[0]) || on_rim(1, l[1])) return;
    } else if (t == N[2] && a.what == 0) {                  // the pressure anchor
        for (int q = 0; q < 3; q++) l[q] = a.op.anchor[q] - g.o[q];
        if (on_rim(0, l[0]) || on_rim(1, l[1]) || on_rim(2, l[2])) return;
        anchor_only = true;
    } else return;
    for (int q = 0; q < 3; q++) if (l[q] < 0 || l[q] >= g.n[q]) return;
    const long long c = i3(g, l[0], l[1], l[2]);
    const int idx[3] = {l[0] + g.o[0], l[1] + g.o[1], l[2] + g.o[2]};
    const int i = idx[0], j = idx[1], k = idx[2];
    const double* v[3] = {a.x.p[0], a.x.p[1], a.x.p[2]};
    if (a.what == 0) {
        const double* __restrict__ P = a.x.p[3];
        const bool SC = a.scaled != 0;
        if (!anchor_only) { a.y.p[0][c] = apply_vel3<0>(a.op, v, P, c, idx, SC); a.y.p[1][c] = apply_vel3<1>(a.op, v, P, c, idx, SC); a.y.p[2][c] = apply_vel3<2>(a.op, v, P, c, idx, SC); }
        long long moff;
        const int cl = cls3_p(a.op, idx, moff);
        double yp;
        if (cl == 0) yp = SC ? P[c] : a.op.Kc * P[c];
        else if (cl == 2) yp = SC ? (P[c + moff] - P[c]) : a.op.Kb * (P[c + moff] - P[c]);
        else {
            const double rz = TB(g.rd[0], i), rx = TB(g.rd[1], j), ry = TB(g.rd[2], k);
            const double div = (v[0][c + g.s[0]] - v[0][c]) * rz + (v[1][c + g.s[1]] - v[1][c]) * rx + (v[2][c + g.s[2]] - v[2][c]) * ry;
            yp = SC ? div * pl_rcp(rz + rx + ry) : a.op.Kc * div;
        }
        a.y.p[3][c] = yp;
    } else if (a.what == 1) {
        a.y.p[0][c] = cheb3<0>(a.op, v, a.vprev.p[0], a.f.p[0], a.c1, a.c2, c, idx, 0);
        a.y.p[1][c] = cheb3<1>(a.op, v, a.vprev.p[1], a.f.p[1], a.c1, a.c2, c, idx, 0);
        a.y.p[2][c] = cheb3<2>(a.op, v, a.vprev.p[2], a.f.p[2], a.c1, a.c2, c, idx, 0);
    } else {
        a.y.p[0][c] = resid3<0>(a.op, v, a.f.p[0], c, idx, 0); a.y.p[1][c] = resid3<1>(a.op, v, a.f.p[1], c, idx, 0); a.y.p[2][c] = resid3<2>(a.op, v, a.f.p[2], c, idx, 0);
    }
}
__global__ __launch_bounds__(256) void k3_rim(RimArgs a) { k3_rim_body(a, (long long)blockIdx.x * 256 + threadIdx.x); }
// Tile of a workgroup.  The hardware deals consecutive workgroup ids round-robin to the 8 XCDs, each with an L2 of its own; with the
// plain (k, j, z-chunk) order the neighbours that share a tile's halo rows and the cache lines of its halo columns sit on 8 different
// L2s and the halo is fetched from the fabric every time (measured: 2.6x the algorithmic bytes).  band != 0: XCD x gets the x-th eighth
// of the tile list, so neighbours meet in one L2.
struct K3Tile { int bx, by, bz; long long rim; };          // rim >= 0: not a tile -- the rim.th workgroup of the rim
__device__ inline K3Tile k3m_tile(const G3& g, int band, int zc) {
    const unsigned nx = (g.n[2] + 63) / 64, ny = (g.n[1] + 3) / 4, nz = (g.n[0] + zc - 1) / zc;
    const unsigned total = band == 2 ? nx * 8 * ((ny * nz + 7) / 8) : nx * ny * nz, id = blockIdx.x;
    if (id >= total) { K3Tile t; t.bx = t.by = t.bz = 0; t.rim = id - total; return t; }
    unsigned lid = id;
    if (band == 2) {       // the nx tiles of a k-row on ONE XCD (they share the cache lines of their halo columns); rows round-robin as before
        const unsigned xcd = id % 8, m = id / 8, R = (m / nx) * 8 + xcd;
        K3Tile t; t.bx = m % nx; t.by = R % ny; t.bz = R / ny; t.rim = R < ny * nz ? -1 : (1LL << 40);      // (padding: a rim index beyond the rim)
        return t;
    }
    if (band == 1) { const unsigned fl = total / 8, rem = total % 8, xcd = id % 8; lid = xcd * fl + min(xcd, rem) + id / 8; }
    K3Tile t; t.bx = lid % nx; t.by = (lid / nx) % ny; t.bz = lid / (nx * ny); t.rim = -1;
    return t;
}
template <bool SCALED>
__global__ __launch_bounds__(256, 3) void k3_apply_m(Op3 op, V4 x, W4 y, int band, int zc) {
    // rings: the velocities need the planes i-1, i, i+1 (3 slots), the shear viscosity i, i+1, the normal viscosity and the pressure
    // i-1, i (2 slots each): 48 KB -> three workgroups per CU
    __shared__ double WV[3][3 * K3T_SP];
    __shared__ double WS[2 * K3T_SP], WN[2 * K3T_SP], WP[2 * K3T_SP];
    const G3& g = op.g;
    const K3Tile tl = k3m_tile(g, band, zc);
    if (tl.rim >= 0) {
        RimArgs ra; ra.op = op; ra.x = x; ra.y = y; ra.what = 0; ra.scaled = SCALED ? 1 : 0; ra.c1 = ra.c2 = 0.0;
        for (int q = 0; q < 3; q++) ra.vprev.p[q] = ra.f.p[q] = nullptr;
        k3_rim_body(ra, tl.rim * 256 + threadIdx.y * 64 + threadIdx.x);
        return;
    }
    const int lj0 = tl.by * 4, lk0 = tl.bx * 64;
    const int z0 = tl.bz * zc, z1 = min(z0 + zc, g.n[0]);
    const K3PSlots ps = k3m_slots(g, lj0, lk0);
    const double* vg[3] = {x.p[0], x.p[1], x.p[2]};
    // element u of plane `plane` of the six arrays (velocities, shear / normal viscosity, pressure)
    const double* src6[6] = {vg[0], vg[1], vg[2], op.es, op.en, x.p[3]};
    auto fetch = [&](int m, int plane, int u) { return src6[m][ps.go[u] + (long long)plane * g.s[0]]; };
    // prologue: plane p of the velocities in slot (p + 3) % 3 ... of the 2-slot rings in slot (p + 2) % 2
#pragma unroll
    for (int u = 0; u < 2; u++) {
        if (u == 1 && !ps.has2) break;
        double t0[9], t1[6];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int m = 0; m < 3; m++) t0[3 * a + m] = fetch(m, z0 + a - 1, u);
        t1[0] = fetch(3, z0, u); t1[1] = fetch(3, z0 + 1, u); t1[2] = fetch(4, z0 - 1, u); t1[3] = fetch(4, z0, u);
        t1[4] = fetch(5, z0 - 1, u); t1[5] = fetch(5, z0, u);
        const int lo = ps.lo[u];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int m = 0; m < 3; m++) WV[m][((z0 + a - 1 + 3) % 3) * K3T_SP + lo] = t0[3 * a + m];
        WS[(z0 & 1) * K3T_SP + lo] = t1[0]; WS[((z0 + 1) & 1) * K3T_SP + lo] = t1[1];
        WN[((z0 + 1) & 1) * K3T_SP + lo] = t1[2]; WN[(z0 & 1) * K3T_SP + lo] = t1[3];
        WP[((z0 + 1) & 1) * K3T_SP + lo] = t1[4]; WP[(z0 & 1) * K3T_SP + lo] = t1[5];
    }
    __syncthreads();
    const int lk = lk0 + threadIdx.x, lj = lj0 + threadIdx.y;
    const bool mine_jk = k3m_inside(g, 1, lj) && k3m_inside(g, 2, lk);
    const bool anchor_jk = lj + g.o[1] == op.anchor[1] && lk + g.o[2] == op.anchor[2];
    const int q = (threadIdx.y + 1) * K3T_SR + (threadIdx.x + 1);
    const double* V[3] = {WV[0], WV[1], WV[2]};
    K3Tab tb;
    {
        const int j = min(lj, g.n[1] - 1) + g.o[1], k = min(lk, g.n[2] - 1) + g.o[2];
        tb.rd[1] = TB(g.rd[1], j); tb.rdm[1] = TB(g.rd[1], j - 1); tb.rD[1] = TB(g.rD[1], j); tb.rDp[1] = TB(g.rD[1], j + 1);
        tb.rd[2] = TB(g.rd[2], k); tb.rdm[2] = TB(g.rd[2], k - 1); tb.rD[2] = TB(g.rD[2], k); tb.rDp[2] = TB(g.rD[2], k + 1);
    }
    for (int li = z0; li < z1; li++) {
        {
            const int i = li + g.o[0];
            tb.rd[0] = TB(g.rd[0], i); tb.rdm[0] = TB(g.rd[0], i - 1); tb.rD[0] = TB(g.rD[0], i); tb.rDp[0] = TB(g.rD[0], i + 1);
        }
        // requested now, written behind the arithmetic: the planes li + 2 (velocities, shear viscosity) and li + 1 (normal viscosity, pressure)
        const bool more = li + 1 < z1;
        double tq[6], tq2[6];
        if (more) {
#pragma unroll
            for (int m = 0; m < 6; m++) tq[m] = fetch(m, m < 4 ? li + 2 : li + 1, 0);
            if (ps.has2) {
#pragma unroll
                for (int m = 0; m < 6; m++) tq2[m] = fetch(m, m < 4 ? li + 2 : li + 1, 1);
            }
        }
        K3Ring rv, rs, rn;
        rv.o[0] = ((li + 2) % 3) * K3T_SP; rv.o[1] = (li % 3) * K3T_SP; rv.o[2] = ((li + 1) % 3) * K3T_SP;        // (li - 1 + 3) % 3 = (li + 2) % 3
        rs.o[0] = 0; rs.o[1] = (li & 1) * K3T_SP; rs.o[2] = ((li + 1) & 1) * K3T_SP;
        rn.o[0] = ((li + 1) & 1) * K3T_SP; rn.o[1] = (li & 1) * K3T_SP; rn.o[2] = 0;
        if (mine_jk && k3m_inside(g, 0, li)) {
            // (nodes strictly inside the domain only: the walls, slaved, ghost and symmetry rows -- a rim two nodes thick -- and the
            //  anchor cell are k3_rim's, launched behind)
            const long long c = i3(g, li, lj, lk);
#define K3M_COMP(D)                                                                                                   \
            {                                                                                                         \
                double Av, dg;                                                                                        \
                row3r<D>(tb, V, WS, WN, rv, rs, rn, q, Av, dg);                                                       \
                Av -= 2.0 * op.Kc * tb.rD[D] * (k3r_at<D, 0, 0, 0>(WP, rn, q) - k3r_at<D, -1, 0, 0>(WP, rn, q));        \
                y.p[D][c] = SCALED ? Av * pl_rcp(dg) : Av;                                                            \
            }
            K3M_COMP(0) K3M_COMP(1) K3M_COMP(2)
#undef K3M_COMP
            const double rz = tb.rd[0], rx = tb.rd[1], ry = tb.rd[2];
            const double div = (WV[0][rv.o[2] + q] - WV[0][rv.o[1] + q]) * rz + (WV[1][rv.o[1] + q + K3T_SR] - WV[1][rv.o[1] + q]) * rx +
                               (WV[2][rv.o[1] + q + 1] - WV[2][rv.o[1] + q]) * ry;
            if (!(anchor_jk && li + g.o[0] == op.anchor[0])) y.p[3][c] = SCALED ? div * pl_rcp(rz + rx + ry) : op.Kc * div;
        }
        __syncthreads();                              // everybody has read the oldest planes
        if (more) {
            const int sl[6] = {((li + 2) % 3) * K3T_SP, ((li + 2) % 3) * K3T_SP, ((li + 2) % 3) * K3T_SP, (li & 1) * K3T_SP, ((li + 1) & 1) * K3T_SP, ((li + 1) & 1) * K3T_SP};
            double* const dst6[6] = {WV[0], WV[1], WV[2], WS, WN, WP};
#pragma unroll
            for (int m = 0; m < 6; m++) dst6[m][sl[m] + ps.lo[0]] = tq[m];
            if (ps.has2) {
#pragma unroll
                for (int m = 0; m < 6; m++) dst6[m][sl[m] + ps.lo[1]] = tq2[m];
            }
        }
        __syncthreads();
    }
}
// the smoother / residual on the same rings (no pressure): MODE 0 one Chebyshev sweep from a non-zero iterate, 1 residual f - A v
template <int MODE>
__global__ __launch_bounds__(256, 3) void k3_sweep_m(Op3 op, V3 vcur, V3 vprev, V3 f, W3 out, double c1, double c2, int band, int zc) {
    __shared__ double WV[3][3 * K3T_SP];
    __shared__ double WS[2 * K3T_SP], WN[2 * K3T_SP];
    const G3& g = op.g;
    const K3Tile tl = k3m_tile(g, band, zc);
    if (tl.rim >= 0) {
        RimArgs ra; ra.op = op; ra.what = MODE == 0 ? 1 : 2; ra.scaled = 0; ra.c1 = c1; ra.c2 = c2; ra.vprev = vprev; ra.f = f;
        for (int q = 0; q < 3; q++) { ra.x.p[q] = vcur.p[q]; ra.y.p[q] = out.p[q]; }
        ra.x.p[3] = nullptr; ra.y.p[3] = nullptr;
        k3_rim_body(ra, tl.rim * 256 + threadIdx.y * 64 + threadIdx.x);
        return;
    }
    const int lj0 = tl.by * 4, lk0 = tl.bx * 64;
    const int z0 = tl.bz * zc, z1 = min(z0 + zc, g.n[0]);
    const K3PSlots ps = k3m_slots(g, lj0, lk0);
    const double* vg[3] = {vcur.p[0], vcur.p[1], vcur.p[2]};
    const double* src5[5] = {vg[0], vg[1], vg[2], op.es, op.en};
    auto fetch = [&](int m, int plane, int u) { return src5[m][ps.go[u] + (long long)plane * g.s[0]]; };
#pragma unroll
    for (int u = 0; u < 2; u++) {
        if (u == 1 && !ps.has2) break;
        double t0[9], t1[4];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int m = 0; m < 3; m++) t0[3 * a + m] = fetch(m, z0 + a - 1, u);
        t1[0] = fetch(3, z0, u); t1[1] = fetch(3, z0 + 1, u); t1[2] = fetch(4, z0 - 1, u); t1[3] = fetch(4, z0, u);
        const int lo = ps.lo[u];
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int m = 0; m < 3; m++) WV[m][((z0 + a - 1 + 3) % 3) * K3T_SP + lo] = t0[3 * a + m];
        WS[(z0 & 1) * K3T_SP + lo] = t1[0]; WS[((z0 + 1) & 1) * K3T_SP + lo] = t1[1];
        WN[((z0 + 1) & 1) * K3T_SP + lo] = t1[2]; WN[(z0 & 1) * K3T_SP + lo] = t1[3];
    }
    __syncthreads();
    const int lk = lk0 + threadIdx.x, lj = lj0 + threadIdx.y;
    const bool mine_jk = k3m_inside(g, 1, lj) && k3m_inside(g, 2, lk);
    const int q = (threadIdx.y + 1) * K3T_SR + (threadIdx.x + 1);
    const double* V[3] = {WV[0], WV[1], WV[2]};
    K3Tab tb;
    {
        const int j = min(lj, g.n[1] - 1) + g.o[1], k = min(lk, g.n[2] - 1) + g.o[2];
        tb.rd[1] = TB(g.rd[1], j); tb.rdm[1] = TB(g.rd[1], j - 1); tb.rD[1] = TB(g.rD[1], j); tb.rDp[1] = TB(g.rD[1], j + 1);
        tb.rd[2] = TB(g.rd[2], k); tb.rdm[2] = TB(g.rd[2], k - 1); tb.rD[2] = TB(g.rD[2], k); tb.rDp[2] = TB(g.rD[2], k + 1);
    }
    for (int li = z0; li < z1; li++) {
        {
            const int i = li + g.o[0];
            tb.rd[0] = TB(g.rd[0], i); tb.rdm[0] = TB(g.rd[0], i - 1); tb.rD[0] = TB(g.rD[0], i); tb.rDp[0] = TB(g.rD[0], i + 1);
        }
        const bool more = li + 1 < z1;
        double tq[5], tq2[5];
        if (more) {
#pragma unroll
            for (int m = 0; m < 5; m++) tq[m] = fetch(m, m < 4 ? li + 2 : li + 1, 0);
            if (ps.has2) {
#pragma unroll
                for (int m = 0; m < 5; m++) tq2[m] = fetch(m, m < 4 ? li + 2 : li + 1, 1);
            }
        }
        K3Ring rv, rs, rn;
        rv.o[0] = ((li + 2) % 3) * K3T_SP; rv.o[1] = (li % 3) * K3T_SP; rv.o[2] = ((li + 1) % 3) * K3T_SP;
        rs.o[0] = 0; rs.o[1] = (li & 1) * K3T_SP; rs.o[2] = ((li + 1) & 1) * K3T_SP;
        rn.o[0] = ((li + 1) & 1) * K3T_SP; rn.o[1] = (li & 1) * K3T_SP; rn.o[2] = 0;
        if (mine_jk && k3m_inside(g, 0, li)) {
            const long long c = i3(g, li, lj, lk);
#define K3M_COMP(D)                                                                                                   \
            {                                                                                                         \
                double Av, dg;                                                                                        \
                row3r<D>(tb, V, WS, WN, rv, rs, rn, q, Av, dg);                                                       \
                if (MODE == 0) {                                                                                      \
                    const double v0 = WV[D][rv.o[1] + q];                                                             \
                    const double mom = (c1 != 0.0) ? c1 * (v0 - (vprev.p[D] ? vprev.p[D][c] : 0.0)) : 0.0;            \
                    out.p[D][c] = v0 + mom + (c2 * (Av - f.p[D][c])) * pl_rcp(dg);                                    \
                } else out.p[D][c] = f.p[D][c] - Av;                                                                  \
            }
            K3M_COMP(0) K3M_COMP(1) K3M_COMP(2)
#undef K3M_COMP
        }
        __syncthreads();
        if (more) {
            const int sl[5] = {((li + 2) % 3) * K3T_SP, ((li + 2) % 3) * K3T_SP, ((li + 2) % 3) * K3T_SP, (li & 1) * K3T_SP, ((li + 1) & 1) * K3T_SP};
            double* const dst5[5] = {WV[0], WV[1], WV[2], WS, WN};
#pragma unroll
            for (int m = 0; m < 5; m++) dst5[m][sl[m] + ps.lo[0]] = tq[m];
            if (ps.has2) {
#pragma unroll
                for (int m = 0; m < 5; m++) dst5[m][sl[m] + ps.lo[1]] = tq2[m];
            }
        }
        __syncthreads();
    }
}
// (measured at 257^3, profiles/r04_3d257_banded_pmc.csv: banding cuts k3_apply_m's fetch from 2091 to 1218 MB per launch and its time
//  goes UP from 455 to 517 us -- the kernel is not bound by fabric traffic; off unless PYLAMP_3D_BAND=1)
// PYLAMP_3D_BAND = 2 (the default): only the tiles of one k-row share an XCD -- they share the cache lines of their halo COLUMNS, the rows
// stay dealt round-robin: k3_apply_m 0.425 -> 0.410 ms (0.41 of the HBM roof on the algorithmic bytes); 0: plain order
static int k3_band() { static const int on = getenv("PYLAMP_3D_BAND") ? atoi(getenv("PYLAMP_3D_BAND")) : 2; return on; }
// planes a workgroup walks: K3M_ZC, shorter on the smaller levels until the launch has ~2 workgroups per slot of the chip (3 per CU)
static int k3m_zc(const G3& g) {
    const long long tiles = (long long)((g.n[2] + 63) / 64) * ((g.n[1] + 3) / 4);
    int zc = K3M_ZC;
    while (zc > 8 && tiles * ((g.n[0] + zc - 1) / zc) < 1536) zc >>= 1;
    return zc;
}
static dim3 grid3m(const G3& g) {          // the tiles, then the rim (one thread per rim node)
    const int zc = k3m_zc(g);
    const long long rim = 3LL * g.n[1] * g.n[2] + 3LL * g.n[0] * g.n[2] + 3LL * g.n[0] * g.n[1] + 1;
    const long long nx = (g.n[2] + 63) / 64, rows = (long long)((g.n[1] + 3) / 4) * ((g.n[0] + zc - 1) / zc);
    return dim3((unsigned)((k3_band() == 2 ? nx * 8 * ((rows + 7) / 8) : nx * rows) + (rim + 255) / 256));
}
static bool k3_use_lds(const G3& g) {
    static const bool on = !(getenv("PYLAMP_3D_LDS") && atoi(getenv("PYLAMP_3D_LDS")) == 0);
    return on && (long long)g.n[0] * g.n[1] * g.n[2] >= 200000;        // the small (latency-bound) levels keep the per-node kernels
}

// full-weighting restriction: vertex-centred [1/4 1/2 1/4] along the component's own axis, cell-centred [1/8 3/8 3/8 1/8]
// along the other two (uniform-grid weights)
template <int D> __device__ inline double restrict3(const G3& gf, const Op3& opc, const double* __restrict__ rf, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    long long moff;
    if (cls3<D>(opc, idx, moff) != C3_INT) return 0.0;
    const long long b = i3(gf, 2 * idx[0] - gf.o[0], 2 * idx[1] - gf.o[1], 2 * idx[2] - gf.o[2]);
    const double wv[3] = {0.25, 0.5, 0.25}, wc[4] = {0.125, 0.375, 0.375, 0.125};
    double acc = 0.0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double s1 = 0.0;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            double s2 = 0.0;
#pragma unroll
            for (int p = 0; p < 4; p++) s2 += wc[p] * rf[b + (a - 1) * gf.s[D] + (q - 1) * gf.s[E] + (p - 1) * gf.s[F]];
            s1 += wc[q] * s2;
        }
        acc += wv[a] * s1;
    }
    return acc;
}
__global__ __launch_bounds__(256) void k3_restrict(G3 gf, Op3 opc, V3 rf, W3 fc) {
    K3_PROLOGUE(opc.g)
    fc.p[0][c] = restrict3<0>(gf, opc, rf.p[0], idx);
    fc.p[1][c] = restrict3<1>(gf, opc, rf.p[1], idx);
    fc.p[2][c] = restrict3<2>(gf, opc, rf.p[2], idx);
}
// (P e)_D at a fine node: linear along the own axis, 3/4-1/4 (clamped) along the other two
template <int D> __device__ inline double prolong3_at(const G3& gc, const double* __restrict__ e, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    const int d0 = idx[D] >> 1, d1 = (idx[D] + 1) >> 1;
    int en_ = idx[E] >> 1, eo = (idx[E] & 1) ? en_ + 1 : en_ - 1;
    int fn = idx[F] >> 1, fo = (idx[F] & 1) ? fn + 1 : fn - 1;
    const int emax = gc.gn[E] - 2, fmax = gc.gn[F] - 2;
    en_ = min(max(en_, 0), emax); eo = min(max(eo, 0), emax); fn = min(max(fn, 0), fmax); fo = min(max(fo, 0), fmax);
    auto at = [&](int a, int b_, int c_) {
        int id[3]; id[D] = a; id[E] = b_; id[F] = c_;
        return e[i3(gc, id[0] - gc.o[0], id[1] - gc.o[1], id[2] - gc.o[2])];
    };
    auto lin = [&](int b_, int c_) { return 0.5 * (at(d0, b_, c_) + at(d1, b_, c_)); };
    return 0.75 * (0.75 * lin(en_, fn) + 0.25 * lin(en_, fo)) + 0.25 * (0.75 * lin(eo, fn) + 0.25 * lin(eo, fo));
}
template <int D> __device__ inline double prolong3(const Op3& opf, const G3& gc, const double* __restrict__ e, const double* __restrict__ vin,
                                                   long long c, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    long long moff;
    const int cl = cls3<D>(opf, idx, moff);
    if (cl == C3_ZERO) return 0.0;
    int im[3] = {idx[0], idx[1], idx[2]};
    if (cl == C3_SLAVE) {
        if (idx[E] == 0) im[E] = 1; else if (idx[E] == opf.g.gn[E] - 2) im[E] = opf.g.gn[E] - 3;
        if (idx[F] == 0) im[F] = 1; else if (idx[F] == opf.g.gn[F] - 2) im[F] = opf.g.gn[F] - 3;
    }
    const double r = vin[c + moff] + prolong3_at<D>(gc, e, im);
    return (cl == C3_SLAVE && opf.noslip != 0) ? fac3<D>(opf, idx) * r : r;
}
__global__ __launch_bounds__(256) void k3_prolong_add(Op3 opf, G3 gc, V3 ec, V3 vin, W3 vout) {
    K3_PROLOGUE(opf.g)
    vout.p[0][c] = prolong3<0>(opf, gc, ec.p[0], vin.p[0], c, idx);
    vout.p[1][c] = prolong3<1>(opf, gc, ec.p[1], vin.p[1], c, idx);
    vout.p[2][c] = prolong3<2>(opf, gc, ec.p[2], vin.p[2], c, idx);
}
// arithmetic viscosity coarsening: nodes by [1 2 1]^3 / 64 (edge-clamped), centres by the mean of the 8 covered fine cells
__global__ __launch_bounds__(256) void k3_coarsen(G3 gf, const double* __restrict__ esf, const double* __restrict__ enf, G3 gc,
                                                  double* __restrict__ esc, double* __restrict__ enc) {
    K3_PROLOGUE(gc)
    double acc = 0.0;
    for (int a = -1; a <= 1; a++)
        for (int q = -1; q <= 1; q++)
            for (int p = -1; p <= 1; p++) {
                const int fi = min(max(2 * i + a, 0), gf.gn[0] - 1), fj = min(max(2 * j + q, 0), gf.gn[1] - 1), fk = min(max(2 * k + p, 0), gf.gn[2] - 1);
                acc += (a == 0 ? 2.0 : 1.0) * (q == 0 ? 2.0 : 1.0) * (p == 0 ? 2.0 : 1.0) * esf[i3(gf, fi - gf.o[0], fj - gf.o[1], fk - gf.o[2])];
            }
    esc[c] = acc * (1.0 / 64.0);
    const int ci = min(i, gc.gn[0] - 2), cj = min(j, gc.gn[1] - 2), ck = min(k, gc.gn[2] - 2);      // ghost entries copy their neighbour
    const long long b = i3(gf, 2 * ci - gf.o[0], 2 * cj - gf.o[1], 2 * ck - gf.o[2]);
    double s = 0.0;
    for (int a = 0; a < 2; a++) for (int q = 0; q < 2; q++) for (int p = 0; p < 2; p++) s += enf[b + a * gf.s[0] + q * gf.s[1] + p * gf.s[2]];
    enc[c] = 0.125 * s;
}
// make x satisfy the constraint rows of A x = b exactly (bs = scaled b): walls / ghosts x = bs, slaves x = (v_slave / v_master) x_master + bs
template <int D> __device__ inline void close3(const Op3& op, double* __restrict__ x, const double* __restrict__ bs, long long c, const int* idx) {
    long long moff;
    const int cl = cls3<D>(op, idx, moff);
    if (cl == C3_ZERO) x[c] = bs[c];
    else if (cl == C3_SLAVE) {
        if (!op.noslip) { x[c] = x[c + moff] + bs[c]; return; }
        // On a cube edge the row couples along E to a node that is itself slaved along F: that node's right-hand side comes along the
        // chain, x = gamma_E (gamma_F x_master + bs_nb) + bs.  It is non-zero next to a moving wall (or in a given right-hand side).
        constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
        const int* n = op.g.gn;
        double b = bs[c];
        if ((idx[E] == 0 || idx[E] == n[E] - 2) && (idx[F] == 0 || idx[F] == n[F] - 2)) {
            const int hi = idx[E] != 0;
            const double bn = bs[hi ? c - op.g.s[E] : c + op.g.s[E]];
            if (bn != 0.0) b += gam3<E>(op, hi) * bn;
        }
        x[c] = fac3<D>(op, idx) * x[c + moff] + b;
    }
}
__global__ __launch_bounds__(256) void k3_close(Op3 op, W3 x, V3 bs) {
    K3_PROLOGUE(op.g)
    close3<0>(op, x.p[0], bs.p[0], c, idx);
    close3<1>(op, x.p[1], bs.p[1], c, idx);
    close3<2>(op, x.p[2], bs.p[2], c, idx);
}

// ---- flat vector kernels (the ring / padding entries of every vector are zero and stay zero) ----------------------
__global__ void k3_axpby(long long n, double* __restrict__ y, double a, const double* __restrict__ x, double b, const double* __restrict__ z) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) y[t] = a * x[t] + b * z[t];
}
__global__ void k3_p_update(long long n, double* __restrict__ p, const double* __restrict__ r, const double* __restrict__ v, double beta, double omega) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) p[t] = r[t] + beta * (p[t] - omega * v[t]);
}
__global__ void k3_xr_update(long long n, double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, double* __restrict__ r,
                             const double* __restrict__ s, const double* __restrict__ t_, double alpha, double omega) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        x[t] += alpha * y[t] + omega * z[t]; r[t] = s[t] - omega * t_[t];
    }
}
// The extrapolated start of a warm Stokes solve: x = sum_k l[k] h[k] over the n kept solutions, newest first and summed in that order.
// (Every h[k] is zero on the rings and the padding, so x is.)
struct X0Start3 { const double* h[X0_HIST + 1]; double l[X0_HIST + 1]; int n; };
__global__ void k3_x0_start(long long n, X0Start3 a, double* __restrict__ x) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        double acc = a.l[0] * a.h[0][t];
        for (int k = 1; k < a.n; k++) acc += a.l[k] * a.h[k][t];
        x[t] = acc;
    }
}
#define D3_BLOCKS 1024
// (every reduction kernel below ends in r3_block of pl_reduce3.h with all-sum slots: part[NQ b + q] = the sum of acc[q] over workgroup b)
// up to five dot products in one pass: part[5 b + q] = sum a_q[t] b_q[t]
struct Dot5 { const double* a[5]; const double* b[5]; int n; };
__global__ __launch_bounds__(256) void k3_dots(long long n, Dot5 d, double* __restrict__ part) {
    double acc[5] = {0, 0, 0, 0, 0};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < n; t += (long long)gridDim.x * 256)
        for (int q = 0; q < d.n; q++) acc[q] += d.a[q][t] * d.b[q][t];
    r3_block<R3All<R3_SUM, 5>>(acc, threadIdx.x, blockIdx.x, part);
}
// The second reduction point of BiCGStab with everything the velocity-error estimate needs, in ONE pass (one rank; vectors of 4 consecutive
// arrays of `vol` elements, the pressure array last): part[11 b + ..] = t.s, t.t, r~.s, r~.t, s.s | the same three of the pressure array
// (t.s, t.t, s.s: the continuity part of |s - omega t|^2 follows) | |(x + dx)_vel|^2 | yw.s_p, yw.t_p (the anchor-mode term).
// Until round 4 the estimate cost three more passes and three more host synchronisations per late iteration.
struct Fuse11 { const double* t; const double* s; const double* rt; const double* x; const double* dx; const double* yw; long long vol; };
__global__ __launch_bounds__(256) void k3_dots11(Fuse11 a, double* __restrict__ part) {
    double acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    const long long n = 4 * a.vol, np = 3 * a.vol;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double T = a.t[e], S = a.s[e], R = a.rt[e];
        acc[0] += T * S; acc[1] += T * T; acc[2] += R * S; acc[3] += R * T; acc[4] += S * S;
        if (e >= np) {
            acc[5] += T * S; acc[6] += T * T; acc[7] += S * S;
            if (a.yw) { const double Y = a.yw[e - np]; acc[9] += Y * S; acc[10] += Y * T; }
        } else if (a.x) { const double X = a.x[e] + (a.dx ? a.dx[e] : 0.0); acc[8] += X * X; }
    }
    r3_block<R3All<R3_SUM, 11>>(acc, threadIdx.x, blockIdx.x, part);
}
// x += alpha y + omega z, r = s - omega t, and the NEXT direction p = r + beta (p - omega v) in the same pass
__global__ void k3_xrp_update(long long n, double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z, double* __restrict__ r,
                              const double* __restrict__ s, const double* __restrict__ t_, double* __restrict__ p, const double* __restrict__ v,
                              double alpha, double omega, double beta) {
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (long long)gridDim.x * blockDim.x) {
        x[t] += alpha * y[t] + omega * z[t];
        const double rn = s[t] - omega * t_[t];
        r[t] = rn;
        p[t] = rn + beta * (p[t] - omega * v[t]);
    }
}
__global__ __launch_bounds__(256) void k3_random(G3 g, double* __restrict__ v, unsigned seed) {
    K3_PROLOGUE(g)
    unsigned h = (unsigned)(((unsigned)i * 73856093u) ^ ((unsigned)j * 19349663u) ^ ((unsigned)k * 83492791u)) ^ seed;
    h ^= h >> 16; h *= 0x7feb352du; h ^= h >> 15; h *= 0x846ca68bu; h ^= h >> 16;
    v[c] = (i < g.gn[0] - 1 && j < g.gn[1] - 1 && k < g.gn[2] - 1) ? (double)h * (2.0 / 4294967296.0) - 1.0 : 0.0;
}

// ---- heat ------------------------------------------------------------------------------------------------------------
struct Heat3 {
    G3 g;
    const double* kk[3];             // conductivity on the faces normal to z, x, y: kz at (z_i+1/2, x_j, y_k) ...
    const double* cdt;               // dt / (rho Cp) at the nodes
    const double* rdb[3];            // 1 / (mid[i] - mid[i-1]) per axis
    int bc[6];                       // z0, x0, y0, zL, xL, yL  (pylamp_diff.py: FIXTEMP 0 / FIXFLOW 1)
};
// pylamp_diff.py:99-179 extended: z-walls own their edges, then x-walls, then y-walls
template <bool SCALED> __global__ __launch_bounds__(256) void k3_heat_apply(Heat3 op, const double* __restrict__ T, double* __restrict__ y) {
    K3_PROLOGUE(op.g)
    const G3& g = op.g;
    const double t = T[c];
    double r, dg = 1.0;
    int wall = -1, ax = 0, hi = 0;
    for (int a = 0; a < 3 && wall < 0; a++) {
        if (idx[a] == 0) { wall = a; ax = a; hi = 0; }
        else if (idx[a] == g.gn[a] - 1) { wall = a + 3; ax = a; hi = 1; }
    }
    if (wall >= 0) {
        if (op.bc[wall] == PL_BC_FIXTEMP) r = t;
        else if (!hi) { const double kq = op.kk[ax][c] * TB(g.rd[ax], 0); r = kq * (T[c + g.s[ax]] - t); dg = -kq; }
        else { const double kq = op.kk[ax][c - g.s[ax]] * TB(g.rd[ax], g.gn[ax] - 2); r = kq * (t - T[c - g.s[ax]]); dg = kq; }
    } else {
        double fl = 0.0, dsum = 0.0;
        for (int a = 0; a < 3; a++) {
            const double kp = op.kk[a][c] * TB(g.rd[a], idx[a]), km = op.kk[a][c - g.s[a]] * TB(g.rd[a], idx[a] - 1);
            const double rb = TB(op.rdb[a], idx[a]);
            fl += (kp * (T[c + g.s[a]] - t) - km * (t - T[c - g.s[a]])) * rb;
            dsum += (kp + km) * rb;
        }
        const double cc = op.cdt[c];
        r = cc * fl - t;
        if (SCALED) dg = -cc * dsum - 1.0;
    }
    y[c] = SCALED ? r / dg : r;
}
// pl3_heat_set_wall_values: v[w] is the plane of wall w over its nodes, C-order (n_p, n_q) with p < q the two other axes in z, x, y order,
// or NULL where the wall keeps its one value bcv[w]
struct Heat3Planes { const double* v[6]; };
// PLANES = false: what a context without planes launches (pl is not read)
template <bool PLANES> __global__ __launch_bounds__(256) void k3_heat_rhs(Heat3 op, const double* __restrict__ Told, const double* __restrict__ H,
                                                                          const double* bcv, Heat3Planes pl, double* __restrict__ rhs, int scaled) {
    K3_PROLOGUE(op.g)
    const G3& g = op.g;
    int wall = -1, ax = 0, hi = 0;
    for (int a = 0; a < 3 && wall < 0; a++) {
        if (idx[a] == 0) { wall = a; ax = a; hi = 0; }
        else if (idx[a] == g.gn[a] - 1) { wall = a + 3; ax = a; hi = 1; }
    }
    double r, dg = 1.0;
    if (wall >= 0) {
        r = bcv[wall];
        if (PLANES && pl.v[wall]) {
            const int p = ax == 0 ? 1 : 0, q = ax == 2 ? 1 : 2;
            r = pl.v[wall][(long long)idx[p] * g.gn[q] + idx[q]];
        }
        if (op.bc[wall] != PL_BC_FIXTEMP) dg = hi ? op.kk[ax][c - g.s[ax]] * TB(g.rd[ax], g.gn[ax] - 2) : -op.kk[ax][c] * TB(g.rd[ax], 0);
    } else {
        r = -Told[c] - op.cdt[c] * H[c];
        if (scaled) {
            double dsum = 0.0;
            for (int a = 0; a < 3; a++)
                dsum += (op.kk[a][c] * TB(g.rd[a], idx[a]) + op.kk[a][c - g.s[a]] * TB(g.rd[a], idx[a] - 1)) * TB(op.rdb[a], idx[a]);
            dg = -op.cdt[c] * dsum - 1.0;
        }
    }
    rhs[c] = scaled ? r / dg : r;
}
__global__ __launch_bounds__(256) void k3_heat_coef(G3 g, const double* __restrict__ rho, const double* __restrict__ cp, double dt, double* __restrict__ out) {
    K3_PROLOGUE(g)
    out[c] = dt / (rho[c] * cp[c]);
}
// pl3_heat_budget (one rank): part[8 b + ..] = workgroup b's share of the heat flow into the box through z0, x0, y0, zL, xL, yL | the
// storage rate | the source, all sums over the INTERIOR nodes with the widths w_a = 1 / rdb_a of their control volumes -- the terms of the
// interior rows of k3_heat_apply times the volume, so that storage - source - the six wall flows telescopes to the rows' residual.  A node
// next to a wall (idx[a] == 1 or gn[a] - 2) carries that wall's face flux over its own w_p w_q.
__global__ __launch_bounds__(256) void k3_heat_budget(Heat3 op, const double* __restrict__ T, const double* __restrict__ Told, const double* __restrict__ H,
                                                      double* __restrict__ part) {
    const G3& g = op.g;
    const long long N = (long long)g.n[0] * g.n[1] * g.n[2];
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < N; t += (long long)gridDim.x * 256) {
        const int idx[3] = {(int)(t / ((long long)g.n[2] * g.n[1])), (int)((t / g.n[2]) % g.n[1]), (int)(t % g.n[2])};
        if (idx[0] == 0 || idx[0] == g.gn[0] - 1 || idx[1] == 0 || idx[1] == g.gn[1] - 1 || idx[2] == 0 || idx[2] == g.gn[2] - 1) continue;
        const long long c = i3(g, idx[0], idx[1], idx[2]);
        const double w[3] = {1.0 / TB(op.rdb[0], idx[0]), 1.0 / TB(op.rdb[1], idx[1]), 1.0 / TB(op.rdb[2], idx[2])};
        const double tc = T[c], V = w[0] * w[1] * w[2];
        acc[6] += (tc - Told[c]) / op.cdt[c] * V;
        acc[7] += H[c] * V;
        for (int a = 0; a < 3; a++) {
            const double area = w[a == 0 ? 1 : 0] * w[a == 2 ? 1 : 2];
            if (idx[a] == 1) acc[a] -= op.kk[a][c - g.s[a]] * (tc - T[c - g.s[a]]) * TB(g.rd[a], 0) * area;
            if (idx[a] == g.gn[a] - 2) acc[a + 3] += op.kk[a][c] * (T[c + g.s[a]] - tc) * TB(g.rd[a], g.gn[a] - 2) * area;
        }
    }
    r3_block<R3All<R3_SUM, 8>>(acc, threadIdx.x, blockIdx.x, part);
}

// ---- host <-> device layout ------------------------------------------------------------------------------------------
// host arrays are C-order (nz, nx, ny) [optionally with ncomp interleaved components last]
// (src / dst: the GLOBAL array; from_host also fills the ring of nodes around the block from it -- coefficient arrays need no exchange)
__global__ __launch_bounds__(256) void k3_from_host(G3 g, const double* __restrict__ src, int ncomp, int comp, double* __restrict__ dst) {
    const int lk = (int)(blockIdx.x * 64 + threadIdx.x) - 1, lj = (int)(blockIdx.y * 4 + threadIdx.y) - 1, li = (int)blockIdx.z - 1;
    if (lk > g.n[2] || lj > g.n[1]) return;
    const int i = li + g.o[0], j = lj + g.o[1], k = lk + g.o[2];
    if (i < 0 || i >= g.gn[0] || j < 0 || j >= g.gn[1] || k < 0 || k >= g.gn[2]) return;
    dst[i3(g, li, lj, lk)] = src[(((long long)i * g.gn[1] + j) * g.gn[2] + k) * ncomp + comp];
}
__global__ __launch_bounds__(256) void k3_to_host(G3 g, const double* __restrict__ src, int ncomp, int comp, double* __restrict__ dst) {
    K3_PROLOGUE(g)
    dst[(((long long)i * g.gn[1] + j) * g.gn[2] + k) * ncomp + comp] = src[c];
}
// one plane of nodes normal to `axis` (local index `plane`, -1 .. n: the rings included) of na arrays <-> a dense buffer; the other
// two axes run over -1 .. n, so that exchanging z, then x, then y carries the edge and corner nodes along (halo3)
struct Slab3 { double* a[4]; int na; };
__global__ __launch_bounds__(256) void k3_slab(G3 g, int axis, int plane, Slab3 sl, double* __restrict__ buf, int to_buf) {
    const int A1 = axis == 0 ? 1 : 0, A2 = axis == 2 ? 1 : 2;       // the two in-plane axes, the faster one second
    const int n1 = g.n[A1] + 2, n2 = g.n[A2] + 2;
    const long long per = (long long)n1 * n2, total = per * sl.na;
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < total; t += (long long)gridDim.x * 256) {
        const int q = (int)(t / per); const long long e = t % per;
        int id[3]; id[axis] = plane; id[A1] = (int)(e / n2) - 1; id[A2] = (int)(e % n2) - 1;
        double* p = sl.a[q] + i3(g, id[0], id[1], id[2]);
        if (to_buf) buf[t] = *p; else *p = buf[t];
    }
}
// up to five dot products over the OWNED nodes of na consecutive arrays per vector (several ranks: the rings hold the neighbours' values)
__global__ __launch_bounds__(256) void k3_dots_own(G3 g, int na, Dot5 d, double* __restrict__ part) {
    double acc[5] = {0, 0, 0, 0, 0};
    const long long rows = (long long)na * g.n[0] * g.n[1];
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const int q = (int)(r / ((long long)g.n[0] * g.n[1])); const int ij = (int)(r % ((long long)g.n[0] * g.n[1]));
        const long long base = (long long)q * g.vol + i3(g, ij / g.n[1], ij % g.n[1], 0);
        for (int kk = threadIdx.x; kk < g.n[2]; kk += 256)
            for (int u = 0; u < d.n; u++) acc[u] += d.a[u][base + kk] * d.b[u][base + kk];
    }
    r3_block<R3All<R3_SUM, 5>>(acc, threadIdx.x, blockIdx.x, part);
}
// sum |v| over the entries of na consecutive arrays that lie OUTSIDE the owned block (the ring of nodes in z and x, the padding of the
// y-lines): part[5 b] -- what the flat kernels above rely on being zero on one rank (pl3_stokes_ring_sum)
__global__ __launch_bounds__(256) void k3_ring_abs(G3 g, int na, const double* __restrict__ v, double* __restrict__ part) {
    double acc[5] = {0, 0, 0, 0, 0};
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g.vol; e += (long long)gridDim.x * 256) {
        const long long li = e / g.s[0] - 1, lj = (e % g.s[0]) / g.s[1] - 1, lk = e % g.s[1] - P3_PAD;
        if (li >= 0 && li < g.n[0] && lj >= 0 && lj < g.n[1] && lk >= 0 && lk < g.n[2]) continue;
        for (int q = 0; q < na; q++) acc[0] += fabs(v[q * g.vol + e]);
    }
    r3_block<R3All<R3_SUM, 5>>(acc, threadIdx.x, blockIdx.x, part);
}

// =====================================================================================================================
// host side
// =====================================================================================================================
// A Krylov vector: na (1, 3 or 4) consecutive arrays of g->vol elements each -- one allocation (need_vecs, need_hvecs).  Array q is
// v[q]; a 4-array Stokes vector is its velocity part vel() followed by its pressure part prs().
struct Vec3 {
    double* p; int na; const G3* g;
    long long n() const { return na * g->vol; }
    double* operator[](int q) const { return p + q * g->vol; }
    Vec3 part(int q, int nq) const { return Vec3{p + q * g->vol, nq, g}; }
    Vec3 vel() const { return part(0, 3); }
    Vec3 prs() const { return part(3, 1); }
};
struct G3Host { G3 d; std::vector<double> c[3]; double* tables = nullptr; };
struct Lev3 {
    G3Host gh; Op3 op{};
    double *es = nullptr, *en = nullptr; bool own = false;
    double* v[3][3] = {{nullptr}}; double* f[3] = {nullptr}; double* r[3] = {nullptr};
    double* dinv[3] = {nullptr, nullptr, nullptr};      // 1 / diag of the velocity rows (k3_dinv)
    double lmax = 3.0;
    double* eig[3] = {nullptr, nullptr, nullptr}; bool eig_valid = false;      // eigenvector of the last power iteration (warm restart)
};
struct pl3_ctx {
    bool have_x = false, have_T = false;      // a device-resident Stokes / heat solution exists (pl3_get_solution)
    int device = 0; hipStream_t stream = nullptr; hipEvent_t ev0 = nullptr, ev1 = nullptr;
    // several ranks (pl3_set_comm): Pz x Px x Py blocks of the node grid, rank = (pz Px + px) Py + py; the messages and host reductions
    // go through a 2-D context that carries the transport (native RCCL / callback table / in-process group, pl_comm.hip) and whose stream
    // this context then shares
    pl_ctx* comm = nullptr; bool own_stream = true;
    int P[3] = {1, 1, 1}, pc[3] = {0, 0, 0}, nranks = 1, rank = 0;
    int gn[3] = {0, 0, 0}; std::vector<double> gcoord[3];     // the global grid
    double* hbuf = nullptr; size_t hbuf_n = 0;                // halo exchange: send lo | send hi | recv lo | recv hi
    long long halo_calls = 0, reduce_calls = 0;
    // State of the RUNNING solve, not of the context: operator and preconditioner applications, counted by stokes_A3 / stokes_M3 / heat_A3
    // (plain functions of the context, so the counters live here).  pl3_stokes_solve and pl3_heat_solve reset them at their start.
    int napply = 0, nprec = 0;
    std::string err;
    G3Host geom;
    double *es = nullptr, *en = nullptr, *rho = nullptr; Op3 op{}; bool op_ready = false;
    int noslip = 0;                 // pl3_stokes_set_walls: bit w of [z0, x0, y0, zL, xL, yL] set = no-slip; kept across pl3_stokes_set_coeffs
    Pl3WallVel wallvel{};           // pl3_stokes_set_wall_velocity: U_w = (Uz, Ux, Uy) per wall and the mask of the moving ones; kept likewise
    // pl3_stokes_set_wall_flow: the six wall planes of the through-flow (over faces) and what the kernels take of them; kept likewise
    Walls3Planes flow; Pl3WallFlow wallflow{};
    std::vector<Lev3*> levels;
    double* vec[14] = {nullptr};                // BiCGStab work vectors: 4 consecutive arrays each (svec)
    double* part = nullptr; double* hpart = nullptr;
    double* stage = nullptr; size_t stage_bytes = 0;
    // heat
    Heat3 hop{}; bool hop_ready = false; double* hk[3] = {nullptr}; double *hT = nullptr, *hH = nullptr, *hcdt = nullptr, *hrho = nullptr, *hcp = nullptr;
    double* hbcv = nullptr; double* htab = nullptr; double* hvec[12] = {nullptr}; double hbcv_host[6] = {0};
    // pl3_heat_set_wall_values: the planes of the heat walls (over nodes) and what the kernels take of them; kept across pl3_heat_set_coeffs
    Walls3Planes hplanes; Heat3Planes hwall{};
    int nu = 2, nu_fine = 0; bool nu_set = false; int coarse_sweeps = 12; double cheb_ratio = 6.0;      // nu_fine: sweeps on the finest level (0 = nu)
    // deflation of the pressure-anchor mode (see pl_solver.hip): the vector w = A^-1 u lives in vec[13], kept between solves
    double *dfl_y = nullptr, *dfl_t = nullptr; bool dfl_valid = false;
    bool dfl_active = false; double dfl_yAw = 0.0, dfl_wvel2 = 0.0;      // of the running solve: the anchor-mode term of the error estimate
    // what the last pl3_stokes_solve did about it (pl3_stokes_defl_info): the deflation was on, the quality of the kept vector as measured
    // (-1: none), iterations and final residual of the inner solve (0 / -1: the vector was reused as it is), true-residual checks
    struct { int active = 0, inner_its = 0, checks = 0, rec_it = 0; double q = -1.0, inner_res = -1.0, rec[6] = {0, 0, 0, 0, 0, 0}; } dfl_last;
    // warm start (pl3_stokes_set_warm_start; off at creation): the last warm_held <= warm_points solutions, newest first, rotated by
    // pointer, and the model time steps between them as pl_x0_weights takes them (dt_hist[0] leads to the solution sought)
    int warm_points = 0, warm_order = 0, warm_held = 0;
    double* hist[X0_HIST + 1] = {nullptr}; double dt_hist[X0_HIST + 1] = {0};
    struct { int start = 0, used = 0; double r0 = 0.0, ref = 0.0, l[3] = {0, 0, 0}; } warm_last;      // of the last solve (pl3_stokes_history_info)
    double etol = 3e-8;                     // bound on the velocity-error estimate of a converged Stokes solve (PYLAMP_STOKES_ETOL)
    void* mic3 = nullptr;                   // pl_mic3.hip: resident tracers and the work buffers of the 3-D marker kernels
    void* step3 = nullptr;                  // pl_step3.hip: state of the device-resident time step
    // yield stress (pl3_stokes_set_yield; off at creation): es / en are then the EFFECTIVE viscosities of the operator, ms / mn the material
    // ones next to them (allocated once a yield stress is set); ytau: tau_y at the nodes z_i [0, nz) and at the cell mid-points [nz, 2 nz);
    // ypart: the per-workgroup partials of k3_yield_visc and, behind them, those of the first finishing launch.  mat_mineta: min(eta) of the material arrays as the last set_coeffs had it
    bool yield_on = false; double ytau0 = 0.0, ydtau = 0.0, yfloor = 0.0, mat_mineta = 0.0;
    double *ms = nullptr, *mn = nullptr, *ytau = nullptr, *ypart = nullptr;
    bool strain_kept = false;               // Stokes work vector 2 still holds the fields of the last pl3_stokes_strain_fields / resident step
    int64_t xfer[4] = {0, 0, 0, 0};         // host <-> device copies (pl3_transfer_stats): count and bytes of those of at least one node field, of the smaller ones
};
static thread_local std::string p3_tls_error;
static int p3_fail(pl3_ctx* ctx, const std::string& m) { if (ctx) ctx->err = m; p3_tls_error = m; return 1; }
#define P3_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return p3_fail(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
#define P3_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
void pl3_count_copy(pl3_ctx* ctx, size_t bytes) {
    const int c = bytes >= sizeof(double) * (size_t)ctx->gn[0] * ctx->gn[1] * ctx->gn[2] ? 0 : 2;
    ctx->xfer[c]++; ctx->xfer[c + 1] += (int64_t)bytes;
}
static std::string num_str3(double v) {          // the shortest decimal that reads back as v
    char b[40];
    for (int p = 15; p <= 17; p++) { snprintf(b, sizeof b, "%.*g", p, v); if (strtod(b, nullptr) == v) break; }
    return b;
}
// The one path of the planes over the walls (pl_walls3.h).  in[w]: the plane of wall w over its nodes or its faces, C-order, or NULL for
// none.  Every plane is checked first -- all entries, or with `owned` only those at nodes that wall w owns (the walls of an axis before a
// in the order z, x, y own the first and last line along it) -- then `also` (NULL: nothing) has its say; only then the stream is
// synchronised (kernels in flight may still read the planes), all six planes go up in one copy, and mask and offsets are committed: a
// rejected call changes nothing.  No plane at all clears: the buffer is freed.
static int planes3_set(pl3_ctx* ctx, Walls3Planes& P, const char* entry, const char* noun, bool nodes, bool owned, const double* const in[6],
                       int (*also)(pl3_ctx*, const double* const[6]) = nullptr) {
    Walls3Planes N;
    for (int w = 0; w < 6; w++) {
        N.off[w + 1] = N.off[w] + walls3_count(ctx->gn, w, nodes);
        if (!in || !in[w]) continue;
        N.mask |= 1 << w;
        int p, q;
        const int a = w % 3;
        walls3_axes(a, p, q);
        const int np = ctx->gn[p] - (nodes ? 0 : 1), nq = ctx->gn[q] - (nodes ? 0 : 1);
        const int i0 = owned && p < a ? 1 : 0, j0 = owned && q < a ? 1 : 0;
        for (int i = i0; i < np - i0; i++)
            for (int j = j0; j < nq - j0; j++) {
                const double u = in[w][(size_t)i * nq + j];
                if (!std::isfinite(u))
                    return p3_fail(ctx, std::string(entry) + ": wall " + walls3_names[w] + " has a non-finite " + noun + " [" + std::to_string(i) + ", " +
                                            std::to_string(j) + "] = " + num_str3(u));
            }
    }
    if (also) P3_TRY(also(ctx, in));
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!N.mask) {
        if (P.dev) (void)hipFree(P.dev);
        P = Walls3Planes{};
        return 0;
    }
    if (!P.dev) P3_HIP(ctx, hipMalloc((void**)&P.dev, N.off[6] * sizeof(double)));      // (P.mask is 0 here: nothing points into it yet)
    N.dev = P.dev;
    std::vector<double> all(N.off[6], 0.0);
    for (int w = 0; w < 6; w++) if ((N.mask >> w) & 1) std::copy(in[w], in[w] + N.count(w), all.begin() + N.off[w]);
    pl3_count_copy(ctx, N.off[6] * sizeof(double));
    P3_HIP(ctx, hipMemcpy(N.dev, all.data(), N.off[6] * sizeof(double), hipMemcpyHostToDevice));
    P = N;
    return 0;
}
// mask: bit w set = wall w has a plane; out[w] (NULL: not wanted) receives that wall's plane as the device holds it
static int planes3_get(pl3_ctx* ctx, const Walls3Planes& P, int* mask, double* const out[6]) {
    if (mask) *mask = P.mask;
    if (!out || !P.mask) return 0;
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int w = 0; w < 6; w++) {
        if (!out[w] || !P.plane(w)) continue;
        pl3_count_copy(ctx, P.count(w) * sizeof(double));
        P3_HIP(ctx, hipMemcpy(out[w], P.plane(w), P.count(w) * sizeof(double), hipMemcpyDeviceToHost));
    }
    return 0;
}
static Vec3 svec(pl3_ctx* ctx, int v) { return Vec3{ctx->vec[v], 4, &ctx->geom.d}; }          // Stokes work vector v
static Vec3 hvec(pl3_ctx* ctx, int v) { return Vec3{ctx->hvec[v], 1, &ctx->geom.d}; }         // heat work vector v
static Vec3 arr3(pl3_ctx* ctx, double* a) { return Vec3{a, 1, &ctx->geom.d}; }                // one array of the finest grid
// the arrays of a vector as the kernels and upload3 / download3 / halo3 take them
static W4 wv4(const Vec3& v) { W4 w{}; for (int q = 0; q < v.na; q++) w.p[q] = v[q]; return w; }
static V4 cv4(const Vec3& v) { V4 w{}; for (int q = 0; q < v.na; q++) w.p[q] = v[q]; return w; }
static W3 wv3(const Vec3& v) { W3 w; for (int q = 0; q < 3; q++) w.p[q] = v[q]; return w; }
static V3 cv3(const Vec3& v) { V3 w; for (int q = 0; q < 3; q++) w.p[q] = v[q]; return w; }
static V3 cv3(double* const* p) { V3 v; for (int q = 0; q < 3; q++) v.p[q] = p[q]; return v; }  // (a multigrid level's three arrays)
static W3 wv3(double* const* p) { W3 v; for (int q = 0; q < 3; q++) v.p[q] = p[q]; return v; }
// a per-node kernel over the block of g
template <typename K, typename... Args> static void launch3(pl3_ctx* ctx, const G3& g, K kernel, Args... args) {
    hipLaunchKernelGGL(kernel, grid3(g), dim3(64, 4), 0, ctx->stream, args...);
}

// gn / c: the GLOBAL grid of the level; the block of this rank follows from ctx->P / ctx->pc: C = (gn - 1) / P cells per block, first
// node pc C, the last block of an axis also owns the last node
static int g3_build(pl3_ctx* ctx, G3Host& gh, const int gn[3], const double* const c[3]) {
    G3& g = gh.d;
    int n[3];
    for (int a = 0; a < 3; a++) {
        if ((gn[a] - 1) % ctx->P[a]) return p3_fail(ctx, "3-D grid: (nodes - 1) must be divisible by the number of blocks along every axis");
        const int C = (gn[a] - 1) / ctx->P[a];
        g.gn[a] = gn[a]; g.o[a] = ctx->pc[a] * C; g.n[a] = n[a] = C + (ctx->pc[a] == ctx->P[a] - 1 ? 1 : 0);
        gh.c[a].assign(c[a], c[a] + gn[a]);
    }
    const long long py = ((P3_PAD + n[2] + 1 + 15) / 16) * 16;
    g.s[2] = 1; g.s[1] = py; g.s[0] = (long long)(n[1] + 2) * py;
    g.vol = (long long)(n[0] + 2) * g.s[0];
    for (int a = 0; a < 3; a++) n[a] = gn[a];                 // the tables are global
    size_t len[3], tot = 0;
    for (int a = 0; a < 3; a++) { len[a] = ((size_t)n[a] + 2 * PL_TOFF + 3) & ~(size_t)1; tot += 2 * len[a]; }
    std::vector<double> t(tot, 0.0);
    size_t off = 0, offs[3][2];
    for (int a = 0; a < 3; a++) {
        offs[a][0] = off; off += len[a]; offs[a][1] = off; off += len[a];
        for (int i = 0; i + 1 < n[a]; i++) t[offs[a][0] + i + PL_TOFF] = 1.0 / (c[a][i + 1] - c[a][i]);
        for (int i = 1; i + 1 < n[a]; i++) t[offs[a][1] + i + PL_TOFF] = 1.0 / (c[a][i + 1] - c[a][i - 1]);
    }
    if (gh.tables) (void)hipFree(gh.tables);
    P3_HIP(ctx, hipMalloc((void**)&gh.tables, tot * sizeof(double)));
    P3_HIP(ctx, hipMemcpy(gh.tables, t.data(), tot * sizeof(double), hipMemcpyHostToDevice));
    for (int a = 0; a < 3; a++) { g.rd[a] = gh.tables + offs[a][0]; g.rD[a] = gh.tables + offs[a][1]; }
    return 0;
}
static int dmal(pl3_ctx* ctx, double** p, long long n) {
    P3_HIP(ctx, hipMalloc((void**)p, (size_t)n * sizeof(double)));
    P3_HIP(ctx, hipMemsetAsync(*p, 0, (size_t)n * sizeof(double), ctx->stream));
    return 0;
}
static dim3 g1(long long n) { long long b = (n + 255) / 256; return dim3((unsigned)(b > 8192 ? 8192 : b)); }

extern "C" const char* pl3_last_error(const pl3_ctx* ctx) { return ctx ? ctx->err.c_str() : p3_tls_error.c_str(); }

// what the marker-in-cell unit (pl_mic3.hip) needs of a context
int pl3_fail(pl3_ctx* ctx, const std::string& m) { return p3_fail(ctx, m); }
int pl3_host_view(pl3_ctx* ctx, Pl3HostView* v) {
    if (!ctx) return p3_fail(nullptr, "3-D marker-in-cell: NULL context");
    v->device = ctx->device; v->stream = ctx->stream; v->nranks = ctx->nranks; v->slot = &ctx->mic3; v->wallflow = ctx->wallflow;
    for (int a = 0; a < 3; a++) { v->gn[a] = ctx->gn[a]; v->coord[a] = ctx->gcoord[a].data(); }
    return 0;
}

extern "C" int pl3_create(pl3_ctx** out, int device, int nz, int nx, int ny, const double* zc, const double* xc, const double* yc) {
    if (!out) return p3_fail(nullptr, "pl3_create: out is NULL");
    *out = nullptr;
    if (nz < 5 || nx < 5 || ny < 5 || !zc || !xc || !yc) return p3_fail(nullptr, "pl3_create: need at least 5 nodes per axis and the three coordinate arrays");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return p3_fail(nullptr, "pl3_create: no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return p3_fail(nullptr, "pl3_create: bad device index");
    pl3_ctx* ctx = new pl3_ctx();
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess) { delete ctx; return p3_fail(nullptr, "pl3_create: stream creation failed"); }
    const int n[3] = {nz, nx, ny}; const double* c[3] = {zc, xc, yc};
    for (int a = 0; a < 3; a++) { ctx->gn[a] = n[a]; ctx->gcoord[a].assign(c[a], c[a] + n[a]); }
    if (g3_build(ctx, ctx->geom, n, c)) { std::string m = ctx->err; delete ctx; return p3_fail(nullptr, m); }
    if (const char* e = getenv("PYLAMP_MG_NU3")) { int a = atoi(e); if (a >= 1 && a <= 6) { ctx->nu = a; ctx->nu_set = true; } }
    if (const char* e = getenv("PYLAMP_MG_NU3_FINE")) { int a = atoi(e); if (a >= 1 && a <= 6) ctx->nu_fine = a; }
    *out = ctx;
    return 0;
}
static void free_levels3(pl3_ctx* ctx) {
    for (Lev3* L : ctx->levels) {
        if (L->own) { (void)hipFree(L->es); (void)hipFree(L->en); }
        for (int b = 0; b < 3; b++) for (int q = 0; q < 3; q++) if (L->v[b][q]) (void)hipFree(L->v[b][q]);
        for (int q = 0; q < 3; q++) { if (L->f[q]) (void)hipFree(L->f[q]); if (L->r[q]) (void)hipFree(L->r[q]); if (L->eig[q]) (void)hipFree(L->eig[q]); if (L->dinv[q]) (void)hipFree(L->dinv[q]); }
        if (L->gh.tables) (void)hipFree(L->gh.tables);
        delete L;
    }
    ctx->levels.clear();
}
extern "C" void pl3_destroy(pl3_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    pl3_step_free(&ctx->step3);
    pl3_mic_free(&ctx->mic3);
    free_levels3(ctx);
    for (double* q : {ctx->es, ctx->en, ctx->rho, ctx->part, ctx->stage, ctx->hT, ctx->hH, ctx->hcdt, ctx->hrho, ctx->hcp, ctx->hbcv, ctx->htab, ctx->hbuf, ctx->flow.dev, ctx->hplanes.dev, ctx->ms, ctx->mn, ctx->ytau, ctx->ypart}) if (q) (void)hipFree(q);
    for (double* q : ctx->vec) if (q) (void)hipFree(q);
    for (double* q : ctx->hist) if (q) (void)hipFree(q);
    for (double* q : ctx->hk) if (q) (void)hipFree(q);
    for (double* q : ctx->hvec) if (q) (void)hipFree(q);
    if (ctx->hpart) (void)hipHostFree(ctx->hpart);
    if (ctx->geom.tables) (void)hipFree(ctx->geom.tables);
    (void)hipEventDestroy(ctx->ev0); (void)hipEventDestroy(ctx->ev1);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}
static int stage3(pl3_ctx* ctx, size_t bytes) {
    if (ctx->stage_bytes >= bytes) return 0;
    if (ctx->stage) { P3_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->stage); ctx->stage = nullptr; }
    P3_HIP(ctx, hipMalloc((void**)&ctx->stage, bytes));
    ctx->stage_bytes = bytes;
    return 0;
}
// host arrays are GLOBAL on every rank: the block and the ring of nodes around it are taken from them; a download assembles the global
// array from the blocks (own block + zeros, summed over the ranks)
static int upload3(pl3_ctx* ctx, const double* host, int ncomp, double* const* dst) {
    const G3& g = ctx->geom.d;
    const size_t bytes = (size_t)g.gn[0] * g.gn[1] * g.gn[2] * ncomp * sizeof(double);
    P3_TRY(stage3(ctx, bytes));
    pl3_count_copy(ctx, bytes);
    P3_HIP(ctx, hipMemcpyAsync(ctx->stage, host, bytes, hipMemcpyHostToDevice, ctx->stream));
    const dim3 gr((g.n[2] + 2 + 63) / 64, (g.n[1] + 2 + 3) / 4, g.n[0] + 2);
    for (int q = 0; q < ncomp; q++) hipLaunchKernelGGL(k3_from_host, gr, dim3(64, 4), 0, ctx->stream, g, (const double*)ctx->stage, ncomp, q, dst[q]);
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
static int download3(pl3_ctx* ctx, double* const* src, int ncomp, double* host) {
    const G3& g = ctx->geom.d;
    const size_t count = (size_t)g.gn[0] * g.gn[1] * g.gn[2] * ncomp, bytes = count * sizeof(double);
    P3_TRY(stage3(ctx, bytes));
    if (ctx->nranks > 1) P3_HIP(ctx, hipMemsetAsync(ctx->stage, 0, bytes, ctx->stream));
    for (int q = 0; q < ncomp; q++) launch3(ctx, g, k3_to_host, g, src[q], ncomp, q, ctx->stage);
    pl3_count_copy(ctx, bytes);
    P3_HIP(ctx, hipMemcpyAsync(host, ctx->stage, bytes, hipMemcpyDeviceToHost, ctx->stream));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->nranks > 1 && pl_allreduce_host(ctx->comm, host, (long long)count, 0)) return p3_fail(ctx, std::string("3-D download: ") + pl_last_error(ctx->comm));
    return 0;
}

// ---- several ranks: halo exchange and reductions ------------------------------------------------------------------------------
// One ring of nodes around the block is all the stencils reach (faces, the edge neighbours (i-1, j+1) ... of the momentum rows, and the
// corner nodes of the full-weighting restriction): exchanged axis by axis -- z planes, then x planes including the z ring just
// received, then y planes including both -- so that 6 messages carry all 26 neighbours' nodes.
static int halo3(pl3_ctx* ctx, const G3& g, double* const* arr, int na) {
    if (ctx->nranks <= 1) return 0;
    ctx->halo_calls++;
    for (int a = 0; a < 3; a++) {
        if (ctx->P[a] == 1) continue;
        int A1, A2;
        walls3_axes(a, A1, A2);
        const long long cnt = (long long)na * (g.n[A1] + 2) * (g.n[A2] + 2);
        if (ctx->hbuf_n < (size_t)(4 * cnt)) {
            if (ctx->hbuf) { P3_HIP(ctx, hipStreamSynchronize(ctx->stream)); (void)hipFree(ctx->hbuf); ctx->hbuf = nullptr; }
            P3_HIP(ctx, hipMalloc((void**)&ctx->hbuf, (size_t)(4 * cnt) * sizeof(double)));
            ctx->hbuf_n = (size_t)(4 * cnt);
        }
        Slab3 sl{}; sl.na = na; for (int q = 0; q < na; q++) sl.a[q] = arr[q];
        const bool lo = ctx->pc[a] > 0, hi = ctx->pc[a] < ctx->P[a] - 1;
        int step = 1; for (int b = a + 1; b < 3; b++) step *= ctx->P[b];          // rank distance of the neighbour along axis a
        const unsigned nb = (unsigned)std::min<long long>((cnt + 255) / 256, 2048);
        PlMsg m[2]; int nm = 0;
        if (lo) { hipLaunchKernelGGL(k3_slab, dim3(nb), dim3(256), 0, ctx->stream, g, a, 0, sl, ctx->hbuf, 1);
                  m[nm++] = PlMsg{ctx->rank - step, ctx->hbuf, cnt, ctx->hbuf + 2 * cnt, cnt}; }
        if (hi) { hipLaunchKernelGGL(k3_slab, dim3(nb), dim3(256), 0, ctx->stream, g, a, g.n[a] - 1, sl, ctx->hbuf + cnt, 1);
                  m[nm++] = PlMsg{ctx->rank + step, ctx->hbuf + cnt, cnt, ctx->hbuf + 3 * cnt, cnt}; }
        if (pl_comm_sendrecv(ctx->comm, m, nm)) return p3_fail(ctx, std::string("3-D halo exchange: ") + pl_last_error(ctx->comm));
        if (lo) hipLaunchKernelGGL(k3_slab, dim3(nb), dim3(256), 0, ctx->stream, g, a, -1, sl, ctx->hbuf + 2 * cnt, 0);
        if (hi) hipLaunchKernelGGL(k3_slab, dim3(nb), dim3(256), 0, ctx->stream, g, a, g.n[a], sl, ctx->hbuf + 3 * cnt, 0);
    }
    P3_HIP(ctx, hipGetLastError());
    return 0;
}
static int halo3(pl3_ctx* ctx, const Vec3& v) { return halo3(ctx, *v.g, wv4(v).p, v.na); }
static int allreduce3(pl3_ctx* ctx, double* v, int n, int op) {
    if (ctx->nranks <= 1) return 0;
    ctx->reduce_calls++;
    if (pl_allreduce_host(ctx->comm, v, n, op)) return p3_fail(ctx, std::string("3-D all-reduce: ") + pl_last_error(ctx->comm));
    return 0;
}
static int need_vecs(pl3_ctx* ctx, int nvec) {
    const long long vol = ctx->geom.d.vol;
    ctx->strain_kept = false;                   // whoever asks for work vectors may write them
    // the four arrays of a work vector are ONE allocation (array q at vec[v] + q vol): the flat vector kernels and the reductions
    // of BiCGStab take a whole vector per launch (and per host synchronisation)
    for (int v = 0; v < nvec; v++) if (!ctx->vec[v]) P3_TRY(dmal(ctx, &ctx->vec[v], 4 * vol));
    if (!ctx->part) {
        P3_TRY(dmal(ctx, &ctx->part, 11 * D3_BLOCKS));
        P3_HIP(ctx, hipHostMalloc((void**)&ctx->hpart, 11 * D3_BLOCKS * sizeof(double)));
    }
    return 0;
}

// Several ranks (right after pl3_create, before any coefficients): this context becomes rank `comm`'s rank of a Pz x Px x Py block
// layout, rank = (pz Px + px) Py + py.  comm: a 2-D context (pl_create on any small grid) whose communicator has been set
// (pl_set_comm / pl_set_comm_2d / pl_set_comm_local with Pz * Px = the number of ranks); it must outlive this context.
extern "C" int pl3_set_comm(pl3_ctx* ctx, pl_ctx* comm, int Pz, int Px, int Py) {
    if (!ctx || !comm) return p3_fail(ctx, "pl3_set_comm: NULL argument");
    if (Pz < 1 || Px < 1 || Py < 1 || Pz * Px * Py != comm->nranks) return p3_fail(ctx, "pl3_set_comm: Pz * Px * Py must equal the number of ranks of the communicator");
    if (ctx->op_ready || ctx->hop_ready || !ctx->levels.empty()) return p3_fail(ctx, "pl3_set_comm: call it right after pl3_create");
    if (ctx->warm_points) return p3_fail(ctx, "pl3_set_comm: the warm start of the Stokes solve (pl3_stokes_set_warm_start) runs on one rank; switch it off first");
    if (ctx->yield_on) return p3_fail(ctx, "pl3_set_comm: the yield stress (pl3_stokes_set_yield) runs on one rank; switch it off first");
    if (comm->device != ctx->device) return p3_fail(ctx, "pl3_set_comm: the communicator context lives on another device");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->own_stream) { (void)hipStreamDestroy(ctx->stream); ctx->own_stream = false; }
    ctx->stream = comm->stream;                      // messages are ordered with this context's kernels
    ctx->comm = comm; ctx->nranks = comm->nranks; ctx->rank = comm->rank;
    ctx->P[0] = Pz; ctx->P[1] = Px; ctx->P[2] = Py;
    ctx->pc[2] = ctx->rank % Py; ctx->pc[1] = (ctx->rank / Py) % Px; ctx->pc[0] = ctx->rank / (Py * Px);
    for (int a = 0; a < 3; a++)
        if (ctx->P[a] > 1 && (ctx->gn[a] - 1) / ctx->P[a] < 4) return p3_fail(ctx, "pl3_set_comm: at least 4 cells per block and axis");
    const double* c[3] = {ctx->gcoord[0].data(), ctx->gcoord[1].data(), ctx->gcoord[2].data()};
    return g3_build(ctx, ctx->geom, ctx->gn, c);
}
extern "C" int pl3_local_block(pl3_ctx* ctx, int first[3], int count[3]) {
    for (int a = 0; a < 3; a++) { if (first) first[a] = ctx->geom.d.o[a]; if (count) count[a] = ctx->geom.d.n[a]; }
    return 0;
}
// halo exchanges (3 phases each) and host all-reduces of this context so far; reset != 0 clears the counters
extern "C" int pl3_comm_stats(pl3_ctx* ctx, int64_t out[2], int reset) {
    if (out) { out[0] = ctx->halo_calls; out[1] = ctx->reduce_calls; }
    if (reset) { ctx->halo_calls = 0; ctx->reduce_calls = 0; }
    return 0;
}

// pylamp_stokes.py:116-122 extended dimension-wise: Kcont = DIM mineta / sum(avgd), Kbond = DIM^2 mineta / sum(avgd)^2
// plain (nz, nx, ny) DEVICE arrays -> the ringed coefficient arrays (the second half of upload3)
static int ring3(pl3_ctx* ctx, const double* src, double* dst) {
    const G3& g = ctx->geom.d;
    const dim3 gr((g.n[2] + 2 + 63) / 64, (g.n[1] + 2 + 3) / 4, g.n[0] + 2);
    hipLaunchKernelGGL(k3_from_host, gr, dim3(64, 4), 0, ctx->stream, g, src, 1, 0, dst);
    P3_HIP(ctx, hipGetLastError());
    return 0;
}
// with a yield stress set: the arrays just written to es / en are the material viscosities, kept next to them (the effective ones start
// as the material ones)
static int yield_keep_material3(pl3_ctx* ctx, double mineta) {
    ctx->mat_mineta = mineta;
    if (!ctx->yield_on) return 0;
    const size_t bytes = (size_t)ctx->geom.d.vol * sizeof(double);
    P3_HIP(ctx, hipMemcpyAsync(ctx->ms, ctx->es, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    P3_HIP(ctx, hipMemcpyAsync(ctx->mn, ctx->en, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}
static void stokes_op3(pl3_ctx* ctx, double mineta, const double grav[3]) {
    const G3& g = ctx->geom.d;
    double sum = 0.0;
    for (int a = 0; a < 3; a++) sum += (ctx->geom.c[a].back() - ctx->geom.c[a].front()) / g.gn[a];     // avgd = L / n (sic, :119-120)
    Op3& op = ctx->op;
    op.g = g; op.es = ctx->es; op.en = ctx->en; op.rho = ctx->rho;
    op.Kc = 3.0 * mineta / sum; op.Kb = 9.0 * mineta / (sum * sum); op.iKc = 1.0 / op.Kc;
    op.slave = 1; op.noslip = ctx->noslip;
    for (int a = 0; a < 3; a++) op.grav[a] = grav ? grav[a] : (a == 0 ? 9.81 : 0.0);
    op.anchor[0] = 3; op.anchor[1] = 2; op.anchor[2] = 2;
    ctx->op_ready = true;
}
// the operator again for another min(eta): gravity and the wall-row mode stay as they are
static void stokes_reop3(pl3_ctx* ctx, double mineta) {
    const double grav[3] = {ctx->op.grav[0], ctx->op.grav[1], ctx->op.grav[2]};
    const int slave = ctx->op.slave;
    stokes_op3(ctx, mineta, grav);
    ctx->op.slave = slave;
}
// python's min(etas.min(), etan.min()), pylamp_stokes.py:116-118, from the two minima over the non-NaN entries and whether each field holds
// a NaN: the minimum of such a field is NaN, and min(a, b) is a unless b is smaller
double nan_min3(double mes, double men, bool nan_s, bool nan_n) {
    if (nan_s) mes = NAN;
    if (nan_n) men = NAN;
    return (men < mes) ? men : mes;
}
extern "C" int pl3_stokes_set_coeffs(pl3_ctx* ctx, const double* etas, const double* etan, const double* rho, const double grav[3]) {
    if (!etas || !etan || !rho) return p3_fail(ctx, "pl3_stokes_set_coeffs: NULL argument");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    const G3& g = ctx->geom.d;
    for (double** q : {&ctx->es, &ctx->en, &ctx->rho}) if (!*q) P3_TRY(dmal(ctx, q, g.vol));
    P3_TRY(upload3(ctx, etas, 1, &ctx->es)); P3_TRY(upload3(ctx, etan, 1, &ctx->en)); P3_TRY(upload3(ctx, rho, 1, &ctx->rho));
    const size_t N = (size_t)g.gn[0] * g.gn[1] * g.gn[2];
    double mes = INFINITY, men = INFINITY; bool nes = false, nen = false;
    for (size_t t = 0; t < N; t++) { if (etas[t] != etas[t]) nes = true; else mes = std::min(mes, etas[t]); if (etan[t] != etan[t]) nen = true; else men = std::min(men, etan[t]); }
    const double mineta = nan_min3(mes, men, nes, nen);
    P3_TRY(yield_keep_material3(ctx, mineta));
    stokes_op3(ctx, mineta, grav);
    return 0;
}
// the same from plain (nz, nx, ny) device arrays, with min(eta) reduced by the caller (pl_step3.hip): nothing crosses the bus
int pl3i_stokes_set_coeffs_dev(pl3_ctx* ctx, const double* etas, const double* etan, const double* rho, const double grav[3], double mineta) {
    if (ctx->nranks > 1) return p3_fail(ctx, "device-source Stokes coefficients run on one rank");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    for (double** q : {&ctx->es, &ctx->en, &ctx->rho}) if (!*q) P3_TRY(dmal(ctx, q, ctx->geom.d.vol));
    P3_TRY(ring3(ctx, etas, ctx->es)); P3_TRY(ring3(ctx, etan, ctx->en)); P3_TRY(ring3(ctx, rho, ctx->rho));
    P3_TRY(yield_keep_material3(ctx, mineta));
    stokes_op3(ctx, mineta, grav);
    return 0;
}
// slaved != 0 (default): the reference's wall treatment extended to 3-D -- the outermost in-domain tangential velocities are
// slaved to their inner neighbours (pylamp_stokes.py:170-175,209-214,249-255,296-301), which imposes free slip half a cell
// inside the wall: first-order accurate.  0: natural (mirror) wall rows, second-order accurate.
extern "C" int pl3_stokes_set_wall_rows(pl3_ctx* ctx, int slaved) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    ctx->op.slave = slaved ? 1 : 0;
    return 0;
}
static void history_clear3(pl3_ctx* ctx) { ctx->warm_held = 0; for (double& d : ctx->dt_hist) d = 0.0; }
// bc = [z0, x0, y0, zL, xL, yL], each PL_BC_FREESLIP or PL_BC_NOSLIP.  A change of a wall's kind clears the warm-start history.  Kept on the context (which starts all free-slip) across
// pl3_stokes_set_coeffs; read by the solves, pl3_resident_step and pl3_advection_velocity.
static std::string wallvel_str3(const double* u) { return "(" + num_str3(u[0]) + ", " + num_str3(u[1]) + ", " + num_str3(u[2]) + ")"; }
extern "C" int pl3_stokes_set_walls(pl3_ctx* ctx, const int bc[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_set_walls: NULL context");
    if (!bc) return p3_fail(ctx, "pl3_stokes_set_walls: NULL argument");
    int m = 0;
    for (int w = 0; w < 6; w++) {
        if (bc[w] == PL_BC_NOSLIP) m |= 1 << w;
        else if (bc[w] != PL_BC_FREESLIP)
            return p3_fail(ctx, std::string("pl3_stokes_set_walls: wall ") + walls3_names[w] + " has kind " + std::to_string(bc[w]) +
                                    ": a 3-D Stokes wall is FREESLIP (1) or NOSLIP (0)");
    }
    for (int w = 0; w < 6; w++)
        if (((ctx->wallvel.moving >> w) & 1) && !((m >> w) & 1)) {
            const double* u = ctx->wallvel.u + 3 * w;
            return p3_fail(ctx, std::string("pl3_stokes_set_walls: wall ") + walls3_names[w] + " moves with velocity " + wallvel_str3(u) +
                                    " and cannot become FREESLIP: only a NOSLIP wall carries a velocity (set it to zero first)");
        }
    if (m != ctx->noslip) history_clear3(ctx);          // solutions of other wall kinds are no start for these
    ctx->noslip = m;
    if (ctx->op_ready) ctx->op.noslip = m;
    return 0;
}
// vel[3 w + q]: component q of (Uz, Ux, Uy) of wall w of [z0, x0, y0, zL, xL, yL].  Only the two tangential components of a NOSLIP
// wall may be non-zero.  Kept on the context (which starts at rest) across pl3_stokes_set_coeffs; read by pl3_stokes_rhs, the solves of
// the operator's own right-hand side, pl3_resident_step and pl3_advection_velocity.
extern "C" int pl3_stokes_set_wall_velocity(pl3_ctx* ctx, const double vel[18]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_set_wall_velocity: NULL context");
    if (!vel) return p3_fail(ctx, "pl3_stokes_set_wall_velocity: NULL argument");
    static const char* const comp[3] = {"Uz", "Ux", "Uy"};
    Pl3WallVel mv{};
    for (int w = 0; w < 6; w++) {
        const double* u = vel + 3 * w;
        const std::string who = std::string("pl3_stokes_set_wall_velocity: wall ") + walls3_names[w];
        for (int q = 0; q < 3; q++)
            if (!std::isfinite(u[q])) return p3_fail(ctx, who + " has a non-finite velocity component " + comp[q] + " = " + num_str3(u[q]));
        if (u[w % 3] != 0.0)
            return p3_fail(ctx, who + " has the normal velocity component " + comp[w % 3] + " = " + num_str3(u[w % 3]) +
                                    ": only the tangential components may be non-zero -- flow through a wall needs the marker deletion path, which is not built in 3-D");
        const bool moves = u[0] != 0.0 || u[1] != 0.0 || u[2] != 0.0;
        if (moves && !((ctx->noslip >> w) & 1))
            return p3_fail(ctx, who + " is FREESLIP and cannot move with velocity " + wallvel_str3(u) + ": only a NOSLIP wall carries a velocity (pl3_stokes_set_walls)");
        for (int q = 0; q < 3; q++) mv.u[3 * w + q] = u[q];
        if (moves) mv.moving |= 1 << w;
    }
    ctx->wallvel = mv;
    return 0;
}
extern "C" int pl3_stokes_get_wall_velocity(pl3_ctx* ctx, double vel[18]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_get_wall_velocity: NULL context");
    if (!vel) return p3_fail(ctx, "pl3_stokes_get_wall_velocity: NULL argument");
    for (int e = 0; e < 18; e++) vel[e] = ctx->wallvel.u[e];
    return 0;
}
// the net flux of the six flow planes (finite: planes3_set has looked), summed in long double by wall, row and column
static int flow_balance3(pl3_ctx* ctx, const double* const flow[6]) {
    long double flux[6] = {0, 0, 0, 0, 0, 0}, phi = 0.0L, tot = 0.0L;
    for (int w = 0; w < 6; w++) {
        if (!flow || !flow[w]) continue;
        int p, q;
        walls3_axes(w % 3, p, q);
        const int np = ctx->gn[p] - 1, nq = ctx->gn[q] - 1;
        const std::vector<double>&cp = ctx->gcoord[p], &cq = ctx->gcoord[q];
        long double f = 0.0L;
        for (int i = 0; i < np; i++)
            for (int j = 0; j < nq; j++) {
                const double u = flow[w][(size_t)i * nq + j];
                const long double area = ((long double)cp[i + 1] - (long double)cp[i]) * ((long double)cq[j + 1] - (long double)cq[j]);
                f += (long double)u * area;
                tot += std::fabs((long double)u) * area;
            }
        flux[w] = w < 3 ? f : -f;                             // inflow positive
        phi += flux[w];
    }
    if (std::fabs(phi) > 1e-10L * tot) {
        std::string six;
        for (int w = 0; w < 6; w++) six += std::string(w ? ", " : "") + walls3_names[w] + " " + num_str3((double)flux[w]);
        return p3_fail(ctx, "pl3_stokes_set_wall_flow: the net flux through the walls is " + num_str3((double)phi) + " (inflow positive), more than 1e-10 of the sum " +
                                num_str3((double)tot) + " of |Un| over the wall faces: the walls must balance, or the pressure anchor cell absorbs the rest as a "
                                "divergence; fluxes into the box: " + six);
    }
    return 0;
}
// Flow through the walls: flow[w] is the plane of wall w over its faces ("Wall planes"), wall-normal velocities
// along +a, or NULL for no flow; all NULL clears the setting.  All six walls are set in one call because the net flux must vanish: the
// anchor cell would absorb it as a divergence.  Kept on the context like the kinds and the velocities; a rejected call changes nothing.
extern "C" int pl3_stokes_set_wall_flow(pl3_ctx* ctx, const double* const flow[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_set_wall_flow: NULL context");
    P3_TRY(planes3_set(ctx, ctx->flow, "pl3_stokes_set_wall_flow", "flow entry", false, false, flow, flow_balance3));
    ctx->wallflow.mask = ctx->flow.mask;
    for (int w = 0; w < 6; w++) ctx->wallflow.un[w] = ctx->flow.plane(w);
    return 0;
}
extern "C" int pl3_stokes_get_wall_flow(pl3_ctx* ctx, int* mask, double* const flow[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_get_wall_flow: NULL context");
    return planes3_get(ctx, ctx->flow, mask, flow);
}
extern "C" int pl3_stokes_get_scaling(pl3_ctx* ctx, double* kc, double* kb) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    if (kc) *kc = ctx->op.Kc; if (kb) *kb = ctx->op.Kb;
    return 0;
}

// y = A x (scaled: D_r A x): the marching LDS kernel for the interior rows + the per-node kernel on the rim, or the per-node kernel alone
template <bool SCALED> static void launch_apply3(pl3_ctx* ctx, const Op3& op, const Vec3& in, const Vec3& out) {
    if (k3_use_lds(op.g)) {
        hipLaunchKernelGGL(k3_apply_m<SCALED>, grid3m(op.g), dim3(64, 4), 0, ctx->stream, op, cv4(in), wv4(out), k3_band(), k3m_zc(op.g));
    } else launch3(ctx, op.g, k3_apply<SCALED>, op, cv4(in), wv4(out), 0);
}
extern "C" int pl3_stokes_apply(pl3_ctx* ctx, const double* x, double* y) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 2));
    P3_TRY(upload3(ctx, x, 4, wv4(svec(ctx, 0)).p));         // (the upload fills the ring of nodes around the block as well)
    launch_apply3<false>(ctx, ctx->op, svec(ctx, 0), svec(ctx, 1));
    P3_HIP(ctx, hipGetLastError());
    return download3(ctx, wv4(svec(ctx, 1)).p, 4, y);
}
static int stokes_rhs3(pl3_ctx* ctx, double* rhs, int scaled) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 2));
    launch3(ctx, ctx->op.g, k3_rhs, ctx->op, wv4(svec(ctx, 1)), scaled, ctx->wallvel, ctx->wallflow);
    P3_HIP(ctx, hipGetLastError());
    return download3(ctx, wv4(svec(ctx, 1)).p, 4, rhs);
}
extern "C" int pl3_stokes_rhs(pl3_ctx* ctx, double* rhs) { return stokes_rhs3(ctx, rhs, 0); }
// the row-scaled right-hand side D_r b that pl3_stokes_solve(rhs = NULL) iterates on
extern "C" int pl3_stokes_rhs_scaled(pl3_ctx* ctx, double* rhs) { return stokes_rhs3(ctx, rhs, 1); }
extern "C" int pl3_stokes_apply_bench(pl3_ctx* ctx, int scaled, int reps, double* avg_ms) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 2));
    const Vec3 in = svec(ctx, 0), out = svec(ctx, 1);
    for (int q = 0; q < 4; q++) launch3(ctx, ctx->op.g, k3_random, ctx->op.g, in[q], 99u + q);
    auto launch = [&]() {
        if (scaled) launch_apply3<true>(ctx, ctx->op, in, out);
        else launch_apply3<false>(ctx, ctx->op, in, out);
    };
    launch();
    P3_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; r++) launch();
    P3_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    P3_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0; P3_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    if (avg_ms) *avg_ms = ms / reps;
    return 0;
}

// ---- reductions -----------------------------------------------------------------------------------------------------------
// the end of every reduction on the host: the stride x D3_BLOCKS block partials of the kernel come over in one copy and one synchronisation
// and are summed per quantity, block 0 upward
static int sum_partials3(pl3_ctx* ctx, int stride, int nq, double* out) {
    pl3_count_copy(ctx, stride * D3_BLOCKS * sizeof(double));
    P3_HIP(ctx, hipMemcpyAsync(ctx->hpart, ctx->part, stride * D3_BLOCKS * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int q = 0; q < nq; q++) { double s = 0.0; for (int k = 0; k < D3_BLOCKS; k++) s += ctx->hpart[stride * k + q]; out[q] = s; }
    return 0;
}
// nd <= 5 dot products a[q] . b[q] of vectors of one shape in one pass.  Several ranks: only the OWNED nodes count (the rings hold copies
// of the neighbours' values), and the sums go over the ranks.
static int dots3(pl3_ctx* ctx, int nd, const Vec3* a, const Vec3* b, double* out) {
    Dot5 d{}; d.n = nd;
    for (int q = 0; q < nd; q++) { d.a[q] = a[q].p; d.b[q] = b[q].p; }
    if (ctx->nranks > 1) hipLaunchKernelGGL(k3_dots_own, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, *a[0].g, a[0].na, d, ctx->part);
    else hipLaunchKernelGGL(k3_dots, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, a[0].n(), d, ctx->part);
    P3_TRY(sum_partials3(ctx, 5, nd, out));
    return allreduce3(ctx, out, nd, 0);
}
static int dot3(pl3_ctx* ctx, const Vec3& a, const Vec3& b, double* out) { return dots3(ctx, 1, &a, &b, out); }

// ---- multigrid -----------------------------------------------------------------------------------------------------------
static int build_levels3(pl3_ctx* ctx) {
    if (ctx->levels.empty()) {
        int n[3] = {ctx->gn[0], ctx->gn[1], ctx->gn[2]};                     // GLOBAL node counts of the level
        std::vector<double> c[3] = {ctx->gcoord[0], ctx->gcoord[1], ctx->gcoord[2]};
        for (int l = 0;; l++) {
            Lev3* L = new Lev3();
            const double* cc[3] = {c[0].data(), c[1].data(), c[2].data()};
            if (g3_build(ctx, L->gh, n, cc)) { delete L; return 1; }
            const long long vol = L->gh.d.vol;
            if (l > 0) { L->own = true; P3_TRY(dmal(ctx, &L->es, vol)); P3_TRY(dmal(ctx, &L->en, vol)); }
            for (int b = 0; b < 3; b++) for (int q = 0; q < 3; q++) P3_TRY(dmal(ctx, &L->v[b][q], vol));
            for (int q = 0; q < 3; q++) { P3_TRY(dmal(ctx, &L->f[q], vol)); P3_TRY(dmal(ctx, &L->r[q], vol)); P3_TRY(dmal(ctx, &L->dinv[q], vol)); }
            ctx->levels.push_back(L);
            bool stop = false;
            for (int a = 0; a < 3; a++) if ((n[a] - 1) % 2 || (n[a] - 1) / 2 < 4) stop = true;
            // several ranks: every block is halved with the grid -- a block with an odd number of cells (or one that would shrink below
            // two) ends the hierarchy here, and this level is smoothed as the coarsest one (more sweeps: coarse_sweeps by its size)
            for (int a = 0; a < 3; a++) if (ctx->P[a] > 1 && (((n[a] - 1) / ctx->P[a]) % 2 || (n[a] - 1) / ctx->P[a] / 2 < 2)) stop = true;
            if (stop) break;
            for (int a = 0; a < 3; a++) {
                std::vector<double> c2;
                for (int i = 0; i < n[a]; i += 2) c2.push_back(c[a][i]);
                c[a].swap(c2); n[a] = (n[a] - 1) / 2 + 1;
            }
        }
    }
    ctx->levels[0]->es = ctx->es; ctx->levels[0]->en = ctx->en;
    for (size_t l = 0; l < ctx->levels.size(); l++) {
        Lev3* L = ctx->levels[l];
        if (l > 0) {
            Lev3* F = ctx->levels[l - 1];
            launch3(ctx, L->gh.d, k3_coarsen, F->gh.d, F->es, F->en, L->gh.d, L->es, L->en);
            P3_TRY(halo3(ctx, L->gh.d, &L->es, 1)); P3_TRY(halo3(ctx, L->gh.d, &L->en, 1));  // the rows of this level and the next coarsening read the ring
        }
        L->op = ctx->op; L->op.g = L->gh.d; L->op.es = L->es; L->op.en = L->en; L->op.slave = (l == 0) ? ctx->op.slave : 0;
        const G3& g = L->gh.d;
        launch3(ctx, g, k3_dinv, L->op, wv3(L->dinv));
        P3_TRY(halo3(ctx, g, L->dinv, 3));                  // (a slaved row reads its master's entry, possibly in the neighbour block)
        // lambda_max of D^-1 A_vv by power iteration
        const long long vol = g.vol;
        // Warm restart as in the 2-D solver (pl_solver.hip): consecutive solves on one context (a time loop, or the same operator
        // again) start from the eigenvector of the last one and stop as soon as an iteration confirms the last estimate to 1 % --
        // 12 cold iterations per level were 5 % of a 257^3 solve.
        const bool warm = L->eig_valid && L->eig[0];
        if (warm) for (int q = 0; q < 3; q++) P3_HIP(ctx, hipMemcpyAsync(L->v[0][q], L->eig[q], (size_t)vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        else for (int q = 0; q < 3; q++) launch3(ctx, g, k3_random, g, L->v[0][q], 777u + q);
        {   // the start vector must satisfy the constraints of THIS operator: close it
            for (int q = 0; q < 3; q++) P3_HIP(ctx, hipMemsetAsync(L->r[q], 0, (size_t)vol * sizeof(double), ctx->stream));
            P3_TRY(halo3(ctx, g, L->v[0], 3));
            launch3(ctx, g, k3_close, L->op, wv3(L->v[0]), cv3(L->r));
        }
        double lam = warm ? L->lmax / 1.1 : 2.5, lam_prev = 0.0;
        for (int it = 0; it < 12; it++) {
            if (warm && it >= 1 && std::fabs(lam - lam_prev) < 0.01 * lam) break;
            lam_prev = lam;
            P3_TRY(halo3(ctx, g, L->v[0], 3));
            launch3(ctx, g, k3_resid, L->op, cv3(L->v[0]), cv3(L->f), wv3(L->v[1]), 1, 0);
            // |A v|^2 and |v|^2.  The three arrays of a level vector are separate allocations: the one per-array reduction left, one pass
            // per array and the three results added here (contiguous level storage would change the order of these sums, and lmax)
            double nn[2] = {0.0, 0.0};
            for (int q = 0; q < 3; q++) {
                const Vec3 a[2] = {Vec3{L->v[1][q], 1, &g}, Vec3{L->v[0][q], 1, &g}}; double o[2];
                P3_TRY(dots3(ctx, 2, a, a, o));
                nn[0] += o[0]; nn[1] += o[1];
            }
            if (!(nn[0] > 0.0) || !(nn[1] > 0.0)) break;
            lam = std::sqrt(nn[0] / nn[1]);
            for (int q = 0; q < 3; q++) hipLaunchKernelGGL(k3_axpby, g1(vol), dim3(256), 0, ctx->stream, vol, L->v[0][q], 1.0 / std::sqrt(nn[0]), (const double*)L->v[1][q], 0.0, (const double*)L->v[1][q]);
        }
        L->lmax = 1.1 * lam;
        if (!L->eig[0]) for (int q = 0; q < 3; q++) P3_TRY(dmal(ctx, &L->eig[q], vol));
        for (int q = 0; q < 3; q++) P3_HIP(ctx, hipMemcpyAsync(L->eig[q], L->v[0][q], (size_t)vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        L->eig_valid = std::isfinite(lam) && lam > 0.0;
    }
    P3_HIP(ctx, hipGetLastError());
    return 0;
}
// nsweep sweeps; cur = index of the buffer holding the iterate on entry (ignored if zero_guess) and on exit
static int smooth3(pl3_ctx* ctx, Lev3* L, double* const* f, int nsweep, double ratio, bool zero_guess, int& cur, const W3* final_out = nullptr) {
    const G3& g = L->gh.d;
    const double lmax = L->lmax, lmin = lmax / ratio, theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta;
    double rho_old = 1.0 / sigma;
    int prev = (cur + 1) % 3;
    for (int k = 0; k < nsweep; k++) {
        double c1, c2;
        if (k == 0) { c1 = 0.0; c2 = 1.0 / theta; }
        else { const double rho = 1.0 / (2.0 * sigma - rho_old); c1 = rho * rho_old; c2 = 2.0 * rho / delta; rho_old = rho; }
        int nxt = 0; while (nxt == cur || nxt == prev) nxt++;
        V3 vp = cv3(L->v[prev]);
        if (k == 1 && zero_guess) for (int q = 0; q < 3; q++) vp.p[q] = nullptr;
        // the last sweep may write straight into the caller's arrays (the preconditioner's output) instead of a level buffer
        const W3 dst = (final_out && k == nsweep - 1) ? *final_out : wv3(L->v[nxt]);
        // several ranks: the sweep reads the iterate one node into the ring (the first sweep from the zero guess: only the right-hand
        // side, at a slave's master)
        const bool first = k == 0 && zero_guess;
        P3_TRY(halo3(ctx, g, first ? f : L->v[cur], 3));
        if (first) launch3(ctx, g, k3_cheb0, L->op, cv3(f), cv3(L->dinv), dst, c2);
        else if (k3_use_lds(g))                 // interior rows: the marching LDS kernel; the rim: the per-node kernel
            hipLaunchKernelGGL(k3_sweep_m<0>, grid3m(g), dim3(64, 4), 0, ctx->stream, L->op, cv3(L->v[cur]), vp, cv3(f), dst, c1, c2, k3_band(), k3m_zc(g));
        else launch3(ctx, g, k3_cheb, L->op, cv3(L->v[cur]), vp, cv3(f), dst, c1, c2, 0, 0);
        prev = cur; cur = nxt;
    }
    return 0;
}
// the coarsest level's smoothing: ratio by its size (floor 30), sweeps sqrt(ratio) within coarse_sweeps .. 150
static void coarsest_plan3(const pl3_ctx* ctx, const G3& g, int& n, double& ratio) {
    ratio = 0.4 * std::pow((double)g.gn[0] * g.gn[1] * g.gn[2], 2.0 / 3.0); if (ratio < 30.0) ratio = 30.0;
    n = std::max((int)std::sqrt(ratio), ctx->coarse_sweeps); if (n > 150) n = 150;
}
// sweeps on the finest level and on the others
static void level_nu3(const pl3_ctx* ctx, int& nu_fine, int& nu_rest) {
    const bool big = (long long)ctx->gn[0] * ctx->gn[1] * ctx->gn[2] >= 1000000;
    nu_fine = ctx->nu_fine > 0 ? ctx->nu_fine : (big && !ctx->nu_set ? 1 : ctx->nu);
    nu_rest = (big && !ctx->nu_set) ? 3 : ctx->nu;
}
// one V-cycle of level l for the right-hand side f; the result is in buffer out_buf of the level (or in final_out)
static int vcycle3(pl3_ctx* ctx, size_t l, double* const* f, int& out_buf, const W3* final_out = nullptr) {
    Lev3* L = ctx->levels[l];
    const G3& g = L->gh.d;
    int cur = 0;
    if (l + 1 == ctx->levels.size()) {
        double ratio; int n;
        coarsest_plan3(ctx, g, n, ratio);
        P3_TRY(smooth3(ctx, L, f, n, ratio, true, cur));
        out_buf = cur;
        return 0;
    }
    // From 10^6 nodes up: V(1,1) on the finest level, V(3,3) below (the 2-D solver's choice, pl_solver.hip) -- 257^3: 494 ms per solve
    // pair with 24 iterations against 539 ms with 23 for V(2,2) throughout (1/4: 492, 2/3: 499, 1/2: 504; tools/run_nu3.sh).
    // PYLAMP_MG_NU3 / PYLAMP_MG_NU3_FINE override the two counts.
    int nu_fine, nu_rest;
    level_nu3(ctx, nu_fine, nu_rest);
    const int nu = l == 0 ? nu_fine : nu_rest;
    P3_TRY(smooth3(ctx, L, f, nu, ctx->cheb_ratio, true, cur));
    P3_TRY(halo3(ctx, g, L->v[cur], 3));
    if (k3_use_lds(g)) {
        V3 none{};
        hipLaunchKernelGGL(k3_sweep_m<1>, grid3m(g), dim3(64, 4), 0, ctx->stream, L->op, cv3(L->v[cur]), none, cv3(f), wv3(L->r), 0.0, 0.0, k3_band(), k3m_zc(g));
    } else launch3(ctx, g, k3_resid, L->op, cv3(L->v[cur]), cv3(f), wv3(L->r), 0, 0);
    Lev3* C = ctx->levels[l + 1];
    P3_TRY(halo3(ctx, g, L->r, 3));
    launch3(ctx, C->gh.d, k3_restrict, g, C->op, cv3(L->r), wv3(C->f));
    int cb = 0;
    P3_TRY(vcycle3(ctx, l + 1, C->f, cb));
    const int nxt = (cur + 1) % 3;
    P3_TRY(halo3(ctx, C->gh.d, C->v[cb], 3));            // (the ring of L->v[cur] is still the one exchanged for the residual)
    launch3(ctx, g, k3_prolong_add, L->op, C->gh.d, cv3(C->v[cb]), cv3(L->v[cur]), wv3(L->v[nxt]));
    cur = nxt;
    P3_TRY(smooth3(ctx, L, f, nu, ctx->cheb_ratio, false, cur, final_out));
    out_buf = cur;
    return 0;
}

// ---- deflation of the pressure-anchor mode and the velocity-error estimate: the 3-D counterparts of pl_solver.hip --------------
// u: the continuity residual that the block preconditioner turns into a constant pressure; yw: cell volume x (rdz + rdx + rdy) on the
// continuity rows, so that yw . (scaled continuity row of v) = sum of volume x div(v)
__global__ __launch_bounds__(256) void k3_defl_setup(Op3 op, W4 u, double* __restrict__ yw) {
    K3_PROLOGUE(op.g)
    long long moff;
    const bool cont = cls3_p(op, idx, moff) == 1;
    const G3& g = op.g;
    const double rs = TB(g.rd[0], i) + TB(g.rd[1], j) + TB(g.rd[2], k);
    u.p[0][c] = 0.0; u.p[1][c] = 0.0; u.p[2][c] = 0.0;
    u.p[3][c] = cont ? 1.0 / (op.en[c] * rs) : 0.0;
    yw[c] = cont ? rs / (TB(g.rd[0], i) * TB(g.rd[1], j) * TB(g.rd[2], k)) : 0.0;
}
// the scaled continuity rows of a velocity field (0 on the other pressure rows)
__global__ __launch_bounds__(256) void k3_cont_rows(Op3 op, V3 v, double* __restrict__ out) {
    K3_PROLOGUE(op.g)
    long long moff;
    double o = 0.0;
    if (cls3_p(op, idx, moff) == 1) {
        const G3& g = op.g;
        const double rz = TB(g.rd[0], i), rx = TB(g.rd[1], j), ry = TB(g.rd[2], k);
        o = ((v.p[0][c + g.s[0]] - v.p[0][c]) * rz + (v.p[1][c + g.s[1]] - v.p[1][c]) * rx + (v.p[2][c + g.s[2]] - v.p[2][c]) * ry) / (rz + rx + ry);
    }
    out[c] = o;
}

// ---- right-preconditioned BiCGStab on Krylov vectors (correction form, true-residual stopping) ----------------------------------
typedef int (*Op3Fn)(pl3_ctx*, const Vec3& in, const Vec3& out);
// rec_it > 0: the iteration at which the estimate between the checks was last evaluated, with its value and what went into est_rec3
struct Stats3 { int iterations, converged; double rel_residual; double error_estimate; int checks; int rec_it; double rec[6]; };enum { K_R, K_RT, K_P, K_V, K_S, K_T, K_Y, K_Z, K_DX, K_R0, K_NW };      // the work vectors of bicgstab3
static void axpby3(pl3_ctx* ctx, const Vec3& y, double a, const Vec3& x, double b, const Vec3& z) {
    hipLaunchKernelGGL(k3_axpby, g1(y.n()), dim3(256), 0, ctx->stream, y.n(), y.p, a, (const double*)x.p, b, (const double*)z.p);
}
static int zero3(pl3_ctx* ctx, const Vec3& y) { P3_HIP(ctx, hipMemsetAsync(y.p, 0, (size_t)y.n() * sizeof(double), ctx->stream)); return 0; }
// the shadow residual of bicgstab3: array c of rt from the hash of the global node index, seed + c
static void random3(pl3_ctx* ctx, const Vec3& rt, unsigned seed) {
    for (int c = 0; c < rt.na; c++) launch3(ctx, *rt.g, k3_random, *rt.g, rt[c], seed + c);
}
// the fused reduction of bicgstab3 (one rank, Stokes vectors): the 11 sums of k3_dots11; x / dx / yw as the iteration has them (x NULL:
// no |x_vel|^2; dx the vector x itself: x alone; yw NULL: no anchor sums)
static int dots11_3(pl3_ctx* ctx, const Vec3& t, const Vec3& s, const Vec3& rt, const Vec3* x, const Vec3* dx, const double* yw, double* f11) {
    Fuse11 fa{}; fa.t = t.p; fa.s = s.p; fa.rt = rt.p; fa.vol = t.g->vol;
    if (x) { fa.x = x->p; fa.dx = (dx && dx->p != x->p) ? dx->p : nullptr; }
    fa.yw = yw;
    hipLaunchKernelGGL(k3_dots11, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, fa, ctx->part);
    return sum_partials3(ctx, 11, 11, f11);
}
static bool trace3() { static const bool on = getenv("PYLAMP_SOLVER_TRACE") != nullptr; return on; }

// The velocity-error estimate (n |r_cont| + |(M^-1 r)_vel|) / |x_vel| of a Stokes solve, as in pl_solver.hip.  anchor: the component of
// the residual along the deflated anchor mode has its own amplification |w| / |u|.  a_mom stands for |(M^-1 r)_vel| / |r_mom| between
// the true-residual checks that measure it.
// tol, bnorm: the residual test of the iteration (tol tightens while the estimate is above etol); rec: the estimate between the checks;
// est: that of the last check; resume: the check sends the iteration on.
struct Est3 { bool on, anchor, resume; double etol, n_amp, a_mom, rec, est, tol, bnorm; int checks; };
static void note_rec3(Stats3* st, int it, const Est3& e, double rr, double rc, double xx, double ap) {
    st->rec_it = it; st->rec[0] = e.rec; st->rec[1] = rr; st->rec[2] = rc; st->rec[3] = xx; st->rec[4] = ap; st->rec[5] = e.a_mom;
}
static double anchor_amp3(const pl3_ctx* ctx, double yr, double xx) { return std::fabs(yr / ctx->dfl_yAw) * std::sqrt(ctx->dfl_wvel2 / xx); }
static int anchor_part3(pl3_ctx* ctx, const Est3& e, const Vec3& res, double xx, double* out) {
    *out = 0.0;
    if (!e.anchor || !(xx > 0.0)) return 0;
    double o;
    P3_TRY(dot3(ctx, arr3(ctx, ctx->dfl_y), res.prs(), &o));
    *out = anchor_amp3(ctx, o, xx);
    return 0;
}
// |(x0 + dx)_vel|^2, through t as scratch
static int vel_norm2_3(pl3_ctx* ctx, const Vec3& x, const Vec3& dx, const Vec3& t, double* xx) {
    Vec3 src = dx.vel();
    if (dx.p != x.p) { src = t.vel(); axpby3(ctx, src, 1.0, x.vel(), 1.0, dx.vel()); }
    return dot3(ctx, src, src, xx);
}
// the estimate between the checks: from |r|^2 = rr and |r_cont|^2 = rc of the recurrence residual, |x_vel|^2 = xx and the anchor part ap
static double est_rec3(const Est3& e, double rr, double rc, double xx, double ap) {
    if (!(xx > 0.0)) return 0.0;
    const double rm = rr - rc > 0.0 ? rr - rc : 0.0;
    return (e.n_amp * std::sqrt(rc > 0.0 ? rc : 0.0) + e.a_mom * std::sqrt(rm)) / std::sqrt(xx) + ap;
}
// The true residual s (norm true_norm) has met the tolerance: the estimate from it (e.est), with the velocity norm of the preconditioned
// residual itself (which also renews a_mom).  Above etol the tolerance tightens and the iteration resumes.
static int true_check3(pl3_ctx* ctx, Op3Fn M, Est3& e, const Vec3* w, const Vec3& x, const Vec3& dx, double true_norm, int it) {
    const Vec3 &s = w[K_S], &z = w[K_Z];
    double rc, zz, xx = 0.0, ap = 0.0;
    P3_TRY(dot3(ctx, s.prs(), s.prs(), &rc));
    P3_TRY(M(ctx, s, z));
    P3_TRY(dot3(ctx, z.vel(), z.vel(), &zz));
    P3_TRY(vel_norm2_3(ctx, x, dx, w[K_T], &xx));
    e.checks++;
    const double rcc = rc > 0.0 ? rc : 0.0, rm = true_norm * true_norm - rcc;
    P3_TRY(anchor_part3(ctx, e, s, xx, &ap));
    e.est = (xx > 0.0 ? (e.n_amp * std::sqrt(rcc) + std::sqrt(zz > 0.0 ? zz : 0.0)) / std::sqrt(xx) : 0.0) + ap;
    if (rm > 0.0 && zz > 0.0) e.a_mom = std::min(std::max(std::sqrt(zz / rm), 1.0), e.n_amp * e.n_amp);
    if (trace3()) fprintf(stderr, "[pylamp3 bicgstab] it %3d  velocity-error estimate %.3e (etol %.1e)\n", it, e.est, e.etol);
    e.resume = e.est > e.etol && e.tol > 1e-15;
    if (e.resume) { e.tol = std::min(e.tol, true_norm / e.bnorm) * std::min(0.5, 0.7 * e.etol / e.est); e.rec = e.est; }
    return 0;
}

// Solves A x = b (from x if use_x0, else from zero); w: K_NW work vectors of b's shape.  ref_norm > 0 replaces |b| in the stopping test;
// etol > 0 (Stokes vectors with M): also bound the velocity-error estimate.  r0_ready (with use_x0): w[K_R0] holds b - A x already.
static int bicgstab3(pl3_ctx* ctx, Op3Fn A, Op3Fn M, const Vec3& b, const Vec3& x, bool use_x0, double rtol, int maxit, const Vec3* w,
                     Stats3* st, double ref_norm, double etol = 0.0, bool r0_ready = false) {
    const Vec3 &r = w[K_R], &rt = w[K_RT], &p = w[K_P], &v = w[K_V], &s = w[K_S], &t = w[K_T], &y = w[K_Y], &z = w[K_Z];
    const G3& g = *b.g;
    const int na = b.na; const long long n = b.n();
    double d[5];
    P3_TRY(dot3(ctx, b, b, d));
    double bnorm = std::sqrt(d[0]);
    if (ref_norm > 0.0 && bnorm > 0.0) bnorm = ref_norm;
    st->iterations = 0; st->converged = 0; st->rel_residual = 0.0; st->error_estimate = 0.0; st->rec_it = 0;
    if (!(bnorm > 0.0)) { P3_TRY(zero3(ctx, x)); st->converged = 1; return 0; }
    Vec3 dx = x, r0 = b;
    if (use_x0) { dx = w[K_DX]; r0 = w[K_R0]; if (!r0_ready) { P3_TRY(A(ctx, x, v)); axpby3(ctx, r0, 1.0, b, -1.0, v); } }
    P3_TRY(zero3(ctx, dx));
    axpby3(ctx, r, 1.0, r0, 0.0, r0);
    random3(ctx, rt, 1234u);
    int it = 0, restarts = 0; double true_norm = -1.0, last_true = -1.0;
    Est3 e{};
    e.on = etol > 0.0 && na == 4 && M; e.anchor = e.on && ctx->dfl_active && ctx->dfl_yAw != 0.0;
    e.etol = etol; e.n_amp = (double)std::max(g.gn[0], std::max(g.gn[1], g.gn[2])); e.a_mom = 1.0;
    e.tol = rtol; e.bnorm = bnorm;
    bool broke = false, p_fused = false;
    // one rank, Stokes vectors: the fused reduction / update kernels
    const bool fused = ctx->nranks == 1 && na == 4 && M && !(getenv("PYLAMP_3D_FUSED") && atoi(getenv("PYLAMP_3D_FUSED")) == 0);
    double rho = 1.0, alpha = 1.0, omega = 1.0, rho_new = 0.0, rnorm = 0.0, best = 0.0; int best_it = 0;
    for (;;) {
        if (!e.resume) {
            P3_TRY(zero3(ctx, p)); P3_TRY(zero3(ctx, v));
            rho = alpha = omega = 1.0; p_fused = false;
            { const Vec3 aa[2] = {rt, r}, bb[2] = {r, r}; P3_TRY(dots3(ctx, 2, aa, bb, d)); }
            rho_new = d[0]; rnorm = std::sqrt(d[1]);
            broke = false;
            best = rnorm; best_it = it;
        }
        e.resume = false;
        while (it < maxit && (rnorm > e.tol * bnorm || (e.on && e.rec > 0.7 * etol))) {
            it++;
            if (!(std::fabs(rho_new) > 0.0) || !std::isfinite(rho_new)) { broke = true; break; }
            const double beta = (rho_new / rho) * (alpha / omega);
            if (p_fused) p_fused = false;                   // (written by k3_xrp_update of the previous iteration)
            else hipLaunchKernelGGL(k3_p_update, g1(n), dim3(256), 0, ctx->stream, n, p.p, (const double*)r.p, (const double*)v.p, beta, omega);
            Vec3 yv = p, zv = s;
            if (M) { P3_TRY(M(ctx, p, y)); yv = y; }
            P3_TRY(A(ctx, yv, v));
            P3_TRY(dot3(ctx, rt, v, d));
            if (!(std::fabs(d[0]) > 0.0) || !std::isfinite(d[0])) { broke = true; break; }
            alpha = rho_new / d[0];
            axpby3(ctx, s, 1.0, r, -alpha, v);
            if (M) { P3_TRY(M(ctx, s, z)); zv = z; }
            P3_TRY(A(ctx, zv, t));
            // one reduction: t.s, t.t, rt.s, rt.t, s.s  ->  omega, rho' = rt.s - omega rt.t, |r|^2 = s.s - 2 omega t.s + omega^2 t.t
            double f11[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
            const bool late = e.on && rnorm <= 1e3 * e.tol * bnorm;
            if (fused) {       // ... and, near the end, everything the error estimate of the updated iterate needs, in the same pass
                P3_TRY(dots11_3(ctx, t, s, rt, late ? &x : nullptr, &dx, (late && e.anchor) ? ctx->dfl_y : nullptr, f11));
                for (int q = 0; q < 5; q++) d[q] = f11[q];
            } else { const Vec3 aa[5] = {t, t, rt, rt, s}, bb[5] = {s, t, s, t, s}; P3_TRY(dots3(ctx, 5, aa, bb, d)); }
            omega = (d[1] > 0.0) ? d[0] / d[1] : 0.0;
            if (fused) {
                const double rho_next = d[2] - omega * d[3];
                const double beta_next = (rho_next / rho_new) * (alpha / omega);
                hipLaunchKernelGGL(k3_xrp_update, g1(n), dim3(256), 0, ctx->stream, n, dx.p, (const double*)yv.p, (const double*)zv.p, r.p,
                                   (const double*)s.p, (const double*)t.p, p.p, (const double*)v.p, alpha, omega, beta_next);
                p_fused = std::isfinite(beta_next);
            } else
                hipLaunchKernelGGL(k3_xr_update, g1(n), dim3(256), 0, ctx->stream, n, dx.p, (const double*)yv.p, (const double*)zv.p, r.p,
                                   (const double*)s.p, (const double*)t.p, alpha, omega);
            rho = rho_new; rho_new = d[2] - omega * d[3];
            const double rr = d[4] - 2.0 * omega * d[0] + omega * omega * d[1];
            rnorm = rr > 0.0 ? std::sqrt(rr) : 0.0;
            if (!std::isfinite(rnorm) || !(std::fabs(omega) > 0.0)) { broke = true; break; }
            if (rnorm < best) { best = rnorm; best_it = it; }
            if (trace3()) fprintf(stderr, "[pylamp3 bicgstab] it %3d  |r|/|b| %.3e\n", it, rnorm / bnorm);
            e.rec = 0.0;
            if (fused && late) {                                  // (sums of the fused reduction; |x_vel| of the iterate BEFORE this update: needed to ~10 %)
                const double rc = f11[7] - 2.0 * omega * f11[5] + omega * omega * f11[6], xx = f11[8];
                const double ap = (e.anchor && xx > 0.0) ? anchor_amp3(ctx, f11[9] - omega * f11[10], xx) : 0.0;
                e.rec = est_rec3(e, rr, rc > 0.0 ? rc : 0.0, xx, ap);
                note_rec3(st, it, e, rr, rc, xx, ap);
            } else if (e.on && rnorm <= 1e3 * e.tol * bnorm) {    // near the end: the estimate from the recurrence residual
                double rc, xx = 0.0, ap = 0.0;
                P3_TRY(dot3(ctx, r.prs(), r.prs(), &rc));
                P3_TRY(vel_norm2_3(ctx, x, dx, t, &xx));
                P3_TRY(anchor_part3(ctx, e, r, xx, &ap));
                e.rec = est_rec3(e, rr, rc, xx, ap);
                note_rec3(st, it, e, rr, rc, xx, ap);
            }
            if (it - best_it > 80 || rnorm > 1e8 * best) { broke = true; break; }
        }
        P3_TRY(A(ctx, dx, t));
        axpby3(ctx, s, 1.0, r0, -1.0, t);
        P3_TRY(dot3(ctx, s, s, d));
        last_true = true_norm; true_norm = std::sqrt(d[0]);
        if (true_norm <= e.tol * bnorm && !broke && it < maxit && e.on && e.checks < 6) {
            P3_TRY(true_check3(ctx, M, e, w, x, dx, true_norm, it));
            st->error_estimate = e.est;
            if (e.resume) continue;
        }
        if (true_norm <= e.tol * bnorm || broke || it >= maxit || restarts >= 4) break;
        if (last_true >= 0.0 && !(true_norm < 0.5 * last_true)) break;
        restarts++;
        axpby3(ctx, r, 1.0, s, 0.0, s);
    }
    if (dx.p != x.p) axpby3(ctx, x, 1.0, x, 1.0, dx);
    st->iterations = it; st->rel_residual = true_norm / bnorm; st->checks = e.checks;
    st->converged = (st->rel_residual <= rtol && !(e.on && st->error_estimate > 1.5 * etol)) ? 1 : 0;
    return 0;
}

// hydrostatic pressure guess: with v = 0 the interior z-momentum rows reduce to -2 Kc rDz_i (P[i] - P[i-1]) = b_z; integrate down
// every column, anchor cell to zero (same construction as pl_solver.hip)
// (several ranks: every block integrates from zero at its own top; coltot receives the block's column totals, and k3_hydro_add the sum
//  of the totals of the blocks above -- pl3_stokes_solve)
__global__ __launch_bounds__(256) void k3_hydro(Op3 op, double* __restrict__ P, double* __restrict__ coltot) {
    const int lk = blockIdx.x * 64 + threadIdx.x, lj = blockIdx.y * 4 + threadIdx.y;
    const G3& g = op.g;
    if (lk >= g.n[2] || lj >= g.n[1]) return;
    const int j = lj + g.o[1], k = lk + g.o[2];
    const double* r = op.rho;
    const int jn = (j + 1 < g.gn[1]) ? 1 : 0, kn = (k + 1 < g.gn[2]) ? 1 : 0;
    double acc = 0.0;
    for (int li = 0; li < g.n[0]; li++) {
        const int i = li + g.o[0];
        const long long c = i3(g, li, lj, lk);
        if (i >= 1 && i <= g.gn[0] - 2)
            acc += 0.25 * ((r[c] + r[c + jn * g.s[1]]) + (r[c + kn * g.s[2]] + r[c + jn * g.s[1] + kn * g.s[2]])) * op.grav[0] / (2.0 * op.Kc * TB(g.rD[0], i));
        P[c] = (i >= g.gn[0] - 1 || j >= g.gn[1] - 1 || k >= g.gn[2] - 1) ? 0.0 : acc;
    }
    if (coltot) coltot[(long long)lj * g.n[2] + lk] = acc;
}
__global__ __launch_bounds__(256) void k3_hydro_add(G3 g, double* __restrict__ P, const double* __restrict__ above) {
    K3_PROLOGUE(g)
    if (i < g.gn[0] - 1 && j < g.gn[1] - 1 && k < g.gn[2] - 1) P[c] += above[(long long)lj * g.n[2] + lk];
}
__global__ __launch_bounds__(256) void k3_shift(G3 g, double* __restrict__ P, const double* __restrict__ anchor_val) {
    K3_PROLOGUE(g)
    if (i < g.gn[0] - 1 && j < g.gn[1] - 1 && k < g.gn[2] - 1) P[c] -= *anchor_val;
}


// ---- the Stokes solve: operator, preconditioner, hydrostatic start, deflation vector ---------------------------------------------
static int stokes_A3(pl3_ctx* ctx, const Vec3& in, const Vec3& out) {
    P3_TRY(halo3(ctx, in));
    launch_apply3<true>(ctx, ctx->op, in, out);
    ctx->napply++;
    return 0;
}
// block-triangular [[A_vv, A_vp], [0, S^]]: the pressure by S^-1, one V-cycle for the velocities, then the deflation correction
static int stokes_M3(pl3_ctx* ctx, const Vec3& in, const Vec3& out) {
    const G3& g = ctx->geom.d;
    Lev3* L0 = ctx->levels[0];
    P3_TRY(halo3(ctx, in.prs()));                // S^-1 r_p of the neighbour cell (A_vp z_p) reads the pressure residual one node beyond the block
    launch3(ctx, g, k3_stage1, ctx->op, cv4(in), out[3], wv3(L0->f));
    int ob = 0;
    if (ctx->levels.size() > 1) {           // the post-smoothing sweep of the finest level writes the velocities into out[0..2] itself
        const W3 fo = wv3(out);
        P3_TRY(vcycle3(ctx, 0, L0->f, ob, &fo));
    } else {
        P3_TRY(vcycle3(ctx, 0, L0->f, ob));
        for (int q = 0; q < 3; q++) P3_HIP(ctx, hipMemcpyAsync(out[q], L0->v[ob][q], (size_t)g.vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    }
    ctx->nprec++;
    if (ctx->dfl_active) {                  // z += w yw.(r - A z) / yw.(A w); the continuity rows of A z come from z's velocities alone
        const Vec3 W = svec(ctx, 13), yw = arr3(ctx, ctx->dfl_y);
        const Vec3 a1[2] = {yw, yw}, b1[2] = {in.prs(), arr3(ctx, ctx->dfl_t)}; double o[2];
        P3_TRY(halo3(ctx, out.vel()));
        launch3(ctx, g, k3_cont_rows, ctx->op, cv3(out), ctx->dfl_t);
        P3_TRY(dots3(ctx, 2, a1, b1, o));
        const double coef = (o[0] - o[1]) / ctx->dfl_yAw;
        for (int c = 0; c < 4; c++) axpby3(ctx, out.part(c, 1), 1.0, out.part(c, 1), coef, W.part(c, 1));
    }
    return 0;
}
// The hydrostatic pressure x_h (zero velocities) into XH, and the dynamic-load reference norm |b - A x_h| (0: not usable) into ref.
// vec[4], vec[5]: work vectors of the iteration, free before it starts.
static int hydrostatic_start3(pl3_ctx* ctx, const Vec3& B, const Vec3& XH, double* ref) {
    const G3& g = ctx->geom.d;
    const Vec3 res = svec(ctx, 4), AX = svec(ctx, 5);
    double* P = XH[3];
    double* coltot = ctx->nranks > 1 ? AX.p : nullptr;      // several ranks: the column totals of this block
    P3_TRY(zero3(ctx, XH.vel()));
    hipLaunchKernelGGL(k3_hydro, dim3((g.n[2] + 63) / 64, (g.n[1] + 3) / 4), dim3(64, 4), 0, ctx->stream, ctx->op, P, coltot);
    if (ctx->nranks == 1)
        P3_HIP(ctx, hipMemcpyAsync(ctx->part, P + i3(g, 3, 2, 2), sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));     // anchor value
    else {
        // every block integrated from zero at its top: add the column totals of the blocks above (same block column), then the anchor
        // value -- one table [Pz][nx][ny] and one scalar summed over the ranks on the host (once per solve)
        const long long cols = (long long)g.n[1] * g.n[2], gcols = (long long)g.gn[1] * g.gn[2];
        std::vector<double> mine((size_t)cols), tab((size_t)ctx->P[0] * gcols, 0.0);
        P3_HIP(ctx, hipMemcpyAsync(mine.data(), coltot, (size_t)cols * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (int jj = 0; jj < g.n[1]; jj++) for (int kk = 0; kk < g.n[2]; kk++)
            tab[(size_t)ctx->pc[0] * gcols + (size_t)(g.o[1] + jj) * g.gn[2] + (g.o[2] + kk)] = mine[(size_t)jj * g.n[2] + kk];
        P3_TRY(allreduce3(ctx, tab.data(), (int)tab.size(), 0));
        for (int jj = 0; jj < g.n[1]; jj++) for (int kk = 0; kk < g.n[2]; kk++) {
            double a = 0.0;
            for (int q = 0; q < ctx->pc[0]; q++) a += tab[(size_t)q * gcols + (size_t)(g.o[1] + jj) * g.gn[2] + (g.o[2] + kk)];
            mine[(size_t)jj * g.n[2] + kk] = a;
        }
        P3_HIP(ctx, hipMemcpyAsync(coltot, mine.data(), (size_t)cols * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        launch3(ctx, g, k3_hydro_add, g, P, coltot);
        double av[1] = {0.0};
        const int ai = ctx->op.anchor[0] - g.o[0], aj = ctx->op.anchor[1] - g.o[1], ak = ctx->op.anchor[2] - g.o[2];
        if (ai >= 0 && ai < g.n[0] && aj >= 0 && aj < g.n[1] && ak >= 0 && ak < g.n[2])
            P3_HIP(ctx, hipMemcpyAsync(av, P + i3(g, ai, aj, ak), sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
        P3_TRY(allreduce3(ctx, av, 1, 0));
        P3_HIP(ctx, hipMemcpyAsync(ctx->part, av, sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
        P3_HIP(ctx, hipMemsetAsync(coltot, 0, (size_t)cols * sizeof(double), ctx->stream));
    }
    launch3(ctx, g, k3_shift, g, P, ctx->part);
    P3_TRY(stokes_A3(ctx, XH, AX));
    axpby3(ctx, res, 1.0, B, -1.0, AX);
    const Vec3 aa[2] = {res, B}; double d[2];
    P3_TRY(dots3(ctx, 2, aa, aa, d));
    *ref = std::sqrt(d[0]);
    if (!(*ref > 1e-9 * std::sqrt(d[1]))) *ref = 0.0;
    return 0;
}
// The deflation vector w = A^-1 u (pl_solver.hip, "deflation of the pressure-anchor mode"), kept in vec[13] between solves: tested
// against this operator, improved or solved for anew, and switched on (ctx->dfl_active, dfl_yAw, dfl_wvel2) if it is good.
// U: scratch for u; w: the work vectors of bicgstab3.
static int deflation_setup3(pl3_ctx* ctx, const Vec3& U, const Vec3* w) {
    const G3& g = ctx->geom.d;
    const Vec3 W = svec(ctx, 13);
    if (!ctx->dfl_y) { P3_TRY(dmal(ctx, &ctx->dfl_y, g.vol)); P3_TRY(dmal(ctx, &ctx->dfl_t, g.vol)); ctx->dfl_valid = false; }
    launch3(ctx, g, k3_defl_setup, ctx->op, wv4(U), ctx->dfl_y);
    auto activate = [&]() -> int {          // yw.(A w), from the continuity rows of w's velocities
        P3_TRY(halo3(ctx, W.vel()));
        launch3(ctx, g, k3_cont_rows, ctx->op, cv3(W), ctx->dfl_t);
        P3_TRY(dot3(ctx, arr3(ctx, ctx->dfl_y), arr3(ctx, ctx->dfl_t), &ctx->dfl_yAw));
        ctx->dfl_active = ctx->dfl_yAw != 0.0 && std::isfinite(ctx->dfl_yAw);
        return 0;
    };
    double q = 1.0;
    if (ctx->dfl_valid) {                   // quality of the kept vector for this operator: ||u - A w|| / ||u||
        const Vec3 res = w[K_S], AW = w[K_T]; double dq[2];
        P3_TRY(stokes_A3(ctx, W, AW));
        axpby3(ctx, res, 1.0, U, -1.0, AW);
        const Vec3 aa[2] = {res, U};
        P3_TRY(dots3(ctx, 2, aa, aa, dq));
        q = (dq[1] > 0.0 && std::isfinite(dq[0])) ? std::sqrt(dq[0] / dq[1]) : 1.0;
        ctx->dfl_last.q = q;
    }
    const bool reuse = ctx->dfl_valid && q < 0.5;
    if (reuse) P3_TRY(activate());
    if (!reuse || q > 0.1) {
        if (!reuse) P3_TRY(zero3(ctx, W));
        Stats3 st{};
        P3_TRY(bicgstab3(ctx, stokes_A3, stokes_M3, U, W, reuse, 1e-3, 80, w, &st, 0.0));
        ctx->dfl_valid = st.rel_residual < 0.05 && std::isfinite(st.rel_residual);
        ctx->dfl_last.inner_its = st.iterations; ctx->dfl_last.inner_res = st.rel_residual;
        ctx->dfl_active = false;
        if (ctx->dfl_valid) P3_TRY(activate());
    }
    if (ctx->dfl_active) P3_TRY(dot3(ctx, W.vel(), W.vel(), &ctx->dfl_wvel2));
    return 0;
}
// ---- warm start of the Stokes solve from its solution history (opt-in, one rank) -----------------------------------------------
static void history_free3(pl3_ctx* ctx) {
    for (double*& q : ctx->hist) { if (q) (void)hipFree(q); q = nullptr; }
    history_clear3(ctx);
}
// points: solutions kept, 0 (off, frees the history) or 2 .. X0_HIST + 1; order: degree of the extrapolating polynomial, 1 .. 3, with
// points >= order + 1.  A change of either clears the history.
extern "C" int pl3_stokes_set_warm_start(pl3_ctx* ctx, int points, int order) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_set_warm_start: NULL context");
    if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, "pl3_stokes_set_warm_start: a context with pl3_set_comm attached has no warm start (one rank)");
    if (points != 0) {
        if (points < 2 || points > X0_HIST + 1)
            return p3_fail(ctx, "pl3_stokes_set_warm_start: points = " + std::to_string(points) + " must be 0 (off) or 2 .. " + std::to_string(X0_HIST + 1));
        if (order < 1 || order > 3) return p3_fail(ctx, "pl3_stokes_set_warm_start: order = " + std::to_string(order) + " must be 1 .. 3");
        if (points < order + 1)
            return p3_fail(ctx, "pl3_stokes_set_warm_start: order = " + std::to_string(order) + " needs points >= " + std::to_string(order + 1) +
                                    ", got points = " + std::to_string(points));
    }
    if (points == ctx->warm_points && (points == 0 || order == ctx->warm_order)) return 0;
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    history_free3(ctx);
    ctx->warm_points = 0; ctx->warm_order = 0; ctx->warm_last = {};
    for (int k = 0; k < points; k++)
        if (dmal(ctx, &ctx->hist[k], 4 * ctx->geom.d.vol)) { const std::string m = ctx->err; history_free3(ctx); return p3_fail(ctx, "pl3_stokes_set_warm_start: " + m); }
    ctx->warm_points = points; ctx->warm_order = points ? order : 0;
    return 0;
}
extern "C" int pl3_stokes_get_warm_start(pl3_ctx* ctx, int* points, int* order) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_get_warm_start: NULL context");
    if (points) *points = ctx->warm_points;
    if (order) *order = ctx->warm_order;
    return 0;
}
// The device solution of the last pl3_stokes_solve becomes the newest time level; dt > 0: the model time from it to the next solve.
// Warm start off: nothing happens.
extern "C" int pl3_stokes_history_commit(pl3_ctx* ctx, double dt) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_history_commit: NULL context");
    if (!ctx->warm_points) return 0;
    if (!(dt > 0.0) || !std::isfinite(dt)) return p3_fail(ctx, "pl3_stokes_history_commit: dt = " + num_str3(dt) + " must be positive and finite");
    if (!ctx->have_x) return p3_fail(ctx, "pl3_stokes_history_commit: no Stokes solution to commit (pl3_stokes_solve has not run on this context)");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    const int np = ctx->warm_points;
    double* newest = ctx->hist[np - 1];                 // the oldest level's storage takes the new one
    for (int k = np - 1; k > 0; k--) ctx->hist[k] = ctx->hist[k - 1];
    ctx->hist[0] = newest;
    P3_HIP(ctx, hipMemcpyAsync(newest, ctx->vec[11], (size_t)4 * ctx->geom.d.vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    for (int k = X0_HIST; k > 0; k--) ctx->dt_hist[k] = ctx->dt_hist[k - 1];
    ctx->dt_hist[0] = dt;
    ctx->warm_held = std::min(ctx->warm_held + 1, np);
    return 0;
}
extern "C" int pl3_stokes_history_clear(pl3_ctx* ctx) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_history_clear: NULL context");
    history_clear3(ctx);
    return 0;
}
// X = sum_k L_k h_k with the weights of pl_x0.h (the header of the 2-D step: its fall-backs for a doubled time step and a short
// history come with it); what it used goes into ctx->warm_last
static int x0_start3(pl3_ctx* ctx, const Vec3& X) {
    const X0Weights wt = pl_x0_weights(ctx->dt_hist, ctx->warm_held - 1, ctx->warm_points - 1, ctx->warm_order, 1.0);
    X0Start3 a{};
    a.n = wt.nh + 1;
    for (int k = 0; k < a.n; k++) { a.h[k] = ctx->hist[k]; a.l[k] = k ? wt.l[k - 1] : wt.l0; }
    if (wt.nh >= 2 && wt.nh <= ctx->warm_order) {
        // The fit interpolates: its weights are the Lagrange basis values at the time of the solve.  The normal equations of the
        // header leave some 30 eps in them, more than the kernel's own rounding, so they are evaluated directly, in long double,
        // on the header's choice of levels (times 0, -d[1], -d[1] - d[2], ...; the solve at +d[0]).
        long double t[X0_HIST + 1] = {0.0L};
        for (int k = 1; k < a.n; k++) t[k] = t[k - 1] - (long double)ctx->dt_hist[k];
        for (int i = 0; i < a.n; i++) {
            long double l = 1.0L;
            for (int j = 0; j < a.n; j++) if (j != i) l *= ((long double)ctx->dt_hist[0] - t[j]) / (t[i] - t[j]);
            a.l[i] = (double)l;
        }
    }
    ctx->warm_last.used = a.n;
    for (int k = 0; k < 3; k++) ctx->warm_last.l[k] = k < a.n ? a.l[k] : 0.0;
    hipLaunchKernelGGL(k3_x0_start, g1(X.n()), dim3(256), 0, ctx->stream, X.n(), a, X.p);
    P3_HIP(ctx, hipGetLastError());
    return 0;
}
// out: levels held; start of the last solve (0 cold: off or no history, 1 warm, 2 warm rejected by the guard); levels it used; |r0| of
// the warm candidate; ref; its first three weights (newest first)
extern "C" int pl3_stokes_history_info(pl3_ctx* ctx, double out[8]) {
    if (!ctx || !out) return p3_fail(ctx, "pl3_stokes_history_info: NULL argument");
    out[0] = ctx->warm_held; out[1] = ctx->warm_last.start; out[2] = ctx->warm_last.used; out[3] = ctx->warm_last.r0; out[4] = ctx->warm_last.ref;
    for (int k = 0; k < 3; k++) out[5 + k] = ctx->warm_last.l[k];
    return 0;
}
// The linear combination as the next solve would form it, before halo3 and k3_close: out (nz, nx, ny, 4).  Leaves the record of the last
// solve (pl3_stokes_history_info) alone.
extern "C" int pl3_stokes_start_vector(pl3_ctx* ctx, double* out) {
    if (!ctx || !out) return p3_fail(ctx, "pl3_stokes_start_vector: NULL argument");
    if (!ctx->warm_points) return p3_fail(ctx, "pl3_stokes_start_vector: warm start is off (pl3_stokes_set_warm_start)");
    if (ctx->warm_held < 1) return p3_fail(ctx, "pl3_stokes_start_vector: the history is empty (pl3_stokes_history_commit)");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    const auto keep = ctx->warm_last;
    const Vec3 S = svec(ctx, K_T);
    const int rc = x0_start3(ctx, S);
    ctx->warm_last = keep;
    if (rc) return rc;
    return download3(ctx, wv4(S).p, 4, out);
}
extern "C" int pl3_stokes_solve(pl3_ctx* ctx, const double* rhs, double* x, int use_x0, double rtol, int maxit, pl_solve_stats* stats) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    // x == NULL: device-resident solve -- the solution stays in the context (pl3_get_solution fetches it), use_x0 starts from the
    // solution the context holds from its previous solve
    if (!x && use_x0 && !ctx->have_x) return p3_fail(ctx, "pl3_stokes_solve: no resident solution to start from");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    if (rtol <= 0) rtol = 1e-7;
    if (maxit <= 0) maxit = 600;
    const G3& g = ctx->geom.d;
    P3_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    P3_TRY(build_levels3(ctx));
    Vec3 w[K_NW];
    for (int q = 0; q < K_NW; q++) w[q] = svec(ctx, q);
    const Vec3 B = svec(ctx, 10), X = svec(ctx, 11), XH = svec(ctx, 12);
    if (rhs) { P3_TRY(upload3(ctx, rhs, 4, wv4(B).p)); launch3(ctx, g, k3_scale_rows, ctx->op, wv4(B)); }
    else launch3(ctx, g, k3_rhs, ctx->op, wv4(B), 1, ctx->wallvel, ctx->wallflow);
    ctx->napply = ctx->nprec = 0;
    ctx->dfl_active = false; ctx->dfl_yAw = 1.0; ctx->dfl_wvel2 = 0.0;
    double ref = 0.0;
    P3_TRY(hydrostatic_start3(ctx, B, XH, &ref));
    // warm start: the operator's own right-hand side, no start given, and at least one committed solution
    const bool warm = !rhs && !use_x0 && ctx->warm_points > 0 && ctx->warm_held > 0;
    ctx->warm_last = {};
    ctx->warm_last.ref = ref;
    if (use_x0) { if (x) P3_TRY(upload3(ctx, x, 4, wv4(X).p)); }
    else if (warm) P3_TRY(x0_start3(ctx, X));
    else P3_HIP(ctx, hipMemcpyAsync(X.p, XH.p, (size_t)X.n() * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    P3_TRY(halo3(ctx, X.vel()));
    launch3(ctx, g, k3_close, ctx->op, wv3(X), cv3(B));
    bool r0_kept = false;          // w[K_R0] holds the residual of the start (the guard's), for bicgstab3 to take over
    if (warm) {
        // the guard: the extrapolated start is kept only if its residual is below the hydrostatic start's, the reference of the stopping
        // test; otherwise the solve is the cold one from here on (w[K_V], w[K_R0]: written before they are read by what follows)
        const int napply0 = ctx->napply; double rr = 0.0;
        P3_TRY(stokes_A3(ctx, X, w[K_V]));
        axpby3(ctx, w[K_R0], 1.0, B, -1.0, w[K_V]);
        P3_TRY(dot3(ctx, w[K_R0], w[K_R0], &rr));
        ctx->warm_last.r0 = std::sqrt(rr);
        ctx->warm_last.start = 1; r0_kept = true;
        if (!(ref > 0.0) || !(ctx->warm_last.r0 < ref)) {          // (a NaN fails)
            ctx->warm_last.start = 2; ctx->napply = napply0; r0_kept = false;
            P3_HIP(ctx, hipMemcpyAsync(X.p, XH.p, (size_t)X.n() * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            P3_TRY(halo3(ctx, X.vel()));
            launch3(ctx, g, k3_close, ctx->op, wv3(X), cv3(B));
        }
    }
    static const bool defl_on = !(getenv("PYLAMP_DEFLATE") && atoi(getenv("PYLAMP_DEFLATE")) == 0);
    if (const char* e = getenv("PYLAMP_STOKES_ETOL")) { const double v = atof(e); if (v >= 0.0) ctx->etol = v; }
    ctx->dfl_last = {};
    if (defl_on && ctx->levels.size() > 1) P3_TRY(deflation_setup3(ctx, XH, w));        // (the hydrostatic vector is not needed any more)
    ctx->dfl_last.active = ctx->dfl_active ? 1 : 0;
    if (!(ctx->dfl_last.inner_res < 0.0)) r0_kept = false;         // the inner solve for the deflation vector ran on the same work vectors
    Stats3 st{};
    P3_TRY(bicgstab3(ctx, stokes_A3, stokes_M3, B, X, true, rtol, maxit, w, &st, ref, ctx->etol, r0_kept));
    ctx->dfl_last.checks = st.checks; ctx->dfl_last.rec_it = st.rec_it;
    for (int q = 0; q < 6; q++) ctx->dfl_last.rec[q] = st.rec_it ? st.rec[q] : 0.0;
    ctx->dfl_active = false;
    P3_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    P3_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0; P3_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->have_x = true;
    if (x) P3_TRY(download3(ctx, wv4(X).p, 4, x));
    if (stats) { stats->iterations = st.iterations; stats->converged = st.converged; stats->rel_residual = st.rel_residual; stats->solve_ms = ms;
                 stats->operator_applies = ctx->napply; stats->precond_applies = ctx->nprec; stats->used_direct = 0; stats->error_estimate = st.error_estimate; }
    return 0;
}
extern "C" int pl3_stokes_mg_info(pl3_ctx* ctx, int* nlevels, double* lmax, int max_levels) {
    if (nlevels) *nlevels = (int)ctx->levels.size();
    for (int l = 0; lmax && l < max_levels && l < (int)ctx->levels.size(); l++) lmax[l] = ctx->levels[l]->lmax;
    return 0;
}
// What vcycle3 does on a hierarchy of this context (read-only; any pointer may be NULL): nu[2] = sweeps on the finest level and on the
// others, the Chebyshev ratio of their window, sweeps and ratio of the coarsest level, and per level whether the marching LDS kernels
// take it.  Valid once the hierarchy is built (a solve or pl3_stokes_precond_apply).
extern "C" int pl3_stokes_mg_plan(pl3_ctx* ctx, int* nu, double* ratio, int* coarse_sweeps, double* coarse_ratio, int* lds, int max_levels) {
    if (nu) level_nu3(ctx, nu[0], nu[1]);
    if (ratio) *ratio = ctx->cheb_ratio;
    int cn = 0; double cr = 0.0;
    if (!ctx->levels.empty()) coarsest_plan3(ctx, ctx->levels.back()->gh.d, cn, cr);
    if (coarse_sweeps) *coarse_sweeps = cn;
    if (coarse_ratio) *coarse_ratio = cr;
    for (int l = 0; lds && l < max_levels && l < (int)ctx->levels.size(); l++) lds[l] = k3_use_lds(ctx->levels[l]->gh.d) ? 1 : 0;
    return 0;
}
// z = M^-1 r by stokes_M3 itself, without the deflation correction: r is the row-scaled residual as bicgstab3 hands it over
static int precond_apply3(pl3_ctx* ctx, const double* r, double* z, bool deflated) {
    if (!ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    if (!r || !z) return p3_fail(ctx, "pl3_stokes_precond_apply: NULL argument");
    if (deflated && !(ctx->dfl_valid && ctx->dfl_last.active)) return p3_fail(ctx, "pl3_stokes_precond_apply_deflated: the last solve of this context did not deflate");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    P3_TRY(build_levels3(ctx));
    const Vec3 R = svec(ctx, 0), Z = svec(ctx, 1);
    P3_TRY(upload3(ctx, r, 4, wv4(R).p));
    ctx->dfl_active = deflated;
    const int rc = stokes_M3(ctx, R, Z);
    ctx->dfl_active = false;
    P3_TRY(rc);
    P3_HIP(ctx, hipGetLastError());
    P3_TRY(download3(ctx, wv4(Z).p, 4, z));
    return 0;
}
extern "C" int pl3_stokes_precond_apply(pl3_ctx* ctx, const double* r, double* z) { return precond_apply3(ctx, r, z, false); }
// ... and with the deflation correction of the last solve: its w (work vector 13), yw and yw.(A w)
extern "C" int pl3_stokes_precond_apply_deflated(pl3_ctx* ctx, const double* r, double* z) { return precond_apply3(ctx, r, z, true); }

// ---- component tests of the Krylov loop (tests/test_hip_3d_krylov.py): the solve's own kernels and host epilogues on given vectors ----
// One launch of one Krylov kernel.  in[q] (q < 10; (nz, nx, ny, 4) host vectors, NULL: none) goes into Stokes work vector q -- equal
// pointers share the work vector of the first -- and out[q] != NULL receives work vector q afterwards.  Slots per kernel:
//   PL3_PROBE_DOTS     scal[0] = nd products (1 .. 5) a_q . b_q, a_q = in[q], b_q = in[5 + q]; sums[0 .. nd - 1] (dots3: k3_dots on one
//                      rank, k3_dots_own and the all-reduce on an attached context)
//   PL3_PROBE_DOTS11   t, s, rt = in[0 .. 2], x = in[3] or NULL, dx = in[4] or NULL or in[3] itself, yw: the (nz, nx, ny) array or NULL;
//                      sums[0 .. 10]
//   PL3_PROBE_AXPBY    work 2 = scal[0] in[0] + scal[1] in[1]
//   PL3_PROBE_P        p, r, v = in[0 .. 2]; beta, omega = scal[0 .. 1]; p in work 0
//   PL3_PROBE_XR       x, y, z, r, s, t = in[0 .. 5]; alpha, omega; x in work 0, r in work 3
//   PL3_PROBE_XRP      x, y, z, r, s, t, p, v = in[0 .. 7]; alpha, omega, beta; x, r, p in work 0, 3, 6
//   PL3_PROBE_RANDOM   scal[0] = seed; the shadow residual in work 0
extern "C" int pl3_krylov_probe(pl3_ctx* ctx, int what, const double* const in[10], const double* yw, const double scal[3], double* const out[10],
                                double* sums) {
    if (!ctx) return p3_fail(ctx, "pl3_krylov_probe: NULL context");
    if (!in || !scal) return p3_fail(ctx, "pl3_krylov_probe: NULL argument");
    static const int nin[7] = {0, 3, 2, 3, 6, 8, 0};
    if (what < 0 || what > PL3_PROBE_RANDOM) return p3_fail(ctx, "pl3_krylov_probe: unknown kernel");
    const int nd = what == PL3_PROBE_DOTS ? (int)scal[0] : 0;
    if (what == PL3_PROBE_DOTS && (nd < 1 || nd > 5)) return p3_fail(ctx, "pl3_krylov_probe: 1 .. 5 products");
    if (what == PL3_PROBE_DOTS11 && ctx->nranks > 1) return p3_fail(ctx, "pl3_krylov_probe: the fused reduction runs on one rank");
    if ((what == PL3_PROBE_DOTS || what == PL3_PROBE_DOTS11) && !sums) return p3_fail(ctx, "pl3_krylov_probe: NULL sums");
    for (int q = 0; q < nin[what]; q++) if (!in[q]) return p3_fail(ctx, "pl3_krylov_probe: an operand is missing");
    for (int q = 0; q < nd; q++) if (!in[q] || !in[5 + q]) return p3_fail(ctx, "pl3_krylov_probe: an operand is missing");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    Vec3 v[10];
    for (int q = 0; q < 10; q++) {
        v[q] = svec(ctx, q);
        if (!in[q]) continue;
        int first = q;
        for (int p = 0; p < q; p++) if (in[p] == in[q]) { first = p; break; }
        if (first != q) v[q] = v[first];
        else P3_TRY(upload3(ctx, in[q], 4, wv4(v[q]).p));
    }
    const long long n = v[0].n();
    const double* ywd = nullptr;
    if (what == PL3_PROBE_DOTS11 && yw) {          // (an array of its own: the solve's yw stays as the last solve left it)
        double* a = svec(ctx, 10).p;
        P3_TRY(upload3(ctx, yw, 1, &a));
        ywd = a;
    }
    switch (what) {
    case PL3_PROBE_DOTS: P3_TRY(dots3(ctx, nd, v, v + 5, sums)); break;
    case PL3_PROBE_DOTS11: P3_TRY(dots11_3(ctx, v[0], v[1], v[2], in[3] ? &v[3] : nullptr, in[4] ? &v[4] : nullptr, ywd, sums)); break;
    case PL3_PROBE_AXPBY: axpby3(ctx, v[2], scal[0], v[0], scal[1], v[1]); break;
    case PL3_PROBE_P:
        hipLaunchKernelGGL(k3_p_update, g1(n), dim3(256), 0, ctx->stream, n, v[0].p, (const double*)v[1].p, (const double*)v[2].p, scal[0], scal[1]);
        break;
    case PL3_PROBE_XR:
        hipLaunchKernelGGL(k3_xr_update, g1(n), dim3(256), 0, ctx->stream, n, v[0].p, (const double*)v[1].p, (const double*)v[2].p, v[3].p,
                           (const double*)v[4].p, (const double*)v[5].p, scal[0], scal[1]);
        break;
    case PL3_PROBE_XRP:
        hipLaunchKernelGGL(k3_xrp_update, g1(n), dim3(256), 0, ctx->stream, n, v[0].p, (const double*)v[1].p, (const double*)v[2].p, v[3].p,
                           (const double*)v[4].p, (const double*)v[5].p, v[6].p, (const double*)v[7].p, scal[0], scal[1], scal[2]);
        break;
    default: random3(ctx, v[0], (unsigned)scal[0]); break;
    }
    P3_HIP(ctx, hipGetLastError());
    for (int q = 0; out && q < 10; q++) if (out[q]) P3_TRY(download3(ctx, wv4(svec(ctx, q)).p, 4, out[q]));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
// The hydrostatic start of pl3_stokes_solve(rhs = NULL): the scaled right-hand side, then hydrostatic_start3, exactly as the solve calls
// them.  xh (nz, nx, ny, 4) receives x_h, *ref the reference norm |b - A x_h| (0: not usable).  Collective on an attached context.
extern "C" int pl3_stokes_hydrostatic(pl3_ctx* ctx, double* xh, double* ref) {
    if (!ctx || !ctx->op_ready) return p3_fail(ctx, "stokes operator not set");
    if (!xh || !ref) return p3_fail(ctx, "pl3_stokes_hydrostatic: NULL argument");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    const G3& g = ctx->geom.d;
    const Vec3 B = svec(ctx, 10), XH = svec(ctx, 12);
    launch3(ctx, g, k3_rhs, ctx->op, wv4(B), 1, ctx->wallvel, ctx->wallflow);
    P3_TRY(hydrostatic_start3(ctx, B, XH, ref));
    P3_HIP(ctx, hipGetLastError());
    return download3(ctx, wv4(XH).p, 4, xh);
}
// Stokes work vector `index` (0 .. 13) as the last solve left it: K_R 0, K_RT 1, K_S 4 (the last true residual), K_DX 8, 10 the scaled
// right-hand side, 13 the deflation vector w
extern "C" int pl3_stokes_work_vector(pl3_ctx* ctx, int index, double* out) {
    if (!ctx || !out) return p3_fail(ctx, "pl3_stokes_work_vector: NULL argument");
    if (index < 0 || index >= 14 || !ctx->vec[index]) return p3_fail(ctx, "pl3_stokes_work_vector: no such work vector (0 .. 13, after a solve)");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    return download3(ctx, wv4(svec(ctx, index)).p, 4, out);
}
// What the last pl3_stokes_solve did about the deflation: out[0] dfl_valid, [1] the deflation was on during the solve, [2] the quality
// |u - A w| / |u| of the kept vector as measured (-1: none was), [3] iterations of the inner solve (0: w reused as it is), [4] its final
// |u - A w| / |u| (-1: no inner solve), [5] yw.(A w), [6] |w_vel|^2, [7] true-residual checks of the solve (Est3::checks).
// [8] the iteration at which the estimate between the checks was last evaluated (0: never), [9] its value, [10 .. 14] what went into it:
// |r|^2, |r_cont|^2, |x_vel|^2, the anchor part, a_mom.
// u, yw (either may be NULL): the (nz, nx, ny) pressure plane of u and yw of k3_defl_setup, meaningful when out[1] or out[2] >= 0.
extern "C" int pl3_stokes_defl_info(pl3_ctx* ctx, double out[15], double* u, double* yw) {
    if (!ctx) return p3_fail(ctx, "pl3_stokes_defl_info: NULL context");
    if (out) {
        out[0] = ctx->dfl_valid ? 1.0 : 0.0; out[1] = ctx->dfl_last.active; out[2] = ctx->dfl_last.q; out[3] = ctx->dfl_last.inner_its;
        out[4] = ctx->dfl_last.inner_res; out[5] = ctx->dfl_yAw; out[6] = ctx->dfl_wvel2; out[7] = ctx->dfl_last.checks;
        out[8] = ctx->dfl_last.rec_it;
        for (int q = 0; q < 6; q++) out[9 + q] = ctx->dfl_last.rec[q];
    }
    if ((u || yw) && !(ctx->dfl_y && ctx->vec[12])) return p3_fail(ctx, "pl3_stokes_defl_info: no deflation set-up has run on this context");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    if (u) { double* a = svec(ctx, 12)[3]; P3_TRY(download3(ctx, &a, 1, u)); }
    if (yw) { double* a = ctx->dfl_y; P3_TRY(download3(ctx, &a, 1, yw)); }
    return 0;
}
// sum |entry| over the ring and padding entries of the 14 Stokes work vectors of THIS rank's block (one rank: they are zero and stay
// zero; on blocks the rings hold the neighbours' values, and the sum is not reduced over the ranks)
extern "C" int pl3_stokes_ring_sum(pl3_ctx* ctx, double* out) {
    if (!ctx || !out) return p3_fail(ctx, "pl3_stokes_ring_sum: NULL argument");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, 14));
    double tot = 0.0;
    for (int q = 0; q < 14; q++) {
        double s;
        hipLaunchKernelGGL(k3_ring_abs, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, ctx->geom.d, 4, (const double*)ctx->vec[q], ctx->part);
        P3_TRY(sum_partials3(ctx, 5, 1, &s));
        tot += s;
    }
    *out = tot;
    return 0;
}

// ---- heat ----------------------------------------------------------------------------------------------------------------------
// src: kz, kx, ky, T, H, rho, cp -- host arrays (upload3) or, with dev, plain device arrays (ring3)
static int heat_set3(pl3_ctx* ctx, const double* const mp[3], const double* const src[7], bool dev, const int bc[6], const double bcvalue[6], double tstep) {
    for (int w = 0; w < 6; w++) if (bc[w] != PL_BC_FIXTEMP && bc[w] != PL_BC_FIXFLOW) return p3_fail(ctx, "heat: boundary condition must be FIXTEMP or FIXFLOW");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    const G3& g = ctx->geom.d;
    for (double** q : {&ctx->hk[0], &ctx->hk[1], &ctx->hk[2], &ctx->hT, &ctx->hH, &ctx->hcdt, &ctx->hrho, &ctx->hcp}) if (!*q) P3_TRY(dmal(ctx, q, g.vol));
    double* dst[7] = {ctx->hk[0], ctx->hk[1], ctx->hk[2], ctx->hT, ctx->hH, ctx->hrho, ctx->hcp};
    for (int q = 0; q < 7; q++) {
        if (dev) P3_TRY(ring3(ctx, src[q], dst[q]));
        else P3_TRY(upload3(ctx, src[q], 1, &dst[q]));
    }
    size_t len[3], tot = 0;
    for (int a = 0; a < 3; a++) { len[a] = (size_t)g.gn[a] + 2 * PL_TOFF + 2; tot += len[a]; }
    std::vector<double> t(tot, 0.0);
    size_t off = 0, offs[3];
    for (int a = 0; a < 3; a++) { offs[a] = off; for (int i = 1; i < g.gn[a]; i++) t[off + i + PL_TOFF] = 1.0 / (mp[a][i] - mp[a][i - 1]); off += len[a]; }
    if (!ctx->htab) P3_HIP(ctx, hipMalloc((void**)&ctx->htab, tot * sizeof(double)));
    pl3_count_copy(ctx, tot * sizeof(double));
    P3_HIP(ctx, hipMemcpy(ctx->htab, t.data(), tot * sizeof(double), hipMemcpyHostToDevice));
    if (!ctx->hbcv) P3_HIP(ctx, hipMalloc((void**)&ctx->hbcv, 6 * sizeof(double)));
    pl3_count_copy(ctx, 6 * sizeof(double));
    P3_HIP(ctx, hipMemcpy(ctx->hbcv, bcvalue, 6 * sizeof(double), hipMemcpyHostToDevice));
    Heat3& op = ctx->hop;
    op.g = g; for (int a = 0; a < 3; a++) { op.kk[a] = ctx->hk[a]; op.rdb[a] = ctx->htab + offs[a]; }
    op.cdt = ctx->hcdt; for (int w = 0; w < 6; w++) op.bc[w] = bc[w];
    launch3(ctx, g, k3_heat_coef, g, ctx->hrho, ctx->hcp, tstep, ctx->hcdt);
    P3_HIP(ctx, hipGetLastError());
    ctx->hop_ready = true;
    return 0;
}
extern "C" int pl3_heat_set_coeffs(pl3_ctx* ctx, const double* zmp, const double* xmp, const double* ymp, const double* T, const double* kz,
                                   const double* kx, const double* ky, const double* cp, const double* rho, const double* H, const int bc[6],
                                   const double bcvalue[6], double tstep) {
    if (!zmp || !xmp || !ymp || !T || !kz || !kx || !ky || !cp || !rho || !H || !bc || !bcvalue) return p3_fail(ctx, "pl3_heat_set_coeffs: NULL argument");
    const double* src[7] = {kz, kx, ky, T, H, rho, cp}; const double* mp[3] = {zmp, xmp, ymp};
    return heat_set3(ctx, mp, src, false, bc, bcvalue, tstep);
}
int pl3i_heat_set_coeffs_dev(pl3_ctx* ctx, const double* const mp[3], const double* const src[7], const int bc[6], const double bcvalue[6], double tstep) {
    if (ctx->nranks > 1) return p3_fail(ctx, "device-source heat coefficients run on one rank");
    return heat_set3(ctx, mp, src, true, bc, bcvalue, tstep);
}
// Values or fluxes of the heat walls as profiles: values[w] is the plane of wall w over its NODES ("Wall planes"), or
// NULL for a wall that keeps its one value bcvalue[w]; all NULL clears the setting and frees the planes.  Kept on the context like the
// Stokes wall settings; a rejected call changes nothing.  Entries at nodes another wall owns are never read and are not looked at here.
extern "C" int pl3_heat_set_wall_values(pl3_ctx* ctx, const double* const values[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_heat_set_wall_values: NULL context");
    if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, "pl3_heat_set_wall_values: profiles over the heat walls run on one rank (this context has pl3_set_comm attached)");
    P3_TRY(planes3_set(ctx, ctx->hplanes, "pl3_heat_set_wall_values", "entry", true, true, values));
    for (int w = 0; w < 6; w++) ctx->hwall.v[w] = ctx->hplanes.plane(w);
    return 0;
}
extern "C" int pl3_heat_get_wall_values(pl3_ctx* ctx, int* mask, double* const values[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_heat_get_wall_values: NULL context");
    if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, "pl3_heat_get_wall_values: profiles over the heat walls run on one rank (this context has pl3_set_comm attached)");
    return planes3_get(ctx, ctx->hplanes, mask, values);
}
// the right-hand side of the heat rows into rhs: the kernel without planes unless the context holds some
static void heat_rhs3(pl3_ctx* ctx, double* rhs, int scaled) {
    if (ctx->hplanes.mask) launch3(ctx, ctx->hop.g, k3_heat_rhs<true>, ctx->hop, ctx->hT, ctx->hH, ctx->hbcv, ctx->hwall, rhs, scaled);
    else launch3(ctx, ctx->hop.g, k3_heat_rhs<false>, ctx->hop, ctx->hT, ctx->hH, ctx->hbcv, Heat3Planes{}, rhs, scaled);
}
static int need_hvecs(pl3_ctx* ctx) {
    for (int v = 0; v < 12; v++) if (!ctx->hvec[v]) P3_TRY(dmal(ctx, &ctx->hvec[v], ctx->geom.d.vol));
    if (!ctx->part) { P3_TRY(dmal(ctx, &ctx->part, 11 * D3_BLOCKS)); P3_HIP(ctx, hipHostMalloc((void**)&ctx->hpart, 11 * D3_BLOCKS * sizeof(double))); }
    return 0;
}
extern "C" int pl3_heat_apply(pl3_ctx* ctx, const double* x, double* y) {
    if (!ctx->hop_ready) return p3_fail(ctx, "heat operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_hvecs(ctx));
    P3_TRY(upload3(ctx, x, 1, &ctx->hvec[0]));
    launch3(ctx, ctx->hop.g, k3_heat_apply<false>, ctx->hop, ctx->hvec[0], ctx->hvec[1]);
    P3_HIP(ctx, hipGetLastError());
    return download3(ctx, &ctx->hvec[1], 1, y);
}
extern "C" int pl3_heat_rhs(pl3_ctx* ctx, double* rhs) {
    if (!ctx->hop_ready) return p3_fail(ctx, "heat operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_hvecs(ctx));
    heat_rhs3(ctx, ctx->hvec[1], 0);
    P3_HIP(ctx, hipGetLastError());
    return download3(ctx, &ctx->hvec[1], 1, rhs);
}
static int heat_A3(pl3_ctx* ctx, const Vec3& in, const Vec3& out) {
    P3_TRY(halo3(ctx, in));
    launch3(ctx, *in.g, k3_heat_apply<true>, ctx->hop, in.p, out.p);
    ctx->napply++;
    return 0;
}
extern "C" int pl3_heat_solve(pl3_ctx* ctx, const double* rhs, double* x, double rtol, int maxit, pl_solve_stats* stats) {
    if (!ctx->hop_ready) return p3_fail(ctx, "heat operator not set");
    P3_HIP(ctx, hipSetDevice(ctx->device));       // x == NULL: the solution stays on the device (pl3_get_solution)
    P3_TRY(need_hvecs(ctx));
    if (rtol <= 0) rtol = 1e-12;
    if (maxit <= 0) maxit = 2000;
    P3_HIP(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const Vec3 B = hvec(ctx, 10), X = hvec(ctx, 11);
    if (rhs) return p3_fail(ctx, "pl3_heat_solve: rhs must be NULL -- the system is solved for the operator's own right-hand side (pl3_heat_rhs)");
    heat_rhs3(ctx, B.p, 1);
    ctx->napply = 0;
    Vec3 w[K_NW];
    for (int q = 0; q < K_NW; q++) w[q] = hvec(ctx, q);
    Stats3 st{};
    P3_TRY(bicgstab3(ctx, heat_A3, nullptr, B, X, false, rtol, maxit, w, &st, 0.0));
    P3_HIP(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    P3_HIP(ctx, hipEventSynchronize(ctx->ev1));
    float ms = 0; P3_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    ctx->have_T = true;
    if (x) P3_TRY(download3(ctx, &ctx->hvec[11], 1, x));
    if (stats) { stats->iterations = st.iterations; stats->converged = st.converged; stats->rel_residual = st.rel_residual; stats->solve_ms = ms;
                 stats->operator_applies = ctx->napply; stats->precond_applies = 0; }
    return 0;
}

// the solution of the last device-resident solve: which = 0 Stokes (nz, nx, ny, 4), 1 heat (nz, nx, ny)
extern "C" int pl3_get_solution(pl3_ctx* ctx, int which, double* out) {
    if (!out) return p3_fail(ctx, "pl3_get_solution: NULL argument");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    if (which == 0) {
        if (!ctx->have_x) return p3_fail(ctx, "pl3_get_solution: no Stokes solution yet");
        return download3(ctx, wv4(svec(ctx, 11)).p, 4, out);
    }
    if (!ctx->have_T) return p3_fail(ctx, "pl3_get_solution: no heat solution yet");
    return download3(ctx, &ctx->hvec[11], 1, out);
}
// The heat budget of a temperature field with the coefficients heat_set3 left on the device (include/pylamp_hip.h): out[0 .. 5] the heat
// flow into the box through z0, x0, y0, zL, xL, yL, out[6] the storage rate, out[7] the source.  T == NULL: the solution of the last
// pl3_heat_solve, still on the device.  One pass, fixed summation order.
extern "C" int pl3_heat_budget(pl3_ctx* ctx, const double* T, double out[8]) {
    if (!ctx) return p3_fail(nullptr, "pl3_heat_budget: NULL context");
    if (!out) return p3_fail(ctx, "pl3_heat_budget: NULL argument");
    if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, "pl3_heat_budget: the heat budget runs on one rank (this context has pl3_set_comm attached)");
    if (!ctx->hop_ready) return p3_fail(ctx, "pl3_heat_budget: heat operator not set (pl3_heat_set_coeffs)");
    if (!T && !ctx->have_T) return p3_fail(ctx, "pl3_heat_budget: NULL T means the solution of the last heat solve, and no heat solve has run on this context");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_hvecs(ctx));
    const double* field = ctx->hvec[11];
    if (T) { P3_TRY(upload3(ctx, T, 1, &ctx->hvec[0])); field = ctx->hvec[0]; }
    hipLaunchKernelGGL(k3_heat_budget, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, ctx->hop, field, (const double*)ctx->hT, (const double*)ctx->hH, ctx->part);
    P3_HIP(ctx, hipGetLastError());
    return sum_partials3(ctx, 8, 8, out);
}

// ---- strain rate, deviatoric stress and viscous dissipation (pl3_stokes_strain_fields; include/pylamp_hip.h) ------------
// Two per-node passes over the K3_PROLOGUE grid.  k3_strain_ce writes, at the element of node (i, j, k), the sum of the squared normal
// strain rates of the CELL whose lowest corner the node is and the squared shear strain rate of the three EDGES that start at the node
// (pair (D, E): along F); k3_strain_node gathers the eight cells and six edges around a node with their shares of the node's control
// volume, in a fixed order.  No atomics: a node's sum is one thread's.  The four intermediate arrays and the three results live in Stokes
// work vectors 1 and 2, which are free outside a solve (the velocities given by the host go to work vector 0).
//
// dv_D/dx_A on the edge of v_D at node idx[A] of axis A (element c): between the two midpoints inside; on a no-slip wall one-sided
// against the wall's velocity component U_D, 2 rd (v - U), as wall_coef3 / wall_rhs3 have it; dropped on a free-slip wall (what the
// zero-padded rD table does in row3)
template <int D, int A> __device__ inline double shear_half3(const Op3& op, const Pl3WallVel& mv, const double* __restrict__ u, long long c, const int* idx) {
    const G3& g = op.g;
    const int ia = idx[A], na = g.gn[A];
    if (ia == 0) return nos3<A>(op, 0) ? 2.0 * TB(g.rd[A], 0) * (u[c] - wall_vel3<A, D>(mv, 0)) : 0.0;
    if (ia == na - 1) return nos3<A>(op, 1) ? 2.0 * TB(g.rd[A], na - 2) * (wall_vel3<A, D>(mv, 1) - u[c - g.s[A]]) : 0.0;
    return 2.0 * TB(g.rD[A], ia) * (u[c] - u[c - g.s[A]]);
}
// eps_DE^2 on the edge of the pair (D, E = D + 1) at node idx[D], node idx[E], cell idx[F]; 0 where there is no such edge
template <int D> __device__ inline double edge_sq3(const Op3& op, const Pl3WallVel& mv, const double* const* v, long long c, const int* idx) {
    constexpr int E = (D + 1) % 3, F = (D + 2) % 3;
    if (idx[F] >= op.g.gn[F] - 1) return 0.0;
    const double e = 0.5 * (shear_half3<D, E>(op, mv, v[D], c, idx) + shear_half3<E, D>(op, mv, v[E], c, idx));
    return e * e;
}
__global__ __launch_bounds__(256) void k3_strain_ce(Op3 op, V3 x, Pl3WallVel mv, W4 o) {
    K3_PROLOGUE(op.g)
    const G3& g = op.g;
    const double* v[3] = {x.p[0], x.p[1], x.p[2]};
    double s = 0.0;
    if (i < g.gn[0] - 1 && j < g.gn[1] - 1 && k < g.gn[2] - 1) {
        const double ez = (v[0][c + g.s[0]] - v[0][c]) * TB(g.rd[0], i), ex = (v[1][c + g.s[1]] - v[1][c]) * TB(g.rd[1], j),
                     ey = (v[2][c + g.s[2]] - v[2][c]) * TB(g.rd[2], k);
        s = ez * ez + ex * ex + ey * ey;
    }
    o.p[0][c] = s;
    o.p[1][c] = edge_sq3<0>(op, mv, v, c, idx);
    o.p[2][c] = edge_sq3<1>(op, mv, v, c, idx);
    o.p[3][c] = edge_sq3<2>(op, mv, v, c, idx);
}
// along axis A at node ia: the shares wl, wh of the node's width that the cell below / above holds (0 and 1 on a wall) and the width h itself
// (half a cell on a wall)
template <int A> __device__ inline void node_w3(const G3& g, int ia, double& wl, double& wh, double& h) {
    const int n = g.gn[A];
    if (ia == 0) { wl = 0.0; wh = 1.0; h = 0.5 / TB(g.rd[A], 0); }
    else if (ia == n - 1) { wl = 1.0; wh = 0.0; h = 0.5 / TB(g.rd[A], n - 2); }
    else { const double rD = TB(g.rD[A], ia); wl = rD / TB(g.rd[A], ia - 1); wh = rD / TB(g.rd[A], ia); h = 0.5 / rD; }
}
// the two edges of the pair (D, D + 1) that meet at the node, the lower one first: t = 2 eta_edge
template <int D> __device__ inline void edges_node3(const Op3& op, const double* __restrict__ q, long long c, const double* wl, const double* wh,
                                                    double& Y, double& T, double& P) {
    constexpr int F = (D + 2) % 3;
    const long long sf = op.g.s[F];
    for (int d = 0; d < 2; d++) {
        const double w = d ? wh[F] : wl[F];
        if (w == 0.0) continue;
        const long long cc = d ? c : c - sf;
        const double e2 = q[cc], t = op.es[cc] + op.es[cc + sf];
        Y += w * (2.0 * e2); T += w * (2.0 * (t * t) * e2); P += w * (2.0 * t * e2);
    }
}
// e2 / t2 / phi: ringed arrays (NULL: not wanted); H: a plain (nz, nx, ny) array that gains phi, one IEEE addition per node (NULL: none)
struct Strain3Out { double* e2; double* t2; double* phi; double* H; };
// the weighted means Y, T, P of eps_ij eps_ij, tau_ij tau_ij and 2 eta eps_ij eps_ij around node (i, j, k) (element c) from the arrays of
// k3_strain_ce: the one order of summation of the node fields and of the node invariant of the yield stress (k3_yield_visc)
__device__ inline void node_sums3(const Op3& op, const V4& ce, long long c, int i, int j, int k, double& Y, double& T, double& P) {
    const G3& g = op.g;
    double wl[3], wh[3], h[3];
    node_w3<0>(g, i, wl[0], wh[0], h[0]); node_w3<1>(g, j, wl[1], wh[1], h[1]); node_w3<2>(g, k, wl[2], wh[2], h[2]);
    Y = 0.0; T = 0.0; P = 0.0;
    for (int dz = 0; dz < 2; dz++) {               // the eight cells: z outermost, the lower one first; t = 2 eta_n
        const double wz = dz ? wh[0] : wl[0];
        if (wz == 0.0) continue;
        for (int dx = 0; dx < 2; dx++) {
            const double wx = dx ? wh[1] : wl[1];
            if (wx == 0.0) continue;
            for (int dy = 0; dy < 2; dy++) {
                const double wy = dy ? wh[2] : wl[2];
                if (wy == 0.0) continue;
                const long long cc = c - (dz ? 0 : g.s[0]) - (dx ? 0 : g.s[1]) - (dy ? 0 : g.s[2]);
                const double w = wz * wx * wy, s = ce.p[0][cc], t = 2.0 * op.en[cc];
                Y += w * s; T += w * ((t * t) * s); P += w * (t * s);
            }
        }
    }
    edges_node3<0>(op, ce.p[1], c, wl, wh, Y, T, P);
    edges_node3<1>(op, ce.p[2], c, wl, wh, Y, T, P);
    edges_node3<2>(op, ce.p[3], c, wl, wh, Y, T, P);
}
__global__ __launch_bounds__(256) void k3_strain_node(Op3 op, V4 ce, Strain3Out o) {
    K3_PROLOGUE(op.g)
    const G3& g = op.g;
    double Y, T, P;
    node_sums3(op, ce, c, i, j, k, Y, T, P);
    if (o.e2) o.e2[c] = sqrt(0.5 * Y);
    if (o.t2) o.t2[c] = sqrt(0.5 * T);
    o.phi[c] = P;
    if (o.H) { const long long t = ((long long)li * g.n[1] + lj) * g.n[2] + lk; o.H[t] = __dadd_rn(o.H[t], P); }
}
// part[b] = the sum over workgroup b's nodes of phi x the node's control volume
__global__ __launch_bounds__(256) void k3_strain_total(G3 g, const double* __restrict__ phi, double* __restrict__ part) {
    const long long N = (long long)g.n[0] * g.n[1] * g.n[2];
    double acc[1] = {0.0};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < N; t += (long long)gridDim.x * 256) {
        const int k = (int)(t % g.n[2]), j = (int)((t / g.n[2]) % g.n[1]), i = (int)(t / ((long long)g.n[2] * g.n[1]));
        double wl, wh, hz, hx, hy;
        node_w3<0>(g, i, wl, wh, hz); node_w3<1>(g, j, wl, wh, hx); node_w3<2>(g, k, wl, wh, hy);
        acc[0] += phi[i3(g, i, j, k)] * (hz * hx * hy);
    }
    r3_block<R3All<R3_SUM, 1>>(acc, threadIdx.x, blockIdx.x, part);
}
static Vec3 strain_out3(pl3_ctx* ctx) { return svec(ctx, 2); }      // strainrate, stress, dissipation (ringed)
// the three node fields of the velocities vel (three ringed arrays; not work vector 1 or 2) into strain_out3; Hplain (NULL: none) gains the
// dissipation; total (NULL: not wanted): its integral over the box
static int strain_run3(pl3_ctx* ctx, const Vec3& vel, double* Hplain, double* total) {
    const G3& g = ctx->geom.d;
    const Vec3 ce = svec(ctx, 1), out = strain_out3(ctx);
    launch3(ctx, g, k3_strain_ce, ctx->op, cv3(vel), ctx->wallvel, wv4(ce));
    launch3(ctx, g, k3_strain_node, ctx->op, cv4(ce), Strain3Out{out[0], out[1], out[2], Hplain});
    P3_HIP(ctx, hipGetLastError());
    ctx->strain_kept = true;
    if (total) {
        hipLaunchKernelGGL(k3_strain_total, dim3(D3_BLOCKS), dim3(256), 0, ctx->stream, g, (const double*)out[2], ctx->part);
        P3_TRY(sum_partials3(ctx, 1, 1, total));
    }
    return 0;
}
// The velocities of the post-solve entry point `who`: the host arrays vz, vx, vy, uploaded to work vector 0, or, with all three NULL, the
// solution of the last Stokes solve (work vector 11).  what: the feature, as the one-rank message names it.
static int post_vel3(pl3_ctx* ctx, const char* who, const char* what, const double* vz, const double* vx, const double* vy, Vec3* vel) {
    const bool given = vz || vx || vy;
    if (given && !(vz && vx && vy)) return p3_fail(ctx, std::string(who) + ": vz, vx, vy must be given all three or all NULL");
    if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, std::string(who) + ": " + what + " on one rank (this context has pl3_set_comm attached)");
    if (!ctx->op_ready) return p3_fail(ctx, std::string(who) + ": no Stokes coefficients set (pl3_stokes_set_coeffs)");
    if (!given && !ctx->have_x) return p3_fail(ctx, std::string(who) + ": NULL velocities mean the solution of the last Stokes solve, and no solve has run on this context");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_TRY(need_vecs(ctx, given ? 3 : 14));
    *vel = svec(ctx, given ? 0 : 11).vel();
    const double* in[3] = {vz, vx, vy};
    for (int q = 0; given && q < 3; q++) { double* d = (*vel)[q]; P3_TRY(upload3(ctx, in[q], 1, &d)); }
    return 0;
}
#define STRAIN3_WHAT "the strain-rate, stress and dissipation fields run"
extern "C" int pl3_stokes_strain_fields(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double* strainrate, double* stress,
                                        double* dissipation, double* total) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_strain_fields: NULL context");
    Vec3 vel;
    P3_TRY(post_vel3(ctx, "pl3_stokes_strain_fields", STRAIN3_WHAT, vz, vx, vy, &vel));
    P3_TRY(strain_run3(ctx, vel, nullptr, total));
    double* host[3] = {strainrate, stress, dissipation};
    for (int q = 0; q < 3; q++) if (host[q]) { double* d = strain_out3(ctx)[q]; P3_TRY(download3(ctx, &d, 1, host[q])); }
    return 0;
}
// the same for the resident solution, for pl_step3.hip: nothing but the total crosses the bus
int pl3i_strain_fields_dev(pl3_ctx* ctx, double* Hplain, double* total) {
    Vec3 vel;
    P3_TRY(post_vel3(ctx, "pl3_resident_step", STRAIN3_WHAT, nullptr, nullptr, nullptr, &vel));
    return strain_run3(ctx, vel, Hplain, total);
}

// ---- yield stress: effective viscosities from the strain rates of a velocity field (pl3_stokes_set_yield / pl3_stokes_yield_update;
// include/pylamp_hip.h, DESIGN.md 6c "Yield stress") -------------------------------------------------------------------------------------
// k3_strain_ce (unchanged) leaves the cell sums and the edge squares in work vector 1; k3_yield_visc then handles, per thread, the eta_s of
// its node and the eta_n of the cell whose lowest corner the node is: eta_eff = min(eta_mat, max(tau_y / (2 e), eta_floor)) from the
// MATERIAL arrays, written over the previous effective ones (a thread reads and writes its own two entries only).  Its epilogue reduces
// nine quantities per workgroup (r3_block, pl_reduce3.h) into ypart, which k_r3_finish combines in a fixed order: no atomics, a call
// repeats bit for bit.
enum { YQ_MIN_S = 0, YQ_NAN_S, YQ_MIN_N, YQ_NAN_N, YQ_CHANGE, YQ_YIELD_S, YQ_YIELD_N, YQ_MAX_ES, YQ_MAX_EC, YQ_N };
using YieldOps = R3Ops<R3_MIN, R3_MAX, R3_MIN, R3_MAX, R3_MAX, R3_SUM, R3_SUM, R3_MAX, R3_MAX>;       // (the two sums are counts)
// ms / mn: material viscosities; es / en: effective ones (in: the previous, out: the new); tau: tau_y at the nodes z_i, then at the cell
// mid-points; floor: eta_floor
struct Yield3 { const double* ms; const double* mn; double* es; double* en; const double* tau; double floor; };
__device__ inline double yield_eta3(double mat, double tau, double e, double floor) {
    double lim = tau / (2.0 * e);                   // e = 0: +inf, the material value stands
    lim = lim > floor ? lim : floor;
    return lim < mat ? lim : mat;
}
__global__ __launch_bounds__(256) void k3_yield_visc(Op3 op, V4 ce, Yield3 y, double* __restrict__ part) {
    const G3& g = op.g;                             // one rank: local and global indices coincide
    const int k = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y, i = blockIdx.z;
    double acc[YQ_N] = {INFINITY, 0.0, INFINITY, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // (every maximum is of figures >= 0)
    if (k < g.n[2] && j < g.n[1]) {                 // (no early return: every thread takes part in the reduction)
        const long long c = i3(g, i, j, k);
        double Y, T, P;
        node_sums3(op, ce, c, i, j, k, Y, T, P);
        const double e_s = sqrt(0.5 * Y);           // the strainrate field of k3_strain_node, bit for bit
        const double mat_s = y.ms[c], prev_s = y.es[c];
        const double new_s = yield_eta3(mat_s, y.tau[i], e_s, y.floor);
        y.es[c] = new_s;
        double mat_n = y.mn[c], prev_n = y.en[c], new_n = mat_n, e_c = 0.0;       // beyond the cells eta_n keeps the material value
        if (i < g.n[0] - 1 && j < g.n[1] - 1 && k < g.n[2] - 1) {
            double a = ce.p[0][c];
#pragma unroll
            for (int p = 0; p < 3; p++) {           // pair p = (D, E): the four edges at the nodes i_D, i_D + 1 x i_E, i_E + 1 of cell i_F
                const long long sD = g.s[p], sE = g.s[(p + 1) % 3];
                const double* __restrict__ q = ce.p[1 + p];
                const double m = 0.25 * (((q[c] + q[c + sE]) + q[c + sD]) + q[c + sD + sE]);
                a += 2.0 * m;
            }
            e_c = sqrt(0.5 * a);
            new_n = yield_eta3(mat_n, y.tau[g.n[0] + i], e_c, y.floor);
        }
        y.en[c] = new_n;
        if (new_s != new_s) acc[YQ_NAN_S] = 1.0; else acc[YQ_MIN_S] = new_s;
        if (new_n != new_n) acc[YQ_NAN_N] = 1.0; else acc[YQ_MIN_N] = new_n;
        acc[YQ_CHANGE] = fmax(fabs(log(new_s / prev_s)), fabs(log(new_n / prev_n)));
        acc[YQ_YIELD_S] = new_s < mat_s ? 1.0 : 0.0;
        acc[YQ_YIELD_N] = new_n < mat_n ? 1.0 : 0.0;
        acc[YQ_MAX_ES] = e_s; acc[YQ_MAX_EC] = e_c;
    }
    r3_block<YieldOps>(acc, 64 * threadIdx.y + threadIdx.x, (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x, part);
}
// Two launches of k_r3_finish combine the partials: YQ_GROUPS workgroups over the kernel's, one over theirs (one workgroup alone walks
// 83 525 partials at 257^3 in 0.86 ms, longer than the kernel that wrote them).
#define YQ_GROUPS 128
static int yield_free3(pl3_ctx* ctx) {
    for (double** q : {&ctx->ms, &ctx->mn, &ctx->ytau, &ctx->ypart}) { if (*q) (void)hipFree(*q); *q = nullptr; }
    return 0;
}
// the effective viscosities become the material ones again, and the operator theirs
static int yield_reset3(pl3_ctx* ctx) {
    if (!ctx->yield_on || !ctx->op_ready) return 0;
    const size_t bytes = (size_t)ctx->geom.d.vol * sizeof(double);
    P3_HIP(ctx, hipMemcpyAsync(ctx->es, ctx->ms, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    P3_HIP(ctx, hipMemcpyAsync(ctx->en, ctx->mn, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    stokes_reop3(ctx, ctx->mat_mineta);
    return 0;
}
extern "C" int pl3_stokes_set_yield(pl3_ctx* ctx, int on, double tau0, double dtau_dz, double eta_floor) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_set_yield: NULL context");
    if (on) {
        if (ctx->nranks > 1 || ctx->comm) return p3_fail(ctx, "pl3_stokes_set_yield: the yield stress runs on one rank (this context has pl3_set_comm attached)");
        if (!std::isfinite(tau0) || !std::isfinite(dtau_dz) || !std::isfinite(eta_floor))
            return p3_fail(ctx, "pl3_stokes_set_yield: tau0 = " + num_str3(tau0) + ", dtau_dz = " + num_str3(dtau_dz) + ", eta_floor = " + num_str3(eta_floor) + " must all be finite");
        const double depth = ctx->gcoord[0].back() - ctx->gcoord[0].front(), low = tau0 + dtau_dz * depth;
        if (!(tau0 > 0.0) || !(low > 0.0))
            return p3_fail(ctx, "pl3_stokes_set_yield: the yield stress tau_y = tau0 + dtau_dz (z - z[0]) must be positive throughout the box, got " + num_str3(tau0) +
                                    " at z[0] and " + num_str3(low) + " at z[n - 1]");
        if (!(eta_floor > 0.0)) return p3_fail(ctx, "pl3_stokes_set_yield: eta_floor = " + num_str3(eta_floor) + " must be positive");
    }
    if ((on != 0) == ctx->yield_on && (!on || (tau0 == ctx->ytau0 && dtau_dz == ctx->ydtau && eta_floor == ctx->yfloor))) return 0;
    P3_HIP(ctx, hipSetDevice(ctx->device));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    history_clear3(ctx);                            // solutions of another rheology are no start for this one
    P3_TRY(yield_reset3(ctx));
    if (!on) {
        P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->yield_on = false; ctx->ytau0 = ctx->ydtau = ctx->yfloor = 0.0;
        return yield_free3(ctx);
    }
    const G3& g = ctx->geom.d;
    const int nz = g.gn[0];
    if (!ctx->ms) {
        const dim3 gr = grid3(g);
        int rc = dmal(ctx, &ctx->ms, g.vol) || dmal(ctx, &ctx->mn, g.vol) || dmal(ctx, &ctx->ytau, 2 * nz) ||
                 dmal(ctx, &ctx->ypart, (long long)YQ_N * ((long long)gr.x * gr.y * gr.z + YQ_GROUPS));
        if (rc) { const std::string m = ctx->err; yield_free3(ctx); return p3_fail(ctx, "pl3_stokes_set_yield: " + m); }
        if (ctx->op_ready) {                        // the coefficients set so far are the material ones
            P3_HIP(ctx, hipMemcpyAsync(ctx->ms, ctx->es, (size_t)g.vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
            P3_HIP(ctx, hipMemcpyAsync(ctx->mn, ctx->en, (size_t)g.vol * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
        }
    }
    const std::vector<double>& z = ctx->gcoord[0];
    std::vector<double> tau(2 * (size_t)nz, 0.0);
    for (int i = 0; i < nz; i++) tau[i] = tau0 + dtau_dz * (z[i] - z[0]);
    for (int i = 0; i + 1 < nz; i++) tau[nz + i] = tau0 + dtau_dz * ((z[i + 1] + z[i]) / 2 - z[0]);
    pl3_count_copy(ctx, tau.size() * sizeof(double));
    P3_HIP(ctx, hipMemcpyAsync(ctx->ytau, tau.data(), tau.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->yield_on = true; ctx->ytau0 = tau0; ctx->ydtau = dtau_dz; ctx->yfloor = eta_floor;
    return 0;
}
extern "C" int pl3_stokes_get_yield(pl3_ctx* ctx, int* on, double* tau0, double* dtau_dz, double* eta_floor) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_get_yield: NULL context");
    if (on) *on = ctx->yield_on ? 1 : 0;
    if (tau0) *tau0 = ctx->ytau0;
    if (dtau_dz) *dtau_dz = ctx->ydtau;
    if (eta_floor) *eta_floor = ctx->yfloor;
    return 0;
}
// which = 0: the effective viscosities the operator holds; 1: the material ones (the same arrays unless a yield stress is set)
extern "C" int pl3_stokes_get_coeffs(pl3_ctx* ctx, int which, double* etas, double* etan) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_get_coeffs: NULL context");
    if (which != 0 && which != 1) return p3_fail(ctx, "pl3_stokes_get_coeffs: which = " + std::to_string(which) + " must be 0 (effective) or 1 (material)");
    if (!ctx->op_ready) return p3_fail(ctx, "pl3_stokes_get_coeffs: no Stokes coefficients set (pl3_stokes_set_coeffs)");
    P3_HIP(ctx, hipSetDevice(ctx->device));
    double* src[2] = {which && ctx->yield_on ? ctx->ms : ctx->es, which && ctx->yield_on ? ctx->mn : ctx->en};
    if (etas) P3_TRY(download3(ctx, &src[0], 1, etas));
    if (etan) P3_TRY(download3(ctx, &src[1], 1, etan));
    return 0;
}
// the update for the velocities vel (three ringed arrays; not work vector 1): out = min eta_eff, change, yielded nodes, yielded cells,
// max e_n, max e_c.  A change other than exactly 0 rebuilds the operator from the new coefficients (stokes_op3; the next solve rebuilds
// the hierarchy) and, since the pressure unknown is scaled by Kcont, keeps the resident solution the same physical pressure.
static int yield_run3(pl3_ctx* ctx, const Vec3& vel, double out[6]) {
    const G3& g = ctx->geom.d;
    const Vec3 ce = svec(ctx, 1);
    const dim3 gr = grid3(g);
    launch3(ctx, g, k3_strain_ce, ctx->op, cv3(vel), ctx->wallvel, wv4(ce));
    launch3(ctx, g, k3_yield_visc, ctx->op, cv4(ce), Yield3{ctx->ms, ctx->mn, ctx->es, ctx->en, ctx->ytau, ctx->yfloor}, ctx->ypart);
    const long long nb = (long long)gr.x * gr.y * gr.z, chunk = (nb + YQ_GROUPS - 1) / YQ_GROUPS;
    double* groups = ctx->ypart + YQ_N * nb;           // the YQ_GROUPS partials of the first finishing launch
    hipLaunchKernelGGL(k_r3_finish<YieldOps>, dim3(YQ_GROUPS), dim3(256), 0, ctx->stream, nb, chunk, (const double*)ctx->ypart, groups);
    hipLaunchKernelGGL(k_r3_finish<YieldOps>, dim3(1), dim3(256), 0, ctx->stream, (long long)YQ_GROUPS, (long long)YQ_GROUPS, (const double*)groups, ctx->part);
    P3_HIP(ctx, hipGetLastError());
    pl3_count_copy(ctx, YQ_N * sizeof(double));
    P3_HIP(ctx, hipMemcpyAsync(ctx->hpart, ctx->part, YQ_N * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    P3_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double* r = ctx->hpart;
    const double mineta = nan_min3(r[YQ_MIN_S], r[YQ_MIN_N], r[YQ_NAN_S] > 0.0, r[YQ_NAN_N] > 0.0);
    // (the three maxima are of figures >= 0 and the fmax of the reduction drops a NaN: 0, not the unit -inf, where every entry is a NaN)
    out[0] = mineta; out[1] = fmax(r[YQ_CHANGE], 0.0); out[2] = r[YQ_YIELD_S]; out[3] = r[YQ_YIELD_N];
    out[4] = fmax(r[YQ_MAX_ES], 0.0); out[5] = fmax(r[YQ_MAX_EC], 0.0);
    if (out[1] != 0.0) {
        const double kc_old = ctx->op.Kc;
        stokes_reop3(ctx, mineta);
        if (ctx->have_x && ctx->vec[11] && ctx->op.Kc != kc_old && std::isfinite(kc_old / ctx->op.Kc)) {
            const Vec3 P = svec(ctx, 11).prs();
            axpby3(ctx, P, kc_old / ctx->op.Kc, P, 0.0, P);
            P3_HIP(ctx, hipGetLastError());
        }
    }
    return 0;
}
// who's velocities (post_vel3) on a context with a yield stress set
static int yield_vel3(pl3_ctx* ctx, const char* who, const double* vz, const double* vx, const double* vy, Vec3* vel) {
    P3_TRY(post_vel3(ctx, who, "the yield stress runs", vz, vx, vy, vel));
    if (!ctx->yield_on) return p3_fail(ctx, std::string(who) + ": no yield stress set (pl3_stokes_set_yield)");
    return 0;
}
extern "C" int pl3_stokes_yield_update(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double out[6]) {
    if (!ctx) return p3_fail(nullptr, "pl3_stokes_yield_update: NULL context");
    Vec3 vel;
    P3_TRY(yield_vel3(ctx, "pl3_stokes_yield_update", vz, vx, vy, &vel));
    double o[6];
    P3_TRY(yield_run3(ctx, vel, o));
    if (out) for (int q = 0; q < 6; q++) out[q] = o[q];
    return 0;
}
// the same for the resident solution, for pl_step3.hip
int pl3i_yield_update_dev(pl3_ctx* ctx, double out[6]) {
    Vec3 vel;
    P3_TRY(yield_vel3(ctx, "pl3_resident_step", nullptr, nullptr, nullptr, &vel));
    return yield_run3(ctx, vel, out);
}

// ---- what the device-resident step (pl_step3.hip) needs of a context ----------------------------------------------------------
int pl3i_dev_view(pl3_ctx* ctx, Pl3DevView* v) {
    P3_HIP(ctx, hipSetDevice(ctx->device));
    const bool kept = ctx->strain_kept;                 // (looking at the context does not touch the work vectors)
    P3_TRY(need_vecs(ctx, 14));
    ctx->strain_kept = kept;
    for (int q = 0; q < 3; q++) v->strain[q] = strain_out3(ctx)[q];
    v->have_strain = kept;
    P3_TRY(need_hvecs(ctx));
    const G3& g = ctx->geom.d;
    v->s0 = g.s[0]; v->s1 = g.s[1]; v->pad = P3_PAD; v->stream = ctx->stream; v->slot = &ctx->step3;
    for (int q = 0; q < 4; q++) { v->X[q] = svec(ctx, 11)[q]; v->scratch[q] = svec(ctx, 0)[q]; }
    v->T = ctx->hvec[11]; v->have_x = ctx->have_x; v->have_T = ctx->have_T; v->noslip = ctx->noslip; v->wallvel = ctx->wallvel;
    v->wallflow = ctx->wallflow;
    v->eta_eff[0] = ctx->es; v->eta_eff[1] = ctx->en; v->yield_on = ctx->yield_on;
    return 0;
}
// counts and bytes of the host <-> device copies of this context's pl3_* calls since the last reset: out = { copies of at least one
// node field (8 nz nx ny bytes), their bytes, smaller copies, their bytes }
extern "C" int pl3_transfer_stats(pl3_ctx* ctx, int64_t out[4], int reset) {
    if (!ctx) return p3_fail(nullptr, "pl3_transfer_stats: NULL context");
    if (out) for (int q = 0; q < 4; q++) out[q] = ctx->xfer[q];
    if (reset) for (int q = 0; q < 4; q++) ctx->xfer[q] = 0;
    return 0;
}
