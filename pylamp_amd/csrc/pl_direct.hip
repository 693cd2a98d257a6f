// Direct solve of the Stokes system on one GPU: banded LU with partial pivoting of the row-scaled operator, used as an
// (exact) preconditioner of the same BiCGStab -- beyond the viscosity-contrast gate up front, elsewhere when the
// multigrid-preconditioned iteration does not converge -- followed by refinement with a compensated (double-double)
// residual of the UNSCALED operator (pl_solver.hip).  The cases it exists for: the reference's stock model (sphere 1e12 in
// 1e2), on which no smoother-based preconditioner reaches the accurate solution, and the reference's free-surface
// stabilisation with the reference's own sign (pylamp_stokes.py:422-426,483-487), which makes the velocity block indefinite
// at the Courant time step -- while the reference itself solves with SuperLU (pylamp2.py:394).
//
// The band is assembled from the matrix-free operator by 27-colour probing (every row reaches nodes within +-1 in i and j),
// (vz, vx, P) per node, nodes numbered ACROSS THE NARROW AXIS: bandwidth 3 (min(nz, nx) + 1) + 2, so a 201 x 4001 box costs
// what a 4001 x 201 one does.  The factorisation is right-looking and blocked (panels of NB columns, LAPACK band layout with
// kl extra rows for the fill-in of pivoting, the unpermuted-L form of dgbtrf/dgbtrs): ONE launch per panel -- every
// workgroup applies the panel's row interchanges, U12 = L11^-1 A12 and the trailing update A22 -= L21 U12 to its own
// NB-column slice of the trailing band in LDS, and the workgroup of the first slice then factors the next panel, which it
// already holds.  The triangular solves run in one workgroup each, NB rows at a time with the window of the right-hand side
// in LDS.  The device memory budget decides where the LU is possible (pl_direct_fits).
#include "pl_internal.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>

struct PlDirect {
    int n = 0, kl = 0, ku = 0, ld = 0, nb = 0, tr = 0, wr = 0;   // wr: LDS ring rows of the triangular solves
    double* ab = nullptr;        // LAPACK band storage with kl extra rows for the fill-in of pivoting: (i,j) at kl+ku+i-j + j*ld
    int* piv = nullptr;
    double* work = nullptr;      // n doubles
    double* probe = nullptr;     // 6 planes: indicator x, y = A x
    double* coef = nullptr;      // 81 planes: the unscaled operator's 27 entries of every row, as probing sees them
    int* info = nullptr;
    size_t lds_fac = 0, lds_fwd = 0, lds_bwd = 0;
    double factor_ms = 0.0, solve_ms = 0.0;
    int nsolve = 0;
};

static constexpr int KD_T = 256;   // threads of the LU and triangular-solve workgroups

__host__ __device__ inline long long kd_node(const PlGeom& g, int tr, int i, int j) {
    return tr ? (long long)j * g.nz + i : (long long)i * g.nx + j;
}

__global__ __launch_bounds__(256) void kd_indicator(PlGeom g, int ci, int cj, int q, double* __restrict__ x) {
    const int lj = blockIdx.x * 64 + threadIdx.x, li = blockIdx.y * 4 + threadIdx.y;
    if (lj >= g.lnx || li >= g.lnz) return;
    const long long c = pl_idx(g, li, lj);
    for (int p = 0; p < 3; p++) x[c + p * g.plane] = (p == q && li % 3 == ci && lj % 3 == cj) ? 1.0 : 0.0;
}
// the probed node within +-1 of (i, j) for colour (ci, cj)
__device__ inline void kd_probed(int i, int j, int ci, int cj, int& pi, int& pj) {
    pi = i + ((ci - i % 3 + 1 + 3) % 3 - 1); pj = j + ((cj - j % 3 + 1 + 3) % 3 - 1);
}
__global__ __launch_bounds__(256) void kd_scatter_band(PlGeom g, int tr, int ci, int cj, int q, const double* __restrict__ y, int kl, int ku, int ld,
                                                       double* __restrict__ ab) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= g.lnx || i >= g.lnz) return;
    const long long c = pl_idx(g, i, j);
    int pi, pj; kd_probed(i, j, ci, cj, pi, pj);
    if (pi < 0 || pi >= g.nz || pj < 0 || pj >= g.nx) return;
    const long long col = kd_node(g, tr, pi, pj) * 3 + q;
    for (int r = 0; r < 3; r++) {
        const double v = y[c + r * g.plane];
        if (v == 0.0) continue;
        const long long row = kd_node(g, tr, i, j) * 3 + r;
        ab[kl + ku + row - col + col * ld] = v;
    }
}
// coef plane ((di+1)*3 + (dj+1))*9 + q*3 + r: entry of row (i, j, r) at column (i+di, j+dj, q); 0 outside the domain
__global__ __launch_bounds__(256) void kd_scatter_coef(PlGeom g, int ci, int cj, int q, const double* __restrict__ y, double* __restrict__ coef) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= g.lnx || i >= g.lnz) return;
    const long long c = pl_idx(g, i, j);
    int pi, pj; kd_probed(i, j, ci, cj, pi, pj);
    const bool in = pi >= 0 && pi < g.nz && pj >= 0 && pj < g.nx;
    const int k = ((pi - i + 1) * 3 + (pj - j + 1)) * 9 + q * 3;
    for (int r = 0; r < 3; r++) coef[c + (k + r) * g.plane] = in ? y[c + r * g.plane] : 0.0;
}

// ---- double-double arithmetic (TwoSum, TwoProd with fma) ---------------------------------------------------------------
// (no contraction: a * b + c fused into one fma would break the error-free transformations)
struct kd_dd { double hi, lo; };
__device__ inline kd_dd kd_two_sum(double a, double b) {
#pragma clang fp contract(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ inline void kd_dd_add_prod(kd_dd& acc, double a, double b) {      // acc += a b, exactly up to the final rounding of lo
#pragma clang fp contract(off)
    const double p = a * b, e = fma(a, b, -p);
    const kd_dd s = kd_two_sum(acc.hi, p);
    const double lo = acc.lo + e + s.lo;
    const kd_dd t = kd_two_sum(s.hi, lo);
    acc.hi = t.hi; acc.lo = t.lo;
}
// r = b - A x of the UNSCALED operator in double-double (rounded once at the end), from the probed entries
__global__ __launch_bounds__(256) void kd_residual_dd(PlGeom g, const double* __restrict__ coef, const double* __restrict__ b,
                                                      const double* __restrict__ x, double* __restrict__ r) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= g.lnx || i >= g.lnz) return;
    const long long c = pl_idx(g, i, j);
    kd_dd acc[3];
    for (int q = 0; q < 3; q++) acc[q] = {b[c + q * g.plane], 0.0};
    for (int di = -1; di <= 1; di++) {
        if (i + di < 0 || i + di >= g.nz) continue;
        for (int dj = -1; dj <= 1; dj++) {
            if (j + dj < 0 || j + dj >= g.nx) continue;
            const long long cn = pl_idx(g, i + di, j + dj);
            const int k = ((di + 1) * 3 + (dj + 1)) * 9;
            for (int q = 0; q < 3; q++) {
                const double xv = x[cn + q * g.plane];
                for (int rr = 0; rr < 3; rr++) kd_dd_add_prod(acc[rr], -coef[c + (k + q * 3 + rr) * g.plane], xv);
            }
        }
    }
    for (int q = 0; q < 3; q++) r[c + q * g.plane] = acc[q].hi + acc[q].lo;
}

// ---- blocked band LU -----------------------------------------------------------------------------------------------------
// workgroup barrier that orders LDS only (a __syncthreads would also wait for every outstanding global store)
__device__ inline void kd_lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// Panel [k0, k1) of width nbk <= NB in LDS, column-major with PR rows (local row = global row - k0): factor it in place
// (dgbtf2 on the panel: pivot search as a workgroup reduction, interchanges over the panel columns to the right of the pivot
// column, multipliers, rank-1 update), record the pivots in spiv (global row indices) and piv.
__device__ void kd_factor_panel(double* __restrict__ P, int PR, int k0, int nbk, int n, int kl, int* __restrict__ spiv,
                                int* __restrict__ piv, int* __restrict__ info, double* __restrict__ sred, int* __restrict__ sidx) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int jj = 0; jj < nbk; jj++) {
        const int j = k0 + jj, km = min(kl, n - 1 - j);
        const double* col = P + (long long)jj * PR + jj;
        double best = -1.0; int bi = 0;
        for (int d = tid; d <= km; d += KD_T) { const double a = fabs(col[d]); if (a > best) { best = a; bi = d; } }
        for (int o = 32; o > 0; o >>= 1) {
            const double ob = __shfl_xor(best, o); const int oi = __shfl_xor(bi, o);
            if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
        }
        if (lane == 0) { sred[wave] = best; sidx[wave] = bi; }
        kd_lds_barrier();
        best = sred[0]; bi = sidx[0];
        for (int w = 1; w < KD_T / 64; w++) if (sred[w] > best || (sred[w] == best && sidx[w] < bi)) { best = sred[w]; bi = sidx[w]; }
        if (tid == 0) {
            spiv[jj] = j + bi;
            if (!(best > 0.0) && *info == 0) *info = j + 1;
        }
        if (bi != 0)
            for (int cc = jj + tid; cc < nbk; cc += KD_T) {
                double* a = P + (long long)cc * PR + jj;
                const double t = a[0]; a[0] = a[bi]; a[bi] = t;
            }
        kd_lds_barrier();
        const double pv = col[0];
        if (pv != 0.0)
            for (int d = 1 + tid; d <= km; d += KD_T) {
                const double m = col[d] / pv;
                P[(long long)jj * PR + jj + d] = m;
                for (int c0 = jj + 1; c0 < nbk; c0 += 8) {      // 8 columns at a time: the LDS reads in flight together
                    double v[8], u[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int cc = min(c0 + q, nbk - 1);
                        v[q] = P[(long long)cc * PR + jj + d]; u[q] = P[(long long)cc * PR + jj];
                    }
#pragma unroll
                    for (int q = 0; q < 8; q++) if (c0 + q < nbk) P[(long long)(c0 + q) * PR + jj + d] = v[q] - m * u[q];
                }
            }
        kd_lds_barrier();
    }
    if (tid < nbk) piv[k0 + tid] = spiv[tid];
}
__device__ inline bool kd_in_band(int i, int c, int kl, int kv) { return i - c <= kl && c - i <= kv; }
// dst[t] = f(t), t in [0, total), by the KD_T threads of the workgroup with 16 loads in flight per thread (the band streams
// from HBM: a loop that waits for each load before storing it to LDS runs at one memory latency per element)
template <class F> __device__ inline void kd_gather(double* __restrict__ dst, int total, F f) {
    for (int t0 = threadIdx.x; t0 < total; t0 += 16 * KD_T) {
        double v[16];
#pragma unroll
        for (int u = 0; u < 16; u++) { const int t = t0 + u * KD_T; v[u] = t < total ? f(t) : 0.0; }
#pragma unroll
        for (int u = 0; u < 16; u++) { const int t = t0 + u * KD_T; if (t < total) dst[t] = v[u]; }
    }
}

// first panel [0, NB): load, factor, store (one workgroup)
__global__ __launch_bounds__(KD_T) void kd_lu_first(int n, int kl, int ku, int ld, int NB, double* __restrict__ ab, int* __restrict__ piv,
                                                     int* __restrict__ info) {
    extern __shared__ double kd_smem[];
    __shared__ double sred[KD_T / 64]; __shared__ int sidx[KD_T / 64]; __shared__ int spiv[64];
    const int kv = kl + ku, PR = NB + kl, k1 = min(NB, n), rows = min(n, k1 + kl);
    double* P = kd_smem;
    kd_gather(P, k1 * PR, [&](int t) {
        const int s = t / PR, i = t % PR;
        return (i < rows && kd_in_band(i, s, kl, kv)) ? ab[kv + i - s + (long long)s * ld] : 0.0;
    });
    kd_lds_barrier();
    kd_factor_panel(P, PR, 0, k1, n, kl, spiv, piv, info, sred, sidx);
    for (int t = threadIdx.x; t < k1 * PR; t += KD_T) {
        const int s = t / PR, i = t % PR;
        if (i < rows && kd_in_band(i, s, kl, kv)) ab[kv + i - s + (long long)s * ld] = P[t];
    }
}

// One panel step.  Panel [k0, k1) is factored (L in the band, pivots in piv).  Workgroup b owns the trailing columns
// [k1 + b NB, k1 + (b+1) NB) up to column k1 - 1 + kl + ku (the last one a row of the panel reaches): it loads their rows
// [k0, k1 + kl) into LDS, runs the panel's interchanges and eliminations on the rows they touch (U12 and the pivot rows
// below), A22 -= L21 U12 on the others, and stores them.  Workgroup 0's slice is the next panel: it factors it from LDS.
__global__ __launch_bounds__(KD_T) void kd_lu_step(int n, int kl, int ku, int ld, int NB, int k0, double* __restrict__ ab,
                                                    int* __restrict__ piv, int* __restrict__ info) {
    extern __shared__ double kd_smem[];
    __shared__ double sred[KD_T / 64]; __shared__ int sidx[KD_T / 64]; __shared__ int spiv[64];
    const int tid = threadIdx.x, kv = kl + ku, PR = NB + kl;
    const int k1 = min(k0 + NB, n), nbk = k1 - k0, r1 = min(n, k1 + kl), prk = r1 - k0;
    const int cmax = min(n - 1, k1 - 1 + kv), c0 = k1 + blockIdx.x * NB, ncw = min(cmax + 1, c0 + NB) - c0;
    if (ncw <= 0) return;
    double* Lp = kd_smem;                       // panel k: PR x NB
    double* T = kd_smem + (long long)PR * NB;    // own slice: PR x NB
    kd_gather(Lp, nbk * PR, [&](int t) {
        const int s = t / PR, il = t % PR, i = k0 + il, c = k0 + s;
        return (il < prk && i > c && i - c <= kl) ? ab[kv + i - c + (long long)c * ld] : 0.0;
    });
    kd_gather(T, NB * PR, [&](int t) {
        const int s = t / PR, il = t % PR, i = k0 + il, c = c0 + s;
        return (s < ncw && il < prk && kd_in_band(i, c, kl, kv)) ? ab[kv + i - c + (long long)c * ld] : 0.0;
    });
    // Rows the panel's interchanges touch: its own nbk rows and the rows below it that became pivots ("active" rows, at most
    // 2 NB).  Their values follow the interchange-and-eliminate sequence of dgbtf2 exactly (the unpermuted-L form does not
    // allow all interchanges first); every other row of the slice only takes the trailing update A22 -= L21 U12.
    int* amap = (int*)(kd_smem + 2LL * PR * NB);   // local row -> active index, -1: not active
    __shared__ int act[64]; __shared__ int spos[64]; __shared__ int snact;
    for (int t = tid; t < PR; t += KD_T) amap[t] = -1;
    if (tid < nbk) spiv[tid] = piv[k0 + tid] - k0;
    kd_lds_barrier();
    if (tid == 0) {
        int na = nbk;
        for (int s = 0; s < nbk; s++) {
            const int p = spiv[s];
            if (p < nbk) spos[s] = p;
            else { if (amap[p] < 0) { amap[p] = na; act[na] = p; na++; } spos[s] = amap[p]; }
        }
        snact = na;
    }
    kd_lds_barrier();
    {                                           // one wave per column, one lane per active row
        const int nact = snact, lane = tid & 63;
        const int ra = lane < nbk ? lane : (lane < nact ? act[lane] : 0);
        for (int cc = tid >> 6; cc < ncw; cc += 2 * (KD_T / 64)) {       // two columns per pass: two independent chains
            const int cc2 = cc + KD_T / 64;
            double* tc = T + (long long)cc * PR;
            double* tc2 = T + (long long)min(cc2, ncw - 1) * PR;
            double v = lane < nact ? tc[ra] : 0.0, v2 = lane < nact ? tc2[ra] : 0.0;
            for (int s = 0; s < nbk; s++) {
                const int ps = spos[s];
                const double a = __shfl(v, s), b = __shfl(v, ps), a2 = __shfl(v2, s), b2 = __shfl(v2, ps);
                if (lane == s) { v = b; v2 = b2; }
                else if (lane == ps) { v = a; v2 = a2; }
                const int km = min(kl, n - 1 - (k0 + s));
                if (lane < nact && ra > s && ra - s <= km) { const double l = Lp[(long long)s * PR + ra]; v -= l * b; v2 -= l * b2; }
            }
            if (lane < nact) { tc[ra] = v; if (cc2 < ncw) tc2[ra] = v2; }
        }
    }
    kd_lds_barrier();
    {                                           // A22 -= L21 U12 on the rows [k1, r1) that are not active: 4 x 4 per thread
        const int nr = prk - nbk, lane = tid & 63, wave = tid >> 6;
        for (int r0 = lane; r0 < nr; r0 += 256)
            for (int c0 = 4 * wave; c0 < ncw; c0 += 4 * (KD_T / 64)) {
                double acc[4][4] = {};
                for (int s = 0; s < nbk; s++) {
                    double l[4], u[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) { const int r = r0 + 64 * i; l[i] = r < nr ? Lp[(long long)s * PR + nbk + r] : 0.0; }
#pragma unroll
                    for (int k = 0; k < 4; k++) u[k] = c0 + k < ncw ? T[(long long)(c0 + k) * PR + s] : 0.0;
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int k = 0; k < 4; k++) acc[i][k] = fma(l[i], u[k], acc[i][k]);
                }
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int rl = nbk + r0 + 64 * i;
                    if (r0 + 64 * i >= nr || amap[rl] >= 0) continue;
#pragma unroll
                    for (int k = 0; k < 4; k++) if (c0 + k < ncw) T[(long long)(c0 + k) * PR + rl] -= acc[i][k];
                }
            }
    }
    kd_lds_barrier();
    const bool next = blockIdx.x == 0;          // slice 0 = the next panel [k1, k1 + ncw)
    if (!next) {
        for (int t = tid; t < ncw * PR; t += KD_T) {
            const int s = t / PR, il = t % PR, i = k0 + il, c = c0 + s;
            if (il < prk && kd_in_band(i, c, kl, kv)) ab[kv + i - c + (long long)c * ld] = T[t];
        }
        return;
    }
    // the U12 rows of the next panel's columns are final
    for (int t = tid; t < ncw * nbk; t += KD_T) {
        const int s = t / nbk, il = t % nbk, i = k0 + il, c = c0 + s;
        if (kd_in_band(i, c, kl, kv)) ab[kv + i - c + (long long)c * ld] = T[(long long)s * PR + il];
    }
    // next panel [k1, k1 + ncw), rows [k1, min(n, k1 + ncw + kl)): rows below r1 from T, the rest untouched in the band
    const int rows2 = min(n, k1 + ncw + kl) - k1;
    kd_gather(Lp, ncw * PR, [&](int t) {
        const int s = t / PR, il = t % PR, i = k1 + il, c = k1 + s;
        double v = 0.0;
        if (il < rows2 && kd_in_band(i, c, kl, kv)) v = (i < r1) ? T[(long long)s * PR + (i - k0)] : ab[kv + i - c + (long long)c * ld];
        return v;
    });
    kd_lds_barrier();
    kd_factor_panel(Lp, PR, k1, ncw, n, kl, spiv, piv, info, sred, sidx);
    for (int t = tid; t < ncw * PR; t += KD_T) {
        const int s = t / PR, il = t % PR, i = k1 + il, c = k1 + s;
        if (il < rows2 && kd_in_band(i, c, kl, kv)) ab[kv + i - c + (long long)c * ld] = Lp[t];
    }
}

// ---- triangular solves (one workgroup each, NB rows at a time) ------------------------------------------------------
// The right-hand side lives in an LDS ring of WR >= kl + ku + 2 NB + 1 rows (row i at i & (WR - 1)): a row is loaded once,
// stored once when final, and never read back from global memory, so every workgroup barrier orders LDS only.
//
// L y = P b in the unpermuted form of dgbtrs: for every column j: swap b[j], b[piv[j]]; b[j+1 .. j+kl] -= l_j b[j].
// Per block [k0, k1): the block's multipliers and the NB rows entering the window go to LDS (all waves), wave 0 runs the
// columns (no workgroup barrier inside a block), all waves store the finished rows.
__global__ __launch_bounds__(KD_T) void kd_lu_fwd(int n, int kl, int ku, int ld, int NB, int WR, const double* __restrict__ ab,
                                                   const int* __restrict__ piv, double* __restrict__ b) {
    extern __shared__ double kd_smem[];
    __shared__ int spiv[64];
    const int tid = threadIdx.x, kv = kl + ku, wm = WR - 1;
    double* Lp = kd_smem;                                // NB x (kl + 1): multipliers d = 1..kl of each column
    double* W = kd_smem + (long long)NB * (kl + 1);      // ring of WR rows
    int loaded = 0;                                      // rows [0, loaded) are in the ring
    for (int k0 = 0; k0 < n; k0 += NB) {
        const int k1 = min(k0 + NB, n), nbk = k1 - k0, rend = min(n, k1 + kl);
        kd_gather(Lp, nbk * (kl + 1), [&](int t) {
            const int s = t / (kl + 1), d = t % (kl + 1), c = k0 + s;
            return (d >= 1 && c + d < n) ? ab[kv + d + (long long)c * ld] : 0.0;
        });
        for (int i = loaded + tid; i < rend; i += KD_T) W[i & wm] = b[i];
        loaded = rend;
        if (tid < nbk) spiv[tid] = piv[k0 + tid];
        kd_lds_barrier();
        if (tid < 64) {
            for (int s = 0; s < nbk; s++) {                  // the interchange folded into the update: row p takes b[j]
                const int j = k0 + s, p = spiv[s];
                const double bp = W[p & wm], bs = W[j & wm];
                const int km = min(kl, n - 1 - j);
                const double* l = Lp + (long long)s * (kl + 1);
                for (int d0 = 1; d0 <= km; d0 += 8 * 64) {           // 8 rows per lane at a time: the LDS reads in flight together
                    double w[8], lv[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) { const int d = min(d0 + q * 64 + tid, km); w[q] = W[(j + d) & wm]; lv[q] = l[d]; }
#pragma unroll
                    for (int q = 0; q < 8; q++) {
                        const int r = j + d0 + q * 64 + tid;
                        if (r - j <= km) W[r & wm] = (r == p ? bs : w[q]) - lv[q] * bp;
                    }
                }
                if (tid == 0) W[j & wm] = bp;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
        }
        kd_lds_barrier();
        if (tid < nbk) b[k0 + tid] = W[(k0 + tid) & wm];  // final rows of this block
    }
}
// U x = y (U has kl + ku superdiagonals), blocks from the last: t_r = y_r - sum_{c >= k1} U[r,c] x_c as a workgroup GEMV
// (all waves; x from the LDS ring), then the NB x NB triangle by wave 0.
__global__ __launch_bounds__(KD_T) void kd_lu_bwd(int n, int kl, int ku, int ld, int NB, int WR, const double* __restrict__ ab,
                                                   double* __restrict__ b) {
    extern __shared__ double kd_smem[];
    const int tid = threadIdx.x, kv = kl + ku, wm = WR - 1;
    double* U = kd_smem;                     // nbk x nbk triangle, column-major
    double* part = kd_smem + NB * NB;        // KD_T partial sums
    double* tv = part + KD_T;                // NB
    double* X = tv + NB;                     // ring of WR solution rows
    const int nsl = KD_T / NB;               // column slices of the GEMV
    const int last = ((n - 1) / NB) * NB;
    for (int k0 = last; k0 >= 0; k0 -= NB) {
        const int k1 = min(k0 + NB, n), nbk = k1 - k0;
        kd_gather(U, nbk * nbk, [&](int t) {
            const int s = t / nbk, r = t % nbk;          // column k0 + s, row k0 + r, at U[s nbk + r]
            return (r <= s) ? ab[kv + r - s + (long long)(k0 + s) * ld] : 0.0;
        });
        {
            const int r = tid % NB, sl = tid / NB;
            double acc = 0.0;
            if (r < nbk) {
                const int i = k0 + r, cend = min(n - 1, i + kv);
                for (int c0 = k1 + sl; c0 <= cend; c0 += 16 * nsl) {    // 16 loads in flight
                    double a[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) { const int c = c0 + u * nsl; a[u] = c <= cend ? ab[kv + i - c + (long long)c * ld] : 0.0; }
#pragma unroll
                    for (int u = 0; u < 16; u++) { const int c = c0 + u * nsl; if (c <= cend) acc = fma(a[u], X[c & wm], acc); }
                }
            }
            part[tid] = acc;
        }
        const double yb = tid < nbk ? b[k0 + tid] : 0.0;
        kd_lds_barrier();
        if (tid < 64) {
            double v = yb;
            if (tid < nbk) for (int sl = 0; sl < nsl; sl++) v -= part[sl * NB + tid];
            for (int s = nbk - 1; s >= 0; s--) {
                const double xs = __shfl(v, s) / U[s * nbk + s];
                if (tid == s) v = xs;
                else if (tid < s) v -= U[s * nbk + tid] * xs;
            }
            if (tid < nbk) { b[k0 + tid] = v; X[(k0 + tid) & wm] = v; }
        }
        kd_lds_barrier();
    }
}

// 3 ring planes <-> interleaved vector in the LU's node order
__global__ __launch_bounds__(256) void kd_planes_to_vec(PlGeom g, int tr, const double* __restrict__ p, double* __restrict__ v) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= g.lnx || i >= g.lnz) return;
    const long long c = pl_idx(g, i, j), r = kd_node(g, tr, i, j) * 3;
    v[r] = p[c]; v[r + 1] = p[c + g.plane]; v[r + 2] = p[c + 2 * g.plane];
}
__global__ __launch_bounds__(256) void kd_vec_to_planes(PlGeom g, int tr, const double* __restrict__ v, double* __restrict__ p) {
    const int j = blockIdx.x * 64 + threadIdx.x, i = blockIdx.y * 4 + threadIdx.y;
    if (j >= g.lnx || i >= g.lnz) return;
    const long long c = pl_idx(g, i, j), r = kd_node(g, tr, i, j) * 3;
    p[c] = v[r]; p[c + g.plane] = v[r + 1]; p[c + 2 * g.plane] = v[r + 2];
}

static dim3 grid2d(const PlGeom& g) { return dim3((g.lnx + 63) / 64, (g.lnz + 3) / 4); }

void pl_direct_free(pl_ctx* ctx) {
    PlDirect* D = (PlDirect*)ctx->direct;
    if (!D) return;
    for (void* q : {(void*)D->ab, (void*)D->piv, (void*)D->work, (void*)D->probe, (void*)D->coef, (void*)D->info}) if (q) (void)hipFree(q);
    delete D;
    ctx->direct = nullptr;
}

// band parameters of this context's system: unknowns, sub-diagonals, node order (1: numbered along z, across the narrow axis)
static void band_shape(pl_ctx* ctx, long long* n, int* kl, int* tr) {
    const int m = std::min(ctx->nz, ctx->nx);
    *n = 3LL * ctx->nz * ctx->nx; *kl = 3 * (m + 1) + 2; *tr = ctx->nz < ctx->nx ? 1 : 0;
}
static size_t direct_bytes(pl_ctx* ctx) {
    long long n; int kl, tr; band_shape(ctx, &n, &kl, &tr);
    return (size_t)n * (3 * kl + 1) * sizeof(double) + (size_t)n * (sizeof(int) + sizeof(double)) +
           (size_t)87 * ctx->geom.d.plane * sizeof(double);
}

// The small-system rule of the first direct fallback (band below 60 M doubles): it still decides what a solve keeps for a
// possible fallback -- the hydrostatic start, no reuse of the reference norm -- so that the systems that never take the LU
// run exactly as they did.
bool pl_direct_possible(pl_ctx* ctx) {
    if (ctx->nranks != 1) return false;
    const long long n = 3LL * ctx->nz * ctx->nx, k = 3LL * (ctx->nx + 1) + 2;
    return n * (3 * k + 1) <= 60000000LL;
}

// Can the LU be built at all?  One rank, and the band (plus the probe and residual planes) within the device memory budget:
// PYLAMP_DIRECT_MAX_GB (read on every call), default half of the free device memory (counting what the LU already holds).
// Called only where the LU is considered: beyond the contrast gate, when forced, or after a failed iteration.
bool pl_direct_fits(pl_ctx* ctx) {
    if (ctx->nranks != 1) return false;
    const size_t need = direct_bytes(ctx);
    double budget;
    if (const char* e = getenv("PYLAMP_DIRECT_MAX_GB")) budget = atof(e) * 1e9;
    else {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
        const PlDirect* D = (const PlDirect*)ctx->direct;
        const size_t held = D ? (size_t)D->n * (D->ld + 1) * sizeof(double) + (size_t)87 * ctx->geom.d.plane * sizeof(double) : 0;
        budget = 0.5 * (double)(fr + held);
    }
    return (double)need <= budget;
}

static int direct_alloc(pl_ctx* ctx) {
    const PlGeom& g = ctx->geom.d;
    long long nl; int kl, tr; band_shape(ctx, &nl, &kl, &tr);
    const int n = (int)nl, ku = kl, ld = 2 * kl + ku + 1;
    PlDirect* D = (PlDirect*)ctx->direct;
    if (D && D->n == n && D->kl == kl && D->tr == tr) return 0;
    pl_direct_free(ctx);
    D = new PlDirect();
    ctx->direct = D;
    D->n = n; D->kl = kl; D->ku = ku; D->ld = ld; D->tr = tr;
    // panel width: the largest of 32, 16, 8 whose two LDS tiles (the panel and a slice, (NB + kl) x NB each) fit the device
    int lmax = 65536;
    (void)hipDeviceGetAttribute(&lmax, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device);
    const size_t avail = (size_t)lmax - 1024;
    int nb = 32;
    while (nb > 4 && (size_t)2 * (nb + kl) * nb * sizeof(double) + (size_t)(nb + kl) * sizeof(int) > avail) nb /= 2;
    nb = std::min(nb, kl + ku);
    D->nb = nb;
    D->lds_fac = (size_t)2 * (nb + kl) * nb * sizeof(double) + (size_t)(nb + kl) * sizeof(int);
    D->wr = 1;
    while (D->wr < 2 * kl + 2 * nb + 1) D->wr *= 2;
    D->lds_fwd = ((size_t)nb * (kl + 1) + D->wr) * sizeof(double);
    D->lds_bwd = ((size_t)nb * nb + KD_T + nb + D->wr) * sizeof(double);
    if (D->lds_fac > avail || D->lds_fwd > avail || D->lds_bwd > avail) return pl_fail(ctx, "direct solve: the band is too wide for the LU's LDS tiles");
    PL_HIP(ctx, hipFuncSetAttribute((const void*)kd_lu_first, hipFuncAttributeMaxDynamicSharedMemorySize, (int)D->lds_fac));
    PL_HIP(ctx, hipFuncSetAttribute((const void*)kd_lu_step, hipFuncAttributeMaxDynamicSharedMemorySize, (int)D->lds_fac));
    PL_HIP(ctx, hipFuncSetAttribute((const void*)kd_lu_fwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)D->lds_fwd));
    PL_HIP(ctx, hipFuncSetAttribute((const void*)kd_lu_bwd, hipFuncAttributeMaxDynamicSharedMemorySize, (int)D->lds_bwd));
    PL_HIP(ctx, hipMalloc((void**)&D->ab, (size_t)n * ld * sizeof(double)));
    PL_HIP(ctx, hipMalloc((void**)&D->piv, (size_t)n * sizeof(int)));
    PL_HIP(ctx, hipMalloc((void**)&D->work, (size_t)n * sizeof(double)));
    PL_HIP(ctx, hipMalloc((void**)&D->probe, (size_t)6 * g.plane * sizeof(double)));
    PL_HIP(ctx, hipMalloc((void**)&D->coef, (size_t)81 * g.plane * sizeof(double)));
    PL_HIP(ctx, hipMalloc((void**)&D->info, sizeof(int)));
    return 0;
}

// probe the 27 entries of every row of the UNSCALED operator (the entries A.tocsc() sees) for the compensated residual
static int direct_coef(pl_ctx* ctx, const PlStokesOp& op) {
    const PlGeom& g = ctx->geom.d;
    PlDirect* D = (PlDirect*)ctx->direct;
    PL_HIP(ctx, hipMemsetAsync(D->probe, 0, (size_t)6 * g.plane * sizeof(double), ctx->stream));
    double* x = D->probe; double* y = D->probe + 3 * g.plane;
    for (int ci = 0; ci < 3; ci++)
        for (int cj = 0; cj < 3; cj++)
            for (int q = 0; q < 3; q++) {
                hipLaunchKernelGGL(kd_indicator, grid2d(g), dim3(64, 4), 0, ctx->stream, g, ci, cj, q, x);
                pl_launch_stokes_apply(ctx, op, x, y);
                hipLaunchKernelGGL(kd_scatter_coef, grid2d(g), dim3(64, 4), 0, ctx->stream, g, ci, cj, q, (const double*)y, D->coef);
            }
    PL_HIP(ctx, hipGetLastError());
    return 0;
}

static double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// factorise D_r A (the row-scaled operator the Krylov solver works on); probe the unscaled op for the compensated residual
int pl_direct_factor(pl_ctx* ctx, const PlStokesOp& op_scaled, const PlStokesOp& op) {
    const PlGeom& g = ctx->geom.d;
    if (ctx->nranks != 1) return pl_fail(ctx, "direct solve: one rank only");
    PL_TRY(direct_alloc(ctx));
    PlDirect* D = (PlDirect*)ctx->direct;
    const int n = D->n, kl = D->kl, ku = D->ku, ld = D->ld, nb = D->nb;
    PL_HIP(ctx, hipMemsetAsync(D->ab, 0, (size_t)n * ld * sizeof(double), ctx->stream));
    PL_HIP(ctx, hipMemsetAsync(D->probe, 0, (size_t)6 * g.plane * sizeof(double), ctx->stream));
    PL_HIP(ctx, hipMemsetAsync(D->info, 0, sizeof(int), ctx->stream));
    double* x = D->probe; double* y = D->probe + 3 * g.plane;
    for (int ci = 0; ci < 3; ci++)
        for (int cj = 0; cj < 3; cj++)
            for (int q = 0; q < 3; q++) {
                hipLaunchKernelGGL(kd_indicator, grid2d(g), dim3(64, 4), 0, ctx->stream, g, ci, cj, q, x);
                pl_launch_stokes_apply(ctx, op_scaled, x, y);
                hipLaunchKernelGGL(kd_scatter_band, grid2d(g), dim3(64, 4), 0, ctx->stream, g, D->tr, ci, cj, q, (const double*)y, kl, ku, ld, D->ab);
            }
    PL_TRY(direct_coef(ctx, op));
    PL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const double t0 = now_ms();
    hipLaunchKernelGGL(kd_lu_first, dim3(1), dim3(KD_T), D->lds_fac, ctx->stream, n, kl, ku, ld, nb, D->ab, D->piv, D->info);
    const int kv = kl + ku;
    for (int k0 = 0; k0 + nb < n; k0 += nb) {
        const int k1 = k0 + nb, nt = std::min(n - 1, k1 - 1 + kv) - k1 + 1;
        hipLaunchKernelGGL(kd_lu_step, dim3((nt + nb - 1) / nb), dim3(KD_T), D->lds_fac, ctx->stream, n, kl, ku, ld, nb, k0, D->ab, D->piv, D->info);
    }
    int info = 0;
    PL_HIP(ctx, hipGetLastError());
    PL_HIP(ctx, hipMemcpyAsync(&info, D->info, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PL_HIP(ctx, hipStreamSynchronize(ctx->stream));
    D->factor_ms = now_ms() - t0; D->solve_ms = 0.0; D->nsolve = 0;
    if (info != 0) return pl_fail(ctx, "direct solve: the matrix is exactly singular");
    return 0;
}

// out = (D_r A)^-1 in   (3 ring planes each)
int pl_direct_solve(pl_ctx* ctx, const double* in, double* out) {
    PlDirect* D = (PlDirect*)ctx->direct;
    if (!D) return pl_fail(ctx, "direct solve: no factorisation");
    const PlGeom& g = ctx->geom.d;
    static const bool timed = getenv("PYLAMP_SOLVER_TRACE") != nullptr;
    double t0 = 0.0;
    if (timed) { PL_HIP(ctx, hipStreamSynchronize(ctx->stream)); t0 = now_ms(); }
    hipLaunchKernelGGL(kd_planes_to_vec, grid2d(g), dim3(64, 4), 0, ctx->stream, g, D->tr, in, D->work);
    hipLaunchKernelGGL(kd_lu_fwd, dim3(1), dim3(KD_T), D->lds_fwd, ctx->stream, D->n, D->kl, D->ku, D->ld, D->nb, D->wr, (const double*)D->ab,
                       (const int*)D->piv, D->work);
    hipLaunchKernelGGL(kd_lu_bwd, dim3(1), dim3(KD_T), D->lds_bwd, ctx->stream, D->n, D->kl, D->ku, D->ld, D->nb, D->wr, (const double*)D->ab,
                       D->work);
    hipLaunchKernelGGL(kd_vec_to_planes, grid2d(g), dim3(64, 4), 0, ctx->stream, g, D->tr, (const double*)D->work, out);
    PL_HIP(ctx, hipGetLastError());
    if (timed) { PL_HIP(ctx, hipStreamSynchronize(ctx->stream)); D->solve_ms += now_ms() - t0; }
    D->nsolve++;
    return 0;
}

// r = b - A x of the unscaled operator in double-double arithmetic (3 ring planes each; b unscaled)
int pl_direct_residual_dd(pl_ctx* ctx, const double* b, const double* x, double* r) {
    PlDirect* D = (PlDirect*)ctx->direct;
    if (!D) return pl_fail(ctx, "direct solve: no probed operator");
    const PlGeom& g = ctx->geom.d;
    hipLaunchKernelGGL(kd_residual_dd, grid2d(g), dim3(64, 4), 0, ctx->stream, g, (const double*)D->coef, b, x, r);
    PL_HIP(ctx, hipGetLastError());
    return 0;
}

void pl_direct_stats(pl_ctx* ctx, int* band, int* nb, double* factor_ms, double* solve_ms, int* nsolve) {
    const PlDirect* D = (const PlDirect*)ctx->direct;
    *band = D ? 2 * D->kl + D->ku + 1 : 0; *nb = D ? D->nb : 0; *factor_ms = D ? D->factor_ms : 0.0; *solve_ms = D ? D->solve_ms : 0.0; *nsolve = D ? D->nsolve : 0;
}

// band width (rows of the LAPACK storage), panel width, factorisation ms and triangular-solve ms (summed, PYLAMP_SOLVER_TRACE only) of the
// last LU on this context; zeros when it has none
extern "C" int pl_stokes_direct_info(pl_ctx* ctx, int* band, int* nb, double* factor_ms, double* solve_ms, int* nsolve) {
    if (!band || !nb || !factor_ms || !solve_ms || !nsolve) return pl_fail(ctx, "pl_stokes_direct_info: NULL argument");
    pl_direct_stats(ctx, band, nb, factor_ms, solve_ms, nsolve);
    return 0;
}

// Diagnostic entry (tests, tools): r = rhs - A x of the current operator, in double-double, with the probed entries.
extern "C" int pl_stokes_residual_dd(pl_ctx* ctx, const double* rhs, const double* x, double* r) {
    if (!ctx->sop_ready) return pl_fail(ctx, "stokes operator not set");
    if (!rhs || !x || !r) return pl_fail(ctx, "pl_stokes_residual_dd: NULL argument");
    if (ctx->nranks != 1) return pl_fail(ctx, "pl_stokes_residual_dd: one rank only");
    PL_HIP(ctx, hipSetDevice(ctx->device));
    PL_TRY(direct_alloc(ctx));
    PL_TRY(direct_coef(ctx, ctx->sop));
    const PlGeom& g = ctx->geom.d;
    size_t vb = (size_t)3 * g.plane * sizeof(double);
    double *db, *dx, *dr;
    PL_TRY(pl_buf(ctx, "api_x", vb, &dx)); PL_TRY(pl_buf(ctx, "api_y", vb, &db)); PL_TRY(pl_buf(ctx, "api_r", vb, &dr));
    PL_TRY(pl_vec3_upload(ctx, g, rhs, db));
    PL_TRY(pl_vec3_upload(ctx, g, x, dx));
    PL_TRY(pl_direct_residual_dd(ctx, db, dx, dr));
    PL_TRY(pl_vec3_download(ctx, g, dr, r));
    return 0;
}
