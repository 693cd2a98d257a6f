// Device-resident 3-D time step: the sequence of Simulation3.step() (pylamp_amd/pylamp3d.py; the loop of pylamp2.py:290-581 with a
// third axis) with every grid field kept on the device.  Scatter, gather, RK4, sort and refill are the kernels of pl_mic3.hip, the
// solvers those of pl_3d.hip; this file joins them: the reductions that the time-step rules and the coefficient scaling need, the
// wall carry and the increment of the temperature, and the advection velocity on the padded centre grid.  Only solver scalars, the
// reduced scalars (a few doubles per step) and the report cross the bus.
//
// All kernels here are bandwidth-bound FP64 passes over plain (nz, nx, ny) arrays or the context's ringed ones, lanes along y, 256
// threads, no floating-point atomics; the reductions are reduce-then-finish in two plain launches (per-workgroup partials, then one
// workgroup), so no workgroup waits on another and the order of every combination is fixed.
#include "pl_internal.h"
#include "pl_mic3.h"
#include "pl_reduce3.h"
#include "pl_step3.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#define S3_HIP(ctx, call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return pl3_fail(ctx, std::string(#call) + ": " + hipGetErrorString(e_)); } while (0)
#define S3_TRY(expr) do { int rc_ = (expr); if (rc_) return rc_; } while (0)
#define S3_MAXPART 1024
#define PL3_PICARD_CAP 32
enum { S3_RHO = 0, S3_ETAS, S3_CP, S3_T, S3_H, S3_MAT, S3_ETAN, S3_KZ, S3_KX, S3_KY, S3_NPLAIN };       // slots of the scattered fields

struct S3Dims { int n[3]; long long s0, s1; int pad; };
__device__ inline long long s3_ring(const S3Dims& d, int i, int j, int k) { return (long long)(i + 1) * d.s0 + (long long)(j + 1) * d.s1 + k + d.pad; }
// node t of the plain (nz, nx, ny) order -> its indices, and its element in a ringed array
__device__ inline void s3_ijk(const S3Dims& d, long long t, int& i, int& j, int& k) {
    k = (int)(t % d.n[2]); j = (int)((t / d.n[2]) % d.n[1]); i = (int)(t / ((long long)d.n[2] * d.n[1]));
}
__device__ inline long long s3_ring(const S3Dims& d, long long t) { int i, j, k; s3_ijk(d, t, i, j, k); return s3_ring(d, i, j, k); }

// One pass over the scattered fields: slot 0 / 1 the NaN counts of rho / etas; 2, 3 the smallest non-NaN etas and whether it holds a NaN;
// 4, 5 the same for etan; 6, 7 the largest 2 kz / (rho cp) -- every operation rounded on its own, as NumPy evaluates it -- and its NaN flag
// (kz == NULL: heat is off, 6 and 7 stay empty)
using S3FieldOps = R3Ops<R3_SUM, R3_SUM, R3_MIN, R3_MAX, R3_MIN, R3_MAX, R3_MAX, R3_MAX>;
__global__ __launch_bounds__(256) void k_s3_reduce_fields(long long N, const double* __restrict__ rho, const double* __restrict__ etas,
                                                         const double* __restrict__ etan, const double* __restrict__ kz, const double* __restrict__ cp,
                                                         double* __restrict__ part) {
    double acc[8] = {0.0, 0.0, INFINITY, 0.0, INFINITY, 0.0, -INFINITY, 0.0};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < N; t += (long long)gridDim.x * 256) {
        const double r = rho[t], es = etas[t], en = etan[t];
        if (r != r) acc[0] += 1.0;
        if (es != es) { acc[1] += 1.0; acc[3] = 1.0; } else acc[2] = fmin(acc[2], es);
        if (en != en) acc[5] = 1.0; else acc[4] = fmin(acc[4], en);
        if (kz) {
            const double d = __dmul_rn(2.0, __ddiv_rn(kz[t], __dmul_rn(r, cp[t])));
            if (d != d) acc[7] = 1.0; else acc[6] = fmax(acc[6], d);
        }
    }
    r3_block<S3FieldOps>(acc, threadIdx.x, blockIdx.x, part);
}
// largest vz, vx, vy over all nodes of the ringed solution (the plain maximum, as step() has it): slots 2 q the maximum of the non-NaN
// entries, 2 q + 1 whether the component holds a NaN
struct S3Vel { const double* v[3]; };
using S3VelOps = R3All<R3_MAX, 6>;
__global__ __launch_bounds__(256) void k_s3_velmax(S3Dims d, S3Vel x, double* __restrict__ part) {
    const long long N = (long long)d.n[0] * d.n[1] * d.n[2];
    double acc[6] = {-INFINITY, 0.0, -INFINITY, 0.0, -INFINITY, 0.0};
    for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < N; t += (long long)gridDim.x * 256) {
        const long long c = s3_ring(d, t);
#pragma unroll
        for (int q = 0; q < 3; q++) { const double u = x.v[q][c]; if (u != u) acc[2 * q + 1] = 1.0; else acc[2 * q] = fmax(acc[2 * q], u); }
    }
    r3_block<S3VelOps>(acc, threadIdx.x, blockIdx.x, part);
}

// Cell-centred velocities on the padded (nz+1, nx+1, ny+1) grid (pylamp2.py:491-545 with a third axis; advection_velocity in
// pylamp3d.py).  Inside, component q is 0.5 (a + b) along its own axis.  The ghost planes are written wall by wall in the order z0, x0,
// y0, zL, xL, yL, each a copy of the neighbouring plane AS IT IS AT THAT MOMENT (normal component negated): a point of an edge or a
// corner takes the value of the LAST wall that holds it, whose source may itself have been written by an earlier wall.  A thread
// walks that chain backwards from its own point until it stands on an inner point; a source that no earlier wall had written yet
// would still hold the initial zero (it cannot occur with this order, the case is kept for exactness).  The pass of a no-slip wall
// (bit w of `noslip`) is skipped, as in the reference: its ghost plane keeps the initial zero but where a later pass writes its edges.
// The pass of a no-slip wall that MOVES (bit w of mv.moving; pl3_stokes_set_wall_velocity) runs in its slot: from the neighbouring plane
// as it is at that moment it writes -V for the normal component and 2 U_c - V for a tangential component c, so that the velocity
// interpolated onto the wall is U.  These steps round, so a chain that holds one is replayed forwards, first wall first, as the passes
// ran; without a moving wall in the chain the walk is the one above.
// The pass of a wall with a FLOW through it (bit w of fl.mask; pl3_stokes_set_wall_flow) runs in its slot as well, even for a no-slip wall
// at rest: the normal component becomes 2 Un[ci, cj] - V, with ci, cj the padded tangential indices minus 1 clamped to the wall's faces
// (a ghost point and its source share them, so they follow from the thread's own point), and the velocity interpolated onto the wall is
// Un; the tangential components are copied on a free-slip wall and follow 2 U_c - V on a no-slip wall (U_c possibly 0).  Such a chain
// is replayed forwards too.  A wall without a flow keeps the arithmetic above (-V, not 2 0 - V: the sign of zero differs).
struct S3Adv { double* V[3]; };
__global__ __launch_bounds__(256) void k_s3_advvel(S3Dims d, S3Vel x, S3Adv o, int noslip, Pl3WallVel mv, Pl3WallFlow fl) {
    const int pn[3] = {d.n[0] + 1, d.n[1] + 1, d.n[2] + 1};
    const long long GN = (long long)pn[0] * pn[1] * pn[2];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= GN) return;
    const int p0[3] = {(int)(t / ((long long)pn[2] * pn[1])), (int)((t / pn[2]) % pn[1]), (int)(t % pn[2])};
    const int skip = noslip & ~mv.moving & ~fl.mask;         // the walls whose pass does not run
    const int replay = mv.moving | fl.mask;                  // the walls whose pass rounds
    const int shear = mv.moving | (fl.mask & noslip);        // the walls whose tangential components follow 2 U_c - V
#pragma unroll
    for (int q = 0; q < 3; q++) {
        int p[3] = {p0[0], p0[1], p0[2]};
        double sign = 1.0;
        int chain = 0, moved = 0;                            // the walls of the walk, 3 bits each (w + 1), the earliest pass in the lowest bits
        for (int w = 5; w >= 0; w--) {                       // walls 0..5 = z0, x0, y0, zL, xL, yL
            const int a = w % 3, ghost = w < 3 ? 0 : pn[a] - 1;
            if (p[a] != ghost || ((skip >> w) & 1)) continue;          // (the pass of a no-slip wall at rest is skipped)
            p[a] = w < 3 ? 1 : pn[a] - 2;
            if (a == q) sign = -sign;
            chain = (chain << 3) | (w + 1);
            moved |= (replay >> w) & 1;
        }
        const bool inner = p[0] >= 1 && p[0] <= pn[0] - 2 && p[1] >= 1 && p[1] <= pn[1] - 2 && p[2] >= 1 && p[2] <= pn[2] - 2;
        double r = 0.0;
        if (inner) {
            // V_q[I, J, K] = 0.5 (v_q[.. own index I ..] + v_q[.. I - 1 ..]) at the nodes (I-1, J-1, K-1) of the other axes
            int hi[3] = {p[0] - 1, p[1] - 1, p[2] - 1}, lo[3] = {p[0] - 1, p[1] - 1, p[2] - 1};
            hi[q] = p[q];
            r = 0.5 * (x.v[q][s3_ring(d, hi[0], hi[1], hi[2])] + x.v[q][s3_ring(d, lo[0], lo[1], lo[2])]);
            if (!moved) r = sign * r;
        }
        if (moved) {
            for (; chain; chain >>= 3) {
                const int w = (chain & 7) - 1;
                if (w % 3 == q) {
                    if ((fl.mask >> w) & 1) {                // (the two other axes P < Q in z, x, y order)
                        const int P = q == 0 ? 1 : 0, Q = q == 2 ? 1 : 2;
                        const int ci = min(max(p0[P] - 1, 0), d.n[P] - 2), cj = min(max(p0[Q] - 1, 0), d.n[Q] - 2);
                        r = 2.0 * fl.un[w][(long long)ci * (d.n[Q] - 1) + cj] - r;
                    } else r = -r;
                }
                else if ((shear >> w) & 1) r = 2.0 * mv.u[3 * w + q] - r;
            }
        }
        o.V[q][t] = r;
    }
}

// pylamp2.py:327-331: from the second step on the six walls of the scattered T take the previous solved temperature
__global__ __launch_bounds__(256) void k_s3_wall_carry(S3Dims d, const double* __restrict__ prev, double* __restrict__ T) {
    const long long N = (long long)d.n[0] * d.n[1] * d.n[2];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    int i, j, k;
    s3_ijk(d, t, i, j, k);
    if (i == 0 || i == d.n[0] - 1 || j == 0 || j == d.n[1] - 1 || k == 0 || k == d.n[2] - 1) T[t] = prev[t];
}
// the solved temperature (ringed) -> plain, and the increment newtemp - T that the gather interpolates to the tracers
__global__ __launch_bounds__(256) void k_s3_increment(S3Dims d, const double* __restrict__ sol, const double* __restrict__ T, double* __restrict__ newtemp,
                                                      double* __restrict__ dT) {
    const long long N = (long long)d.n[0] * d.n[1] * d.n[2];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const double u = sol[s3_ring(d, t)];
    newtemp[t] = u;
    dT[t] = u - T[t];
}
// ringed <-> plain (to_ring: owned nodes only)
__global__ __launch_bounds__(256) void k_s3_layout(S3Dims d, double* __restrict__ ringed, double* __restrict__ plain, int to_ring) {
    const long long N = (long long)d.n[0] * d.n[1] * d.n[2];
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t >= N) return;
    const long long c = s3_ring(d, t);
    if (to_ring) ringed[c] = plain[t]; else plain[t] = ringed[c];
}

// =====================================================================================================================
// host side
// =====================================================================================================================
struct Step3 {
    bool have_scattered = false, have_heat_fields = false, have_vel = false, have_temp = false;
    // pl3_step_set_shear_heating / pl3_step_set_strain_fields (both off at creation), and the integral of the dissipation of the last step
    // that ran with one of them on
    bool shear_heating = false, strain_fields = false, have_strain = false;
    double dissipation_total = 0.0;
    // pl3_step_set_picard, and what the Picard loop of the last step did (pl3_step_picard_report); it runs only with a yield stress set
    int picard_maxit = 10; double picard_tol = 1e-2;
    int picard_its = 0, picard_converged = 0; double picard_log[4 * PL3_PICARD_CAP] = {0};      // per iteration: change, yielded nodes, yielded cells, Stokes iterations
};
void pl3_step_free(void** slot) {
    delete (Step3*)*slot;
    *slot = nullptr;
}
static const char* const S3_NAMES[20] = {"rho", "etas", "cp", "T", "H", "mat", "etan", "kz", "kx", "ky", "velz", "velx", "vely", "pres", "temp",
                                         "strainrate", "stress", "dissipation", "etas_eff", "etan_eff"};

struct S3Open { Pl3HostView h; Pl3DevView d; Step3* S; S3Dims dims; size_t N, GNp; };        // N nodes; GNp points of the padded centre grid
static int s3_open(pl3_ctx* ctx, const char* who, S3Open& o) {
    S3_TRY(pl3_host_view(ctx, &o.h));
    if (o.h.nranks > 1) return pl3_fail(ctx, std::string(who) + ": the device-resident 3-D step runs on one rank (this context has pl3_set_comm attached)");
    S3_TRY(pl3i_dev_view(ctx, &o.d));
    if (!*o.d.slot) *o.d.slot = new Step3();
    o.S = (Step3*)*o.d.slot;
    for (int a = 0; a < 3; a++) o.dims.n[a] = o.h.gn[a];
    o.dims.s0 = o.d.s0; o.dims.s1 = o.d.s1; o.dims.pad = o.d.pad;
    o.N = (size_t)o.h.gn[0] * o.h.gn[1] * o.h.gn[2];
    o.GNp = (size_t)(o.h.gn[0] + 1) * (o.h.gn[1] + 1) * (o.h.gn[2] + 1);
    return 0;
}
static inline dim3 s3_blocks(long long n) { return dim3((unsigned)((std::max<long long>(n, 1) + 255) / 256)); }
static inline int s3_nparts(long long n) { return (int)std::min<long long>(S3_MAXPART, (std::max<long long>(n, 1) + 255) / 256); }
// Python's min(a, b) / max(a, b): the first argument unless the second is smaller / larger (a NaN stays where it is)
static inline double py_min(double a, double b) { return b < a ? b : a; }
static inline double py_max(double a, double b) { return b > a ? b : a; }

// partials -> K values on the host: one launch of one workgroup and one small read-back
template <class OPS>
static int s3_finish(pl3_ctx* ctx, S3Open& o, int nb, const double* part, double* red, double host[OPS::K]) {
    constexpr int K = OPS::K;
    hipLaunchKernelGGL(k_r3_finish<OPS>, dim3(1), dim3(256), 0, o.d.stream, (long long)nb, (long long)nb, part, red);
    S3_HIP(ctx, hipGetLastError());
    pl3_count_copy(ctx, K * sizeof(double));
    S3_HIP(ctx, hipMemcpyAsync(host, red, K * sizeof(double), hipMemcpyDeviceToHost, o.d.stream));
    S3_HIP(ctx, hipStreamSynchronize(o.d.stream));
    return 0;
}
static void s3_advvel(S3Open& o, double* const X[3], double* adv) {
    S3Vel x{{X[0], X[1], X[2]}}; S3Adv a{{adv, adv + o.GNp, adv + 2 * o.GNp}};
    hipLaunchKernelGGL(k_s3_advvel, s3_blocks((long long)o.GNp), dim3(256), 0, o.d.stream, o.dims, x, a, o.d.noslip, o.d.wallvel, o.d.wallflow);
}

extern "C" int pl3_resident_step(pl3_ctx* ctx, const pl3_step_config* cfg, int it, pl3_step_report* rep) {
    if (!ctx) return pl3_fail(nullptr, "pl3_resident_step: NULL context");
    if (!cfg || !rep) return pl3_fail(ctx, "pl3_resident_step: NULL argument");
    const auto wall0 = std::chrono::steady_clock::now();
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_resident_step", o));
    std::memset(rep, 0, sizeof(*rep));
    if (it < 1) return pl3_fail(ctx, "pl3_resident_step: steps count from 1");
    const bool heat = cfg->do_heatdiff != 0;
    if (heat && it > 1 && !o.S->have_temp) return pl3_fail(ctx, "pl3_resident_step: step > 1 with heat needs the temperature of the previous resident step");
    const size_t N = o.N, GNp = o.GNp;
    const int nb = s3_nparts((long long)N);
    double *F, *temp, *dT, *adv, *part, *red;
    S3_TRY(pl3i_mic_buf(ctx, "s_fields", N * S3_NPLAIN, &F));
    S3_TRY(pl3i_mic_buf(ctx, "s_temp", N, &temp));
    S3_TRY(pl3i_mic_buf(ctx, "s_dT", N, &dT));
    S3_TRY(pl3i_mic_buf(ctx, "s_adv", 3 * GNp, &adv));
    S3_TRY(pl3i_mic_buf(ctx, "s_part", (size_t)S3_MAXPART * 8, &part));
    S3_TRY(pl3i_mic_buf(ctx, "s_red", 8, &red));
    double* ms = pl3i_mic_ms(ctx);
    o.S->have_scattered = false; o.S->have_vel = false; o.S->have_strain = false;       // the fields of the previous step go as this one overwrites them
    if (o.S->shear_heating && !heat) return pl3_fail(ctx, "pl3_resident_step: shear heating (pl3_step_set_shear_heating) needs the heat solve, do_heatdiff = 1");

    // 1. properties and the field list of scatter_fields(): node grid, cell centres, the three mixed sets of the conductivity
    // (the two columns the properties overwrite are kept, so that a step that fails its NaN check leaves the tracers as they were)
    double *trf, *keep; long long ntr, cap;
    S3_TRY(pl3i_mic_columns(ctx, &trf, &ntr, &cap));
    S3_TRY(pl3i_mic_buf(ctx, "s_keep", (size_t)2 * cap, &keep));
    S3_HIP(ctx, hipMemcpyAsync(keep, trf, (size_t)2 * cap * sizeof(double), hipMemcpyDeviceToDevice, o.d.stream));       // TR_RHO, TR_ETA
    S3_TRY(pl3_resident_props(ctx, cfg->tdep_rho, cfg->tdep_eta, cfg->tref, cfg->etamin, cfg->etamax));
    std::vector<double> mpv[3];
    for (int a = 0; a < 3; a++) {                           // pylamp2.py:92-95
        const int n = o.h.gn[a]; const double* c = o.h.coord[a];
        mpv[a].resize(n);
        for (int i = 0; i + 1 < n; i++) mpv[a][i] = (c[i + 1] + c[i]) / 2;
        mpv[a][n - 1] = mpv[a][n - 2] + (mpv[a][n - 2] - mpv[a][n - 3]);
    }
    const double* g[3] = {o.h.coord[0], o.h.coord[1], o.h.coord[2]}; const double* mp[3] = {mpv[0].data(), mpv[1].data(), mpv[2].data()};
    const int A = PL_AVG_ARITHMETIC | PL_AVG_WEIGHTED, G = PL_AVG_GEOMETRIC | PL_AVG_WEIGHTED;
    const int eta_col[1] = {1}, hcd_col[1] = {4};         // TR_ETA, TR_HCD
    double ms_scatter = 0.0;
    if (heat) {
        const int cols[6] = {0, 1, 5, 3, 11, 8}, sch[6] = {A, G, A, A, A, A};      // TR_RHO, TR_ETA, TR_HCP, TR_TMP, TR_IHT, TR_MAT
        const int sg[1] = {G}, sa[1] = {A};
        const double* kzc[3] = {mp[0], g[1], g[2]}; const double* kxc[3] = {g[0], mp[1], g[2]}; const double* kyc[3] = {g[0], g[1], mp[2]};
        S3_TRY(pl3i_mic_scatter(ctx, 6, cols, sch, g, o.h.gn, F)); ms_scatter += ms[0];
        S3_TRY(pl3i_mic_scatter(ctx, 1, eta_col, sg, mp, o.h.gn, F + S3_ETAN * N)); ms_scatter += ms[0];
        S3_TRY(pl3i_mic_scatter(ctx, 1, hcd_col, sa, kzc, o.h.gn, F + S3_KZ * N)); ms_scatter += ms[0];
        S3_TRY(pl3i_mic_scatter(ctx, 1, hcd_col, sa, kxc, o.h.gn, F + S3_KX * N)); ms_scatter += ms[0];
        S3_TRY(pl3i_mic_scatter(ctx, 1, hcd_col, sa, kyc, o.h.gn, F + S3_KY * N)); ms_scatter += ms[0];
    } else {
        const int cols[2] = {0, 1}, sch[2] = {A, G}, sg[1] = {PL_AVG_GEOMETRIC};     // etan unweighted, as pylamp2.py:322
        S3_TRY(pl3i_mic_scatter(ctx, 2, cols, sch, g, o.h.gn, F)); ms_scatter += ms[0];
        S3_TRY(pl3i_mic_scatter(ctx, 1, eta_col, sg, mp, o.h.gn, F + S3_ETAN * N)); ms_scatter += ms[0];
    }
    ms[0] = ms_scatter;
    o.S->have_scattered = true; o.S->have_heat_fields = heat;

    // 2. NaN check, min(eta) and the largest diffusivity in one pass
    hipLaunchKernelGGL(k_s3_reduce_fields, dim3(nb), dim3(256), 0, o.d.stream, (long long)N, (const double*)(F + S3_RHO * N), (const double*)(F + S3_ETAS * N),
                       (const double*)(F + S3_ETAN * N), (const double*)(heat ? F + S3_KZ * N : nullptr), (const double*)(heat ? F + S3_CP * N : nullptr), part);
    double r8[8];
    S3_TRY(s3_finish<S3FieldOps>(ctx, o, nb, part, red, r8));
    rep->nan_rho = (int64_t)r8[0]; rep->nan_etas = (int64_t)r8[1];
    if (rep->nan_rho > 0 || rep->nan_etas > 0) {
        const bool rho_bad = rep->nan_rho > 0;
        S3_HIP(ctx, hipMemcpyAsync(trf, keep, (size_t)2 * cap * sizeof(double), hipMemcpyDeviceToDevice, o.d.stream));
        S3_HIP(ctx, hipStreamSynchronize(o.d.stream));
        return pl3_fail(ctx, std::string("pl3_resident_step: the scattered field '") + (rho_bad ? "rho" : "etas") + "' holds NaN at " +
                                 std::to_string((long long)(rho_bad ? rep->nan_rho : rep->nan_etas)) + " nodes (tracers and temperature are left as they were)");
    }
    const double mineta = nan_min3(r8[2], r8[4], r8[3] > 0.0, r8[5] > 0.0);

    // 3. the heat time-step rule (after the wall carry, which touches T alone)
    double dxmin = INFINITY;
    for (int a = 0; a < 3; a++) dxmin = std::min(dxmin, (o.h.coord[a][o.h.gn[a] - 1] - o.h.coord[a][0]) / (o.h.gn[a] - 1));
    double tstep_temp = 0.0;
    if (heat) {
        if (it > 1) hipLaunchKernelGGL(k_s3_wall_carry, s3_blocks((long long)N), dim3(256), 0, o.d.stream, o.dims, (const double*)temp, F + S3_T * N);
        const double maxd = r8[7] > 0.0 ? NAN : r8[6];
        volatile double two = 2.0;                                 // NumPy's scalar ** 2 is the library's pow
        tstep_temp = cfg->tstep_modifier * std::pow(dxmin, two) / maxd;
        tstep_temp = py_max(py_min(tstep_temp, cfg->tstep_dif_max), cfg->tstep_dif_min);
    }

    // 4. Stokes: coefficients from the device fields, resident solve (cold, or warm with pl3_stokes_set_warm_start)
    S3_TRY(pl3i_stokes_set_coeffs_dev(ctx, F + S3_ETAS * N, F + S3_ETAN * N, F + S3_RHO * N, cfg->use_grav ? cfg->grav : nullptr, mineta));
    S3_TRY(pl3_stokes_solve(ctx, nullptr, nullptr, 0, cfg->stokes_rtol, cfg->stokes_maxit, &rep->stokes));
    o.S->have_vel = true;
    // 4a. yield stress (opt-in, pl3_stokes_set_yield): the Picard loop -- update the viscosities from the solution, solve again from it
    // while the change is above the tolerance; as many updates as solves, everything below uses the last solution
    o.S->picard_its = 0; o.S->picard_converged = 0;
    if (o.d.yield_on) {
        for (int n = 0;; n++) {
            double y[6];
            S3_TRY(pl3i_yield_update_dev(ctx, y));
            double* l = o.S->picard_log + 4 * n;
            l[0] = y[1]; l[1] = y[2]; l[2] = y[3]; l[3] = (double)rep->stokes.iterations;
            o.S->picard_its = n + 1; o.S->picard_converged = y[1] <= o.S->picard_tol ? 1 : 0;
            if (!(y[1] > o.S->picard_tol) || n + 1 >= o.S->picard_maxit) break;
            S3_TRY(pl3_stokes_solve(ctx, nullptr, nullptr, 1, cfg->stokes_rtol, cfg->stokes_maxit, &rep->stokes));
        }
    }
    // 4b. strain rate, stress and dissipation of that solution (opt-in); with shear heating H += dissipation, one addition per node,
    // before the heat coefficients are taken from it
    if (o.S->shear_heating || o.S->strain_fields) {
        S3_TRY(pl3i_strain_fields_dev(ctx, o.S->shear_heating ? F + S3_H * N : nullptr, &o.S->dissipation_total));
        o.S->have_strain = true;
    }

    // 5. the Stokes time-step rule, the limiter and the clamps
    hipLaunchKernelGGL(k_s3_velmax, dim3(nb), dim3(256), 0, o.d.stream, o.dims, S3Vel{{o.d.X[0], o.d.X[1], o.d.X[2]}}, part);
    double r6[6];
    S3_TRY(s3_finish<S3VelOps>(ctx, o, nb, part, red, r6));
    double vmax = r6[1] > 0.0 ? NAN : r6[0];
    for (int q = 1; q < 3; q++) vmax = py_max(vmax, r6[2 * q + 1] > 0.0 ? NAN : r6[2 * q]);
    double tstep_stokes = cfg->tstep_modifier * dxmin / vmax;
    tstep_stokes = py_max(py_min(tstep_stokes, cfg->tstep_adv_max), cfg->tstep_adv_min);
    double tstep = tstep_stokes; int limiter = 0;
    if (heat) { limiter = tstep_temp < tstep_stokes ? 1 : 0; tstep = py_min(tstep_temp, tstep_stokes); }
    rep->tstep = tstep; rep->limiter = limiter; rep->tstep_heat = tstep_temp; rep->tstep_stokes = tstep_stokes;
    S3_TRY(pl3_stokes_history_commit(ctx, tstep));          // (nothing unless the warm start is on: the next solve is tstep of model time away)

    // 6. + 7. heat: coefficients from the device fields, resident solve, temperature to the tracers
    if (heat) {
        const double* src[7] = {F + S3_KZ * N, F + S3_KX * N, F + S3_KY * N, F + S3_T * N, F + S3_H * N, F + S3_RHO * N, F + S3_CP * N};
        S3_TRY(pl3i_heat_set_coeffs_dev(ctx, mp, src, cfg->bcheat, cfg->bcheatvals, tstep));
        S3_TRY(pl3_heat_solve(ctx, nullptr, nullptr, cfg->heat_rtol, cfg->heat_maxit, &rep->heat));
        o.S->have_temp = false;
        hipLaunchKernelGGL(k_s3_increment, s3_blocks((long long)N), dim3(256), 0, o.d.stream, o.dims, (const double*)o.d.T, (const double*)(F + S3_T * N), temp, dT);
        S3_HIP(ctx, hipGetLastError());
        o.S->have_temp = true;
        if (it == 1) S3_TRY(pl3i_mic_temp_to_tracers(ctx, 1, temp, 0, 0.0));
        else S3_TRY(pl3i_mic_temp_to_tracers(ctx, 0, dT, cfg->do_subgrid_heatdiff ? 1 : 0, tstep));
    }

    // 8. + 9. advection velocity on the padded centre grid; RK4 + fence (or, with pl3_mic_set_deletion, deletion in the sort) + sort + refill
    s3_advvel(o, o.d.X, adv);
    S3_HIP(ctx, hipGetLastError());
    int64_t cnt[4] = {0, 0, 0, 0};
    S3_TRY(pl3i_mic_advect(ctx, adv, tstep, cfg->tracdens, cfg->tracdens_min, cfg->inject_seed, it, cfg->inject_unique_ids, cnt));
    rep->ninjected = cnt[0]; rep->nrefilled = cnt[1]; rep->nempty = cnt[2]; rep->mincount = cnt[3];
    S3_TRY(pl3_tracers_count(ctx, &rep->ntrac));
    int64_t gone[2];
    S3_TRY(pl3_tracers_removed(ctx, gone));
    rep->nremoved = gone[0];
    rep->ms_scatter = ms[0]; rep->ms_gather = heat ? ms[1] : 0.0; rep->ms_rk4 = ms[2]; rep->ms_sort = ms[3];
    rep->ms_stokes = rep->stokes.solve_ms; rep->ms_heat = rep->heat.solve_ms;
    rep->ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    return 0;
}

// A grid field of the last resident step, (nz, nx, ny): rho, etas, etan, cp, T, H, mat, kz, kx, ky (cp .. ky but etan only with heat
// on), velz, velx, vely, pres (Kcont-scaled), temp; strainrate, stress, dissipation after a step with pl3_step_set_shear_heating or
// pl3_step_set_strain_fields on, until the Stokes work vectors are used again.  One node-sized copy.
extern "C" int pl3_get_field(pl3_ctx* ctx, const char* name, double* out) {
    if (!ctx) return pl3_fail(nullptr, "pl3_get_field: NULL context");
    if (!name || !out) return pl3_fail(ctx, "pl3_get_field: NULL argument");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_get_field", o));
    const Step3& S = *o.S;
    int id = -1;
    std::string have;
    for (int q = 0; q < 20; q++) {
        const bool ok = q < 10 ? S.have_scattered && (S.have_heat_fields || q == S3_RHO || q == S3_ETAS || q == S3_ETAN)
                               : (q < 14 ? S.have_vel : (q == 14 ? S.have_temp : (q < 18 ? S.have_strain && o.d.have_strain : S.have_vel && o.d.yield_on)));
        if (ok) have += std::string(have.empty() ? "" : ", ") + S3_NAMES[q];
        if (ok && !std::strcmp(name, S3_NAMES[q])) id = q;
    }
    if (id < 0) return pl3_fail(ctx, std::string("pl3_get_field: no field '") + name + "' of a resident step (have: " + (have.empty() ? "none yet" : have) + ")");
    const size_t N = o.N;
    double* src;
    if (id < 10) { S3_TRY(pl3i_mic_buf(ctx, "s_fields", N * S3_NPLAIN, &src)); src += (size_t)id * N; }
    else if (id == 14) S3_TRY(pl3i_mic_buf(ctx, "s_temp", N, &src));
    else {
        S3_TRY(pl3i_mic_buf(ctx, "s_stage", 3 * N, &src));
        hipLaunchKernelGGL(k_s3_layout, s3_blocks((long long)N), dim3(256), 0, o.d.stream, o.dims, id < 14 ? o.d.X[id - 10] : (id < 18 ? o.d.strain[id - 15] : o.d.eta_eff[id - 18]), src, 0);
        S3_HIP(ctx, hipGetLastError());
    }
    pl3_count_copy(ctx, N * sizeof(double));
    S3_HIP(ctx, hipMemcpyAsync(out, src, N * sizeof(double), hipMemcpyDeviceToHost, o.d.stream));
    S3_HIP(ctx, hipStreamSynchronize(o.d.stream));
    return 0;
}

// Opt-in switches of the resident step, both off at creation (with both off the step is bit for bit what it is without them).  Shear
// heating: after the Stokes solve the dissipation of the solution (pl3_stokes_strain_fields) is added to the scattered H, and the heat solve
// takes that sum; it needs do_heatdiff.  Strain fields: the step keeps strainrate, stress and dissipation for pl3_get_field; either
// switch makes them available.  pl3_step_dissipation_total: the integral of the dissipation of the last such step.
extern "C" int pl3_step_set_shear_heating(pl3_ctx* ctx, int on) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_set_shear_heating: NULL context");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_set_shear_heating", o));
    o.S->shear_heating = on != 0;
    return 0;
}
extern "C" int pl3_step_shear_heating(pl3_ctx* ctx, int* on) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_shear_heating: NULL context");
    if (!on) return pl3_fail(ctx, "pl3_step_shear_heating: NULL argument");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_shear_heating", o));
    *on = o.S->shear_heating ? 1 : 0;
    return 0;
}
extern "C" int pl3_step_set_strain_fields(pl3_ctx* ctx, int on) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_set_strain_fields: NULL context");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_set_strain_fields", o));
    o.S->strain_fields = on != 0;
    return 0;
}
extern "C" int pl3_step_dissipation_total(pl3_ctx* ctx, double* total) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_dissipation_total: NULL context");
    if (!total) return pl3_fail(ctx, "pl3_step_dissipation_total: NULL argument");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_dissipation_total", o));
    if (!o.S->have_strain) return pl3_fail(ctx, "pl3_step_dissipation_total: no resident step has run with shear heating or the strain fields on (pl3_step_set_shear_heating, pl3_step_set_strain_fields)");
    *total = o.S->dissipation_total;
    return 0;
}

// The Picard loop of the resident step (it runs only with a yield stress set, pl3_stokes_set_yield): at most maxit (1 .. 32) Stokes solves
// per step, stopped once the change max |ln(eta_new / eta_prev)| of an update is at most tol (>= 0).  10 and 1e-2 at creation.
extern "C" int pl3_step_set_picard(pl3_ctx* ctx, int maxit, double tol) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_set_picard: NULL context");
    if (maxit < 1 || maxit > PL3_PICARD_CAP)
        return pl3_fail(ctx, "pl3_step_set_picard: maxit = " + std::to_string(maxit) + " must be 1 .. " + std::to_string(PL3_PICARD_CAP));
    if (!(tol >= 0.0)) return pl3_fail(ctx, "pl3_step_set_picard: tol = " + std::to_string(tol) + " must be >= 0");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_set_picard", o));
    o.S->picard_maxit = maxit; o.S->picard_tol = tol;
    return 0;
}
// out[0] iterations of the last resident step's Picard loop (0: it did not run), out[1] converged, then per iteration change, yielded
// nodes, yielded cells, Stokes iterations; n: the capacity of out (2 + 4 x 32 holds everything), entries beyond it are not written
extern "C" int pl3_step_picard_report(pl3_ctx* ctx, double* out, int n) {
    if (!ctx) return pl3_fail(nullptr, "pl3_step_picard_report: NULL context");
    if (!out || n < 2) return pl3_fail(ctx, "pl3_step_picard_report: out needs room for at least 2 entries");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_step_picard_report", o));
    out[0] = o.S->picard_its; out[1] = o.S->picard_converged;
    for (int q = 0; q < 4 * o.S->picard_its && 2 + q < n; q++) out[2 + q] = o.S->picard_log[q];
    return 0;
}

// The step's advection-velocity kernel on host arrays: vz, vx, vy (nz, nx, ny) -> Vz, Vx, Vy on the padded (nz+1, nx+1, ny+1) grid
extern "C" int pl3_advection_velocity(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double* Vz, double* Vx, double* Vy) {
    if (!ctx) return pl3_fail(nullptr, "pl3_advection_velocity: NULL context");
    if (!vz || !vx || !vy || !Vz || !Vx || !Vy) return pl3_fail(ctx, "pl3_advection_velocity: NULL argument");
    S3Open o;
    S3_TRY(s3_open(ctx, "pl3_advection_velocity", o));
    const size_t N = o.N, GNp = o.GNp;
    double *stage, *adv;
    S3_TRY(pl3i_mic_buf(ctx, "s_stage", 3 * N, &stage));
    S3_TRY(pl3i_mic_buf(ctx, "s_advtest", 3 * GNp, &adv));
    const double* in[3] = {vz, vx, vy}; double* out[3] = {Vz, Vx, Vy};
    for (int q = 0; q < 3; q++) {
        pl3_count_copy(ctx, N * sizeof(double));
        S3_HIP(ctx, hipMemcpyAsync(stage + q * N, in[q], N * sizeof(double), hipMemcpyHostToDevice, o.d.stream));
        hipLaunchKernelGGL(k_s3_layout, s3_blocks((long long)N), dim3(256), 0, o.d.stream, o.dims, o.d.scratch[q], stage + q * N, 1);
    }
    s3_advvel(o, o.d.scratch, adv);
    S3_HIP(ctx, hipGetLastError());
    for (int q = 0; q < 3; q++) {
        pl3_count_copy(ctx, GNp * sizeof(double));
        S3_HIP(ctx, hipMemcpyAsync(out[q], adv + q * GNp, GNp * sizeof(double), hipMemcpyDeviceToHost, o.d.stream));
    }
    S3_HIP(ctx, hipStreamSynchronize(o.d.stream));
    return 0;
}

extern "C" int pl3_abi_layout(size_t out[8]) {
    out[0] = sizeof(pl3_step_config); out[1] = sizeof(pl3_step_report);
    out[2] = offsetof(pl3_step_config, bcheatvals); out[3] = offsetof(pl3_step_config, grav); out[4] = offsetof(pl3_step_config, inject_seed);
    out[5] = offsetof(pl3_step_report, heat); out[6] = offsetof(pl3_step_report, ntrac); out[7] = offsetof(pl3_step_report, ms_total);
    return 0;
}
