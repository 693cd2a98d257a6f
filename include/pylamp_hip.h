/* pylamp_hip.h — C ABI of libpylamp_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for PyLamp's per-time-step hot path.  The reference has no FFI layer:
 * its boundary is the Python module API of pylamp_stokes.py / pylamp_diff.py /
 * pylamp_trac.py called from the loop body of pylamp2.py.  the modules under pylamp_amd/ keep those
 * names and signatures and forwards to the entry points declared here through ctypes
 * (see INTEGRATION.md for the binding a PyLamp maintainer would add).
 *
 * Conventions
 *   - plain pointers and sizes only; all floating point data is IEEE double;
 *   - host arrays are C-contiguous, shape (nz, nx) indexed [i=z][j=x]
 *     (reference: pylamp_const.py:9-13, pylamp2.py:37,100-113);
 *   - Stokes vectors use the reference DOF order: (vz, vx, P) interleaved per node,
 *     nodes row-major, length 3*nz*nx (pylamp_stokes.py:22-35 gidx, 86-101 x2vp);
 *   - every function returns 0 on success, non-zero on error; pl_last_error() gives the
 *     message (the Python side raises Exception(msg), the reference's error convention);
 *   - one context per GPU / rank; calls on one context are not thread-safe;
 *   - the library never keeps a host pointer after a call returns;
 *   - there is no CPU fallback: without a usable HIP device pl_create fails.
 */
#ifndef PYLAMP_HIP_H
#define PYLAMP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pl_ctx pl_ctx;

/* Boundary-condition codes (pylamp_stokes.py:17-20, pylamp_diff.py:12-13). */
enum { PL_BC_NOSLIP = 0, PL_BC_FREESLIP = 1, PL_BC_CYCLIC = 2, PL_BC_FLOWTHRU = 4 };
enum { PL_BC_FIXTEMP = 0, PL_BC_FIXFLOW = 1 };
/* Averaging schemes / interpolation methods (pylamp_trac.py:11-22). */
enum { PL_AVG_ARITHMETIC = 1, PL_AVG_GEOMETRIC = 2, PL_AVG_WEIGHTED = 4 };
enum { PL_INTERP_NEAREST = 8, PL_INTERP_LINEAR = 16, PL_INTERP_VELDIV = 32 };

typedef struct pl_solve_stats {
    int    iterations;      /* outer Krylov iterations used                       */
    int    converged;       /* 1 iff rel_residual <= rtol (the recomputed residual, never the recurrence) and, for Stokes,
                             * error_estimate <= 1.5 x its bound (below) */
    double rel_residual;    /* TRUE residual ||D(r0 - A dx)|| / ref, recomputed with the operator, where
                             * r0 = b - A x0 is evaluated once and x = x0 + dx (correction form);
                             * D = row scaling; ref = ||D b|| (heat) or the dynamic load
                             * ||D(b - A x_hydrostatic)|| (Stokes) */
    double solve_ms;        /* device time of the solve (HIP events)              */
    int    operator_applies;
    int    precond_applies;
    int    used_direct;     /* 1: the banded LU of one GPU solved the system (pl_direct.hip: blocked LU, sized by the device
                             * memory budget PYLAMP_DIRECT_MAX_GB) -- up front beyond the viscosity-contrast gate, refined with
                             * a compensated residual, or after the multigrid-preconditioned iteration did not converge
                             * (indefinite systems: the reference's free-surface stabilisation sign at the Courant step,
                             * pylamp2.py:387-405) */
    int    reserved_;       /* 0 */
    double error_estimate;  /* Stokes: estimate of the relative velocity error of the returned iterate from its true residual r
                             * (the residual norm alone does not bound it: error / residual is ~10 on large smooth problems and
                             * ~1e4 on coarse ones):
                             *     (n |r_cont| + |(M^-1 r)_vel|) / |x_vel|  +  |y.r_p / y.A w| |w_vel| / |x_vel|
                             * n = max(nz, nx, L_z / min dz, L_x / min dx) (graded grids count by their finest cell), M^-1 = one
                             * preconditioner application, the last term = the component of r along the deflated pressure-anchor
                             * mode w (it is amplified by |w| / |x|, not by n).  Between the exact evaluations (each costs a
                             * preconditioner application) the iteration uses (n |r_cont| + a |r_mom|) / |x_vel| on the
                             * recurrence residual, a = |(M^-1 s)_vel| / |s_mom| measured on the way.  A solve whose residual meets
                             * rtol keeps iterating until the estimate is <= 3e-8 (PYLAMP_STOKES_ETOL; 0 switches the test off).
                             * Viscosity contrast above 3e5 (PYLAMP_CONTRAST_GATE): the ROW-SCALED residual no longer bounds
                             * anything (reference model 5, contrast 1e10: scaled residual 7e-11 at a velocity error of 4e-3), so
                             * systems the banded LU can hold go there up front and every result is judged by its UNSCALED
                             * residual: error_estimate = max(nz, nx) |b - A x|_2 / |b - A x_hydrostatic|_2, converged iff that is
                             * <= 1e-6 as well.  0 when not evaluated (heat, or the solve ended otherwise) */
} pl_solve_stats;

/* ---- context --------------------------------------------------------------------- */
/* Global grid of nz x nx nodes with node coordinates zc[nz], xc[nx] (non-uniform
 * allowed for Stokes/heat; MIC requires a regular grid like the reference,
 * pylamp_trac.py:34,162).  The context owns all device memory and one HIP stream. */
int  pl_create(pl_ctx** out, int device, int nz, int nx, const double* zc, const double* xc);
void pl_destroy(pl_ctx* ctx);
const char* pl_last_error(const pl_ctx* ctx);   /* ctx may be NULL: error of a failed pl_create */
int  pl_sync(pl_ctx* ctx);                      /* hipStreamSynchronize on the context stream */
int  pl_device_info(pl_ctx* ctx, char* name, size_t name_len, int* cu_count, size_t* hbm_bytes);

/* ---- multi-GPU: one context per rank, 2-D block decomposition of the node grid ---------------------------------
 * The reference only strides tracers over MPI ranks and replicates every grid array
 * (pylamp2.py:30-32,445-455,550-555); here the grid itself is decomposed into Pz x Px blocks (1x2, 2x2, 2x4 ...).
 * Rank r = pz * Px + px owns node rows [pz*Cz, (pz+1)*Cz) and columns [px*Cx, (px+1)*Cx), Cz = (nz-1)/Pz,
 * Cx = (nx-1)/Px (the last block of an axis also owns the last node row / column); (nz-1) and (nx-1) must be
 * divisible by Pz resp. Px, with even quotients >= 8.  Every plane carries a halo ring filled from the (up to 8)
 * neighbour blocks, corners included (the momentum stencils reach (i-1,j+1) and (i+1,j-1)).
 * Transports: (a) direct RCCL calls on the context stream (opt-in, PYLAMP_RCCL=1, self-tested at start-up);
 * (b) this callback table into the host program (torch.distributed in pylamp_amd/parallel.py); (c) an in-process
 * group of "virtual ranks" sharing one GPU, one host thread per context (pl_local_group_*; tests and rehearsals).
 * Every callback returns 0 on success and must have completed when it returns.  Device pointers are plain HIP
 * allocations of this context's device. */
typedef struct pl_comm_ops {
    /* nmsg point-to-point messages: message k sends nsend[k] doubles at send[k] to rank peer[k] and receives nrecv[k]
     * doubles into recv[k] from it (either count may be 0).  Messages between the same pair of ranks are matched in
     * list order; both sides list them in the same order. */
    int (*sendrecv)(void* user, int nmsg, const int* peer, const double* const* send, const int64_t* nsend,
                    double* const* recv, const int64_t* nrecv);
    /* In-place all-reduce of n doubles in HOST memory; op: 0 sum, 1 min, 2 max. */
    int (*allreduce_host)(void* user, double* buf, int64_t n, int op);
    /* All-gather: every rank contributes count doubles at send; recv receives nranks*count (rank r at r*count). */
    int (*allgather)(void* user, const double* send, double* recv, int64_t count);
    void* user;
} pl_comm_ops;
/* Right after pl_create.  Pz * Px must equal nranks; pl_set_comm chooses the layout itself: PYLAMP_DECOMP="PzxPx",
 * otherwise the most square one with Px >= Pz (2 -> 1x2, 4 -> 2x2, 8 -> 2x4). */
int  pl_set_comm(pl_ctx* ctx, int rank, int nranks, const pl_comm_ops* ops);
int  pl_set_comm_2d(pl_ctx* ctx, int rank, int Pz, int Px, const pl_comm_ops* ops);
int  pl_local_rows(pl_ctx* ctx, int* first_row, int* n_rows);
int  pl_local_block(pl_ctx* ctx, int* first_row, int* n_rows, int* first_col, int* n_cols, int* Pz, int* Px);
/* In-process group of virtual ranks: create one group, then one context per rank (same or different devices), attach
 * each with pl_set_comm_local and drive every context from its OWN host thread (the calls are collective and block
 * until all ranks of the group have entered them). */
typedef struct pl_local_group pl_local_group;
int  pl_local_group_create(pl_local_group** out, int nranks);
void pl_local_group_destroy(pl_local_group* g);
void pl_local_group_abort(pl_local_group* g);    /* a rank's driver thread failed: every collective call of the group returns an error */
int  pl_set_comm_local(pl_ctx* ctx, pl_local_group* g, int rank, int Pz, int Px);
/* Bracket a rank thread's stretch of library calls.  No-ops unless PYLAMP_LOCAL_SERIAL=1 was set when the group was created: then the
 * group has ONE GPU token, held by the thread that runs and handed over (stream drained) while it waits inside a collective call, so
 * that the kernels of virtual ranks sharing a GPU never overlap -- a kernel trace then shows their true durations. */
void pl_local_group_enter(pl_local_group* g);
void pl_local_group_leave(pl_local_group* g, pl_ctx* ctx);
/* *native = 1 when the exchanges run as direct RCCL calls on the context stream (dlopen'ed librccl, self-tested at
 * pl_set_comm), 2 for the in-process group, 0 when they go through the callback table.
 * The native path is opt-in: PYLAMP_RCCL=1 (bench.py sets it for --transport native only; it has not run on a multi-GPU node yet). */
int  pl_comm_info(pl_ctx* ctx, int* rank, int* nranks, int* native);
/* Cumulative numbers of communication calls of this context: out[0] neighbour (halo) exchanges, [1] all-gathers,
 * [2] device all-reduces, [3] host all-reduces; reset != 0 clears the counters after reading. */
int  pl_comm_stats(pl_ctx* ctx, int64_t out[4], int reset);
/* Milliseconds spent in them since the last reset: out_ms[0..2] device time between HIP events recorded around every neighbour
 * exchange (pack -> messages -> unpack), all-gather and device all-reduce on the context stream; out_ms[3] host wall time of
 * the host all-reduces.  Synchronises the stream. */
int  pl_comm_times(pl_ctx* ctx, double out_ms[4], int reset);
/* raw copies between host and this context's device memory (used by the gloo fallback of the
 * communication layer, which stages through host buffers) */
int  pl_memcpy_d2h(pl_ctx* ctx, void* dst_host, const void* src_dev, size_t bytes);
int  pl_memcpy_h2d(pl_ctx* ctx, void* dst_dev, const void* src_host, size_t bytes);
int  pl_dev_add(pl_ctx* ctx, double* dst_dev, const double* src_dev, int64_t n);   /* dst += src */

/* HIP-event timing on the context's stream (bench.py measures kernels with these). */
int  pl_timer_start(pl_ctx* ctx);
int  pl_timer_stop_ms(pl_ctx* ctx, double* ms);

/* ---- Stokes: replaces makeStokesMatrix (pylamp_stokes.py:104-563) + the spsolve call
 *      site pylamp2.py:360 ------------------------------------------------------------ */
/* Upload viscosity/density and fix the operator.  bc = [z0, x0, zL, xL]
 * (index DIM*wall+dir as in pylamp_stokes.py:163,202,242,289).  Computes Kcont/Kbond
 * exactly as pylamp_stokes.py:116-122.  surfstab != 0 adds the stabilisation terms of
 * pylamp_stokes.py:422-426,483-487 with the given tstep and theta.  The terms are linear in
 * theta; the reference's sign makes them ANTI-stabilising (they reduce the momentum diagonal, see
 * DESIGN.md section 5), a negative theta gives the damping sign of Duretz et al. (2011). */
int  pl_stokes_set_coeffs(pl_ctx* ctx, const double* etas, const double* etan, const double* rho,
                          const int bc[4], int surfstab, double tstep, double theta);
int  pl_stokes_get_scaling(pl_ctx* ctx, double* kcont, double* kbond);
/* y = A x, matrix-free (what A@x would give for the lil_matrix the reference builds). */
int  pl_stokes_apply(pl_ctx* ctx, const double* x, double* y);
/* rhs vector of makeStokesMatrix (pylamp_stokes.py:429,490). */
int  pl_stokes_rhs(pl_ctx* ctx, double* rhs);
/* r = rhs - A x in double-double arithmetic from the probed entries of the operator (what A.tocsc() holds), rounded once;
 * one rank.  The residual of the direct solve's refinement (diagnostic entry). */
int  pl_stokes_residual_dd(pl_ctx* ctx, const double* rhs, const double* x, double* r);
/* The last banded LU of this context: storage rows 2 kl + ku + 1, panel width, factorisation ms, triangular-solve ms (summed;
 * timed under PYLAMP_SOLVER_TRACE only) and the number of solves.  Zeros when there is none. */
int  pl_stokes_direct_info(pl_ctx* ctx, int* band, int* nb, double* factor_ms, double* solve_ms, int* nsolve);
/* x = A^-1 rhs by preconditioned BiCGStab (replaces spsolve, pylamp2.py:360,394).
 * rhs == NULL uses the operator's own rhs.  x is output only (initial guess 0) unless
 * use_x0 != 0.
 * Stopping rule: the solve ends when BOTH the true relative residual is <= rtol AND the estimated relative velocity error
 * (pl_solve_stats.error_estimate) is <= 3e-8.  It is an estimate, not a bound: against direct solves it has been seen up to 6 x (10^3
 * block, cold start) and 12 x (sphere at contrast 1e5) below the true error, so 3e-8 leaves a factor of 30 to the 1e-6 the drop-in
 * promises against the reference's direct solve (measured true errors: 1e-9 ... 2e-7).  The Python layers pass rtol = 1e-7 by default; a smaller rtol is honoured as a residual bound. */
int  pl_stokes_solve(pl_ctx* ctx, const double* rhs, double* x, int use_x0, double rtol,
                     int maxit, pl_solve_stats* stats);
/* Times `reps` back-to-back applies of the device-resident operator on device-resident
 * vectors with HIP events (no host transfers); returns average ms per apply. */
int  pl_stokes_apply_bench(pl_ctx* ctx, int reps, double* avg_ms);
/* the same for the row-scaled operator y = D_r A x, the variant the Krylov solver launches */
int  pl_stokes_apply_scaled_bench(pl_ctx* ctx, int reps, double* avg_ms);
/* stream triad a = b + s c on three device arrays of n doubles (24 n bytes per launch): measured HBM rate of the box */
int  pl_stream_triad_bench(pl_ctx* ctx, int64_t n, int reps, double* avg_ms);

/* Diagnostics for component tests of the solver: z = M^-1 r for an UNSCALED residual r in
 * the reference DOF order (builds the multigrid hierarchy for the current coefficients; the
 * wall/slave/ghost velocity rows of r are ignored - they are identically zero in the solver), and
 * the hierarchy's level count / per-level Chebyshev lambda_max. */
int  pl_stokes_precond_apply(pl_ctx* ctx, const double* r, double* z);
/* One launch of the operator with a reduction epilogue, as the Krylov solver uses it (PYLAMP_KRYLOV_FUSED), for the UNSCALED
 * operator of pl_stokes_apply on host vectors.  mode 1: out = A x, sums[0] = aux1 . out.  mode 2: out = A x, sums[0..7] = out.aux1,
 * out.out, aux2.aux1, aux2.out, aux1.aux1, then out.aux1, out.out, aux1.aux1 over the continuity rows.  mode 3: out = aux1 - A x,
 * out2 (may be NULL) = A x, sums[0..4] = |out|^2, its continuity part, |aux1|^2, the sum of (x + aux2)^2 over the velocities
 * (aux2 may be NULL), the deflation's weighted sum of the continuity rows of out.  rows: row-block height of the launch
 * (4 or 16; 0: the default of the grid size).  sums holds 8 doubles. */
int  pl_stokes_apply_reduce(pl_ctx* ctx, int mode, int rows, const double* x, const double* aux1, const double* aux2,
                            double* out, double* out2, double* sums);
/* One launch of the Stokes stencil exactly as pl_stokes_solve issues it, on host vectors in the reference's DOF order.
 * scaled: 0 the operator of pl_stokes_apply, 1 the row-scaled one the solver iterates on.
 * mode 0..3 (0: out = op(x) alone; 1..3 as above); rows: 0 | 2 | 4 | 8 | 16 for mode 0, 0 | 4 | 16 otherwise.
 * add (may be NULL): out = op(x) + coef * add, added after the row scaling as in the solver (the lazy deflation correction).
 * aux1 / aux2 / out2 / sums (8 doubles) as above; for mode 0 they may be NULL.  One rank only. */
int  pl_stokes_apply_probe(pl_ctx* ctx, int scaled, int mode, int rows, const double* x, const double* aux1,
                           const double* aux2, const double* add, double coef, double* out, double* out2, double* sums);
/* out = D_r v by the solver's own kernel: the scaling the right-hand side gets before the Krylov iteration.  One rank only. */
int  pl_stokes_scale_rows(pl_ctx* ctx, const double* v, double* out);
int  pl_stokes_mg_info(pl_ctx* ctx, int* nlevels, double* lmax, int max_levels);
/* What the last hierarchy build and preconditioner application chose (read-only; any pointer may be NULL): smoother[l] of each of the
 * first max_levels levels (-1 point Jacobi, 0 z-lines, 1 x-lines), nu[4] = sweeps (pre, post, pre of level 0, post of level 0), the
 * Chebyshev ratio of the smoothing window, and whether stage 1 applies the wall stencils of the pressure block. */
int  pl_stokes_mg_plan(pl_ctx* ctx, int* smoother, int max_levels, int* nu, double* ratio, int* wall_ps);
/* Average duration (HIP events) of one Chebyshev smoothing sweep on the finest multigrid level -- the kernel
 * with the largest share of a time step (80 B/node algorithmic).  Call after at least one solve. */
int  pl_stokes_sweep_bench(pl_ctx* ctx, int reps, double* avg_ms);
/* Precision of the velocity-block multigrid of the last solve: the first *nlevels_fp32 of the *nlevels levels store and
 * sweep in FP32 (the large, bandwidth-bound ones; off by default, PYLAMP_MG_FP32=1 or pl_stokes_set_mg_precision).  BiCGStab, the operator and
 * the stopping test are FP64 always: the V-cycle only approximates A_vv^-1.  pl_stokes_sweep_bench times the finest
 * level in the precision reported here (40 B/node algorithmic in FP32, 80 in FP64). */
int  pl_stokes_mg_precision(pl_ctx* ctx, int* nlevels, int* nlevels_fp32);
/* fp32 = 0: all levels FP64 (default); 1: the large levels in FP32.  min_nodes > 0: smallest level, in nodes of the rank's block, that
 * runs in FP32 (default 200000: smaller levels are launch-latency bound and gain nothing). */
int  pl_stokes_set_mg_precision(pl_ctx* ctx, int fp32, long long min_nodes);
/* Launches of the one-workgroup V-cycle tail on this context so far: *lds those of k_mg_tail_lds (levels in LDS, rows in registers),
 * *global those of k_mg_tail (levels in global memory: several ranks, PYLAMP_MG_FUSED=0, or a tail that does not fit the LDS pool). */
int  pl_mg_tail_launches(pl_ctx* ctx, long long* lds, long long* global);

/* ---- Heat: replaces makeDiffusionMatrix (pylamp_diff.py:85-183) + spsolve
 *      (pylamp2.py:419) --------------------------------------------------------------- */
int  pl_heat_set_coeffs(pl_ctx* ctx, const double* zmp, const double* xmp, const double* T,
                        const double* kz, const double* kx, const double* cp, const double* rho,
                        const double* H, const int bc[4], const double bcvalue[4], double tstep);
int  pl_heat_apply(pl_ctx* ctx, const double* x, double* y);
int  pl_heat_rhs(pl_ctx* ctx, double* rhs);
int  pl_heat_solve(pl_ctx* ctx, const double* rhs, double* x, double rtol, int maxit,
                   pl_solve_stats* stats);
int  pl_heat_apply_bench(pl_ctx* ctx, int reps, double* avg_ms);
/* Launches of the several-sweeps-per-launch Chebyshev kernel (k_heat_cheb_fused; one rank, PYLAMP_HEAT_FUSE unset or non-zero) by the
 * heat solves of this context so far, pl_step's included: 0 where every sweep was a launch of its own. */
int  pl_heat_fused_launches(pl_ctx* ctx, long long* n);

/* ---- Marker-in-cell: replaces pylamp_trac.trac2grid / grid2trac / RK ----------------- */
/* Tracer -> grid (pylamp_trac.py:161-318, method ELEM).  tr_x is (n,2) [z,x]; tr_f is
 * (n,nf) with leading dimension ld_f; target node set given by its first coordinate and
 * spacing per axis (any of the 4 staggerings; regular grid); out[k] are nf host arrays
 * (nz,nx) written in place.  Nodes outside [0,nz)x[0,nx) are discarded, which is what
 * the reference's grid extension + crop (pylamp_trac.py:207-220,313-316) amounts to. */
int  pl_trac2grid(pl_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f, int64_t ld_f,
                  int nf, const int* avgscheme, double z0, double hz, double x0, double hx,
                  double* const* out);
/* Rectilinear (non-uniform) grids, SURVEY 8 f4 -- beyond the reference, whose marker code is regular-grid
 * only (it picks the cell with the regular-grid formula, pylamp_trac.py:46-47,226-227).  pl_trac2grid_rect takes
 * the coordinates zc[nz], xc[nx] of the target node set and locates cells by per-axis search (outside the
 * axis the grid continues with the spacing of its end cell, as the reference's extension does).
 * pl_mic_set_search(ctx, 1) makes pl_grid2trac and pl_rk4 locate cells the same way in their gz/gx arrays;
 * 0 (default) restores the reference's formula.  On a uniform grid both give the same result. */
int  pl_trac2grid_rect(pl_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f, int64_t ld_f,
                       int nf, const int* avgscheme, const double* zc, const double* xc, double* const* out);
int  pl_mic_set_search(pl_ctx* ctx, int on);
/* Grid -> tracer (pylamp_trac.py:30-158).  fields: nf host arrays (gnz,gnx) on the regular
 * grid gz[gnz], gx[gnx]; out is (n,nf) with leading dimension ld_out (may be a strided
 * view like pylamp2.py:445).  *n_outside returns how many tracers used defval; with
 * stop_on_error != 0 and any outside the call fails (pylamp_trac.py:53-54). */
int  pl_grid2trac(pl_ctx* ctx, int64_t n, const double* tr_x, int nf, const double* const* fields,
                  int gnz, int gnx, const double* gz, const double* gx, int method, double defval,
                  int stop_on_error, double* out, int64_t ld_out, int64_t* n_outside);
/* RK(order=4) (pylamp_trac.py:347-388): vels are (gnz,gnx) on gz,gx (the padded
 * cell-centre grid, pylamp2.py:491-545).  v_out, x_out are (n,2). */
int  pl_rk4(pl_ctx* ctx, int64_t n, const double* tr_x, int gnz, int gnx, const double* gz,
            const double* gx, const double* vz, const double* vx, double tstep, double* v_out,
            double* x_out);

/* ---- Device-resident time step (the build's counterpart of pylamp2.py:273-581) ------- */
typedef struct pl_step_config {
    int    do_heatdiff, do_subgrid_heatdiff, tdep_rho, tdep_eta;
    double etamin, etamax, tref;
    double tstep_adv_max, tstep_adv_min, tstep_dif_max, tstep_dif_min, tstep_modifier;
    int    bcstokes[4];
    int    bcheat[4];
    double bcheatvals[4];
    double stokes_rtol, heat_rtol;
    int    stokes_maxit, heat_maxit;
    double length[2];               /* domain size L[z], L[x] (pylamp2.py:38) */
    /* Tracer census + injection at the end of the step (pylamp2.py:588-633): cells holding fewer
     * than tracdens_min tracers are refilled to tracdens with tracers at (seeded) random positions
     * whose 12 fields are the plain mean of the tracers already in the cell.  tracdens_min <= 0
     * disables it.  IDs follow the reference (pylamp2.py:621-622): the first new ID of every refilled cell repeats
     * the last ID handed out; inject_unique_ids != 0 continues after the current maximum instead.  Positions come
     * from a counter-based generator seeded with inject_seed (the reference draws from numpy's global stream). */
    int    tracdens, tracdens_min;
    uint64_t inject_seed;
    /* Free-surface stabilisation (pylamp2.py:71-73,352-355,368-372,387-405): with
     * surfstab_tstep < 0 the Stokes system is re-assembled with the chosen time step and re-solved
     * until the step no longer shrinks (limiter 's' = the reference's "Ss").  surfstab_theta < 0
     * selects the corrected (damping) sign, see pl_stokes_set_coeffs. */
    int    surface_stabilization;
    double surfstab_theta, surfstab_tstep;
    int    inject_unique_ids;       /* see tracdens above */
    /* pylamp2.py:41,563-581: with the fence off a tracer at or beyond a wall is deleted (TR__ID = -1 -> np.delete)
     * instead of being put back EPS inside the wall.  0 = fence on (the reference's default). */
    int    tracs_fence_disabled;
} pl_step_config;

typedef struct pl_step_report {
    double tstep;                   /* chosen time step (pylamp2.py:374-385) */
    int    limiter;                 /* 'H', 'S' or 's' (= "Ss") */
    double tstep_heat, tstep_stokes;
    pl_solve_stats stokes, heat;
    double ms_props, ms_scatter, ms_stokes, ms_heat, ms_gather, ms_advect, ms_sort, ms_total;
    int64_t ntrac;                  /* tracers on this rank after the step (incl. injected) */
    int64_t ninjected;              /* tracers injected on this rank at the end of this step */
    int     stokes_resolves;        /* extra Stokes solves of the surface-stabilisation loop */
    int64_t nremoved;               /* tracers deleted on this rank at the end of this step (fence off) */
} pl_step_report;

/* Upload tracer state: tr_x (n,2), tr_f (n,13) AoS rows as in pylamp_const.py:29-42. */
int  pl_tracers_upload(pl_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f);
int  pl_tracers_download(pl_ctx* ctx, int64_t n, double* tr_x, double* tr_f);
int  pl_tracers_count(pl_ctx* ctx, int64_t* n);
/* Census of the resident tracers (pylamp2.py:588-598: np.bincount of the cell index): counts[c] for this rank's
 * owned cells, row-major (n_cell_rows x (nx-1)), ncells = their number.  counts == NULL only queries the rows. */
int  pl_tracers_census(pl_ctx* ctx, int64_t ncells, int32_t* counts, int* first_cell_row, int* n_cell_rows);
/* Layout of the resident tracer columns (tests; no counterpart in the reference, whose tracers are plain NumPy rows).  The
 * end-of-step sort of the resident step moves only positions, temperature and a 4-byte slot per tracer:
 *   *epoch_age > 0: the ten columns no stage writes (everything but TR_RHO, TR_ETA, TR_TMP) are still in the order of the sort
 *                   that opened the epoch, *epoch_age sorts ago, and are read through the slot index;
 *   *lazy != 0:     TR_RHO, TR_ETA and the tracer velocities have not been moved by the last sort yet.
 * Downloads (pl_tracers_download, pl_get_tracer_velocity) bring every column into the current order first. */
int  pl_tracers_layout(pl_ctx* ctx, int* epoch_age, int* lazy);
/* One full time step on the device-resident state (pylamp2.py:284-583: properties, tracer -> grid, Stokes, time step, heat,
 * grid -> tracer with subgrid diffusion, RK4 advection, census + injection).  The iterative solves are warm-started from the
 * context's own history -- Stokes from the polynomial through its last three solutions evaluated at the new model time, heat
 * from the old nodal temperature plus the last increment scaled by the time-step ratio; pl_tracers_upload forgets the history.
 * The stopping rules are those of pl_stokes_solve / pl_heat_solve whatever the start, so the reference's results are reproduced
 * within the solver tolerances either way (PYLAMP_X0_EXTRAP=0 / PYLAMP_HEAT_X0=0 start from the last solution / from zero). */
int  pl_step(pl_ctx* ctx, const pl_step_config* cfg, int it, pl_step_report* rep);
/* The marker stages of pl_step ONE AT A TIME on the resident, cell-sorted tracers (one rank) -- the same functions and kernels
 * the timed step runs (fused k_scatter_cells, k_gather<true, 0|1|2>, k_rk4<true>), so that tests can pin them directly against
 * the reference's fixtures (pylamp_trac.py:161-318 trac2grid, :30-158 grid2trac, :321-388 RK) instead of through trajectories.
 * pl_resident_scatter: properties + the step's tracer -> grid calls (pylamp2.py:291-319); results by pl_get_field ("rho", "etas",
 *   "etan", "cp", "f_T", "H", "mat", "kz", "kx").
 * pl_resident_temp_to_tracers: pylamp2.py:436-480 with the new nodal temperature newtemp (nz,nx); the old nodal temperature is
 *   the plane "f_T" of the last scatter; first != 0 is the it == 1 branch; results in column TR_TMP (pl_tracers_download).
 * pl_resident_rk4: RK4 through vz_pad, vx_pad on the padded (nz+1, nx+1) centre grid (pylamp2.py:547-572, fence optional), then
 *   the end-of-step cell sort; positions by pl_tracers_download, velocities by pl_get_tracer_velocity. */
int  pl_resident_scatter(pl_ctx* ctx, const pl_step_config* cfg, int it);
int  pl_resident_temp_to_tracers(pl_ctx* ctx, const pl_step_config* cfg, int first, const double* newtemp, double tstep);
int  pl_resident_rk4(pl_ctx* ctx, const double* vz_pad, const double* vx_pad, double tstep, int fence, const double length[2]);
/* Copy a named grid field of the last step to host, shape (nz,nx): "velz","velx","pres",
 * "rho","etas","etan","temp","f_T","kz","kx","cp","H". */
int  pl_get_field(pl_ctx* ctx, const char* name, double* out);
/* Velocity of the last advection, (n,2) like trac_vel (pylamp2.py:547-555). */
int  pl_get_tracer_velocity(pl_ctx* ctx, int64_t n, double* out);

/* ---- 3-D staggered Stokes + heat (BASELINE config 5) ----------------------------------------------------------------
 * PARITY UNPINNED: the reference implements DIM = 2 only (pylamp_const.py:6; pylamp_stokes.py:30-35 prints "NOT
 * IMPLEMENTED" for dim != 2).  It fixes the intent -- axis order z, x, y (pylamp_const.py:9-13), arrays (nz, nx, ny),
 * IP = DIM, DOF order iz*nx*ny*4 + ix*ny*4 + iy*4 + ieq (pylamp_stokes.py:24) -- and these entry points extend the 2-D
 * rows (pylamp_stokes.py:376-518, pylamp_diff.py:99-179) dimension by dimension: a y-invariant extrusion reproduces the
 * 2-D operator and solution on every y-slice.  Host arrays are C-order (nz, nx, ny) doubles; Stokes vectors are
 * (nz, nx, ny, 4) with components (vz, vx, vy, P).  Walls are numbered [z0, x0, y0, zL, xL, yL]: Stokes walls FREESLIP (the
 * default) or NOSLIP per wall (pl3_stokes_set_walls), heat walls FIXTEMP / FIXFLOW.  The shear viscosity is given at the NODES
 * and averaged onto the edges. */
typedef struct pl3_ctx pl3_ctx;
int  pl3_create(pl3_ctx** out, int device, int nz, int nx, int ny, const double* zc, const double* xc, const double* yc);
void pl3_destroy(pl3_ctx* ctx);
const char* pl3_last_error(const pl3_ctx* ctx);
/* Several ranks (BASELINE config 5: "1 -> 8 MI355X"; the reference has no 3-D code at all, pylamp_const.py:6, pylamp_stokes.py:24-35):
 * right after pl3_create -- with the GLOBAL grid on every rank -- this context becomes one block of a Pz x Px x Py decomposition of
 * the node grid, rank = (pz Px + px) Py + py, (n - 1) divisible by the block count along every axis, >= 4 cells per block.  `comm`
 * is a 2-D context (pl_create on any small grid) that carries the transport: its pl_set_comm / pl_set_comm_2d / pl_set_comm_local must
 * have been called with Pz * Px * Py ranks, and it must outlive this context (whose stream it shares from then on).  Host arrays stay
 * GLOBAL on every rank (the block and the one ring of halo nodes the stencils reach are cut out of them; results are assembled).
 * Every pl3_* call that follows is collective.  Halo: one node deep, exchanged axis by axis (z, x, y planes: 6 messages carry faces,
 * edges and corners); every multigrid level is distributed (blocks halved with the grid), dot products are all-reduced on the host. */
int  pl3_set_comm(pl3_ctx* ctx, pl_ctx* comm, int Pz, int Px, int Py);
int  pl3_local_block(pl3_ctx* ctx, int first[3], int count[3]);
/* out[0] halo exchanges, out[1] host all-reduces of this context so far; reset != 0 clears the counters */
int  pl3_comm_stats(pl3_ctx* ctx, int64_t out[2], int reset);
/* grav = G[3] (NULL: (9.81, 0, 0), pylamp_const.py:21); Kcont = 3 min(eta) / sum(avgd), Kbond = 9 min(eta) / sum(avgd)^2 */
int  pl3_stokes_set_coeffs(pl3_ctx* ctx, const double* etas, const double* etan, const double* rho, const double grav[3]);
/* slaved != 0 (default): the reference's wall rows extended to 3-D (outermost in-domain tangential velocities slaved to their
 * inner neighbours, pylamp_stokes.py:170-175 ...: first-order accurate at the walls); 0: natural mirror rows (second order) */
int  pl3_stokes_set_wall_rows(pl3_ctx* ctx, int slaved);
/* bc[6] = [z0, x0, y0, zL, xL, yL], each PL_BC_FREESLIP or PL_BC_NOSLIP; any other kind is an error that names the wall and the
 * value.  The setting belongs to the context (all free-slip at creation), survives pl3_stokes_set_coeffs and is read by the solves,
 * pl3_resident_step and pl3_advection_velocity.  The rows, with (D, E, F) a cyclic permutation of (z, x, y), v_D tangential to the
 * walls of E and F, and per axis rd[i] = 1/(c[i+1] - c[i]), rD[i] = 1/(c[i+1] - c[i-1]):
 *  - identity rows (wall-normal velocities, ghosts, anchor), pressure rows and the right-hand side do not depend on the kind;
 *  - slaved rows (pl3_stokes_set_wall_rows(1), finest level): a v_D on the outermost in-domain layer couples to its inward neighbour
 *    v_nb along the first boundary axis a, E before F, and the kind of THAT wall sets the coefficients: FREESLIP Kcont (v - v_nb);
 *    NOSLIP the reference's extrapolation row (pylamp_stokes.py:165-166, 204-205), low side
 *    Kcont [-(rD_a[1] + rd_a[0]) v + rD_a[1] v_nb], high side Kcont [(rD_a[n-2] + rd_a[n-2]) v - rD_a[n-2] v_nb]: v_D extrapolated
 *    linearly to the wall is zero (uniform grid: v = v_nb / 3).  Row scale 1 / (Kcont x the coefficient of v);
 *  - natural rows (pl3_stokes_set_wall_rows(0), every coarse multigrid level): on an edge of a NOSLIP wall the shear stress keeps both
 *    halves, dv_D/dx_E one-sided against v_D = 0 on the wall -- low side v_D[0] / ((c_E[1] - c_E[0]) / 2), high side
 *    -v_D[n-2] / ((c_E[n-1] - c_E[n-2]) / 2) -- and dv_E/dx_D as on a FREESLIP wall, which drops the first half. */
int  pl3_stokes_set_walls(pl3_ctx* ctx, const int bc[6]);
/* Moving walls.  vel[18]: vel[3 w + q] is component q of U_w = (Uz, Ux, Uy) of wall w of [z0, x0, y0, zL, xL, yL]; every wall is at
 * rest at creation.  Only the two components tangential to the wall may be non-zero, and only on a NOSLIP wall.  Errors, each naming
 * the wall and the value: a non-finite entry; a non-zero normal component (flow through a wall needs the marker deletion path, which
 * is not built in 3-D); a non-zero velocity on a FREESLIP wall; and pl3_stokes_set_walls turning a moving wall FREESLIP.  The state
 * belongs to the context, survives pl3_stokes_set_coeffs like the kinds, and is read by pl3_stokes_rhs, the solves of the operator's
 * own right-hand side, pl3_resident_step and pl3_advection_velocity.  With all velocities zero everything is bit for bit what it is
 * without this call.  The terms are affine -- the operator, its row scaling, the multigrid hierarchy and a right-hand side given to
 * pl3_stokes_solve are untouched -- and enter the right-hand side alone:
 *  - slaved rows: a v_D slaved along axis a at a NOSLIP wall keeps its row and gains a right-hand side, so that the row states "v_D
 *    extrapolated linearly to the wall is U_D": low side Kcont [-(rD_a[1] + rd_a[0]) v + rD_a[1] v_nb] = -Kcont rd_a[0] U_D, high side
 *    Kcont [(rD_a[n-2] + rd_a[n-2]) v - rD_a[n-2] v_nb] = +Kcont rd_a[n-2] U_D; scaled, v - gamma v_nb = (1 - gamma) U_D.  A row on
 *    a cube edge is slaved along its first boundary axis only (E before F), and the wall it is slaved to supplies U;
 *  - natural rows: the one-sided dv_D/dx_E on the edge of a NOSLIP wall is taken against v_D = U_D on the wall; the constant part of
 *    2 eta_edge rd_E^2 (v_D - U_D) goes to the right-hand side, -2 eta_edge rd_E^2 U_D; on a cube edge both walls contribute;
 *  - identity rows, pressure rows and all coarse levels are unchanged: corrections are homogeneous. */
int  pl3_stokes_set_wall_velocity(pl3_ctx* ctx, const double vel[18]);
int  pl3_stokes_get_wall_velocity(pl3_ctx* ctx, double vel[18]);
/* Flow through walls.  flow[w] is the plane Un_w of wall w over its FACES (the layout of every wall plane -- wall order, the axes p < q,
 * faces and nodes, C order, who owns the edges -- is in DESIGN.md section 6c, "Wall planes"): the wall-normal velocity on each face --
 * where v_a lives on that wall plane -- as the component along +a (the convention of pl3_stokes_set_wall_velocity): positive is inflow
 * on z0, x0, y0 and outflow on zL, xL, yL.  flow[w] == NULL: no flow through wall w;
 * all NULL (or flow == NULL) clears the setting, the state at creation.  A wall of either kind may carry a flow; a NOSLIP wall keeps
 * its tangential velocity, possibly zero.  The indices are GLOBAL: every rank of a pl3_set_comm decomposition is given the same six
 * planes.  The state belongs to the context, survives pl3_stokes_set_coeffs and pl3_stokes_set_walls, and is read by
 * pl3_stokes_rhs[_scaled], the solves of the operator's own right-hand side, pl3_resident_step and pl3_advection_velocity.
 *  - Matrix: unchanged.  So on the edge of a FREESLIP wall whose Un varies along the wall the rows keep their dv_a/dx half of the shear
 *    stress (the wall is free of the OTHER half only), and with slaved rows the cube-edge cells keep their pressure-symmetry rows in
 *    place of continuity.
 *  - Right-hand side: the identity rows of the wall-normal velocities -- component a at global index 0 or n_a - 1 along a and at most
 *    n_p - 2, n_q - 2 along p, q -- gain Kcont Un_w[i, j] (row-scaled: Un_w[i, j]); the ghost entries beyond stay 0 and no other row
 *    changes.  A right-hand side handed to pl3_stokes_solve stays as given.
 *  - Net flux: Phi = sum_w s_w sum_ij Un_w[i, j] dp_i dq_j with s = +1 on z0, x0, y0 and -1 on zL, xL, yL, summed in long double on
 *    the host.  |Phi| > 1e-10 sum |Un| dp dq is an error that gives Phi and the six wall fluxes: the pressure anchor cell would absorb
 *    Phi as a divergence (1e-10 is a thousand times below the solve's rtol of 1e-7 and far above the rounding of the sum).  Hence all
 *    six walls in one call.
 *  - Advection ghosts (pl3_advection_velocity, pl3_resident_step): the pass of a wall with a flow runs in its slot of the order z0 ..
 *    yL, even for a NOSLIP wall at rest.  From the neighbouring plane as it is at that moment it writes 2 Un_w[ci, cj] - V for the
 *    normal component (ci, cj: the padded tangential indices minus 1, clamped to [0, n - 2]), so that the velocity interpolated onto
 *    the wall is Un; tangential components are copied on a FREESLIP wall and follow 2 U_c - V on a NOSLIP wall.  Walls without a flow
 *    keep their arithmetic bit for bit.
 * Errors, a rejected call changing nothing: a NULL context; a non-finite entry (names the wall and the index); the net flux. */
int  pl3_stokes_set_wall_flow(pl3_ctx* ctx, const double* const flow[6]);
/* *mask: bit w set = wall w carries a flow; flow[w] != NULL receives the plane of such a wall, downloaded from the device (either
 * argument may be NULL) */
int  pl3_stokes_get_wall_flow(pl3_ctx* ctx, int* mask, double* const flow[6]);
int  pl3_stokes_get_scaling(pl3_ctx* ctx, double* kcont, double* kbond);
int  pl3_stokes_apply(pl3_ctx* ctx, const double* x, double* y);
int  pl3_stokes_rhs(pl3_ctx* ctx, double* rhs);
/* the same right-hand side row-scaled, as pl3_stokes_solve(rhs = NULL) iterates on it: every row divided by its coefficient of the
 * row's own unknown (interior momentum rows: by minus that coefficient, the sum of their own-component couplings) */
int  pl3_stokes_rhs_scaled(pl3_ctx* ctx, double* rhs);
/* x == NULL: device-resident solve -- nothing crosses PCIe, the solution stays in the context (pl3_get_solution), and use_x0 != 0
 * starts from the solution of the context's previous solve. */
int  pl3_stokes_solve(pl3_ctx* ctx, const double* rhs, double* x, int use_x0, double rtol, int maxit, pl_solve_stats* stats);
int  pl3_stokes_apply_bench(pl3_ctx* ctx, int scaled, int reps, double* avg_ms);     /* 80 B/node algorithmic */
int  pl3_stokes_mg_info(pl3_ctx* ctx, int* nlevels, double* lmax, int max_levels);
/* Diagnostics for component tests of the 3-D solver (the counterparts of pl_stokes_precond_apply / pl_stokes_mg_plan).
 * pl3_stokes_precond_apply: z = M^-1 r on host vectors (nz, nx, ny, 4); r is the ROW-SCALED residual exactly as the Krylov iteration
 * hands it to the preconditioner (rows without an equation are ignored).  Builds or refreshes the multigrid hierarchy as a solve does
 * (lmax is re-estimated), applies the solve's own preconditioner once without the deflation correction.  Collective on a context with
 * pl3_set_comm attached; every rank receives the global z.
 * pl3_stokes_mg_plan (read-only; any pointer may be NULL; valid once the hierarchy is built): nu[2] = Chebyshev sweeps before and after
 * the coarse correction on the finest level and on the other levels (the >= 10^6-node rule, PYLAMP_MG_NU3 / PYLAMP_MG_NU3_FINE), the
 * ratio lmax / lmin of their window, sweeps and ratio of the coarsest level, and lds[l] != 0 where the marching LDS kernels take level l. */
int  pl3_stokes_precond_apply(pl3_ctx* ctx, const double* r, double* z);
int  pl3_stokes_mg_plan(pl3_ctx* ctx, int* nu, double* ratio, int* coarse_sweeps, double* coarse_ratio, int* lds, int max_levels);
/* Diagnostics for component tests of the 3-D Krylov loop (tests/test_hip_3d_krylov.py).  Each runs the solve's own
 * kernels and host epilogues; none changes what pl3_stokes_solve computes.  Host vectors are (nz, nx, ny, 4), global on every rank.
 * pl3_stokes_precond_apply_deflated: as pl3_stokes_precond_apply, with the deflation correction of the last solve of this context (an
 *   error if that solve did not deflate).
 * pl3_krylov_probe: ONE launch of one Krylov kernel.  in[q], q < 10 (NULL: none), is uploaded into Stokes work vector q -- equal
 *   pointers share the work vector of the first -- and out[q] != NULL (out itself may be NULL) receives work vector q afterwards:
 *     PL3_PROBE_DOTS    scal[0] = nd products (1 .. 5) in[q] . in[5 + q] -> sums[0 .. nd - 1]; on a context with pl3_set_comm attached
 *                       the owned-nodes kernel and the all-reduce, as the solve chooses (collective)
 *     PL3_PROBE_DOTS11  the fused reduction (one rank): t, s, rt = in[0 .. 2]; x = in[3] or NULL; dx = in[4], NULL or in[3] itself; yw the
 *                       (nz, nx, ny) array or NULL -> sums[0 .. 10] = t.s, t.t, rt.s, rt.t, s.s | t.s, t.t, s.s of the pressure array |
 *                       |(x + dx)_vel|^2 | yw.s_p, yw.t_p
 *     PL3_PROBE_AXPBY   work 2 = scal[0] in[0] + scal[1] in[1]
 *     PL3_PROBE_P       p, r, v = in[0 .. 2], beta, omega = scal[0 .. 1]:  p = r + beta (p - omega v) in work 0
 *     PL3_PROBE_XR      x, y, z, r, s, t = in[0 .. 5], alpha, omega:  x += alpha y + omega z (work 0), r = s - omega t (work 3)
 *     PL3_PROBE_XRP     ... and p, v = in[6 .. 7], beta = scal[2]:  also p = r + beta (p - omega v) (work 6)
 *     PL3_PROBE_RANDOM  the shadow residual with seed scal[0] (the solve's is 1234) in work 0
 * pl3_stokes_hydrostatic: the scaled right-hand side and the hydrostatic start exactly as pl3_stokes_solve(rhs = NULL) runs them:
 *   xh = the start vector, *ref = the reference norm |b - A x_h| (0: not usable).  Collective on an attached context.
 * pl3_stokes_work_vector: Stokes work vector `index` as the last solve left it -- 0 the recurrence residual r, 1 the shadow residual,
 *   4 the last true residual, 8 the correction dx, 10 the scaled right-hand side, 13 the deflation vector w.
 * pl3_stokes_defl_info (about the last solve): out[0] a deflation vector is kept, [1] the deflation was on during the solve, [2] the
 *   quality |u - A w| / |u| measured on the kept vector (-1: none was), [3] iterations of the inner solve for w (0: reused as it is),
 *   [4] its final |u - A w| / |u| (-1: no inner solve), [5] yw.(A w), [6] |w_vel|^2, [7] the true-residual checks the solve took,
 *   [8] the iteration at which the estimate between the checks was last evaluated (0: never), [9] its value, [10 .. 14] what went into
 *   it: |r|^2 and |r_cont|^2 of the recurrence residual, |x_vel|^2, the anchor part, a_mom.
 *   u, yw (either may be NULL): the (nz, nx, ny) pressure plane of u and the weights yw of the deflation set-up.
 * pl3_stokes_ring_sum: sum |entry| over the ring and padding entries of the 14 Stokes work vectors of this rank's block.  On one rank
 *   the flat reductions rely on it being zero; on blocks the rings hold the neighbours' values (the sum is per rank, not reduced). */
enum { PL3_PROBE_DOTS = 0, PL3_PROBE_DOTS11 = 1, PL3_PROBE_AXPBY = 2, PL3_PROBE_P = 3, PL3_PROBE_XR = 4, PL3_PROBE_XRP = 5, PL3_PROBE_RANDOM = 6 };
int  pl3_stokes_precond_apply_deflated(pl3_ctx* ctx, const double* r, double* z);
int  pl3_krylov_probe(pl3_ctx* ctx, int what, const double* const in[10], const double* yw, const double scal[3], double* const out[10],
                      double* sums);
int  pl3_stokes_hydrostatic(pl3_ctx* ctx, double* xh, double* ref);
int  pl3_stokes_work_vector(pl3_ctx* ctx, int index, double* out);
int  pl3_stokes_defl_info(pl3_ctx* ctx, double out[15], double* u, double* yw);
int  pl3_stokes_ring_sum(pl3_ctx* ctx, double* out);
/* Warm start of pl3_stokes_solve from its solution history (opt-in, off at creation, one rank).  The context keeps the last `points`
 * committed solutions on the device (points x 32 B per padded node) and the model time steps between them.  A solve of the operator's
 * own right-hand side (rhs == NULL) with use_x0 == 0 then starts from the polynomial of degree `order` through (least squares: more
 * than order + 1 levels) those solutions, evaluated at the time of the solve, with the weights of the 2-D step (a time step that more
 * than doubled, or one older level only, falls back to the linear formula with its weight capped at 2).  The right-hand side, the
 * hydrostatic start and its reference norm `ref` are computed as in a cold solve, so the stopping test is the cold solve's.  Guard: if
 * ref is unusable or the scaled residual |r0| of the closed extrapolated start is not below ref, the solve falls back to the hydrostatic
 * start and is the cold solve bit for bit, counters included.  An accepted start hands its residual on to the iteration, so the guard
 * costs one reduction (and one operator application when the deflation vector had to be solved for anew in between).  With the warm
 * start off every solve launches what it launched before.  Explicit right-hand sides and use_x0 != 0 ignore it.
 * pl3_stokes_set_warm_start: points = 0 (off; frees the history) or 2 .. 6, order = 1 .. 3 with points >= order + 1; a change clears
 *   the history.  Errors name the argument; a context with pl3_set_comm attached is refused.
 * pl3_stokes_history_commit: the device solution of the last pl3_stokes_solve becomes the newest level; dt > 0 is the model time from
 *   it to the next solve.  Error: no solution yet, dt not positive.  Returns 0 and does nothing with the warm start off.
 *   pl3_resident_step commits with its time step.
 * pl3_stokes_history_clear: forgets the levels (the storage stays).  pl3_stokes_set_walls does it when a wall's kind changes;
 *   pl3_stokes_set_wall_velocity, pl3_stokes_set_wall_flow and pl3_stokes_set_coeffs keep the history.
 * pl3_stokes_history_info: out[0] levels held, [1] start of the last solve (0 cold: off or no history, 1 warm, 2 warm rejected by the
 *   guard), [2] levels it used, [3] |r0| of the warm candidate, [4] ref, [5 .. 7] the first three weights, newest level first.
 * pl3_stokes_start_vector: the linear combination as the next solve would form it, before the closure of the identity rows, as
 *   (nz, nx, ny, 4).  Error: warm start off or no level held. */
int  pl3_stokes_set_warm_start(pl3_ctx* ctx, int points, int order);
int  pl3_stokes_get_warm_start(pl3_ctx* ctx, int* points, int* order);
int  pl3_stokes_history_commit(pl3_ctx* ctx, double dt);
int  pl3_stokes_history_clear(pl3_ctx* ctx);
int  pl3_stokes_history_info(pl3_ctx* ctx, double out[8]);
int  pl3_stokes_start_vector(pl3_ctx* ctx, double* out);
int  pl3_heat_set_coeffs(pl3_ctx* ctx, const double* zmp, const double* xmp, const double* ymp, const double* T, const double* kz,
                         const double* kx, const double* ky, const double* cp, const double* rho, const double* H, const int bc[6],
                         const double bcvalue[6], double tstep);
int  pl3_heat_apply(pl3_ctx* ctx, const double* x, double* y);
int  pl3_heat_rhs(pl3_ctx* ctx, double* rhs);
/* rhs must be NULL (the operator's own right-hand side, pl3_heat_rhs); x == NULL keeps the solution on the device */
int  pl3_heat_solve(pl3_ctx* ctx, const double* rhs, double* x, double rtol, int maxit, pl_solve_stats* stats);
/* solution of the last solve of this context: which = 0 Stokes (nz, nx, ny, 4), 1 heat (nz, nx, ny) */
int  pl3_get_solution(pl3_ctx* ctx, int which, double* out);
/* Heat walls with a profile (one rank).  values[w] is the plane of wall w over its NODES ("Wall planes").
 * values[w] == NULL: the wall keeps the one
 * value bcvalue[w] of pl3_heat_set_coeffs; values == NULL or six NULL pointers clear the setting and free the planes, the state at
 * creation.  The state belongs to the context, survives pl3_heat_set_coeffs and is read whenever the right-hand side is formed:
 * pl3_heat_rhs, pl3_heat_solve and the heat solve of pl3_resident_step, which ignores cfg->bcheatvals[w] for a wall that has a plane.
 *  - Meaning: that of the scalar, by the wall's kind at the time the right-hand side is formed.  FIXTEMP: the temperature of the node.
 *    FIXFLOW: k dT/dx_a at the node, the derivative taken along +a on the low AND on the high wall.  So a positive entry is heat LEAVING
 *    through z0, x0, y0 (the temperature rises into the box) and heat ENTERING through zL, xL, yL: the heat flow into the box per area
 *    is -v on a low wall and +v on a high wall.  The row scaling of the solve is unchanged.
 *  - Entries of a plane at nodes another wall owns (the ownership of the rows, as in "Wall planes") are never read and not checked.
 *  - Without planes the right-hand side is formed by the kernel it was formed by before.
 * Errors, a rejected call changing nothing: a NULL context; a non-finite entry that is read (names the wall and the indices); a context
 * with pl3_set_comm attached. */
int  pl3_heat_set_wall_values(pl3_ctx* ctx, const double* const values[6]);
/* *mask: bit w set = wall w has a plane; values[w] != NULL receives the plane of such a wall, downloaded from the device (either
 * argument may be NULL) */
int  pl3_heat_get_wall_values(pl3_ctx* ctx, int* mask, double* const values[6]);
/* Heat budget of a temperature field under the operator of the last pl3_heat_set_coeffs / resident step (one rank).  T: a host
 * (nz, nx, ny) field, or NULL for the solution of the last pl3_heat_solve of this context, still on the device (whether or not it was
 * downloaded).  Every term is a sum over the INTERIOR nodes of the terms of their rows times the control volume.  With w_a[i] =
 * mp_a[i] - mp_a[i-1] for the midpoints mp given to pl3_heat_set_coeffs, V = w_z w_x w_y, rd_a[i] = 1 / (c_a[i+1] - c_a[i]), and k_a[i]
 * the conductivity on the face between the nodes i and i + 1 along a:
 *  - out[0 .. 5]: the heat flow INTO the box through z0, x0, y0, zL, xL, yL [W].  For a wall of axis a, summed over the nodes interior
 *    in the two other axes p, q:  low wall  - k_a[0] (T[1] - T[0]) rd_a[0] w_p w_q,  high wall  + k_a[n-2] (T[n-1] - T[n-2]) rd_a[n-2]
 *    w_p w_q -- the face fluxes the FIXFLOW rows prescribe.  The sums cover the control areas of the interior nodes: on a uniform grid
 *    (n_p - 2)(n_q - 2) faces of the wall, not the half cells along its rim.
 *  - out[6]: the storage rate  sum (T - T_old) / cdt V  with cdt = tstep / (rho Cp), that is rho Cp (T - T_old) / tstep V.
 *  - out[7]: the source  sum H V.
 * The wall terms telescope, so for any T that satisfies the interior rows  out[6] - out[7] - (out[0] + .. + out[5]) = 0  whatever the
 * kinds of the walls; for the result of a solve what remains is its residual.  One pass over the nodes, summed in a fixed order: two
 * calls give the same bits.
 * Errors name the entry: no heat operator set; T == NULL before any heat solve; a context with pl3_set_comm attached. */
int  pl3_heat_budget(pl3_ctx* ctx, const double* T, double out[8]);
/* Strain rate, deviatoric stress and viscous dissipation of a velocity field, as the operator's own rows define them (one rank).
 * vz, vx, vy: host (nz, nx, ny) arrays on the staggered positions of the solution vector; all three NULL: the solution of the last
 * pl3_stokes_solve of this context, still on the device.  strainrate, stress, dissipation: host (nz, nx, ny) node fields, total: the
 * integral of the dissipation over the box; any of them may be NULL.  The coefficients (pl3_stokes_set_coeffs), wall kinds, wall
 * velocities and wall flow currently set on the context are used.
 * The strain rates are those of the momentum rows, div(2 eta eps) written out; (D, E, F) is a cyclic permutation of (z, x, y), rd_A[i] =
 * 1 / (c_A[i+1] - c_A[i]), rD_A[i] = 1 / (c_A[i+1] - c_A[i-1]) inside and 0 on the two walls:
 *  - normal components at the cell centres, viscosity eta_n:  eps_DD = (v_D[i_D + 1] - v_D[i_D]) rd_D[i_D];
 *  - shear components on the edges: the edge of the pair (D, E) lies at node i_D, node i_E, cell i_F, its viscosity is the mean of the two
 *    nodal eta_s at its ends along F, and  eps_DE = 1/2 (g_DE + g_ED)  with  g_DE = dv_D/dx_E = 2 rD_E[i_E] (v_D[i_E] - v_D[i_E - 1])
 *    inside (v_D at the cells i_E, i_E - 1 of axis E).  On a wall of E: FREESLIP, g_DE = 0 (the zero-padded table, as in the rows);
 *    NOSLIP, the one-sided value against the wall's tangential velocity U_D (pl3_stokes_set_wall_velocity) that the natural rows use,
 *    2 rd_E[0] (v_D[0] - U_D) on the low wall and 2 rd_E[n_E - 2] (U_D - v_D[n_E - 2]) on the high one.  The same rule holds in strict mode
 *    (pl3_stokes_set_wall_rows) and on the cube edges, where v_D is a wall-normal velocity of the solution vector (0, or the through-flow).
 *  - no trace is removed: the flow is incompressible to the solver's tolerance.
 * A node field is the control-volume weighted mean around the node: the node's control volume reaches half a cell to either side (half
 * widths on the walls); a cell holds 1/8 of its volume in each corner's control volume, an edge's control volume (half a cell to either
 * side of its two nodes, its own length along F) is halved between its end nodes.  With < > that mean,
 *    dissipation = < 2 eta_n sum_D eps_DD^2 >_cells + < 4 eta_edge eps_DE^2 >_edges summed over the three pairs     [W/m^3]
 *    strainrate  = sqrt(1/2 (< sum_D eps_DD^2 >_cells + 2 sum_pairs < eps_DE^2 >_edges))                              [1/s]
 *    stress      = sqrt(1/2 (< (2 eta_n)^2 sum_D eps_DD^2 >_cells + 2 sum_pairs < (2 eta_edge eps_DE)^2 >_edges))     [Pa]
 * so that total = sum_nodes dissipation x V_node = the sum of the cell and edge dissipations times their volumes.  The sums run in a
 * fixed order without atomics: a call repeats bit for bit.  Work: two per-node kernels on Stokes work vectors 0 .. 2.
 * Errors (each names the entry): a context with pl3_set_comm attached; no coefficients set; NULL velocities before any solve; only some of
 * vz, vx, vy given. */
int  pl3_stokes_strain_fields(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double* strainrate, double* stress,
                              double* dissipation, double* total);
/* Yield stress (opt-in, off at creation; one rank): the viscosities the operator solves with are limited by a yield stress, from the strain
 * rates of a velocity field.
 * Symbols.  The material viscosities are etas (nodes) and etan (cell centres) as pl3_stokes_set_coeffs receives them.  eps_DD (centres) and
 * eps_DE (edges) are exactly the strain rates of pl3_stokes_strain_fields above, wall rules, moving walls and through-flow included.
 * Yield stress:      tau_y(z) = tau0 + dtau_dz (z - z[0]), z the coordinate along axis 0 (depth); evaluated at z_i for node i and at the
 *                    cell's mid-point (z[i] + z[i+1]) / 2 for the centres.
 * Node invariant:    e_n = the strainrate field of pl3_stokes_strain_fields (the same device function and order of summation: bit for bit).
 * Centre invariant:  e_c = sqrt(1/2 (sum_D eps_DD^2 + 2 sum_pairs m_p)), m_p the plain mean of eps_DE^2 over the cell's four edges of pair
 *                    p = (D, E): nodes i_D, i_D + 1 x i_E, i_E + 1, cell i_F.  Summation: pairs 0, 1, 2 ((z, x), (x, y), (y, z)); within a
 *                    pair D outermost, the lower index first.
 * Effective viscosity, nodes and centres alike:   eta_eff = min(eta_mat, max(tau_y / (2 e), eta_floor)).
 * It never raises a viscosity, is continuous in e, and is eta_mat where e = 0.  An entry is "yielded" when eta_eff < eta_mat.  Entries of
 * etan beyond the cells (the last index of an axis) keep the material value; nothing is written to the ring.
 * The effective viscosities are stateless: always derived from the material ones, never from the previous effective ones.  The context
 * keeps the material arrays next to the operator's once a yield stress is set; pl3_stokes_set_coeffs resets both to the material ones.
 *
 * pl3_stokes_set_yield(on, tau0, dtau_dz, eta_floor): on = 0 switches off (the operator takes the material viscosities again, the other
 * arguments are ignored).  Rejected by name: a context with pl3_set_comm attached; tau_y <= 0 anywhere between z[0] and z[n - 1];
 * eta_floor <= 0; non-finite values.  A change of the setting clears the warm-start history and makes the effective viscosities the
 * material ones.
 * pl3_stokes_yield_update(vz, vx, vy, out): the update for host velocities ((nz, nx, ny) each; all three NULL: the resident solution of
 * the last solve, with the rule and the errors of pl3_stokes_strain_fields).  Needs coefficients and a yield stress set.  It replaces the
 * operator's viscosities; out = { min eta_eff over nodes and centres (NaN rule of pl3_stokes_set_coeffs), change = max |ln(eta_new /
 * eta_prev)| over nodes and centres (eta_prev: the effective viscosities before the call), yielded nodes, yielded centres, max e_n,
 * max e_c }.  Unless the change is exactly 0 the operator's scaling follows the new minimum (Kcont, Kbond as in pl3_stokes_set_coeffs),
 * the next solve rebuilds the hierarchy, and the resident solution's Kcont-scaled pressure is rescaled to stay the same pressure.  One
 * pass of the strain kernel and one per-node kernel with a fixed-order reduction, no atomics: a call repeats bit for bit.
 * pl3_stokes_get_coeffs(which, etas, etan): which = 0 the effective, 1 the material viscosities, (nz, nx, ny) each, either may be NULL. */
int  pl3_stokes_set_yield(pl3_ctx* ctx, int on, double tau0, double dtau_dz, double eta_floor);
int  pl3_stokes_get_yield(pl3_ctx* ctx, int* on, double* tau0, double* dtau_dz, double* eta_floor);
int  pl3_stokes_yield_update(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double out[6]);
int  pl3_stokes_get_coeffs(pl3_ctx* ctx, int which, double* etas, double* etan);

/* ---- 3-D marker-in-cell (one rank; every entry point fails on a context that has pl3_set_comm attached) -------------
 * The dimension-by-dimension extension of pylamp_trac.py:30-388.  tr_x is (n, 3) in [z, x, y] order, tr_f is (n, ld_f) with the
 * 2-D columns of pylamp_const.py, grid arrays are C-order (nz, nx, ny).  Cells are found per axis by the regular-grid formula
 * floor((n-1)(x-x0)/L).
 * pl3_trac2grid: averages nf <= 8 tracer fields (the first nf columns of tr_f) onto the node set given by its three coordinate
 * arrays; the four PL_AVG_* schemes, trilinear weights, auto-extension and crop as in 2-D (a contribution to a node outside the
 * set is dropped, a node that receives nothing is NaN).  Built as a gather over cell-sorted tracers without floating-point
 * atomics: two calls with the same input give bitwise the same output.
 * pl3_grid2trac: PL_INTERP_LINEAR (trilinear), PL_INTERP_NEAREST (nearest of the eight corners, ties by corner index
 * (di 2 + dj) 2 + dk) or PL_INTERP_VELDIV (divergence-conserving, exactly the three fields vz, vx, vy).  A tracer outside the grid
 * gets defval in EVERY column -- the 2-D quirk that leaves vz extrapolated under VELDIV is deliberately not copied.
 * pl3_rk4: four VELDIV evaluations on the padded (nz+1, nx+1, ny+1) centre grid, out-of-grid velocity 0, the reference's weights
 * (1,1,1,1)/6; v_out = (x_new - x)/tstep and x_out, both (n, 3). */
int  pl3_trac2grid(pl3_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f, int64_t ld_f, int nf, const int* avgscheme,
                   const double* zc, int nzc, const double* xc, int nxc, const double* yc, int nyc, double* const* out);
int  pl3_grid2trac(pl3_ctx* ctx, int64_t n, const double* tr_x, int nf, const double* const* fields, int gnz, int gnx, int gny,
                   const double* gz, const double* gx, const double* gy, int method, double defval, int stop_on_error, double* out,
                   int64_t ld_out, int64_t* n_outside);
int  pl3_rk4(pl3_ctx* ctx, int64_t n, const double* tr_x, int gnz, int gnx, int gny, const double* gz, const double* gx, const double* gy,
             const double* vz, const double* vx, const double* vy, double tstep, double* v_out, double* x_out);
/* Resident tracers of a context: (n, 3) positions and (n, 13) fields, kept on the device sorted by cell of the context's node grid
 * (tracers outside it count to the nearest cell).  Download returns them in the resident order: TR__ID identifies a tracer.
 * Census: tracers per cell, (nz-1, nx-1, ny-1) int32, a by-product of the sort. */
/* Rectilinear grids: an opt-in per-axis cell search (default off = the regular-grid formula above, bit for bit).  With the switch
 * on, every marker call of the context (pl3_trac2grid, pl3_grid2trac, pl3_rk4, pl3_tracers_*, every pl3_resident_* marker call and
 * pl3_resident_step) finds cells from the stored coordinates -- the 3-D extension of the 2-D rule of pl_mic_set_search.  Per axis,
 * with strictly increasing c[0..n-1], h0 = c[1] - c[0], h1 = c[n-1] - c[n-2], the cell of a position p is
 *   c[0] <= p < c[n-1]:  the i with c[i] <= p < c[i+1], decided by exact comparisons with c[] (searchsorted(c, p, 'right') - 1);
 *   p < c[0]:            floor((p - c[0]) / h0) < 0 (the auto-extended node set);
 *   p >= c[n-1]:         n - 1 + floor((p - c[n-1]) / h1).
 * Sort and census clamp the cell into 0..n-2 (NaN: cell 0).  Grid -> tracer and RK4: a tracer is outside (defval / velocity 0) when
 * p < c[0], p >= c[n-1] or p is NaN on any axis; weights d0 / (d0 + d1); VELDIV uses the spacings of the found cell.  Tracer -> grid:
 * node i receives t = (p - c(i-1)) / (c(i) - c(i-1)) from a tracer in [c(i-1), c(i)) and 1 - t, t = (p - c(i)) / (c(i+1) - c(i)), from
 * one in [c(i), c(i+1)), with c(-1) = c[0] - h0 and c(n) = c[n-1] + h1; contributions to nodes outside the set are dropped.  A
 * bucket table per axis only shortens the search: results rest on comparisons with c[] alone.  On a regular grid the rule agrees
 * with the formula except within rounding of a cell face.  Not changed by the switch: the time-step rules and the subgrid time
 * scale use the mean spacing L / (n - 1), the padded centre grid's ghost coordinate is m[0] - (m[1] - m[0]), the fence is EPS.
 * Changing the switch while tracers are resident re-sorts them by the new rule. */
int  pl3_mic_set_search(pl3_ctx* ctx, int on);
int  pl3_mic_get_search(pl3_ctx* ctx, int* on);
/* Deletion of the tracers that leave the box (pylamp2.py:563-581), opt-in per context, default off = every kernel, message and
 * result as without it.  With deletion on, a resident tracer is OUTSIDE when, for any axis d, x_d <= 0 or x_d >= L_d, L_d = the last
 * node coordinate of the context's grid (the comparison of the 2-D sort key; a NaN coordinate compares false and the tracer is
 * kept).  An outside tracer is removed by the next sort of the resident tracers: pl3_tracers_upload, pl3_resident_refill,
 * pl3_resident_rk4 / pl3_resident_advect, the re-sort of pl3_mic_set_search, the sort of pl3_resident_step, and switching deletion
 * on (which re-sorts when tracers are resident; switching it off changes nothing).  Removal takes the position, the 13 fields and
 * the stored velocity; the survivors keep the order the plain sort would give them alone (cell by cell, stable within a cell).
 * The census counts survivors only and the refill of the same sort sees the counts after the removal: a cell the removal emptied
 * counts in out[2] and its new tracers carry NaN fields.  The largest ID the refill numbers from is the largest among the
 * survivors, reduced again in every refilling sort (-1 when no survivor has a finite ID).  All tracers may leave: count 0 is a valid
 * state of every call.  `fence` of pl3_resident_rk4 / pl3_resident_advect keeps its meaning; with deletion on, fence == 0 may
 * inject, and pl3_resident_step runs fence off exactly when deletion is on.  One rank only.
 * pl3_tracers_removed: out = { tracers removed by the last sort, removed since the last pl3_tracers_upload (its own included) }. */
int  pl3_mic_set_deletion(pl3_ctx* ctx, int on);
int  pl3_mic_get_deletion(pl3_ctx* ctx, int* on);
/* RK4 weights of the 3-D marker advection of this context (pl3_rk4, pl3_resident_rk4, pl3_resident_advect, pl3_resident_step).  Off,
 * the default: the reference's x + dt (k1 + k2 + k3 + k4) / 6 (pylamp_trac.py:385), whose weights sum to 4/6, so that a uniform field U
 * moves a tracer by 2/3 U dt; every result is what it was.  On: the classical x + dt (k1 + 2 k2 + 2 k3 + k4) / 6, which moves it by U dt.
 * A flow through the walls (pl3_stokes_set_wall_flow) wants it on: the markers then carry the volume that the wall flux brings in. */
int  pl3_mic_set_rk4_classic(pl3_ctx* ctx, int on);
int  pl3_mic_get_rk4_classic(pl3_ctx* ctx, int* on);
int  pl3_tracers_removed(pl3_ctx* ctx, int64_t out[2]);
int  pl3_tracers_upload(pl3_ctx* ctx, int64_t n, const double* tr_x, const double* tr_f);
int  pl3_tracers_download(pl3_ctx* ctx, int64_t n, double* tr_x, double* tr_f);
int  pl3_tracers_count(pl3_ctx* ctx, int64_t* n);
int  pl3_tracers_census(pl3_ctx* ctx, int64_t ncell, int32_t* counts);
/* Stages of a time step on the resident tracers -- the same kernels as the host-array calls; only grid fields cross PCIe.
 * props: rho(T) and eta(T) with clamps (pylamp2.py:291-303).  trac2grid: tracer columns `columns` onto a node set, to host arrays.
 * temp_to_tracers: field (nz, nx, ny) = the new nodal temperature (absolute != 0, first step) or its increment, then with
 * subgrid != 0 the subgrid-diffusion update of pylamp2.py:471-480 with (2/dz)^2 + (2/dx)^2 + (2/dy)^2 in the time scale; a tracer
 * outside the grid is an error.  rk4: advection on the padded centre grid, fence != 0: x <= 0 -> EPS, x >= L -> L - EPS per axis
 * (pylamp2.py:558-572), then the re-sort; the tracer velocities of the last call stay retrievable (n, 3).
 * times: device milliseconds of the last resident scatter, temperature stage, RK4 kernel and sort. */
int  pl3_resident_props(pl3_ctx* ctx, int tdep_rho, int tdep_eta, double tref, double etamin, double etamax);
int  pl3_resident_trac2grid(pl3_ctx* ctx, int nf, const int* columns, const int* avgscheme, const double* zc, int nzc, const double* xc,
                            int nxc, const double* yc, int nyc, double* const* out);
int  pl3_resident_temp_to_tracers(pl3_ctx* ctx, int absolute, const double* field, int subgrid, double tstep);
int  pl3_resident_rk4(pl3_ctx* ctx, const double* gz, const double* gx, const double* gy, const double* vz, const double* vx,
                      const double* vy, double tstep, int fence);
int  pl3_get_tracer_velocity(pl3_ctx* ctx, int64_t n, double* out);
/* Census + refill of depleted cells (the extension of pylamp2.py:588-633 by one axis), fused into the sort by cell.  The census is
 * the sort's own count array.  A cell with fewer than tracdens_min tracers receives tracdens - count new ones, written directly
 * behind its residents, so the resident state stays cell-sorted and pl3_tracers_census counts them.  New tracer q of cell
 * c = (i (nx-1) + j)(ny-1) + k sits at g_d[i_d] + u_d (g_d[i_d+1] - g_d[i_d]) with u_d a counter-based uniform of
 * (seed, c, q, 3 it + d) alone, d = 0, 1, 2 = z, x, y; every field but TR__ID is the plain mean of the cell's residents, summed
 * in resident order (an EMPTY cell gives 0/0 = NaN as in the reference: it is counted in out[2], and the next scatter shows it);
 * the stored velocity is 0.  IDs: the reference's rule (numbering starts AT the largest ID and the first new ID of every refilled
 * cell repeats the last one handed out) or, with unique_ids, largest ID + 1, + 2, ... in cell order.  No floating-point atomics
 * and a fixed order of summation: two runs agree bitwise.  tracdens_min <= 0, or no deficient cell: the state is bit for bit
 * what the plain sort leaves.  The arrays grow inside the sort when the new total exceeds their capacity.
 * refill: sort + refill without advection (top up a sparse initial set).  advect: pl3_resident_rk4 with the refill in its sort.
 * out = { tracers injected, cells refilled, cells that were empty, smallest count of a cell before the refill }.
 * Errors: tracdens < tracdens_min; tracdens_min > 0 with fence == 0 on a context without pl3_mic_set_deletion (a tracer outside
 * the box would be counted in the nearest cell); a context with pl3_set_comm attached. */
int  pl3_resident_refill(pl3_ctx* ctx, int tracdens, int tracdens_min, uint64_t seed, int it, int unique_ids, int64_t out[4]);
int  pl3_resident_advect(pl3_ctx* ctx, const double* gz, const double* gx, const double* gy, const double* vz, const double* vx,
                         const double* vy, double tstep, int fence, int tracdens, int tracdens_min, uint64_t seed, int it,
                         int unique_ids, int64_t out[4]);
int  pl3_resident_times(pl3_ctx* ctx, double ms[4]);
/* Inflow material: what the refill's new tracers carry where a wall flow (pl3_stokes_set_wall_flow) brings material into the box.
 * Opt-in per wall, default none = every kernel and result as without it.  An overlay on the refill above: positions, IDs, stored
 * velocities, counts, the sort, the census and the deletion are bit for bit what they are without a material; only field values of
 * new tracers change.  Per wall w of [z0, x0, y0, zL, xL, yL] (axis a = w mod 3, p < q the two other axes in z, x, y order) a context
 * may hold a set of tracer columns -- bits 0 ... 11 of `columns`; TR__ID, column 12, is never allowed -- and one plane per column over
 * the wall's faces: the planes of pl3_stokes_set_wall_flow ("Wall planes").  `values` holds popcount(columns) planes in ascending column order.
 * In every sort that refills (pl3_resident_refill, pl3_resident_advect, pl3_resident_step) a refilled cell c = (i_z, i_x, i_y) is an
 * INFLOW CELL of wall w when (a) w has a material, (b) the cell touches w: its index along a is 0 for z0, x0, y0 and n_a - 2 for zL,
 * xL, yL, and (c) the context's wall flow at the time of the sort is non-zero and inward at the cell's own face (i_p, i_q) of w:
 * Un_w > 0 on z0, x0, y0, Un_w < 0 on zL, xL, yL; no flow on w, or Un_w == 0, means no.  If several walls qualify (edge and corner
 * cells) the first in the order z0, x0, y0, zL, xL, yL decides alone.
 * For an inflow cell of wall w let s(x) be the distance of a position from the wall, x_a - c_a[0] for a low wall and c_a[n_a - 1] - x_a
 * for a high one, and dmin the minimum of s over the cell's residents after the deletion (the residents the refill averages; a NaN
 * coordinate is ignored; +inf when the cell has none).  New tracer q of the cell is an INFLOW TRACER exactly when s(x_q) < dmin,
 * strictly: it lies between the wall and every resident, in the gap the wall flux opened.  It takes mat_w[col][i_p (n_q - 1) + i_q] in
 * every column of the wall's set and the residents' mean (possibly NaN) in the others; a new tracer that is no inflow tracer keeps the
 * mean in every column.  In an inflow cell the removal emptied every new tracer is an inflow tracer, so the prescribed columns are
 * finite there (a column the material leaves out is still 0/0 = NaN).  The rule needs no time step and no random numbers of its own:
 * a function of the sorted state and the two wall settings, so two runs agree bitwise.  A prescribed TR_TMP is a tracer temperature
 * like any other: with heat diffusion on it enters the next step's temperature scatter.
 * set: columns == 0 clears the wall (values may then be NULL); a new context has none.  The state belongs to the context like the
 * search, the deletion and the RK4 weights: it survives uploads, pl3_stokes_set_wall_flow and pl3_stokes_set_walls, a wall without a
 * flow may hold a material (the rule never fires there), and setting it changes no resident tracer.
 * get: either pointer may be NULL; values receives the wall's planes, downloaded from the device.
 * pl3_mic_inflow_count: out = { inflow tracers of the last sort, since the last pl3_tracers_upload }.
 * Errors, a rejected call changing nothing: a NULL context; wall outside 0 ... 5; a bit >= 12 in columns (bit 12 is named as TR__ID);
 * columns != 0 with values == NULL; a non-finite value (names the wall, the column and the index); a context with pl3_set_comm
 * attached. */
int  pl3_mic_set_inflow(pl3_ctx* ctx, int wall, unsigned columns, const double* values);
int  pl3_mic_get_inflow(pl3_ctx* ctx, int wall, unsigned* columns, double* values);
int  pl3_mic_inflow_count(pl3_ctx* ctx, int64_t out[2]);

/* ---- device-resident 3-D time step (one rank) ------------------------------------------------------------------------
 * pl3_resident_step is one step of the loop of pylamp2.py:290-581 with a third axis on the resident tracers, with every grid field
 * kept on the device: properties -> tracer->grid (nodes: rho, etas, cp, T, H, mat; cell centres: etan; the three mixed sets of the
 * conductivity; with do_heatdiff == 0 only rho, etas and the unweighted geometric etan) -> NaN check -> heat time-step rule ->
 * Stokes coefficients and a cold resident solve -> Stokes time-step rule, limiter and clamps -> heat coefficients and a resident
 * solve -> temperature to the tracers (absolute when it == 1, otherwise the increment newtemp - T, with the subgrid diffusion if
 * enabled) -> advection velocity on the padded centre grid -> RK4 + fence + sort + refill.  From it == 2 on the six walls of the
 * scattered T take the previous solved temperature (pylamp2.py:327-331).  The kernels and solvers are those of the host-array
 * entry points, called in the same order, and the scalars of the time-step rules (min(eta), max(2 kz / (rho cp)), max(vz), max(vx),
 * max(vy): reduced on the device, NaN-propagating like NumPy's) are combined as Python combines them; only those scalars, the
 * solvers' own and the report cross the bus.  `it` counts from 1 and selects the random stream of the refill.
 * Errors: NaN in the scattered rho or etas (the message names the field and the count, report->nan_rho / nan_etas are set, the
 * tracers' positions and temperature and the previous temperature are untouched); it > 1 with heat on and no previous resident step;
 * a context with pl3_set_comm attached. */
typedef struct pl3_step_config {
    int    do_heatdiff, do_subgrid_heatdiff, tdep_rho, tdep_eta;
    double etamin, etamax, tref;
    double tstep_adv_max, tstep_adv_min, tstep_dif_max, tstep_dif_min, tstep_modifier;
    int    bcheat[6];          /* z0, x0, y0, zL, xL, yL */
    double bcheatvals[6];
    double stokes_rtol, heat_rtol;
    int    stokes_maxit, heat_maxit;
    int    use_grav;           /* 0: gravity (9.81, 0, 0) */
    int    reserved_;          /* 0 */
    double grav[3];
    int    tracdens, tracdens_min;
    uint64_t inject_seed;
    int    inject_unique_ids;
    int    reserved2_;         /* 0 */
} pl3_step_config;
typedef struct pl3_step_report {
    double tstep;
    int    limiter;            /* 0: the Stokes (advection) rule set the step, 1: the heat rule */
    int    reserved_;
    double tstep_heat, tstep_stokes;
    pl_solve_stats stokes, heat;
    int64_t ninjected, nrefilled, nempty, mincount;     /* the four counters of pl3_resident_refill */
    int64_t ntrac;
    int64_t nan_rho, nan_etas; /* nodes of the scattered rho / etas that hold NaN */
    double ms_scatter, ms_stokes, ms_heat, ms_gather, ms_rk4, ms_sort;      /* device time of the stages */
    double ms_total;           /* host wall time of the call */
    int64_t nremoved;          /* tracers the step's sort removed (pl3_mic_set_deletion; 0 without it) */
} pl3_step_report;
int  pl3_resident_step(pl3_ctx* ctx, const pl3_step_config* cfg, int it, pl3_step_report* report);
/* A grid field of the last resident step, downloaded on demand into out (nz, nx, ny): rho, etas, etan, cp, T, H, mat, kz, kx, ky,
 * velz, velx, vely, pres (Kcont-scaled, ghosts retained), temp; after a step with pl3_step_set_shear_heating or
 * pl3_step_set_strain_fields on also strainrate, stress, dissipation (they live in a Stokes work vector: until the next call that uses
 * the work vectors); with a yield stress set (pl3_stokes_set_yield) also etas_eff, etan_eff, the effective viscosities the operator holds
 * after the step's Picard loop, while etas and etan stay the scattered material fields.  An unknown or not-yet-computed name is an error
 * that lists the available ones. */
int  pl3_get_field(pl3_ctx* ctx, const char* name, double* out);
/* Opt-in switches of pl3_resident_step, context state, both off at creation; with both off the step is bit for bit what it is without
 * them.  Shear heating: after the Stokes solve the dissipation of the solution (pl3_stokes_strain_fields) is added to the scattered H,
 * one IEEE addition per node, and the heat solve takes the sum (pl3_get_field("H") returns it); wall nodes keep their boundary rows, the
 * dissipation there is diagnostic only; a step with do_heatdiff == 0 fails by name.  Strain fields: the step computes the three fields
 * without touching H.  Either switch makes strainrate, stress and dissipation available to pl3_get_field and the integral of the
 * dissipation to pl3_step_dissipation_total (an error before the first such step).  The time-step rules are unchanged. */
int  pl3_step_set_shear_heating(pl3_ctx* ctx, int on);
int  pl3_step_shear_heating(pl3_ctx* ctx, int* on);
int  pl3_step_set_strain_fields(pl3_ctx* ctx, int on);
int  pl3_step_dissipation_total(pl3_ctx* ctx, double* total);
/* The Picard loop of pl3_resident_step, run only with a yield stress set (pl3_stokes_set_yield); the settings are context state, maxit = 10
 * and tol = 1e-2 at creation.  Step 4 of the resident step then is: solve 1 with the material viscosities (cold, or warm with
 * pl3_stokes_set_warm_start); update the viscosities (pl3_stokes_yield_update on the resident solution); while the change of the update is
 * above tol and fewer than maxit solves have run: solve again from the resident solution (use_x0; the reference norm is the one the solve
 * computes from the hydrostatic state), update again.  As many updates as solves; the step is converged when the last change is <= tol.
 * Reaching maxit is no error: the step goes on with the last solution.  The time-step rule, the strain fields and shear heating, the heat
 * solve, the advection velocity and the one history commit of the warm start use the last solution, with the last effective viscosities
 * where they need any; report->stokes holds the statistics of the last solve.  When nothing yields the first update returns change 0 and
 * the step is, array for array, the step without a yield stress.
 * pl3_step_set_picard: maxit 1 .. 32, tol >= 0, else an error by name.
 * pl3_step_picard_report: out[0] iterations of the last resident step's loop (0: no yield stress was set), out[1] converged, then per
 * iteration { change, yielded nodes, yielded centres, iterations of its Stokes solve }; n = capacity of out (2 + 4 x 32 holds it all). */
int  pl3_step_set_picard(pl3_ctx* ctx, int maxit, double tol);
int  pl3_step_picard_report(pl3_ctx* ctx, double* out, int n);
/* The step's advection-velocity kernel on host arrays: vz, vx, vy (nz, nx, ny) -> Vz, Vx, Vy on the padded (nz+1, nx+1, ny+1)
 * centre grid: every component averaged along its own axis, then the ghosts wall by wall in the order z0, x0, y0, zL, xL, yL: a
 * FREESLIP wall mirrors the normal component with a sign flip and copies the tangential ones, the pass of a NOSLIP wall
 * (pl3_stokes_set_walls) is skipped and its ghosts keep what they hold (pylamp2.py:491-545); the order decides the edge and corner
 * values.  The pass of a NOSLIP wall with a non-zero velocity (pl3_stokes_set_wall_velocity) runs in its slot and writes, from the
 * neighbouring plane as it is at that moment, -V for the normal component and 2 U_c - V for each tangential component c: the velocity
 * interpolated onto the wall is U.  This is deliberately discontinuous at U = 0, where the pass is skipped: walls at rest keep the
 * reference's behaviour. */
int  pl3_advection_velocity(pl3_ctx* ctx, const double* vz, const double* vx, const double* vy, double* Vz, double* Vx, double* Vy);
/* Host <-> device copies issued by the pl3_* entry points of this context since the last reset: out = { copies of at least one node
 * field (8 nz nx ny bytes), their bytes, smaller copies, their bytes }; reset != 0 clears the counters after reading. */
int  pl3_transfer_stats(pl3_ctx* ctx, int64_t out[4], int reset);
/* out = { sizeof(pl3_step_config), sizeof(pl3_step_report), offsetof(config.bcheatvals), offsetof(config.grav),
 * offsetof(config.inject_seed), offsetof(report.heat), offsetof(report.ntrac), offsetof(report.ms_total) } */
int  pl3_abi_layout(size_t out[8]);

/* sizeof / offsetof of the structs above as compiled into the library: out = { sizeof(pl_solve_stats),
 * sizeof(pl_step_config), sizeof(pl_step_report), offsetof(config.length), offsetof(config.inject_seed),
 * offsetof(config.tracs_fence_disabled), offsetof(report.ntrac), offsetof(report.nremoved) } -- lets a binding
 * verify its mirror of the layout (tests/test_cabi.py). */
int  pl_abi_layout(size_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PYLAMP_HIP_H */
