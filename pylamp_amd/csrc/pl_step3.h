// What pl_step3.hip (the device-resident 3-D time step) needs of pl_3d.hip (the context and the solvers) and of pl_mic3.hip (the
// resident tracers): device-source variants of the entry points that otherwise take host arrays.
#pragma once
#include "pl_internal.h"

// Velocities of the six Stokes walls (pl3_stokes_set_wall_velocity): u[3 w + q] = component q of (Uz, Ux, Uy) of wall w of [z0, x0, y0, zL,
// xL, yL]; bit w of `moving`: that wall has a non-zero velocity.  Passed by value to k3_rhs and k_s3_advvel, and to no other kernel.
struct Pl3WallVel { double u[18]; int moving; };
// Flow through the six Stokes walls (pl3_stokes_set_wall_flow): un[w] is the device plane of wall w over its faces, GLOBAL indices (the
// layout is in DESIGN.md section 6c, "Wall planes"), the wall-normal velocity along +a; bit w of `mask`: that wall carries a flow (its
// pointer is NULL otherwise).  Passed by value to k3_rhs, k_s3_advvel and, inside M3Inject, to k_m3_inject<true> (the inflow rule of
// pl3_mic_set_inflow), and to no other kernel.
struct Pl3WallFlow { const double* un[6]; int mask; };
// the context's ringed device arrays: node (i, j, k) of an array sits at (i + 1) s0 + (j + 1) s1 + k + pad
struct Pl3DevView {
    long long s0, s1; int pad; hipStream_t stream;
    double* X[4];                           // Stokes solution of the last solve: vz, vx, vy, P (Kcont-scaled)
    double* T;                              // heat solution of the last solve
    double* scratch[4];                     // work vectors that are free outside a solve
    bool have_x, have_T;
    int noslip;                             // Stokes walls (pl3_stokes_set_walls): bit w of [z0, x0, y0, zL, xL, yL] set = no-slip
    Pl3WallVel wallvel;                     // ... and their velocities
    Pl3WallFlow wallflow;                   // ... and the flow through them
    double* strain[3];                      // strainrate, stress, dissipation of the last pl3i_strain_fields_dev (Stokes work vector 2) ...
    bool have_strain;                       // ... and whether nothing has asked for the work vectors since
    double* eta_eff[2];                     // the operator's (effective) viscosities etas, etan, ringed ...
    bool yield_on;                          // ... and whether a yield stress is set (pl3_stokes_set_yield): they may then differ from the scattered ones
    void** slot;                            // opaque state owned by pl_step3.hip, released by pl3_step_free
};
// pl_3d.hip
int  pl3i_dev_view(pl3_ctx* ctx, Pl3DevView* v);
int  pl3i_stokes_set_coeffs_dev(pl3_ctx* ctx, const double* etas, const double* etan, const double* rho, const double grav[3], double mineta);
double nan_min3(double mes, double men, bool nan_s, bool nan_n);     // min(etas.min(), etan.min()) as NumPy has it: NaN where a field holds one
int  pl3i_heat_set_coeffs_dev(pl3_ctx* ctx, const double* const mp[3], const double* const src[7], const int bc[6], const double bcvalue[6], double tstep);
int  pl3i_strain_fields_dev(pl3_ctx* ctx, double* Hplain, double* total);     // the fields of the resident solution; Hplain (NULL: none) += dissipation
int  pl3i_yield_update_dev(pl3_ctx* ctx, double out[6]);     // pl3_stokes_yield_update for the resident solution
void pl3_count_copy(pl3_ctx* ctx, size_t bytes);          // every host <-> device copy of a pl3_* entry point reports here
// pl_mic3.hip (plain (nz, nx, ny) device arrays in and out)
int  pl3i_mic_scatter(pl3_ctx* ctx, int nf, const int* columns, const int* avgscheme, const double* const tc[3], const int tn[3], double* dout);
int  pl3i_mic_temp_to_tracers(pl3_ctx* ctx, int absolute, const double* dfield, int subgrid, double tstep);
int  pl3i_mic_advect(pl3_ctx* ctx, const double* dV, double tstep, int tracdens, int tracdens_min, uint64_t seed, int it, int unique_ids, int64_t out[4]);
int  pl3i_mic_buf(pl3_ctx* ctx, const char* name, size_t count, double** out);      // a device buffer that lives as long as the tracers' state
int  pl3i_mic_columns(pl3_ctx* ctx, double** f, long long* n, long long* cap);    // the resident tracer fields: column j at f + j cap
double* pl3i_mic_ms(pl3_ctx* ctx);                        // the four stage times of pl3_resident_times
// pl_step3.hip
void pl3_step_free(void** slot);
