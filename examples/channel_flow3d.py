"""The dense sphere of falling_sphere3d.py sinking in a cross-flow: material enters through the wall x0 and leaves through xL between
no-slip z-walls (Options3.bcstokesflow).  The profile is the parabola 4 s (1 - s) over the height s = z / Lz, which vanishes towards
the no-slip walls -- a uniform inflow next to a no-slip wall is singular along their common edge.  Both walls carry the same profile,
so the net flux is zero (pylamp3d.wall_fluxes prints it).  The fence is off and the marker deletion on: markers that leave through xL
are removed by the end-of-step sort, and the census refill inside the same sort keeps the cells along x0 filled; the new markers carry
the mean of their cell's residents (a zero-gradient inflow) unless --mark-inflow gives x0 a material (Options3.bcinflow): the new markers
between the wall and the residents of their cell then enter as TR_MAT = 3 with TR_MRK = 7, and every step prints how far that material
has come -- the largest x among the TR_MAT == 3 markers -- next to the integral of max(Un) dt, which it cannot overtake.  Options3.rk4_classic takes the classical RK4 weights, with which the
markers move by U tstep (the reference's weights, the default, carry them 2/3 of that, less than the walls bring in).  Writes griddata.NNNNNN.npz / tracs.NNNNNN.npz as the other examples do.

    python examples/channel_flow3d.py [n=65] [steps=20] [outdir=out] [umax=3e-9] [--resident] [--mark-inflow]

umax: the largest inflow speed in m/s (3e-9 is about 10 cm/yr, a few times the sphere's sinking speed).
--resident runs the device-resident step (Options3.resident).  --mark-inflow marks what enters through x0.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402

resident = "--resident" in sys.argv[1:]
mark = "--mark-inflow" in sys.argv[1:]
argv = [a for a in sys.argv if not a.startswith("--")]
n = int(argv[1]) if len(argv) > 1 else 65
steps = int(argv[2]) if len(argv) > 2 else 20
outdir = argv[3] if len(argv) > 3 else "out"
umax = float(argv[4]) if len(argv) > 4 else 3e-9

nx = [n, n, n]; L = [100e3, 100e3, 100e3]
grid = [np.linspace(0, L[d], nx[d]) for d in range(3)]
s = 0.5 * (grid[0][1:] + grid[0][:-1]) / L[0]                                    # the faces of x0 / xL: (nz - 1, ny - 1)
profile = umax * (4 * s * (1 - s))[:, None] * np.ones(nx[2] - 1)[None, :]
flow = [None, profile, None, None, profile, None]                                # [z0, x0, y0, zL, xL, yL], along +x: in at x0, out at xL
fluxes, phi = P3.wall_fluxes(grid, flow)
print("wall fluxes into the box [z0, x0, y0, zL, xL, yL] (m3/s): %s, net %.3e" % (", ".join("%.4e" % v for v in fluxes), phi))

N, F = P3.BC_TYPE_NOSLIP, P3.BC_TYPE_FREESLIP
tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(1))
opt = P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False,             # isothermal, constant properties
                  tracdens=8, tracdens_min=4, inject_unique_ids=True, resident=resident,
                  bcstokes=[N, F, F, N, F, F], bcstokesflow=flow, tracs_fence_enabled=False, marker_deletion=True,
                  rk4_classic=True,                                              # the markers move by U tstep, as the wall flux does
                  bcinflow=[None, {P3.TR_MAT: 3, P3.TR_MRK: 7}, None, None, None, None] if mark else None)
sim = P3.Simulation3(nx, L, tr_x, tr_f, opt)
travelled = 0.0                                                                  # the integral of max(Un) dt
for it in range(1, steps + 1):
    rep = sim.step()
    x, f = sim.tracers()
    ball = f[:, 8] == 2
    print("step %3d  t = %8.3f Myr  dt = %.3e s (%s)  Stokes %3d its %s  sphere at z = %.2f km, x = %.2f km  %d tracers, %d removed, %d injected into %d "
          "cells, %d empty" % (it, sim.totaltime / 3.15576e13, rep["tstep"], rep["limiter"], rep["stokes"]["iterations"],
                               "ok" if rep["stokes"]["converged"] else "NOT CONVERGED", x[ball, 0].mean() / 1e3, x[ball, 1].mean() / 1e3,
                               rep["ntrac"], rep["nremoved"], rep["ninjected"], rep["nrefilled"], rep["nempty"]), flush=True)
    if mark:
        travelled += umax * rep["tstep"]
        new = f[:, P3.TR_MAT] == 3
        print("          inflow: %d markers took the material of x0 in this step, %d carry it; front at x = %.3f km, max(Un) dt summed = %.3f km"
              % (rep["ninflow"], new.sum(), x[new, 1].max() / 1e3 if new.any() else 0.0, travelled / 1e3), flush=True)
    if it % 10 == 0 or it == steps:
        sim.write_snapshot(outdir)
sim.close()
