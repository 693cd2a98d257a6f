"""A dense, stiff sphere sinking in a box with free-slip or sticking walls: the 3-D marker-in-cell time step (pylamp3d.Simulation3).  Writes
griddata.NNNNNN.npz / tracs.NNNNNN.npz in the style of the 2-D example, with a third axis (gridy, vely, tr_x (n, 3)).
Cells that run below tracdens_min markers are refilled to tracdens inside the end-of-step sort (0 0 switches that off).

    python examples/falling_sphere3d.py [n=65] [steps=20] [outdir=out] [tracdens=8] [tracdens_min=4] [--resident] [--refine=R] [--noslip=z] [--fence-off] [--warm] [--strain] [--yield=TAU[,DTAU]]

--resident runs the device-resident step (Options3.resident): the grid fields stay on the GPU and are downloaded for the snapshots only.
--refine=R (e.g. 3) makes the cells R times finer around the sphere's path than far from it (pylamp3d.refined_grid) and switches
the markers' per-axis cell search on (Options3.marker_search), which a grid that is not regular needs; the markers start denser
so that the fine cells are populated.
--noslip=z makes the two z-walls (lid and base) no-slip, --noslip=zx the z- and x-walls, --noslip=zxy all six (Options3.bcstokes); the
other walls stay free-slip.
--fence-off switches the fence off and the marker deletion on (Options3.tracs_fence_enabled = False, marker_deletion = True): markers that
leave the box are removed by the end-of-step sort instead of being parked 2^-10 m from the wall.  Meant for --noslip=z with injection:
the velocity interpolated onto a no-slip wall at rest is half the last centre value, so markers are carried through such a wall, and the
census and refill inside the same sort restore the density behind them.  Every step prints the markers removed and injected.
--warm starts every Stokes solve from the extrapolated history of the last three solutions instead of the hydrostatic state
(Options3.stokes_warm_start); every step then prints how its solve started (cold, warm, or rejected by the guard).
--strain keeps the second invariants of the strain rate and of the stress and the viscous dissipation of every step
(Options3.strain_fields): the snapshots gain strainrate, stress and dissipation, and every step prints the total dissipation.
--yield=TAU[,DTAU] limits the viscosity by the yield stress TAU + DTAU z [Pa, Pa/m] (Options3.yield_stress; e.g. --yield=2e6): every step
runs a Picard loop of Stokes solves and prints its figures, and the snapshots gain the effective viscosities etas_eff, etan_eff.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402

resident = "--resident" in sys.argv[1:]
refine = [float(a.split("=", 1)[1]) for a in sys.argv[1:] if a.startswith("--refine=")]
refine = refine[0] if refine else 0.0
fence_off = "--fence-off" in sys.argv[1:]
warm = "--warm" in sys.argv[1:]
strain = "--strain" in sys.argv[1:]
yield_stress = [tuple(float(v) for v in a.split("=", 1)[1].split(",")) for a in sys.argv[1:] if a.startswith("--yield=")]
yield_stress = (yield_stress[0] + (0.0,))[:2] if yield_stress else None
noslip = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--noslip=")]
noslip = noslip[0] if noslip else ""
if noslip not in ("", "z", "zx", "zxy"):
    sys.exit("--noslip takes z, zx or zxy")
bcstokes = [P3.BC_TYPE_NOSLIP if "zxy"[w % 3] in noslip else P3.BC_TYPE_FREESLIP for w in range(6)]      # [z0, x0, y0, zL, xL, yL]
argv = [a for a in sys.argv if not a.startswith("--")]
n = int(argv[1]) if len(argv) > 1 else 65
steps = int(argv[2]) if len(argv) > 2 else 20
outdir = argv[3] if len(argv) > 3 else "out"
tracdens = int(argv[4]) if len(argv) > 4 else 8
tracdens_min = int(argv[5]) if len(argv) > 5 else 4

nx = [n, n, n]; L = [100e3, 100e3, 100e3]
grid = None
per_axis = 2                                                                     # 2 x 2 x 2 jittered markers per (mean) cell
if refine > 1.0:                                                                 # the sphere starts at z = 0.3 L and sinks along +z
    grid = [P3.refined_grid(n, L[0], 0.45, refine, 0.35), P3.refined_grid(n, L[1], 0.5, refine, 0.2), P3.refined_grid(n, L[2], 0.5, refine, 0.2)]
    per_axis = int(np.ceil(2 * refine / 1.5))
tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(1), per_axis=per_axis)
opt = P3.Options3(do_heatdiff=False, tdep_rho=False, tdep_eta=False,             # isothermal, constant properties
                  tracdens=tracdens, tracdens_min=tracdens_min, inject_unique_ids=True, resident=resident, marker_search=grid is not None,
                  bcstokes=bcstokes, tracs_fence_enabled=not fence_off, marker_deletion=fence_off, stokes_warm_start=warm, strain_fields=strain, yield_stress=yield_stress)
sim = P3.Simulation3(nx, L, tr_x, tr_f, opt, grid=grid)
sphere = None
for it in range(1, steps + 1):
    rep = sim.step()
    x, f = sim.tracers()
    print("step %3d  t = %8.3f Myr  dt = %.3e s (%s)  Stokes %3d its %s%s  sphere at z = %.2f km  %d tracers, %d removed, %d injected into %d cells" %
          (it, sim.totaltime / 3.15576e13, rep["tstep"], rep["limiter"], rep["stokes"]["iterations"],
           "ok" if rep["stokes"]["converged"] else "NOT CONVERGED", " (%s start)" % rep["stokes_start"] if warm else "", x[f[:, 8] == 2, 0].mean() / 1e3, rep["ntrac"], rep["nremoved"], rep["ninjected"],
           rep["nrefilled"]), flush=True)
    if strain:
        print("          dissipation %.4e W, largest strain rate %.3e 1/s" % (rep["dissipation_total"], sim.field("strainrate").max()), flush=True)
    if yield_stress:
        p = rep["picard"]
        print("          Picard %d solves%s: change %s, yielded nodes %s, cells %s, Stokes iterations %s" %
              (p["iterations"], "" if p["converged"] else " (not converged)", " ".join("%.2e" % c for c in p["change"]), p["yielded_nodes"], p["yielded_cells"],
               p["stokes_iterations"]), flush=True)
    if it % 10 == 0 or it == steps:
        sim.write_snapshot(outdir)
sim.close()
