"""A hot patch under a free-slip box: uniform fluid at 1000 K, the top z0 held at 1000 K, the base zL held at 1000 K except for a disc
of radius L/4 at its centre held at --hot K, the side walls insulating -- the heat walls with a profile of pylamp3d.Simulation3
(Options3.bcheatprofile, Simulation3.set_heat_profile).  The patch warms the fluid above it, the thermal expansion drives a plume, and
every step prints the heat budget of its heat solve (Simulation3.heat_budget): what enters through the base, what leaves through the top,
the storage rate, and the imbalance of the three.

    python examples/hot_patch3d.py [n=33] [steps=5] [--hot=1300] [--resident] [--move=K]

--resident runs the device-resident step (Options3.resident).
--move=K shifts the disc by a quarter of the box along x after K steps (set_heat_profile between two steps).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402
from pylamp_amd.pylamp_const import TR_ALP, TR_ET0                                # noqa: E402


def flag(name, default):
    v = [a.split("=", 1)[1] for a in sys.argv[1:] if a.startswith("--%s=" % name)]
    return float(v[0]) if v else default


resident = "--resident" in sys.argv[1:]
hot, move = flag("hot", 1300.0), int(flag("move", 0))
argv = [a for a in sys.argv if not a.startswith("--")]
n = int(argv[1]) if len(argv) > 1 else 33
steps = int(argv[2]) if len(argv) > 2 else 5

nx = [n, n, n]; L = [100e3, 100e3, 100e3]
tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(1))          # 2 x 2 x 2 jittered markers per cell ...
tr_f[:, P3.TR_RHO] = tr_f[:, P3.TR_RH0] = 3300.0; tr_f[:, TR_ET0] = 1e20         # ... of one uniform fluid (TR_MAT still marks the sphere)
tr_f[:, P3.TR_TMP] = 1000.0; tr_f[:, P3.TR_HCD] = 4.0; tr_f[:, P3.TR_HCP] = 1250.0; tr_f[:, TR_ALP] = 3.5e-5


def disc(cx):
    """The plane of zL over its nodes, (nx, ny): `hot` inside the disc around (cx, L/2), 1000 K outside."""
    X, Y = np.meshgrid(np.linspace(0, L[1], n), np.linspace(0, L[2], n), indexing="ij")
    return np.where((X - cx) ** 2 + (Y - L[2] / 2) ** 2 < (L[1] / 4) ** 2, hot, 1000.0)


opt = P3.Options3(tdep_eta=False, Tref=1000.0, resident=resident, bcheatvals=[1000.0, 0.0, 0.0, 1000.0, 0.0, 0.0],
                  bcheatprofile={"zL": disc(L[1] / 2)})
sim = P3.Simulation3(nx, L, tr_x, tr_f, opt)
for it in range(1, steps + 1):
    if move and it == move + 1:
        sim.set_heat_profile({"zL": disc(3 * L[1] / 4)})
    rep = sim.step()
    b = sim.heat_budget()
    print("step %3d  t = %8.3f Myr  dt = %.3e s  heat %3d its  warmest node %.2f K  max |vz| %.3e m/s" %
          (it, sim.totaltime / 3.15576e13, rep["tstep"], rep["heat"]["iterations"], sim.field("temp").max(), np.abs(sim.field("velz")).max()), flush=True)
    print("          in through zL %.4e W, z0 %.4e W, sides %.1e W; storage %.4e W, source %.4e W, imbalance %.1e W" %
          (b["wall_flow"][3], b["wall_flow"][0], sum(b["wall_flow"][w] for w in (1, 2, 4, 5)), b["storage"], b["source"], b["imbalance"]), flush=True)
sim.close()
