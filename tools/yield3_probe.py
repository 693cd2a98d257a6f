"""The yield-stress update next to one scaled operator application, for a kernel trace (profiles/yield3.json):

    rocprofv3 --kernel-trace --stats -d DIR -- python tools/yield3_probe.py [--n 129] [--updates 25] [--applies 250]

A dense, stiff blob in a box with no-slip z walls: one resident solve, `--applies` scaled operator applications (pl3_stokes_apply_bench)
and `--updates` calls of yield_update on the resident solution (k3_strain_ce + k3_yield_visc + two k_r3_finish; each call derives the
viscosities from the material ones, so every call does the same work).  tau0 is the median of the node stress of the solve.  Prints one
JSON line with the host times per call; tools/kernel_stats.py turns the trace's database into the per-kernel averages."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=129); ap.add_argument("--updates", type=int, default=25); ap.add_argument("--applies", type=int, default=250)
a = ap.parse_args()
n = [a.n] * 3; L = [1.0e5] * 3
grid = [np.linspace(0, L[d], n[d]) for d in range(3)]
Z, X, Y = np.meshgrid(*grid, indexing="ij")
inside = ((Z - 0.4 * L[0]) ** 2 + (X - 0.5 * L[1]) ** 2 + (Y - 0.45 * L[2]) ** 2) < (0.25 * L[0]) ** 2
eta = np.where(inside, 1e21, 1e20); rho = np.where(inside, 3400.0, 3300.0)
del Z, X, Y
A, _ = P3.makeStokesMatrix(n, grid, eta, eta, rho, bc=[P3.BC_TYPE_NOSLIP, 1, 1, P3.BC_TYPE_NOSLIP, 1, 1])
ctx = A._ctx
P3.solve(A, resident=True)
tau0 = float(np.median(P3.strain_fields(A)["stress"]))
ctx.set_yield(tau0, 0.0, 1e19)
ms = C.c_double()
ctx.check(ctx.lib.pl3_stokes_apply_bench(ctx.handle(), 1, a.applies, C.byref(ms)))
first = P3.yield_update(A)
t0 = time.perf_counter()
for _ in range(a.updates):
    u = P3.yield_update(A)
update_ms = (time.perf_counter() - t0) * 1e3 / a.updates
print(json.dumps(dict(n=a.n, solve=A.last_stats, tau0=tau0, apply_scaled_ms=ms.value, yield_update_call_ms=update_ms, first_update=first,
                      repeated_update=u)))
ctx.close()
