"""One process = one sample of the numbers in profiles/stokes3_walls.json: the scaled 3-D Stokes operator (StokesOperator3.apply_bench)
and a cold device-resident solve on the problem of `bench.py --config 3d257`, at the given sizes, with free-slip walls or with
no-slip z-walls.  Prints one JSON line.  Run it in alternating processes for the two builds that are compared:

    python tools/stokes3_walls_probe.py [--root CHECKOUT] [--noslip z] [--plug U] [--sizes 129,257] [--tag NAME]

--root: import pylamp_amd from that checkout (a build of another commit) instead of this one; without --noslip no wall call is made,
so the script also runs on a commit that has none.
--plug U: a uniform flow of U m/s in through z0 and out through zL (makeStokesMatrix(wallflow=...)); without it no flow call is made.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
ap.add_argument("--noslip", default="", choices=["", "z", "zx", "zxy"])
ap.add_argument("--plug", type=float, default=0.0)
ap.add_argument("--sizes", default="129,257")
ap.add_argument("--tag", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402

out = {"tag": args.tag, "noslip": args.noslip, "plug": args.plug, "sizes": {}}
for nb in [int(v) for v in args.sizes.split(",")]:
    n = [nb] * 3; L = [660e3] * 3
    grid = [np.linspace(0, L[d], n[d]) for d in range(3)]
    mid = [np.append(0.5 * (g[1:] + g[:-1]), g[-1] + 0.5 * (g[-1] - g[-2])) for g in grid]

    def field(c):
        Z, X, Y = np.meshgrid(*c, indexing="ij", sparse=True)
        return 273 + 1350 * np.clip(Z / L[0], 0, 1) + 60 * np.sin(3 * np.pi * X / L[1]) * np.sin(np.pi * Z / L[0]) * np.cos(2 * np.pi * Y / L[2])
    eta = lambda T: np.clip(1e20 * np.exp(120e3 / (8.31446 * T) - 120e3 / (8.31446 * 1623)), 1e17, 1e23)
    Tn = field(grid)
    es, en, rho = eta(Tn), eta(field(mid)), 3300 / (3.5e-5 * (Tn - 1623) + 1)
    ctx = P3.Context3(n, grid)
    kw = {}
    if args.noslip:
        kw["bc"] = [0 if "zxy"[w % 3] in args.noslip else 1 for w in range(6)]
    if args.plug:
        kw["wallflow"] = [args.plug, None, None, args.plug, None, None]
    A, _ = P3.makeStokesMatrix(n, grid, es, en, rho, ctx=ctx, **kw)
    A.apply_bench(20, True)                                                        # warm-up
    apply_ms = [A.apply_bench(50, True) for _ in range(5)]
    P3.solve(A, resident=True)                                                     # warm-up (allocations, the power iteration's cold start)
    solves = []
    for _ in range(3):
        t0 = time.perf_counter()
        P3.solve(A, resident=True)
        solves.append(1e3 * (time.perf_counter() - t0))
    st = A.last_stats
    out["sizes"][str(nb)] = {"apply_scaled_ms": float(np.median(apply_ms)), "apply_scaled_ms_all": apply_ms, "solve_ms": float(np.median(solves)),
                             "solve_ms_all": solves, "iterations": int(st["iterations"]), "converged": int(st["converged"])}
    ctx.close()
print(json.dumps(out))
