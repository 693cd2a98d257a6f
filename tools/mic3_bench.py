"""Times the resident 3-D marker stages -- scatter of a step's field list, temperature to tracers, RK4 (+ the re-sort) -- and
writes one JSON line.  Device-event times of the stages' kernel windows (pl3_resident_times), median over the repetitions after
a warm-up; bytes per tracer are the algorithmic minimum, the roof is 8 TB/s.

    python tools/mic3_bench.py [--n 129] [--per-axis 2] [--reps 20] [--warmup 3] [--out profiles/mic3_129.json] [--search | --graded R]

--search runs the stages with the per-axis cell search (Options3.marker_search) on the same regular grid; --graded R on a grid
whose spacings grow smoothly by the factor R along every axis (search on; every cell keeps its per-axis^3 tracers).  The JSON line
then carries "search" and "graded".

--sort-only times the end-of-step sort alone, in up to three states, and writes profiles/mic3_129_refill.json:
  sort_off       RK4 + sort with injection off (the only state a tree without Simulation3.refill has),
  sort_on_idle   the same with tracdens = 8, tracdens_min = 4 and no deficient cell (the two alternate inside one loop),
  sort_on_1pct   sort + refill of a set in which 1 % of the cells were thinned to 2 tracers (uploaded afresh for every repetition:
                 a refilled set has nothing left to inject), --refill-reps repetitions.
--parent FILE [FILE ...] embeds the sort_off figures that the same script wrote for another tree (the parent commit's), run in
separate processes alternating with this one, and reports the run-to-run spread of both next to the medians.

--delete runs with the fence off and the marker deletion on (Options3.tracs_fence_enabled = False, marker_deletion = True): the
stages and --step as they are (nothing leaves the box: what the switch itself costs), and --sort-only as two states written to
profiles/mic3_129_delete.json:
  sort_none_leaving   RK4 + deleting sort of a set that stays where it is,
  sort_layer_leaving  the same under a uniform velocity along +z that carries the outermost cell layer out of the box (uploaded
                      afresh for every repetition, --refill-reps repetitions),
  sort_layer_fenced   that motion with the fence on and deletion off: every tracer changes its cell, none leaves.
--off FILE [FILE ...] / --parent FILE [FILE ...] embed, per stage, the figures the plain script wrote for this tree with deletion off
and for the parent commit's tree (separate processes, alternating), with the ratio of the medians and both run-to-run spreads.

--inflow times the refilling sort along an inflow wall and writes profiles/mic3_129_inflow.json: a plug flow z0 -> zL is set (fence
off, deletion on), the cell layer along z0 is thinned to 2 of its 8 tracers per cell and uploaded afresh for every repetition
(--refill-reps), and pl3_resident_refill tops the layer up -- one wave of k_m3_inject per cell of the layer:
  sort_layer_refill   no inflow material: k_m3_inject<false>, every new tracer the mean of its cell,
  sort_layer_inflow   a material {TR_MAT, TR_TMP, TR_RH0} on z0: k_m3_inject<true>, the new tracers below the lowest resident take it
(the two alternate inside one loop).  --parent-sort / --this-sort FILE ... and --parent-step / --this-step FILE ... embed what
--sort-only and --step --resident wrote for the parent commit's tree and for this one without a material (separate processes,
alternating): the sort with refill (sort_on_1pct) and the resident step, ratio of the medians next to the parent's own spread.

--step [--resident] times whole steps of Simulation3 -- the falling sphere with heat on, --n nodes per axis, 8 tracers per cell:
host wall time per step (device synchronisation, then perf_counter, on either side of step()), median and min-max over --reps
steps after --warmup, and the medians of the stage times (device events); writes profiles/mic3_step_129.json unless --out says
otherwise.  --resident selects Options3.resident (one pl3_resident_step call per step, the grid fields stay on the device).
--warm switches Options3.stokes_warm_start on (three solutions kept, quadratic extrapolation) and adds how the timed solves started
and the guard's residuals; writes profiles/mic3_step_129_warm.json unless --out says otherwise (profiles/stokes3_warm.json holds the
medians of three such processes alternating with three without --warm).
--yield TAU switches Options3.yield_stress on (with --picard-maxit / --picard-tol) and adds every timed step's Picard figures.
--shear-heating switches Options3.shear_heating on (the dissipation of the Stokes solution is added to H before the heat solve; --out is
wanted: profiles/strain3.json holds the medians of three such processes next to three without).
--tree DIR imports pylamp_amd from another checkout: the host-staged yardstick is run on the parent commit's library, in
separate processes alternating with the resident runs of this one.
"""
import argparse
import json
import os
import sys

import numpy as np

_TREE = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv[1:-1] else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.abspath(_TREE))
from pylamp_amd import pylamp3d as P3                                             # noqa: E402

ROOF = 8.0e12
# positions 24 B; scatter reads the 7 columns rho, eta, cp, T, H, mat, k and writes 10 nodal fields (80 B per node, one node per cell);
# gather reads and writes T; RK4 writes the new position and the velocity
BYTES = dict(scatter=lambda tpc: 24 + 56 + 80.0 / tpc, gather=lambda tpc: 24 + 16, gather_subgrid=lambda tpc: 24 + 16 + 32 + 8.0 / tpc,
             rk4=lambda tpc: 72, sort=lambda tpc: 2 * 8 * 19 + 12)      # sort: every one of the 19 columns read and written, key + index


def _stat(v, n):
    ms = float(np.median(v))
    return dict(ms=round(ms, 4), ms_min=round(float(np.min(v)), 4), ms_max=round(float(np.max(v)), 4), ps_per_tracer=round(ms * 1e9 / n, 2), reps=len(v))


def _delete_kw(a):
    return dict(tracs_fence_enabled=False, marker_deletion=True) if a.delete else {}


def _spread(files, pick):
    """Median and min-max over the medians that separate processes wrote."""
    v = [pick(json.loads(open(f).read())) for f in files]
    return dict(ms=round(float(np.median(v)), 4), ms_min=round(float(np.min(v)), 4), ms_max=round(float(np.max(v)), 4), runs=len(v))


def sort_delete(a):
    """The deleting sort: nothing leaving, and one cell layer leaving."""
    nx = [a.n] * 3; L = [100e3] * 3
    rng = np.random.default_rng(0)
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, rng, per_axis=a.per_axis)
    n = tr_x.shape[0]
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(**_delete_kw(a)))
    h = L[0] / (a.n - 1); dt = 1e12
    vel = [rng.standard_normal(nx) * (1e-3 * h / dt) for _ in range(3)]
    grids, V = P3.advection_velocity(vel, sim.gridmp, nx)
    t = []
    for rep in range(a.warmup + a.reps):
        c = sim.advect(grids, V, dt)
        assert c["nremoved"] == 0, c
        if rep >= a.warmup:
            t.append(sim.stage_times()["sort"])
    out = dict(config="mic3_%d_delete" % a.n, nodes=a.n ** 3, tracers=n, reps=a.reps, warmup=a.warmup, states=dict(sort_none_leaving=_stat(t, n)))
    W = [np.zeros_like(V[0]) for _ in range(3)]
    W[0][...] = 1.5 * h / dt                     # the reference's weights (1,1,1,1)/6 carry a tracer 2/3 w dt: one cell
    t, gone = [], 0
    for rep in range(1 + a.refill_reps):
        sim.upload(tr_x, tr_f)
        c = sim.advect(grids, W, dt)
        gone = c["nremoved"]
        if rep >= 1:
            t.append(sim.stage_times()["sort"])
    out["states"]["sort_layer_leaving"] = dict(_stat(t, n), removed=int(gone), tracers_after=int(sim.count()))
    sim.close()
    # the same motion with the fence on and deletion off: what moving every tracer by one cell costs the sort by itself
    sim = P3.Simulation3(nx, L, tr_x, tr_f)
    t = []
    for rep in range(1 + a.refill_reps):
        sim.upload(tr_x, tr_f)
        sim.advect(grids, W, dt)
        if rep >= 1:
            t.append(sim.stage_times()["sort"])
    out["states"]["sort_layer_fenced"] = _stat(t, n)
    sim.close()
    return out


def sort_only(a):
    nx = [a.n] * 3; L = [100e3] * 3
    rng = np.random.default_rng(0)
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, rng, per_axis=a.per_axis)
    n = tr_x.shape[0]
    have = hasattr(P3.Simulation3, "refill")
    sim = P3.Simulation3(nx, L, tr_x, tr_f)
    h = L[0] / (a.n - 1); dt = 1e12
    vel = [rng.standard_normal(nx) * (1e-3 * h / dt) for _ in range(3)]          # the tracers stay where they are
    grids, V = P3.advection_velocity(vel, sim.gridmp, nx)
    t = dict(sort_off=[], sort_on_idle=[])
    for rep in range(a.warmup + a.reps):
        for key, dens, dmin in (("sort_off", 0, 0), ("sort_on_idle", 8, 4)):
            if key != "sort_off" and not have:
                continue
            sim.opt.tracdens, sim.opt.tracdens_min = dens, dmin
            c = sim.advect(grids, V, dt)
            assert not have or c["ninjected"] == 0, c
            if rep >= a.warmup:
                t[key].append(sim.stage_times()["sort"])
    out = dict(config="mic3_%d_sort" % a.n, nodes=a.n ** 3, tracers=n, reps=a.reps, warmup=a.warmup, states={})
    out["states"]["sort_off"] = _stat(t["sort_off"], n)
    if have:
        out["states"]["sort_on_idle"] = _stat(t["sort_on_idle"], n)
        # 1 % of the cells thinned to 2 of their tracers
        m = (a.n - 1) ** 3
        cell = np.zeros(n, dtype=np.int64)
        for d in range(3):
            cell = cell * (a.n - 1) + np.clip(np.floor(tr_x[:, d] / h).astype(np.int64), 0, a.n - 2)
        thin = np.zeros(m, dtype=bool); thin[rng.choice(m, m // 100, replace=False)] = True
        order = np.argsort(cell, kind="stable")
        first = np.concatenate([[0], np.cumsum(np.bincount(cell, minlength=m))[:-1]])
        rank = np.empty(n, dtype=np.int64); rank[order] = np.arange(n) - first[cell[order]]
        keep = ~thin[cell] | (rank < 2)
        sx, sf = np.ascontiguousarray(tr_x[keep]), np.ascontiguousarray(tr_f[keep])
        del tr_x, tr_f, cell, order, rank
        sim.opt.tracdens, sim.opt.tracdens_min = 8, 4
        ts, inj = [], 0
        for rep in range(1 + a.refill_reps):
            sim.upload(sx, sf)
            c = sim.refill(it=1)
            inj = c["ninjected"]
            if rep >= 1:
                ts.append(sim.stage_times()["sort"])
        out["states"]["sort_on_1pct"] = dict(_stat(ts, sx.shape[0]), tracers_before=int(sx.shape[0]), cells_refilled=int(c["nrefilled"]), injected=int(inj))
    if a.parent:
        runs = [json.loads(open(f).read())["states"]["sort_off"] for f in a.parent]
        out["parent_sort"] = dict(ms=round(float(np.median([r["ms"] for r in runs])), 4), runs=runs)
    sim.close()
    return out


def sort_inflow(a):
    """The refill of the cell layer along an inflow wall, without and with a material on that wall."""
    nx = [a.n] * 3; L = [100e3] * 3
    rng = np.random.default_rng(0)
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, rng, per_axis=a.per_axis)
    h = L[0] / (a.n - 1)
    layer = tr_x[:, 0] < h
    cell = np.clip(np.floor(tr_x[:, 1] / h).astype(np.int64), 0, a.n - 2) * (a.n - 1) + np.clip(np.floor(tr_x[:, 2] / h).astype(np.int64), 0, a.n - 2)
    order = np.argsort(np.where(layer, cell, -1), kind="stable")
    key = np.where(layer, cell, -1)[order]
    rank = np.empty(tr_x.shape[0], dtype=np.int64)
    rank[order] = np.arange(key.size) - np.searchsorted(key, key, side="left")
    keep = ~layer | (rank < 2)
    sx, sf = np.ascontiguousarray(tr_x[keep]), np.ascontiguousarray(tr_f[keep])
    del tr_x, tr_f, cell, order, key, rank
    n = sx.shape[0]
    U = 1e-9
    sim = P3.Simulation3(nx, L, options=P3.Options3(tracs_fence_enabled=False, marker_deletion=True, tracdens=8, tracdens_min=4,
                                                    bcstokesflow=[U, None, None, U, None, None]))
    mat = [{P3.TR_MAT: 3, P3.TR_TMP: 1500.0, P3.TR_RH0: 3200.0}, None, None, None, None, None]
    t = dict(sort_layer_refill=[], sort_layer_inflow=[])
    last = {}
    for rep in range(1 + a.refill_reps):
        for key, m in (("sort_layer_refill", None), ("sort_layer_inflow", mat)):
            sim.set_inflow_material(m)
            sim.upload(sx, sf)
            last[key] = sim.refill(it=1)
            if rep >= 1:
                t[key].append(sim.stage_times()["sort"])
    sim.close()
    out = dict(config="mic3_%d_inflow" % a.n, nodes=a.n ** 3, tracers_before=n, refill_reps=a.refill_reps, states={})
    for key in t:
        out["states"][key] = dict(_stat(t[key], n), cells_refilled=int(last[key]["nrefilled"]), injected=int(last[key]["ninjected"]),
                                  inflow=int(last[key].get("ninflow", 0)))
    out["inflow_over_refill"] = round(out["states"]["sort_layer_inflow"]["ms"] / out["states"]["sort_layer_refill"]["ms"], 4)
    for name, mine, theirs, pick in (("sort_on_1pct", a.this_sort, a.parent_sort, lambda r: r["states"]["sort_on_1pct"]["ms"]),
                                     ("resident_step", a.this_step, a.parent_step, lambda r: r["step_ms"])):
        if mine and theirs:
            me, pa = _spread(mine, pick), _spread(theirs, pick)
            out["no_material_" + name] = dict(this=me, parent=pa, ratio=round(me["ms"] / pa["ms"], 4),
                                              parent_spread=round((pa["ms_max"] - pa["ms_min"]) / pa["ms"], 4))
    return out


def step_bench(a):
    import time
    import torch
    nx = [a.n] * 3; L = [100e3] * 3
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, np.random.default_rng(0), per_axis=a.per_axis)
    n = tr_x.shape[0]
    tr_f[:, 3] = 273 + 1350 * tr_x[:, 0] / L[0]; tr_f[:, 4] = 4.0; tr_f[:, 5] = 1250; tr_f[:, 7] = 3.5e-5; tr_f[:, 11] = 1e-9
    kw = dict(resident=True) if a.resident else {}
    if a.warm:
        kw["stokes_warm_start"] = True
    if a.shear_heating:
        kw["shear_heating"] = True
    if a.yield_stress is not None:
        kw.update(yield_stress=a.yield_stress, picard_maxit=a.picard_maxit, picard_tol=a.picard_tol)
    sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(**kw, **_delete_kw(a)))
    del tr_x, tr_f
    wall, stages, its, starts, guard, picard = [], {}, [], [], [], []
    for rep in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = sim.step()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        assert r["stokes"]["converged"] == 1 and r["heat"]["converged"] == 1, r
        if rep >= a.warmup:
            wall.append(ms); its.append(r["stokes"]["iterations"])
            if "picard" in r:
                picard.append(r["picard"])
            if a.warm:
                h = sim.ctx.history_info()
                starts.append(r["stokes_start"]); guard.append(h["r0"] / h["ref"] if h["ref"] > 0 else None)
            st = dict(sim.stage_times(), stokes=r["stokes"]["solve_ms"], heat=r["heat"]["solve_ms"])
            for k, v in st.items():
                stages.setdefault(k, []).append(v)
    out = dict(config="mic3_%d_step" % a.n, mode="resident" if a.resident else "staged", delete=bool(a.delete), tree=a.tree or ".", nodes=a.n ** 3, tracers=n,
               reps=a.reps, warmup=a.warmup, step_ms=round(float(np.median(wall)), 2), step_ms_min=round(float(np.min(wall)), 2),
               step_ms_max=round(float(np.max(wall)), 2), stokes_iterations=its,
               stage_ms={k: round(float(np.median(v)), 3) for k, v in stages.items()})
    if a.shear_heating:
        out.update(shear_heating=True, dissipation_total=r["dissipation_total"])
    if picard:          # (stage_ms["stokes"] is the LAST solve of a step's Picard loop)
        out.update(yield_stress=a.yield_stress, picard_maxit=a.picard_maxit, picard_tol=a.picard_tol, picard=picard)
    if a.warm:          # r0_over_ref: the guard's |r0| / ref of every timed solve (below 1: the extrapolated start was taken)
        out.update(warm_start=list(sim.warm_start), stokes_start=starts, r0_over_ref=[None if g is None else float("%.3e" % g) for g in guard])
    # what the stage times do not cover: host work and copies (staged: "scatter" is the LAST of the step's five scatters alone)
    out["other_ms"] = round(out["step_ms"] - sum(out["stage_ms"].values()), 2)
    if hasattr(sim, "transfer_stats"):
        sim.transfer_stats(reset=True); sim.step()
        out["transfers_per_step"] = sim.transfer_stats()
    sim.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=129); ap.add_argument("--per-axis", type=int, default=2)
    ap.add_argument("--reps", type=int, default=20); ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sort-only", action="store_true"); ap.add_argument("--refill-reps", type=int, default=7)
    ap.add_argument("--parent", nargs="*", default=[])
    ap.add_argument("--step", action="store_true"); ap.add_argument("--resident", action="store_true"); ap.add_argument("--tree", default=None)
    ap.add_argument("--warm", action="store_true"); ap.add_argument("--shear-heating", action="store_true")
    ap.add_argument("--search", action="store_true"); ap.add_argument("--graded", type=float, default=0.0)
    ap.add_argument("--delete", action="store_true"); ap.add_argument("--off", nargs="*", default=[])
    ap.add_argument("--inflow", action="store_true")
    ap.add_argument("--yield", dest="yield_stress", type=float, default=None); ap.add_argument("--picard-maxit", type=int, default=10)
    ap.add_argument("--picard-tol", type=float, default=1e-2)
    for name in ("--parent-sort", "--this-sort", "--parent-step", "--this-step"):
        ap.add_argument(name, nargs="*", default=[])
    a = ap.parse_args()
    if a.out is None and not a.inflow:
        a.out = os.path.join("profiles", ("mic3_step_129_warm.json" if a.warm else "mic3_step_129.json") if a.step else ("mic3_129_delete.json" if a.sort_only and a.delete else
                                                                              ("mic3_129_refill.json" if a.sort_only else "mic3_129.json")))
    if a.inflow and a.out is None:
        a.out = os.path.join("profiles", "mic3_129_inflow.json")
    if a.inflow or a.sort_only or a.step:
        line = json.dumps(sort_inflow(a) if a.inflow else (step_bench(a) if a.step else (sort_delete(a) if a.delete else sort_only(a))))
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
        print(line)
        return
    nx = [a.n] * 3; L = [100e3] * 3
    rng = np.random.default_rng(0)
    tr_x, tr_f = P3.falling_sphere_tracers(nx, L, rng, per_axis=a.per_axis)
    n = tr_x.shape[0]
    tr_f[:, 3] = 273 + 1350 * tr_x[:, 0] / L[0]; tr_f[:, 4] = 4.0; tr_f[:, 5] = 1250; tr_f[:, 7] = 3.5e-5; tr_f[:, 9] = 120e3
    if a.graded > 0.0:
        # the lattice mapped cell by cell onto the graded grid: the same tracers per cell as on the regular one
        grid = [P3.graded_grid(a.n, L[d], a.graded) for d in range(3)]
        for d in range(3):
            u = tr_x[:, d] / (L[d] / (a.n - 1))
            i = np.clip(np.floor(u).astype(np.int64), 0, a.n - 2)
            tr_x[:, d] = grid[d][i] + (u - i) * (grid[d][i + 1] - grid[d][i])
        tr_x = np.clip(tr_x, 1e-6 * L[0], (1 - 1e-6) * L[0])
        sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(marker_search=True), grid=grid)
    elif a.search:
        sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(marker_search=True))
    else:
        sim = P3.Simulation3(nx, L, tr_x, tr_f, P3.Options3(**_delete_kw(a)))
    del tr_x, tr_f
    h = L[0] / (a.n - 1)
    dT = rng.standard_normal(nx)
    dt = 1e12
    vel = [rng.standard_normal(nx) * (1e-3 * h / dt) for _ in range(3)]          # the tracers stay where they are: every repetition sees the same load
    grids, V = P3.advection_velocity(vel, sim.gridmp, nx)
    t = {k: [] for k in ("scatter", "gather", "gather_subgrid", "rk4", "sort")}
    mp, g = sim.gridmp, sim.grid
    sets = [([0, 1, 5, 3, 11, 8], [5, 6, 5, 5, 5, 5], g), ([1], [6], mp), ([4], [5], [mp[0], g[1], g[2]]), ([4], [5], [g[0], mp[1], g[2]]),
            ([4], [5], [g[0], g[1], mp[2]])]
    for rep in range(a.warmup + a.reps):
        sim.update_properties()
        ms = 0.0
        for cols, sch, tg in sets:
            sim.scatter(cols, sch, tg); ms += sim.stage_times()["scatter"]
        sim.opt.do_subgrid_heatdiff = False
        sim.temp_to_tracers(dT, False, dt); tg_ = sim.stage_times()["gather"]
        sim.opt.do_subgrid_heatdiff = True
        sim.temp_to_tracers(-dT, False, dt); ts_ = sim.stage_times()["gather"]
        sim.advect(grids, V, dt); st = sim.stage_times()
        if rep >= a.warmup:
            t["scatter"].append(ms); t["gather"].append(tg_); t["gather_subgrid"].append(ts_); t["rk4"].append(st["rk4"]); t["sort"].append(st["sort"])
    tpc = n / float((a.n - 1) ** 3)
    out = dict(config="mic3_%d" % a.n, nodes=a.n ** 3, tracers=n, tracers_per_cell=tpc, reps=a.reps, warmup=a.warmup, stages={})
    if a.search or a.graded > 0.0:
        out["search"] = True; out["graded"] = a.graded
    if a.tree:
        out["tree"] = a.tree
    if a.delete:
        out["delete"] = True
    for k, v in t.items():
        ms = float(np.median(v)); b = BYTES[k](tpc)
        out["stages"][k] = dict(ms=round(ms, 4), ms_min=round(float(np.min(v)), 4), ms_max=round(float(np.max(v)), 4),
                                ps_per_tracer=round(ms * 1e9 / n, 2), bytes_per_tracer=round(b, 1), fraction_of_8TBs_roof=round(b * n / (ms * 1e-3) / ROOF, 4))
    for name, files in (("off", a.off), ("parent", a.parent)):
        if files:
            out[name] = {k: _spread(files, lambda r, k=k: r["stages"][k]["ms"]) for k in t}
    if a.off and a.parent:
        out["off_over_parent"] = {k: round(out["off"][k]["ms"] / out["parent"][k]["ms"], 4) for k in t}
    if a.off:
        out["on_over_off"] = {k: round(out["stages"][k]["ms"] / out["off"][k]["ms"], 4) for k in t}
    sim.close()
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
