"""A plain NumPy model of the 3-D yield stress, written from the statement of the definition in include/pylamp_hip.h
(pl3_stokes_set_yield) and DESIGN.md section 6c, "Yield stress"; the HIP kernel is compared with it in tests/test_hip_3d_yield.py.  No GPU,
no project code: NumPy, everything in np.longdouble.  The strain rates eDD, eDE and the node invariant are those of
tests/stokes3_strain_model.py, which tests/test_strain3_model.py ties to the operator models.

    tau_y(z)  = tau0 + dtau_dz (z - z[0])          at z_i for node i, at the cell's mid-point for the centres
    e_n       = the strainrate field of the strain model
    e_c       = sqrt(1/2 (sum_D eDD^2 + 2 sum_pairs m_p)),  m_p the plain mean of eDE^2 over the cell's four edges of pair p
    eta_eff   = min(eta_mat, max(tau_y / (2 e), eta_floor))                  yielded: eta_eff < eta_mat

Bound.  Per entry B = ((32 mag_e / e + 4) eps) tau_y / (2 e), with mag_e the magnitude of the invariant (the strain model's convention: the
same expression with |a| + |b| for every difference a - b, propagated through the root).  The invariant is within 32 eps of its magnitude
(the bound of tests/test_hip_3d_strain.py; the centre sum has 15 terms of about 5 eps each with exact power-of-two weights, halved by the
root), and tau_y and the quotient add four roundings.  Where the floor or the material value is taken the float64 result is exact, unless
the entry is ambiguous: |eta_mat - max(tau_y / (2 e), eta_floor)| <= B, which the test inputs avoid (tests/test_yield3_model.py).
"""
import numpy as np

import stokes3_flow_model as F
import stokes3_model as M
import stokes3_moving_model as V
import stokes3_strain_model as S
import stokes3_walls_model as W

LD = np.longdouble
EPS = np.finfo(np.float64).eps
_ld = S._ld


def tau_y(grid, n, tau0, dtau_dz):
    """(nodes, centres): tau_y along axis 0, broadcastable over (nz, nx, ny) and over the cells (nz - 1, nx - 1, ny - 1)."""
    z = _ld(grid[0])
    node = LD(tau0) + LD(dtau_dz) * (z - z[0])
    mid = LD(tau0) + LD(dtau_dz) * ((z[1:] + z[:-1]) / 2 - z[0])
    return S._along(node, 0), S._along(mid, 0)


def centre_invariant(res):
    """(e_c, its magnitude) over the cells from the components of S.strain_fields."""
    def radicand(dd, de):
        a = sum(q * q for q in dd)
        for p, (D, E, F) in enumerate(S.PAIRS):
            q = de[p] * de[p]                          # nodes along D and E, cells along F
            lo, hi = slice(0, -1), slice(1, None)
            m = 0
            for sd in (lo, hi):
                for se in (lo, hi):
                    m = m + S._take(S._take(q, D, sd), E, se)
            a = a + 2 * (m / 4)
        return a
    Y, MY = radicand(res["eDD"], res["eDE"]), radicand(res["mDD"], res["mDE"])
    e = np.sqrt(Y / 2)
    with np.errstate(divide="ignore", invalid="ignore"):
        mag = np.where(e > 0, MY / (4 * e), np.inf)
    return e, mag


def _limit(mat, tau, e, mag, floor):
    with np.errstate(divide="ignore", invalid="ignore"):
        lim = np.where(e > 0, tau / (2 * e), np.inf)
        B = np.where(e > 0, (32 * mag / e + 4) * EPS * tau / (2 * e), 0)
    lim = np.maximum(lim, LD(floor))
    eff = np.minimum(mat, lim)
    return eff, eff < mat, B, np.abs(mat - lim) <= B


def effective(nx, grid, etas, etan, v, tau0, dtau_dz, eta_floor, bc=None, wallvel=None, prev=None):
    """The update for the velocities v.  Returns a dict: etas_eff (nodes), etan_eff ((nz, nx, ny): the entries beyond the cells keep the
    material value), yielded_s / yielded_n (masks of the same shapes), B_s / B_n (the bound per entry; 0 beyond the cells), ambiguous_s /
    ambiguous_n, e_n / e_c (e_c over the cells), change = max |ln(eta_new / eta_prev)| against prev = (etas_prev, etan_prev) (None: the
    material arrays), min_eta."""
    n = [int(k) for k in nx]
    res = S.strain_fields(n, grid, etas, etan, v, bc=bc, wallvel=wallvel)
    tn, tc = tau_y(grid, n, tau0, dtau_dz)
    ms, mn = _ld(etas), _ld(etan)
    cells = tuple(slice(0, k - 1) for k in n)
    e_n, mag_n = res["strainrate"], res["mag"]["strainrate"]
    e_c, mag_c = centre_invariant(res)
    es, ys, Bs, amb_s = _limit(ms, tn + np.zeros(n, dtype=LD), e_n, mag_n, eta_floor)
    ec, yc, Bc, amb_c = _limit(mn[cells], tc + np.zeros(e_c.shape, dtype=LD), e_c, mag_c, eta_floor)
    en = mn.copy(); en[cells] = ec
    yn = np.zeros(n, dtype=bool); yn[cells] = yc
    Bn = np.zeros(n, dtype=LD); Bn[cells] = Bc
    an = np.zeros(n, dtype=bool); an[cells] = amb_c
    ps, pn = (ms, mn) if prev is None else (_ld(prev[0]), _ld(prev[1]))
    change = max(float(np.abs(np.log(es / ps)).max()), float(np.abs(np.log(en[cells] / pn[cells])).max()))
    return dict(etas_eff=es, etan_eff=en, yielded_s=ys, yielded_n=yn, B_s=Bs, B_n=Bn, ambiguous_s=amb_s, ambiguous_n=an, e_n=e_n, e_c=e_c,
                change=change, min_eta=min(float(es.min()), float(en.min())), strain=res)


def node_stress(nx, grid, etas, etan, v, bc=None, wallvel=None):
    """The stress field of the strain model (second invariant of the deviatoric stress at the nodes)."""
    return S.strain_fields(nx, grid, etas, etan, v, bc=bc, wallvel=wallvel)["stress"]


def direct(nx, grid, etas, etan, rho, bc=None, wallvel=None, grav=None, strict=True, reuse=None, keep=None, wallflow=None):
    """The model's direct solve of the operator's own right-hand side with the viscosities (etas, etan): the flat float64 solution, the
    pressure Kcont-scaled.  wallflow (None: no flow): the flow through the six walls, which enters the right-hand side alone
    (stokes3_flow_model.stokes_rhs).  reuse: a solver of a nearby operator (one `keep` has received) whose factors precondition the refinement
    with THIS operator's longdouble residual -- the same solution to the same tolerance, without a factorisation of its own; if the
    refinement does not get there, the operator is factorised after all.  keep (a list): gains the solver used."""
    n = [int(k) for k in nx]
    es, en = np.asarray(etas, dtype=np.float64), np.asarray(etan, dtype=np.float64)
    ap = lambda x, rounded=True: W.stokes_apply(n, grid, es, en, x, bc=bc, strict=strict, rounded=rounded)
    if wallflow is None:
        b = V.stokes_rhs(n, grid, es, en, rho, grav=grav, bc=bc, wallvel=wallvel, strict=strict)
    else:
        b = F.stokes_rhs(n, grid, es, en, rho, grav=grav, bc=bc, wallvel=wallvel, wallflow=wallflow, strict=strict)
    if reuse is not None:
        near = M.DirectSolver.__new__(M.DirectSolver)
        near.apply, near.dr, near.dc, near.lu = ap, reuse.dr, reuse.dc, reuse.lu
        try:
            return np.asarray(near.solve(b, maxref=30), dtype=np.float64)
        except Exception:
            pass
    solver = M.DirectSolver(M.assemble(ap, n), ap)
    if keep is not None:
        keep.append(solver)
    return np.asarray(solver.solve(b), dtype=np.float64)


def picard(nx, grid, etas, etan, rho, tau0, dtau_dz, eta_floor, maxit, tol=0.0, bc=None, wallvel=None, grav=None, strict=True, perturb=None,
           reuse=None, wallflow=None):
    """The loop of the step: solve with the material viscosities, update, and while the change is above tol and fewer than maxit solves
    have run solve with the effective ones and update again.  perturb (None: nothing) is called as perturb(x) on every direct solution and
    returns the vector the loop goes on with.  wallflow: as in direct.  reuse: the `solvers` of an earlier, nearby run (see direct).  Returns a dict: solvers (one per
    iteration), x (the last solution), etas_eff, etan_eff (after the last update), change
    (per iteration), yielded_nodes, yielded_cells, converged."""
    n = [int(k) for k in nx]
    es, en = np.asarray(etas, dtype=np.float64), np.asarray(etan, dtype=np.float64)
    out = dict(change=[], yielded_nodes=[], yielded_cells=[], solvers=[])
    prev = None
    while True:
        k = len(out["change"])
        x = direct(n, grid, es, en, rho, bc=bc, wallvel=wallvel, grav=grav, strict=strict, keep=out["solvers"], wallflow=wallflow,
                   reuse=reuse[k] if reuse is not None and k < len(reuse) else None)
        if perturb is not None:
            x = perturb(x)
        X = x.reshape(n + [4])
        u = effective(n, grid, etas, etan, [X[..., q] for q in range(3)], tau0, dtau_dz, eta_floor, bc=bc, wallvel=wallvel, prev=prev)
        out["change"].append(u["change"]); out["yielded_nodes"].append(int(u["yielded_s"].sum())); out["yielded_cells"].append(int(u["yielded_n"].sum()))
        es, en = u["etas_eff"].astype(np.float64), u["etan_eff"].astype(np.float64)
        prev = (es, en)
        if not u["change"] > tol or len(out["change"]) >= maxit:
            break
    out.update(x=x, etas_eff=es, etan_eff=en, converged=bool(out["change"][-1] <= tol), iterations=len(out["change"]))
    return out
