"""3-D staggered Stokes + heat on HIP kernels (BASELINE config 5) -- pinned to the NumPy model tests/stokes3_model.py.

The reference implements DIM = 2 only (pylamp_const.py:6; pylamp_stokes.gidx prints "NOT IMPLEMENTED" for dim != 2,
pylamp_stokes.py:30-35).  What it fixes is the intent: axis order z, x, y (pylamp_const.py:9-13), arrays (nz, nx, ny),
IP = DIM = 3 and the DOF order of the comment at pylamp_stokes.py:24.  The functions below mirror the 2-D module API
(makeStokesMatrix / x2vp / solve, makeDiffusionMatrix / x2t / solve) with those conventions; the operators extend the
2-D rows dimension by dimension (pylamp_amd/csrc/pl_3d.hip) so that a y-invariant extrusion reproduces the 2-D
operator and solution on every y-slice.  The row rules are written out in DESIGN.md section 6c.
"""
import ctypes as C
import weakref

import numpy as np

from . import _lib

DIM3 = 3
IZ, IX, IY, IP3 = 0, 1, 2, 3
BC_TYPE_NOSLIP = 0
BC_TYPE_FREESLIP = 1
WALL_NAMES = ("z0", "x0", "y0", "zL", "xL", "yL")
BC_TYPE_FIXTEMP = 0
BC_TYPE_FIXFLOW = 1
DEFAULT_RTOL = 1e-7        # residual bound; the solve also has to meet the velocity-error estimate 3e-8 (as pylamp_stokes.solve)
DEFAULT_MAXIT = 600
# StokesOperator3.krylov_probe / work_vector (include/pylamp_hip.h at pl3_krylov_probe, pl3_stokes_work_vector)
PROBE_DOTS, PROBE_DOTS11, PROBE_AXPBY, PROBE_P, PROBE_XR, PROBE_XRP, PROBE_RANDOM = range(7)
WORK_R, WORK_RT, WORK_S, WORK_DX, WORK_B, WORK_W = 0, 1, 4, 8, 10, 13


def gidx(idxs, nx):
    """iz*nx*ny*4 + ix*ny*4 + iy*4 (+ IZ / IX / IY / IP3 for the equation): the order of the comment at pylamp_stokes.py:24."""
    if len(idxs) != 3:
        raise Exception("num of idxs != dimensions")
    return idxs[IZ] * nx[IX] * nx[IY] * 4 + idxs[IX] * nx[IY] * 4 + idxs[IY] * 4


def x2vp(x, nx):
    """([vz, vx, vy], P), each (nz, nx, ny); pressure in Kcont-scaled units, ghosts retained (cf. pylamp_stokes.py:86-101)."""
    X = np.asarray(x).reshape(int(nx[0]), int(nx[1]), int(nx[2]), 4)
    return [X[..., 0], X[..., 1], X[..., 2]], X[..., 3]


def x2t(x, nx):
    return np.asarray(x).reshape(int(nx[0]), int(nx[1]), int(nx[2]))


def stokes_walls(bc, who="3-D Stokes"):
    """bc = [z0, x0, y0, zL, xL, yL] (None: all free-slip) as six ints; a kind other than FREESLIP / NOSLIP is rejected with
    the wall's name and the value (CYCLIC and FLOWTHRU walls do not exist in 3-D)."""
    if bc is None:
        return [BC_TYPE_FREESLIP] * 6
    bc = list(bc)
    if len(bc) != 6:
        raise Exception("%s: the wall kinds need six entries [z0, x0, y0, zL, xL, yL] (got %d)" % (who, len(bc)))
    for w, b in enumerate(bc):
        if b not in (BC_TYPE_FREESLIP, BC_TYPE_NOSLIP) or int(b) != b:
            raise Exception("%s: wall %s has kind %r: a wall is BC_TYPE_FREESLIP (1) or BC_TYPE_NOSLIP (0)" % (who, WALL_NAMES[w], b))
    return [int(b) for b in bc]


VEL_NAMES = ("Uz", "Ux", "Uy")


def wall_velocities(wallvel, bc=None, who="3-D Stokes"):
    """wallvel: the velocities U_w = (Uz, Ux, Uy) of the six walls [z0, x0, y0, zL, xL, yL] as a (6, 3) array (None: all at rest).
    The checks and messages of pl3_stokes_set_wall_velocity: every entry finite, the component normal to the wall zero
    (through-flow needs the marker deletion path, which is not built in 3-D) and -- where the kinds bc are given -- a non-zero
    velocity on a NOSLIP wall only."""
    if wallvel is None:
        return np.zeros((6, 3))
    try:
        v = np.array(wallvel, dtype=np.float64)
    except (TypeError, ValueError):
        v = None
    if v is None or v.shape != (6, 3):
        raise Exception("%s: the wall velocities need the shape (6, 3): (Uz, Ux, Uy) for each of [z0, x0, y0, zL, xL, yL]" % who)
    for w in range(6):
        for q in range(3):
            if not np.isfinite(v[w, q]):
                raise Exception("%s: wall %s has a non-finite velocity component %s = %r" % (who, WALL_NAMES[w], VEL_NAMES[q], float(v[w, q])))
        if v[w, w % 3] != 0.0:
            raise Exception("%s: wall %s has the normal velocity component %s = %r: only the tangential components may be non-zero -- "
                            "flow through a wall needs the marker deletion path, which is not built in 3-D"
                            % (who, WALL_NAMES[w], VEL_NAMES[w % 3], float(v[w, w % 3])))
        if bc is not None and v[w].any() and int(bc[w]) != BC_TYPE_NOSLIP:
            raise Exception("%s: wall %s is FREESLIP and cannot move with velocity %s: only a NOSLIP wall carries a velocity"
                            % (who, WALL_NAMES[w], tuple(float(u) for u in v[w])))
    return v


FLOW_AXES = ((1, 2), (0, 2), (0, 1))        # the two axes p < q of a wall plane of axis a, in z, x, y order
_AXIS_N = ("nz", "nx", "ny")


def _plane_shape(nx, w, nodes=False):
    """(shape, its two extents as text) of wall w's plane over the wall's faces, or over its nodes ("Wall planes")."""
    p, q = FLOW_AXES[w % 3]
    if nodes:
        return (int(nx[p]), int(nx[q])), (_AXIS_N[p], _AXIS_N[q])
    return (int(nx[p]) - 1, int(nx[q]) - 1), (_AXIS_N[p] + " - 1", _AXIS_N[q] + " - 1")


def _six_entries(entries, who, needs, names=None, each=""):
    """The six per-wall entries of a setting as a list: None gives six None, a dict by wall name is spread over the walls where the
    caller allows it (names: its words for the error about an unknown name), anything else has to be six entries long."""
    if entries is None:
        return [None] * 6
    if isinstance(entries, dict) and names is not None:
        for k in entries:
            if k not in WALL_NAMES:
                raise Exception("%s: %s a wall '%s' (the walls are %s)" % (who, names, k, ", ".join(WALL_NAMES)))
        return [entries.get(k) for k in WALL_NAMES]
    try:
        six = None if isinstance(entries, dict) else list(entries)
    except TypeError:
        six = None
    if six is None:
        raise Exception("%s: %s six entries [z0, x0, y0, zL, xL, yL]%s (got %s)" % (who, needs, each, type(entries).__name__))
    if len(six) != 6:
        raise Exception("%s: %s six entries [z0, x0, y0, zL, xL, yL] (got %d)" % (who, needs, len(six)))
    return six


def _checked_plane(value, shape, extents, who, needs, has, read=None):
    """value, a scalar (broadcast) or an array of the given shape, as a contiguous float64 plane.  needs / has: the subjects of the two
    errors, a wrong shape and the first non-finite entry; read: the mask of the entries that are checked (None: all)."""
    try:
        a = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        a = None
    if a is not None and a.ndim == 0:
        a = np.full(shape, float(a))
    if a is None or a.shape != shape:
        raise Exception("%s: %s the shape (%s, %s) = %r or a scalar (got %s)"
                        % (who, needs, extents[0], extents[1], shape, "an object that is no array" if a is None else a.shape))
    bad = np.argwhere(~np.isfinite(a) if read is None else ~np.isfinite(a) & read)
    if bad.size:
        i, j = (int(v) for v in bad[0])
        raise Exception("%s: %s [%d, %d] = %r" % (who, has, i, j, float(a[i, j])))
    return np.ascontiguousarray(a)


def wall_flows(flow, nx, who="3-D Stokes"):
    """flow: the wall-normal velocities through the six walls [z0, x0, y0, zL, xL, yL] -- a list of six entries (or a dict by wall
    name), each None (no flow), a scalar (the constant profile) or an array Un of shape (n_p - 1, n_q - 1) over the wall's faces, p < q
    the two other axes in z, x, y order; the value is the component along +a, so positive is inflow on z0, x0, y0 and outflow on zL,
    xL, yL.  None: no flow anywhere.  Returns six entries, None or a contiguous float64 array; shapes and non-finite entries are
    rejected by name (the rule is in include/pylamp_hip.h at pl3_stokes_set_wall_flow)."""
    out = []
    for w, f in enumerate(_six_entries(flow, who, "the wall flow needs", "the wall flow names")):
        name = WALL_NAMES[w]
        out.append(None if f is None else _checked_plane(f, *_plane_shape(nx, w), who, "the flow of wall %s needs" % name,
                                                         "wall %s has a non-finite flow entry" % name))
    return out


def wall_heat_values(values, nx, who="3-D heat"):
    """values: the boundary values of the six heat walls [z0, x0, y0, zL, xL, yL] as profiles -- a list of six entries (or a dict by
    wall name), each None (the wall keeps its one value of bcvalue), a scalar (the constant plane) or an array of shape (n_p, n_q) over
    the wall's NODES, p < q the two other axes in z, x, y order: (nx, ny) on z-walls, (nz, ny) on x-walls, (nz, nx) on y-walls.  An
    entry is the node's temperature on a FIXTEMP wall and k dT/dx_a along +a on a FIXFLOW wall, low or high (so the heat flow into the
    box per area is -v on z0, x0, y0 and +v on zL, xL, yL).  None: no planes.  Returns six entries, None or a contiguous float64
    array.  z-walls own their edges, then x-walls, then y-walls: entries at nodes another wall owns (rows 0 and nz - 1 of an x- or
    y-wall's plane, also columns 0 and nx - 1 of a y-wall's) are never read and not checked; a non-finite entry that is read and a
    wrong shape are rejected by name (the rule is in include/pylamp_hip.h at pl3_heat_set_wall_values)."""
    out = []
    for w, f in enumerate(_six_entries(values, who, "the heat wall values need", "the heat wall values name")):
        if f is None:
            out.append(None)
            continue
        a, name = w % 3, WALL_NAMES[w]
        shp, extents = _plane_shape(nx, w, nodes=True)
        read = np.ones(shp, dtype=bool)              # the nodes of the plane that this wall owns
        if FLOW_AXES[a][0] < a:
            read[0, :] = read[-1, :] = False
        if FLOW_AXES[a][1] < a:
            read[:, 0] = read[:, -1] = False
        out.append(_checked_plane(f, shp, extents, who, "the values of heat wall %s need" % name, "heat wall %s has a non-finite entry" % name, read))
    return out


def wall_materials(material, nx, who="3-D markers"):
    """material: what the new tracers of the refill carry where a wall flow brings material into the box (the rule is in
    include/pylamp_hip.h at pl3_mic_set_inflow) -- None, or six entries [z0, x0, y0, zL, xL, yL], each None or a dict {column: value}
    with the TR_* constants as keys and a scalar or an array of shape (n_p - 1, n_q - 1) over the wall's faces as value (the planes of
    wall_flows).  Scalars are broadcast to planes.  Returns six entries, None or (mask, float64 array (ncol, n_p - 1, n_q - 1)) with
    the planes in ascending column order; a wrong length, a wrong plane shape, TR__ID, an unknown column and a non-finite value are
    rejected by name."""
    out = []
    for w, m in enumerate(_six_entries(material, who, "the inflow material needs", each=", each None or a dict")):
        if m is None or (isinstance(m, dict) and not m):
            out.append(None)
            continue
        if not isinstance(m, dict):
            raise Exception("%s: the inflow material of wall %s needs a dict {column: value} or None (got %s)" % (who, WALL_NAMES[w], type(m).__name__))
        cols = {}
        for key, val in m.items():
            col = int(key) if isinstance(key, (int, np.integer)) and not isinstance(key, bool) else None
            if col == TR__ID:
                raise Exception("%s: the inflow material of wall %s names TR__ID: the IDs are handed out by the refill and cannot be prescribed"
                                % (who, WALL_NAMES[w]))
            if col is None or not 0 <= col < TR__ID:
                raise Exception("%s: the inflow material of wall %s names an unknown column %r (the tracer columns are the TR_* constants 0 ... %d)"
                                % (who, WALL_NAMES[w], key, TR__ID - 1))
            subject = "column %d of the inflow material of wall %s" % (col, WALL_NAMES[w])
            cols[col] = _checked_plane(val, *_plane_shape(nx, w), who, subject + " needs", subject + " has a non-finite value")
        order = sorted(cols)
        out.append((sum(1 << c for c in order), np.ascontiguousarray(np.stack([cols[c] for c in order]))))
    return out


def wall_fluxes(grid, flow):
    """(fluxes, Phi) of a wall flow on the grid [z, x, y]: fluxes[w] = s_w sum_ij Un_w[i, j] dp_i dq_j, the volume per second that
    enters the box through wall w (s = +1 on z0, x0, y0, -1 on zL, xL, yL; 0 for a wall without flow), and their sum Phi, which
    Context3.set_wall_flow requires to vanish to 1e-10 of sum |Un| dp dq.  Summed in np.longdouble."""
    g = [np.asarray(c, dtype=np.float64).reshape(-1) for c in grid]
    fl = wall_flows(flow, [c.size for c in g], "wall_fluxes")
    out = np.zeros(6, dtype=np.longdouble)
    for w, a in enumerate(fl):
        if a is None:
            continue
        p, q = FLOW_AXES[w % 3]
        dp, dq = np.diff(g[p].astype(np.longdouble)), np.diff(g[q].astype(np.longdouble))
        out[w] = (1 if w < 3 else -1) * np.sum(a.astype(np.longdouble) * dp[:, None] * dq[None, :])
    return out.astype(np.float64), float(out.sum())


class Context3:
    def __init__(self, nx, grid, device=0):
        lib = _lib.load()
        self.lib = lib
        self.nx = [int(v) for v in nx]
        self.grid = [np.array(g, dtype=np.float64) for g in grid]
        if [g.size for g in self.grid] != self.nx:
            raise Exception("grid arrays do not match nx")
        h = C.c_void_p()
        rc = lib.pl3_create(C.byref(h), int(device), *self.nx, *[_lib.dptr(g) for g in self.grid])
        if rc != 0:
            msg = lib.pl3_last_error(None)
            raise Exception(msg.decode() if msg else "pl3_create failed")
        self.h = h
        self._fin = weakref.finalize(self, lib.pl3_destroy, h)

    def attach_comm(self, comm_ctx, Pz, Px, Py):
        """Make this context one block of a Pz x Px x Py decomposition (right after construction).  comm_ctx: a 2-D
        pylamp_amd Context whose communicator is set (torch.distributed under torchrun, or Context.attach_local for virtual
        ranks) with Pz * Px * Py ranks; it is kept alive with this context."""
        self.check(self.lib.pl3_set_comm(self.handle(), comm_ctx.handle(), int(Pz), int(Px), int(Py)))
        self._comm_ctx = comm_ctx
        self.layout = (int(Pz), int(Px), int(Py))

    def comm_stats(self, reset=False):
        v = (C.c_int64 * 2)()
        self.check(self.lib.pl3_comm_stats(self.handle(), v, 1 if reset else 0))
        return int(v[0]), int(v[1])

    def nranks_attached(self):
        """True once attach_comm has made this context one block of several."""
        return getattr(self, "layout", None) is not None and int(np.prod(self.layout)) > 1

    def handle(self):
        """Native handle for a library call; a closed context raises instead of handing NULL to C."""
        if self.h is None:
            raise Exception("pylamp_amd: this 3-D context has been closed")
        return self.h

    def check(self, rc):
        if self.h is None:
            raise Exception("pylamp_amd: this 3-D context has been closed")
        if rc != 0:
            msg = self.lib.pl3_last_error(self.h)
            raise Exception(msg.decode() if msg else "libpylamp_hip error %d" % rc)

    def set_warm_start(self, points, order=2):
        """Warm start of the Stokes solves of this context from the extrapolated history of their solutions (off at creation): points =
        solutions kept, 0 (off) or 2 .. 6; order = degree of the extrapolation, 1 .. 3, points >= order + 1.  The rule and the guard
        are in include/pylamp_hip.h at pl3_stokes_set_warm_start."""
        self.check(self.lib.pl3_stokes_set_warm_start(self.handle(), int(points), int(order)))

    def warm_start(self):
        """(points, order) of set_warm_start; (0, 0): off."""
        p, o = C.c_int(), C.c_int()
        self.check(self.lib.pl3_stokes_get_warm_start(self.handle(), C.byref(p), C.byref(o)))
        return p.value, o.value

    def commit_solution(self, dt):
        """The device solution of the last Stokes solve becomes the newest level of the history; dt > 0 is the model time to the next
        solve.  Does nothing with the warm start off."""
        self.check(self.lib.pl3_stokes_history_commit(self.handle(), float(dt)))

    def clear_history(self):
        self.check(self.lib.pl3_stokes_history_clear(self.handle()))

    _START_NAMES = ("cold", "warm", "rejected")

    def history_info(self):
        """Levels held, and of the last Stokes solve: its start ("cold": warm start off or no history; "warm"; "rejected": the guard
        fell back to the hydrostatic start), the levels it used, |r0| of the extrapolated start, the reference norm and the first
        three weights (newest level first)."""
        o = np.zeros(8)
        self.check(self.lib.pl3_stokes_history_info(self.handle(), _lib.dptr(o)))
        return dict(held=int(o[0]), start=self._START_NAMES[int(o[1])], used=int(o[2]), r0=float(o[3]), ref=float(o[4]),
                    weights=[float(v) for v in o[5:8]])

    def start_vector(self):
        """The extrapolated start as the next Stokes solve would form it, before the closure of the identity rows: (nz nx ny 4,)."""
        x = np.zeros(int(np.prod(self.nx)) * 4)
        self.check(self.lib.pl3_stokes_start_vector(self.handle(), _lib.dptr(x)))
        return x

    def set_shear_heating(self, on):
        """Shear heating in the resident step of this context (default off): the viscous dissipation of the Stokes solution is added to
        the scattered H before the heat solve.  The rule is in include/pylamp_hip.h at pl3_step_set_shear_heating."""
        self.check(self.lib.pl3_step_set_shear_heating(self.handle(), 1 if on else 0))

    def shear_heating(self):
        on = C.c_int()
        self.check(self.lib.pl3_step_shear_heating(self.handle(), C.byref(on)))
        return bool(on.value)

    def set_strain_fields(self, on):
        """The resident step of this context keeps strainrate, stress and dissipation for pl3_get_field (default off)."""
        self.check(self.lib.pl3_step_set_strain_fields(self.handle(), 1 if on else 0))

    def dissipation_total(self):
        """The integral of the dissipation over the box, of the last resident step that ran with one of the two switches on."""
        t = C.c_double()
        self.check(self.lib.pl3_step_dissipation_total(self.handle(), C.byref(t)))
        return t.value

    def set_yield(self, tau0, dtau_dz=0.0, eta_floor=None, on=True):
        """Yield stress of the Stokes operator of this context (off at creation): tau_y = tau0 + dtau_dz (z - z[0]) [Pa], and the floor
        eta_floor [Pa s] of the effective viscosity (None: the smallest positive float64, no floor).  on=False (or tau0 None)
        switches it off.  yield_update then limits the viscosities; the definition is in include/pylamp_hip.h at
        pl3_stokes_set_yield.  One rank."""
        if not on or tau0 is None:
            self.check(self.lib.pl3_stokes_set_yield(self.handle(), 0, 0.0, 0.0, 0.0))
            return
        floor = np.finfo(np.float64).tiny if eta_floor is None else float(eta_floor)
        self.check(self.lib.pl3_stokes_set_yield(self.handle(), 1, float(tau0), float(dtau_dz), floor))

    def yield_setting(self):
        """(tau0, dtau_dz, eta_floor) of set_yield, or None: off."""
        on = C.c_int(); v = [C.c_double() for _ in range(3)]
        self.check(self.lib.pl3_stokes_get_yield(self.handle(), C.byref(on), *[C.byref(a) for a in v]))
        return tuple(a.value for a in v) if on.value else None

    def set_picard(self, maxit, tol):
        """The Picard loop of the resident step of this context (it runs with a yield stress set): at most maxit (1 .. 32) Stokes solves,
        stopped once the change of a viscosity update is at most tol (>= 0)."""
        self.check(self.lib.pl3_step_set_picard(self.handle(), int(maxit), float(tol)))

    def picard_report(self):
        """What the Picard loop of the last resident step did: iterations (0: no yield stress was set), converged, and per iteration the
        change, the yielded nodes and cells and the iterations of its Stokes solve."""
        o = np.zeros(2 + 4 * PICARD_MAXIT_CAP)
        self.check(self.lib.pl3_step_picard_report(self.handle(), _lib.dptr(o), o.size))
        n = int(o[0])
        rows = o[2:2 + 4 * n].reshape(n, 4)
        return dict(iterations=n, converged=bool(o[1]), change=[float(v) for v in rows[:, 0]], yielded_nodes=[int(v) for v in rows[:, 1]],
                    yielded_cells=[int(v) for v in rows[:, 2]], stokes_iterations=[int(v) for v in rows[:, 3]])

    def set_marker_search(self, on):
        """Per-axis cell search for the 3-D marker kernels of this context (rectilinear grids; default off = the regular-grid
        formula).  Resident tracers are re-sorted by the new rule."""
        self.check(self.lib.pl3_mic_set_search(self.handle(), 1 if on else 0))

    def marker_search(self):
        on = C.c_int()
        self.check(self.lib.pl3_mic_get_search(self.handle(), C.byref(on)))
        return bool(on.value)

    def set_marker_deletion(self, on):
        """Deletion of the resident tracers that leave the box (default off): with it on, every sort of the resident tracers drops
        those with x_d <= 0 or x_d >= L_d on any axis (the rule is in include/pylamp_hip.h at pl3_mic_set_deletion).  Switching it on
        re-sorts resident tracers, which removes those already outside."""
        self.check(self.lib.pl3_mic_set_deletion(self.handle(), 1 if on else 0))

    def marker_deletion(self):
        on = C.c_int()
        self.check(self.lib.pl3_mic_get_deletion(self.handle(), C.byref(on)))
        return bool(on.value)

    def set_rk4_classic(self, on):
        """RK4 weights of the marker advection of this context: off (default) the reference's (1, 1, 1, 1) / 6, which sum to 4 / 6 and
        move a tracer by 2/3 U dt in a uniform field U; on the classical (1, 2, 2, 1) / 6, which move it by U dt (the rule is in
        include/pylamp_hip.h at pl3_mic_set_rk4_classic)."""
        self.check(self.lib.pl3_mic_set_rk4_classic(self.handle(), 1 if on else 0))

    def rk4_classic(self):
        on = C.c_int()
        self.check(self.lib.pl3_mic_get_rk4_classic(self.handle(), C.byref(on)))
        return bool(on.value)

    def tracers_removed(self):
        """(removed by the last sort of the resident tracers, removed since the last upload)."""
        v = (C.c_int64 * 2)()
        self.check(self.lib.pl3_tracers_removed(self.handle(), v))
        return int(v[0]), int(v[1])

    def set_inflow_material(self, material):
        """What the refill's new tracers carry where a wall flow brings material in (wall_materials: six entries, each None or a dict
        {TR_* column: scalar or plane}; None clears all six); kept until set again, like the search and the deletion.  All six are
        checked before the first is set, so a rejected call changes nothing.  A material on a wall without a flow is accepted: the
        rule (include/pylamp_hip.h at pl3_mic_set_inflow) fires only where the wall flow is inward at the time of a sort."""
        ms = wall_materials(material, self.nx, "Context3.set_inflow_material")
        h = self.handle()
        for w, m in enumerate(ms):
            if m is None:
                self.check(self.lib.pl3_mic_set_inflow(h, w, 0, None))
            else:
                self.check(self.lib.pl3_mic_set_inflow(h, w, m[0], _lib.dptr(m[1])))

    def inflow_material(self):
        """Six entries, None or the dict {column: plane} of the wall as the device holds it."""
        out = []
        for w in range(6):
            mask = C.c_uint()
            self.check(self.lib.pl3_mic_get_inflow(self.handle(), w, C.byref(mask), None))
            if not mask.value:
                out.append(None)
                continue
            cols = [c for c in range(NFTRAC) if (mask.value >> c) & 1]
            planes = np.zeros((len(cols),) + _plane_shape(self.nx, w)[0])
            self.check(self.lib.pl3_mic_get_inflow(self.handle(), w, None, _lib.dptr(planes)))
            out.append({c: planes[r] for r, c in enumerate(cols)})
        return out

    def inflow_count(self):
        """(tracers given a wall's material by the last sort of the resident tracers, since the last upload)."""
        v = (C.c_int64 * 2)()
        self.check(self.lib.pl3_mic_inflow_count(self.handle(), v))
        return int(v[0]), int(v[1])

    def set_stokes_walls(self, bc):
        """The kinds of the six Stokes walls [z0, x0, y0, zL, xL, yL] of this context (None: all free-slip); kept until set again."""
        self.check(self.lib.pl3_stokes_set_walls(self.handle(), (C.c_int * 6)(*stokes_walls(bc))))

    def set_wall_velocity(self, wallvel):
        """The velocities (Uz, Ux, Uy) of the six Stokes walls of this context, a (6, 3) array-like (None: all at rest); kept until
        set again.  Only the tangential components of a NOSLIP wall may be non-zero (include/pylamp_hip.h at
        pl3_stokes_set_wall_velocity)."""
        v = np.ascontiguousarray(wall_velocities(wallvel))
        self.check(self.lib.pl3_stokes_set_wall_velocity(self.handle(), _lib.dptr(v)))

    def wall_velocity(self):
        v = np.zeros((6, 3))
        self.check(self.lib.pl3_stokes_get_wall_velocity(self.handle(), _lib.dptr(v)))
        return v

    @staticmethod
    def _plane_pointers(planes):
        """Six planes, None or a contiguous float64 array each, as the double*[6] of the library."""
        return (_lib.c_double_p * 6)(*[None if a is None else _lib.dptr(a) for a in planes])

    def _fetch_planes(self, get, nodes):
        """The planes the device holds, by the library's getter: its mask first, then zeros for the walls that have one, filled."""
        mask = C.c_int()
        self.check(get(self.handle(), C.byref(mask), None))
        out = [np.zeros(_plane_shape(self.nx, w, nodes)[0]) if (mask.value >> w) & 1 else None for w in range(6)]
        self.check(get(self.handle(), None, self._plane_pointers(out)))
        return out

    def set_wall_flow(self, flow):
        """The flow through the six Stokes walls of this context (wall_flows: six entries, each None, a scalar or the plane Un of
        the wall; None clears it); kept until set again.  All six are set at once because their net flux must vanish
        (include/pylamp_hip.h at pl3_stokes_set_wall_flow; wall_fluxes gives the figures)."""
        fl = wall_flows(flow, self.nx)          # (named: the planes live until the call returns)
        self.check(self.lib.pl3_stokes_set_wall_flow(self.handle(), self._plane_pointers(fl)))

    def wall_flow(self):
        """Six entries, None or the plane of the wall as the device holds it."""
        return self._fetch_planes(self.lib.pl3_stokes_get_wall_flow, nodes=False)

    def set_heat_wall_values(self, values):
        """Profiles over the six heat walls of this context (wall_heat_values: six entries, each None, a scalar or the plane over the
        wall's nodes; None or six None clear them); kept until set again, across makeDiffusionMatrix and the steps.  A wall with a plane
        ignores its entry of bcvalue (include/pylamp_hip.h at pl3_heat_set_wall_values).  One rank."""
        V = wall_heat_values(values, self.nx)
        self.check(self.lib.pl3_heat_set_wall_values(self.handle(), self._plane_pointers(V)))

    def heat_wall_values(self):
        """Six entries, None or the plane of the wall as the device holds it."""
        return self._fetch_planes(self.lib.pl3_heat_get_wall_values, nodes=True)

    def close(self):
        if self.h is not None:
            self._fin()
            self.h = None


def _f3(a, shp):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != tuple(shp):
        raise Exception("field shape does not match nx")
    return a


class StokesOperator3:
    def __init__(self, ctx):
        self._ctx = ctx
        n = 4 * int(np.prod(ctx.nx))
        self.shape = (n, n)
        self.dtype = np.dtype(np.float64)
        self.last_stats = None
        kc = C.c_double(); kb = C.c_double()
        ctx.check(ctx.lib.pl3_stokes_get_scaling(ctx.handle(), C.byref(kc), C.byref(kb)))
        self.Kcont, self.Kbond = kc.value, kb.value

    def matvec(self, x):
        x = _lib.f64(x).reshape(-1)
        if x.size != self.shape[0]:
            raise Exception("dimension mismatch")
        y = np.empty_like(x)
        self._ctx.check(self._ctx.lib.pl3_stokes_apply(self._ctx.handle(), _lib.dptr(x), _lib.dptr(y)))
        return y

    dot = matvec

    def __matmul__(self, x):
        return self.matvec(x)

    def rhs(self, scaled=False):
        """The operator's own right-hand side (gravity and the moving walls); scaled=True: row-scaled, as solve(A) iterates on it."""
        r = np.empty(self.shape[0])
        fn = self._ctx.lib.pl3_stokes_rhs_scaled if scaled else self._ctx.lib.pl3_stokes_rhs
        self._ctx.check(fn(self._ctx.handle(), _lib.dptr(r)))
        return r

    def apply_bench(self, reps=20, scaled=True):
        ms = C.c_double()
        self._ctx.check(self._ctx.lib.pl3_stokes_apply_bench(self._ctx.handle(), 1 if scaled else 0, int(reps), C.byref(ms)))
        return ms.value

    def mg_info(self):
        n = C.c_int(); lm = (C.c_double * 32)()
        self._ctx.check(self._ctx.lib.pl3_stokes_mg_info(self._ctx.handle(), C.byref(n), lm, 32))
        return n.value, [lm[k] for k in range(n.value)]

    def precond(self, r):
        """z = M^-1 r by the solve's own preconditioner (no deflation correction); r: the row-scaled residual, (nz, nx, ny, 4).
        Builds or refreshes the hierarchy first, as a solve does.  Collective on an attached context; returns the global z."""
        r = _lib.f64(r).reshape(-1)
        if r.size != self.shape[0]:
            raise Exception("dimension mismatch")
        z = np.empty_like(r)
        self._ctx.check(self._ctx.lib.pl3_stokes_precond_apply(self._ctx.handle(), _lib.dptr(r), _lib.dptr(z)))
        return z

    def mg_plan(self):
        """What the V-cycle does on the built hierarchy: sweeps on the finest level and on the others, the Chebyshev ratio, the
        coarsest level's sweeps and ratio, and per level whether the marching LDS kernels take it."""
        nu = (C.c_int * 2)(); ratio = C.c_double(); cn = C.c_int(); cr = C.c_double(); lds = (C.c_int * 32)()
        n = self.mg_info()[0]
        self._ctx.check(self._ctx.lib.pl3_stokes_mg_plan(self._ctx.handle(), nu, C.byref(ratio), C.byref(cn), C.byref(cr), lds, 32))
        return dict(nu_fine=nu[0], nu=nu[1], ratio=ratio.value, coarse_sweeps=cn.value, coarse_ratio=cr.value,
                    lds=[bool(lds[k]) for k in range(n)])

    # ---- diagnostics for component tests of the Krylov loop (include/pylamp_hip.h at pl3_krylov_probe) ----
    def precond_deflated(self, r):
        """precond(r) with the deflation correction of the last solve of this context."""
        r = _lib.f64(r).reshape(-1)
        if r.size != self.shape[0]:
            raise Exception("dimension mismatch")
        z = np.empty_like(r)
        self._ctx.check(self._ctx.lib.pl3_stokes_precond_apply_deflated(self._ctx.handle(), _lib.dptr(r), _lib.dptr(z)))
        return z

    def krylov_probe(self, what, vectors, scalars=(), yw=None, fetch=()):
        """One launch of Krylov kernel `what` (PROBE_*): vectors[q] (None: none; the same array object twice shares one work vector)
        goes into Stokes work vector q, `fetch` lists the work vectors to return.  Returns (the 11 sums, {q: vector})."""
        vec = list(vectors) + [None] * (10 - len(vectors))
        held = {}
        for q, a in enumerate(vec):
            if a is not None:
                same = [p for p in range(q) if vec[p] is a]
                held[q] = held[same[0]] if same else _lib.f64(a).reshape(-1)
                if held[q].size != self.shape[0]:
                    raise Exception("dimension mismatch")
        ins = (_lib.c_double_p * 10)(*[_lib.dptr(held[q]) if q in held else None for q in range(10)])
        outs = {q: np.empty(self.shape[0]) for q in fetch}
        outp = (_lib.c_double_p * 10)(*[_lib.dptr(outs[q]) if q in outs else None for q in range(10)])
        sc = np.zeros(3); sc[:len(scalars)] = scalars
        sums = np.full(11, np.nan)
        y = None if yw is None else _f3(yw, self._ctx.nx)
        self._ctx.check(self._ctx.lib.pl3_krylov_probe(self._ctx.handle(), int(what), ins, None if y is None else _lib.dptr(y), _lib.dptr(sc),
                                                       outp, _lib.dptr(sums)))
        return sums, outs

    def hydrostatic(self):
        """(x_h, ref): the hydrostatic start vector and the reference norm |b - A x_h| of solve(A), 0 where it is not usable."""
        xh = np.empty(self.shape[0]); ref = C.c_double()
        self._ctx.check(self._ctx.lib.pl3_stokes_hydrostatic(self._ctx.handle(), _lib.dptr(xh), C.byref(ref)))
        return xh, ref.value

    def work_vector(self, index):
        """Stokes work vector `index` (WORK_*) as the last solve left it."""
        v = np.empty(self.shape[0])
        self._ctx.check(self._ctx.lib.pl3_stokes_work_vector(self._ctx.handle(), int(index), _lib.dptr(v)))
        return v

    def defl_info(self, vectors=False):
        """What the last solve did about the deflation of the pressure-anchor mode; vectors=True adds u (pressure plane) and yw."""
        o = np.zeros(15)
        u, yw = (np.empty(self._ctx.nx), np.empty(self._ctx.nx)) if vectors else (None, None)
        self._ctx.check(self._ctx.lib.pl3_stokes_defl_info(self._ctx.handle(), _lib.dptr(o), None if u is None else _lib.dptr(u),
                                                           None if yw is None else _lib.dptr(yw)))
        d = dict(valid=bool(o[0]), active=bool(o[1]), q=o[2], inner_iterations=int(o[3]), inner_residual=o[4], yAw=o[5], wvel2=o[6],
                 checks=int(o[7]), rec_iteration=int(o[8]), rec=o[9], rec_rr=o[10], rec_rc=o[11], rec_xx=o[12], rec_anchor=o[13],
                 rec_a_mom=o[14])
        if vectors:
            d.update(u=u, yw=yw)
        return d

    def ring_sum(self):
        """Sum |entry| over the ring and padding entries of the Stokes work vectors of this rank's block: on one rank 0.0 unless a kernel
        wrote there; on blocks the rings hold the neighbours' values."""
        s = C.c_double()
        self._ctx.check(self._ctx.lib.pl3_stokes_ring_sum(self._ctx.handle(), C.byref(s)))
        return s.value


def makeStokesMatrix(nx, grid, f_etas, f_etan, f_rho, bc=None, grav=None, device=0, ctx=None, strict_reference=True, wallvel=None,
                     wallflow=None, yield_stress=None):
    """3-D counterpart of pylamp_stokes.makeStokesMatrix: f_etas at the NODES (averaged onto the edges by the kernels),
    f_etan at the cell centres, f_rho at the nodes; bc = [z0, x0, y0, zL, xL, yL], each BC_TYPE_FREESLIP or BC_TYPE_NOSLIP.
    bc=None leaves the walls of the context as they are: all free-slip on a new context, or what Context3.set_stokes_walls /
    an earlier call with bc= has set on the ctx= that is passed in.
    strict_reference=True keeps the reference's wall rows (outermost in-domain tangential velocities slaved to their
    inner neighbours -- free slip imposed half a cell inside the wall, first-order accurate -- or, on a no-slip wall, the
    reference's extrapolation row); False uses natural rows (mirror rows on a free-slip wall, the one-sided shear stress
    against v = 0 on a no-slip wall; second-order accurate).  The rows are written out in include/pylamp_hip.h at
    pl3_stokes_set_walls.
    wallvel: the velocities (Uz, Ux, Uy) of the six walls, (6, 3); only the tangential components of a NOSLIP wall may be
    non-zero.  They enter the returned right-hand side (and solve(A) without rhs=) and nothing else; None leaves the velocities
    of the context as they are (at rest on a new context).  The rule is in include/pylamp_hip.h at pl3_stokes_set_wall_velocity.
    wallflow: the flow through the six walls (wall_flows: six entries, each None, a scalar or the plane Un of the wall-normal
    velocity); it enters the returned right-hand side likewise, and its net flux must vanish.  None leaves the flow of the context as
    it is (none on a new context); six None clear it.  The rule is in include/pylamp_hip.h at pl3_stokes_set_wall_flow.
    yield_stress: tau0 [Pa], (tau0, dtau_dz) or (tau0, dtau_dz, eta_floor) sets the yield stress of the context (Context3.set_yield), False
    switches it off, None leaves it as it is (off on a new context).  The operator starts with the material viscosities either way;
    yield_update(A, x) limits them."""
    walls = None if bc is None else stokes_walls(bc)
    vel = None if wallvel is None else wall_velocities(wallvel, walls)
    flows = None if wallflow is None else wall_flows(wallflow, nx)
    ctx = ctx or Context3(nx, grid, device)
    if flows is not None:
        ctx.set_wall_flow(flows)
    if vel is not None and walls is not None:
        ctx.set_wall_velocity(None)                 # (the new kinds are checked against the new velocities, not the old ones)
    if walls is not None:
        ctx.set_stokes_walls(walls)
    if vel is not None:
        ctx.set_wall_velocity(vel)
    if yield_stress is False:
        ctx.set_yield(None)
    elif yield_stress is not None:
        ys = (float(yield_stress),) if np.ndim(yield_stress) == 0 else tuple(yield_stress)
        if not 1 <= len(ys) <= 3:
            raise Exception("3-D Stokes: yield_stress needs tau0, (tau0, dtau_dz) or (tau0, dtau_dz, eta_floor), got %r" % (yield_stress,))
        ctx.set_yield(*ys)
    shp = ctx.nx
    es, en, rho = _f3(f_etas, shp), _f3(f_etan, shp), _f3(f_rho, shp)
    g = None if grav is None else (C.c_double * 3)(*[float(v) for v in grav])
    ctx.check(ctx.lib.pl3_stokes_set_coeffs(ctx.handle(), _lib.dptr(es), _lib.dptr(en), _lib.dptr(rho), g))
    ctx.check(ctx.lib.pl3_stokes_set_wall_rows(ctx.handle(), 1 if strict_reference else 0))
    A = StokesOperator3(ctx)
    return A, A.rhs()


def solve(A, rhs=None, x0=None, rtol=DEFAULT_RTOL, maxit=DEFAULT_MAXIT, resident=False, warm=False):
    """x = A^-1 rhs (rhs None: the operator's own right-hand side): multigrid-preconditioned BiCGStab on the GPU.
    resident=True: nothing crosses PCIe -- the operator's own right-hand side, the solution stays on the device (returns None;
    solution(A) fetches it), warm=True starts from the previous resident solution."""
    ctx = A._ctx
    if resident:
        if rhs is not None or x0 is not None:
            raise Exception("solve(resident=True) works on the operator's own right-hand side and the resident solution")
        st = _lib.SolveStats()
        ctx.check(ctx.lib.pl3_stokes_solve(ctx.handle(), None, None, 1 if warm else 0, float(rtol), int(maxit), C.byref(st)))
        A.last_stats = st.as_dict()
        return None
    x = np.zeros(A.shape[0]) if x0 is None else _lib.f64(x0).reshape(-1).copy()
    st = _lib.SolveStats()
    r = None if rhs is None else _lib.dptr(_lib.f64(rhs).reshape(-1))
    ctx.check(ctx.lib.pl3_stokes_solve(ctx.handle(), r, _lib.dptr(x), 0 if x0 is None else 1, float(rtol), int(maxit), C.byref(st)))
    A.last_stats = st.as_dict()
    return x


STRAIN_FIELDS = ("strainrate", "stress", "dissipation")


def strain_fields(A, x=None):
    """Second invariants of the strain rate [1/s] and of the deviatoric stress [Pa] and the viscous dissipation [W/m^3] at the nodes,
    (nz, nx, ny) each, and dissipation_total [W], the integral of the dissipation over the box, for the velocities of the solution
    vector x (nz nx ny 4) with the coefficients, walls, wall velocities and wall flow of A's context; x=None: the solution of the last
    solve(A), still on the device.  The definition is in include/pylamp_hip.h at pl3_stokes_strain_fields.  One rank."""
    ctx = A._ctx
    out = {k: np.empty(ctx.nx) for k in STRAIN_FIELDS}
    tot = C.c_double()
    if x is None:
        v = [None, None, None]
    else:
        x = _lib.f64(x).reshape(-1)
        if x.size != A.shape[0]:
            raise Exception("dimension mismatch")
        v = [_lib.dptr(np.ascontiguousarray(c)) for c in x2vp(x, ctx.nx)[0]]
    ctx.check(ctx.lib.pl3_stokes_strain_fields(ctx.handle(), v[0], v[1], v[2], *[_lib.dptr(out[k]) for k in STRAIN_FIELDS], C.byref(tot)))
    out["dissipation_total"] = tot.value
    return out


PICARD_MAXIT_CAP = 32               # most Stokes solves of one step's Picard loop (pl3_step_set_picard)
YIELD_UPDATE_KEYS = ("min_eta", "change", "yielded_nodes", "yielded_cells", "max_strainrate_nodes", "max_strainrate_cells")


def yield_setting(value, who="yield_stress"):
    """(tau0, dtau_dz) of a yield_stress value: None / False -> None, off; a number tau0 -> (tau0, 0.0); a pair (tau0, dtau_dz)."""
    if value is None or value is False:
        return None
    try:
        pair = (float(value), 0.0) if np.ndim(value) == 0 else tuple(float(v) for v in value)
    except (TypeError, ValueError):
        pair = ()
    if len(pair) != 2 or isinstance(value, (bool, np.bool_)):
        raise Exception("%s: expected None, a yield stress tau0 [Pa] or a pair (tau0, dtau_dz), got %r" % (who, value))
    return pair


def yield_update(A, x=None):
    """Limit the viscosities of A's operator by the yield stress of its context (Context3.set_yield) for the velocities of the solution
    vector x (nz nx ny 4), or with x=None for the solution of the last solve(A), still on the device:
    eta_eff = min(eta_mat, max(tau_y / (2 e), eta_floor)) at the nodes and the cell centres, always from the material viscosities.
    Returns min_eta, change = max |ln(eta_new / eta_prev)|, yielded_nodes, yielded_cells and the largest node and centre strain-rate
    invariants; coefficients(A) fetches the arrays.  The definition is in include/pylamp_hip.h at pl3_stokes_set_yield.  One rank."""
    ctx = A._ctx
    if x is None:
        v = [None, None, None]
    else:
        x = _lib.f64(x).reshape(-1)
        if x.size != A.shape[0]:
            raise Exception("dimension mismatch")
        v = [_lib.dptr(np.ascontiguousarray(c)) for c in x2vp(x, ctx.nx)[0]]
    o = np.zeros(6)
    ctx.check(ctx.lib.pl3_stokes_yield_update(ctx.handle(), v[0], v[1], v[2], _lib.dptr(o)))
    out = dict(zip(YIELD_UPDATE_KEYS, (float(a) for a in o)))
    out["yielded_nodes"], out["yielded_cells"] = int(o[2]), int(o[3])
    return out


def picard_loop(A, picard_maxit, picard_tol, rtol=DEFAULT_RTOL, maxit=DEFAULT_MAXIT):
    """The Picard loop of a step with a yield stress, after the first solve(A) (with the material viscosities) has left its solution on
    the device: update the viscosities (yield_update); while the change is above picard_tol and fewer than picard_maxit solves have run,
    solve again from the resident solution and update again.  As many updates as solves; reaching picard_maxit is no error.  Returns
    iterations, converged (the last change <= picard_tol) and per iteration change, yielded_nodes, yielded_cells and the iterations of its
    Stokes solve; solution(A) and coefficients(A) fetch the last solution and the last effective viscosities."""
    if isinstance(picard_maxit, (bool, np.bool_)) or not isinstance(picard_maxit, (int, np.integer)) or not 1 <= picard_maxit <= PICARD_MAXIT_CAP:
        raise Exception("picard_loop: picard_maxit = %r must be an integer 1 .. %d" % (picard_maxit, PICARD_MAXIT_CAP))
    if not float(picard_tol) >= 0:
        raise Exception("picard_loop: picard_tol = %r must be >= 0" % (picard_tol,))
    rep = dict(iterations=0, converged=False, change=[], yielded_nodes=[], yielded_cells=[], stokes_iterations=[])
    while True:
        u = yield_update(A)                      # (of the solution on the device)
        rep["iterations"] += 1
        rep["change"].append(u["change"]); rep["yielded_nodes"].append(u["yielded_nodes"]); rep["yielded_cells"].append(u["yielded_cells"])
        rep["stokes_iterations"].append(int(A.last_stats["iterations"]))
        rep["converged"] = bool(u["change"] <= picard_tol)
        if not u["change"] > picard_tol or rep["iterations"] >= picard_maxit:
            return rep
        solve(A, rtol=rtol, maxit=maxit, resident=True, warm=True)


def coefficients(A, material=False):
    """(etas, etan) of A's operator, (nz, nx, ny) each: the effective viscosities it solves with, or with material=True the material
    ones it was given (the same arrays unless a yield stress is set and yield_update has run)."""
    ctx = A._ctx
    es, en = np.empty(ctx.nx), np.empty(ctx.nx)
    ctx.check(ctx.lib.pl3_stokes_get_coeffs(ctx.handle(), 1 if material else 0, _lib.dptr(es), _lib.dptr(en)))
    return es, en


class HeatOperator3:
    def __init__(self, ctx):
        self._ctx = ctx
        n = int(np.prod(ctx.nx))
        self.shape = (n, n)
        self.last_stats = None

    def matvec(self, x):
        x = _lib.f64(x).reshape(-1)
        y = np.empty_like(x)
        self._ctx.check(self._ctx.lib.pl3_heat_apply(self._ctx.handle(), _lib.dptr(x), _lib.dptr(y)))
        return y

    def __matmul__(self, x):
        return self.matvec(x)

    def rhs(self):
        r = np.empty(self.shape[0])
        self._ctx.check(self._ctx.lib.pl3_heat_rhs(self._ctx.handle(), _lib.dptr(r)))
        return r


def makeDiffusionMatrix(nx, grid, gridmp, f_T, f_k, f_Cp, f_rho, f_H, bc, bcvalue, tstep, device=0, ctx=None, wallvalues=None):
    """3-D counterpart of pylamp_diff.makeDiffusionMatrix: f_k = [kz, kx, ky] on the faces normal to z, x, y;
    bc / bcvalue = [z0, x0, y0, zL, xL, yL].  wallvalues (wall_heat_values): profiles over the walls, set on the context before the
    right-hand side is formed -- per wall a plane (or a scalar) replaces bcvalue[w], None keeps it, six None clear the context's planes;
    wallvalues=None leaves the context's planes as they are."""
    ctx = ctx or Context3(nx, grid, device)
    if wallvalues is not None:
        ctx.set_heat_wall_values(wallvalues)
    shp = ctx.nx
    arrs = [_f3(a, shp) for a in (f_T, f_k[0], f_k[1], f_k[2], f_Cp, f_rho, f_H)]
    mp = [np.ascontiguousarray(m, dtype=np.float64) for m in gridmp]
    bc_arr = (C.c_int * 6)(*[int(b) for b in bc]); bv = (C.c_double * 6)(*[float(b) for b in bcvalue])
    ctx.check(ctx.lib.pl3_heat_set_coeffs(ctx.handle(), *[_lib.dptr(m) for m in mp], *[_lib.dptr(a) for a in arrs], bc_arr, bv, float(tstep)))
    A = HeatOperator3(ctx)
    return A, A.rhs()


def solution(A, heat=False):
    """The device-resident solution of the last solve(A, resident=True) / solve_heat(A, resident=True)."""
    ctx = A._ctx
    x = np.zeros(A.shape[0])
    ctx.check(ctx.lib.pl3_get_solution(ctx.handle(), 1 if heat else 0, _lib.dptr(x)))
    return x


def solve_heat(A, rtol=1e-12, maxit=2000, resident=False):
    ctx = A._ctx
    if resident:
        st = _lib.SolveStats()
        ctx.check(ctx.lib.pl3_heat_solve(ctx.handle(), None, None, float(rtol), int(maxit), C.byref(st)))
        A.last_stats = st.as_dict()
        return None
    x = np.zeros(A.shape[0])
    st = _lib.SolveStats()
    ctx.check(ctx.lib.pl3_heat_solve(ctx.handle(), None, _lib.dptr(x), float(rtol), int(maxit), C.byref(st)))
    A.last_stats = st.as_dict()
    return x


def _budget(ctx, T):
    out = np.zeros(8)
    ctx.check(ctx.lib.pl3_heat_budget(ctx.handle(), None if T is None else _lib.dptr(T), _lib.dptr(out)))
    wall = [float(v) for v in out[:6]]
    storage, source = float(out[6]), float(out[7])
    return dict(wall_flow=wall, storage=storage, source=source, imbalance=storage - source - sum(wall))


def heat_budget(A, T=None):
    """The heat budget [W] of the temperature field T (nz nx ny values) under the operator A: wall_flow, the heat flow INTO the box
    through [z0, x0, y0, zL, xL, yL]; storage, rho Cp (T - T_old) / tstep summed over the control volumes of the interior nodes;
    source, H summed likewise; imbalance = storage - source - sum(wall_flow), which vanishes for a T that satisfies the interior rows.
    T=None: the solution of the last solve_heat(A), still on the device.  The sums are those of the discrete rows (include/pylamp_hip.h
    at pl3_heat_budget); the wall sums cover the control areas of the interior nodes, not the rim of the wall.  One rank."""
    ctx = A._ctx
    if T is not None:
        T = _lib.f64(T).reshape(-1)
        if T.size != A.shape[0]:
            raise Exception("dimension mismatch")
    return _budget(ctx, T)


class VirtualCluster3:
    """Pz x Px x Py virtual ranks in ONE process on one GPU, each a Context3 block with its own host thread, joined by the
    library's in-process transport (as driver.VirtualCluster for the 2-D step): the rehearsal of BASELINE config 5 on several
    GPUs -- the same halo pack / unpack kernels, block-wise multigrid levels and all-reduced dot products, only the wire is a
    device-to-device copy."""

    def __init__(self, nx, grid, Pz, Px, Py, device=0):
        import concurrent.futures
        from ._context import Context
        lib = _lib.load()
        self.lib = lib
        self.size = int(Pz) * int(Px) * int(Py)
        g = C.c_void_p()
        if lib.pl_local_group_create(C.byref(g), self.size) != 0:
            raise Exception("pl_local_group_create failed")
        self.group = g
        self.pool = concurrent.futures.ThreadPoolExecutor(max_workers=self.size)
        ncol = 16 * self.size + 1                      # the carrier context only carries the transport: any grid its 1 x size layout divides
        tiny = [np.linspace(0, 1, 17), np.linspace(0, 1, ncol)]
        self.comms, self.ctxs = [], []
        for r in range(self.size):
            c2 = Context([17, ncol], tiny, device=device, attach_dist=False)
            c2.attach_local(g, r, 1, self.size)
            c3 = Context3(nx, grid, device)
            c3.attach_comm(c2, Pz, Px, Py)
            self.comms.append(c2); self.ctxs.append(c3)

    def all(self, fn, timeout=1800):
        """fn(ctx3, rank) on every rank at once (the calls are collective); results in rank order."""
        import concurrent.futures as cf
        futs = [self.pool.submit(fn, c, r) for r, c in enumerate(self.ctxs)]
        done, pending = cf.wait(futs, timeout=timeout, return_when=cf.FIRST_EXCEPTION)
        if pending:
            self.lib.pl_local_group_abort(self.group)
            cf.wait(futs, timeout=60)
        errs = [(r, f.exception()) for r, f in enumerate(futs) if f.done() and f.exception() is not None]
        if errs:       # every rank's message: the first one in rank order is often only the consequence of another rank's failure
            raise Exception("virtual ranks failed: " + " | ".join("rank %d: %s" % (r, e) for r, e in errs)) from errs[0][1]
        return [f.result(timeout=1) for f in futs]

    def close(self):
        for c in self.ctxs:
            c.close()
        for c in self.comms:
            c.close()
        self.pool.shutdown(wait=False)
        self.lib.pl_local_group_destroy(self.group)


# =====================================================================================================================
# 3-D marker-in-cell: tracers, advection and a time step (one rank)
# =====================================================================================================================
# The reference's marker code is 2-D (pylamp_trac.py); these are its functions extended by one axis.  tr_x is (n, 3) in
# [z, x, y] order, tr_f has the 2-D columns of pylamp_const.py, grid arrays are C-order (nz, nx, ny).
from .pylamp_const import (NFTRAC, EPS, TR_RHO, TR_ETA, TR_MRK, TR_TMP, TR_HCD, TR_HCP, TR_RH0, TR_MAT, TR_IHT, TR__ID)  # noqa: E402,F401

INTERP_AVG_ARITHMETIC = 1
INTERP_AVG_GEOMETRIC = 2
INTERP_AVG_WEIGHTED = 4
INTERP_AVG_ARITHW = INTERP_AVG_ARITHMETIC + INTERP_AVG_WEIGHTED
INTERP_AVG_GEOMW = INTERP_AVG_GEOMETRIC + INTERP_AVG_WEIGHTED
INTERP_METHOD_ELEM = 4
INTERP_METHOD_NEAREST = 8
INTERP_METHOD_LINEAR = 16
INTERP_METHOD_VELDIV = 32
SECINYR = 60 * 60 * 24 * 365.25

_MAXF = 8
_carrier = None


def _mic_ctx(ctx):
    """The marker kernels need a context only for its device and stream: any Context3 will do, a tiny one is kept."""
    global _carrier
    if ctx is not None:
        return ctx
    if _carrier is None or _carrier.h is None:
        _carrier = Context3([5, 5, 5], [np.linspace(0, 1, 5)] * 3)
    return _carrier


class _searching:
    """The context's marker search set to `on` for one call and restored afterwards (the shared carrier must not keep it)."""

    def __init__(self, ctx, on):
        self.ctx, self.on = ctx, bool(on)

    def __enter__(self):
        self.was = self.ctx.marker_search()
        if self.was != self.on:
            self.ctx.set_marker_search(self.on)

    def __exit__(self, *exc):
        if self.was != self.on and self.ctx.h is not None:
            self.ctx.set_marker_search(self.was)
        return False


def _x3(tr_x):
    x = _lib.f64(tr_x)
    if x.ndim != 2 or x.shape[1] != DIM3:
        raise Exception("tracer positions must be (n, 3) in [z, x, y] order")
    return x


def trac2grid(tr_x, tr_f, mesh, grid, gridfield, nx, distweight=None, avgscheme=None, method=INTERP_METHOD_ELEM, debug=False,
              ctx=None, search=False):
    """Average tracer values onto the node set `grid` = [z, x, y] coordinates, writing gridfield[k][:, :, :] in place:
    pylamp_trac.trac2grid (method ELEM) extended by one axis.  Two calls with the same input agree bitwise.
    search=True: cells by per-axis search in the coordinates (rectilinear grids) instead of the regular-grid formula."""
    if avgscheme is None:
        avgscheme = [INTERP_AVG_ARITHW] * len(gridfield)
    if len(gridfield) != tr_f.shape[1] or len(avgscheme) != len(gridfield) or tr_x.shape[0] != tr_f.shape[0]:
        raise Exception("trac2grid: tr_f, gridfield and avgscheme do not match")
    if not (method & INTERP_METHOD_ELEM):
        raise Exception("trac2grid: only INTERP_METHOD_ELEM is implemented on the GPU")
    ctx = _mic_ctx(ctx)
    txc = _x3(tr_x)
    n = txc.shape[0]
    g = [_lib.f64(grid[d]) for d in range(3)]
    shp = tuple(int(v) for v in nx)
    if tuple(c.size for c in g) != shp:
        raise Exception("trac2grid: grid arrays do not match nx")
    nf = len(gridfield)
    with _searching(ctx, search):
        for k0 in range(0, nf, _MAXF):
            k1 = min(nf, k0 + _MAXF)
            sub = _lib.f64(tr_f[:, k0:k1])
            outs = [np.empty(shp) for _ in range(k1 - k0)]
            op = (_lib.c_double_p * (k1 - k0))(*[_lib.dptr(a) for a in outs])
            sch = (C.c_int * (k1 - k0))(*[int(s) for s in avgscheme[k0:k1]])
            ctx.check(ctx.lib.pl3_trac2grid(ctx.handle(), n, _lib.dptr(txc), _lib.dptr(sub), k1 - k0, k1 - k0, sch, _lib.dptr(g[0]), shp[0],
                                            _lib.dptr(g[1]), shp[1], _lib.dptr(g[2]), shp[2], op))
            for k in range(k0, k1):
                gridfield[k][...] = outs[k - k0]


def grid2trac(tr_x, tr_f, grid, gridfield, nx, defval=np.nan, method=INTERP_METHOD_LINEAR, stopOnError=False, ctx=None, search=False):
    """Interpolate gridfield (list of (nz, nx, ny) arrays) to the tracers, writing tr_f in place.  LINEAR is trilinear, NEAREST
    the nearest of the eight corners, VELDIV the divergence-conserving interpolation of (vz, vx, vy).
    Out-of-grid tracers get defval in every column.  search=True: cells by per-axis search (rectilinear grids)."""
    nf = len(gridfield)
    if nf != tr_f.shape[1] or tr_x.shape[0] != tr_f.shape[0]:
        raise Exception("grid2trac: tr_f and gridfield do not match")
    if not method & (INTERP_METHOD_LINEAR | INTERP_METHOD_NEAREST | INTERP_METHOD_VELDIV):
        raise Exception("grid2trac: unknown interpolation method")
    ctx = _mic_ctx(ctx)
    txc = _x3(tr_x)
    n = txc.shape[0]
    shp = tuple(int(v) for v in nx)
    g = [_lib.f64(grid[d]) for d in range(3)]
    out = np.empty((n, nf))
    nout = C.c_int64(0); total = 0
    with _searching(ctx, search):
        for k0 in range(0, nf, _MAXF):
            k1 = min(nf, k0 + _MAXF)
            fl = [_f3(gridfield[k], shp) for k in range(k0, k1)]
            fp = (_lib.c_double_p * (k1 - k0))(*[_lib.dptr(a) for a in fl])
            sub = np.empty((n, k1 - k0))
            ctx.check(ctx.lib.pl3_grid2trac(ctx.handle(), n, _lib.dptr(txc), k1 - k0, fp, shp[0], shp[1], shp[2], _lib.dptr(g[0]),
                                            _lib.dptr(g[1]), _lib.dptr(g[2]), int(method), float(defval), 1 if stopOnError else 0,
                                            _lib.dptr(sub), k1 - k0, C.byref(nout)))
            out[:, k0:k1] = sub
            total = max(total, nout.value)
    if total > 0:
        print("!!! Warning, grid2trac(): Using default value for extrapolation in ", total, "tracers")
    tr_f[:, :] = out


def RK(tr_x, grids, vels, nx, tstep, order=4, ctx=None, search=False):
    """Runge-Kutta advection; returns (vel_final, tr_x_final), both (n, 3).  grids / vels live on the padded
    (nz+1, nx+1, ny+1) cell-centre grid (advection_velocity); the reference's weights (1,1,1,1)/6 are kept unless the context has
    Context3.set_rk4_classic(True).
    search=True: cells by per-axis search (rectilinear grids)."""
    if order != 4:
        raise Exception("RK: only order=4 is functional (as in 2-D)")
    if len(nx) != 3:
        raise Exception("RK: nx must have three entries")
    ctx = _mic_ctx(ctx)
    shp = tuple(int(v) + 1 for v in nx)
    txc = _x3(tr_x)
    n = txc.shape[0]
    g = [_lib.f64(grids[d]) for d in range(3)]
    if tuple(c.size for c in g) != shp:
        raise Exception("RK: velocity grids must have shape (nz+1, nx+1, ny+1)")
    V = [_f3(vels[d], shp) for d in range(3)]
    v = np.empty((n, 3)); xn = np.empty((n, 3))
    with _searching(ctx, search):
        ctx.check(ctx.lib.pl3_rk4(ctx.handle(), n, _lib.dptr(txc), shp[0], shp[1], shp[2], *[_lib.dptr(c) for c in g], *[_lib.dptr(a) for a in V],
                                  float(tstep), _lib.dptr(v), _lib.dptr(xn)))
    return v, xn


def gridmp_of(grid):
    """Midpoint coordinates with one extrapolated extra entry per axis (pylamp2.py:92-95)."""
    out = []
    for c in grid:
        c = np.asarray(c, dtype=np.float64)
        m = (c[1:] + c[:-1]) / 2
        out.append(np.append(m, m[-1] + (m[-1] - m[-2])))
    return out


def graded_grid(n, L, ratio):
    """n coordinates from 0 to L whose spacings grow smoothly (geometrically) by `ratio` from the first cell to the last: a
    rectilinear grid for Simulation3(..., grid=, options=Options3(marker_search=True))."""
    h = float(ratio) ** np.linspace(0.0, 1.0, int(n) - 1)
    c = np.concatenate([[0.0], np.cumsum(h)]) * (float(L) / h.sum())
    c[-1] = float(L)
    return c


def refined_grid(n, L, centre=0.5, ratio=3.0, width=0.2):
    """n coordinates from 0 to L with cells `ratio` times finer around cell number centre * (n - 1) than far from it; the
    spacing follows a Gaussian of width * (n - 1) cells, so neighbouring cells differ little."""
    s = (np.arange(int(n) - 1) + 0.5) / (int(n) - 1)
    h = 1.0 / (1.0 + (float(ratio) - 1.0) * np.exp(-((s - centre) / width) ** 2))
    c = np.concatenate([[0.0], np.cumsum(h)]) * (float(L) / h.sum())
    c[-1] = float(L)
    return c


def advection_velocity(newvel, gridmp, nx, bc=None, wallvel=None, wallflow=None):
    """Cell-centred velocities on the padded (nz+1, nx+1, ny+1) grid (pylamp2.py:491-545 extended by one axis): every
    component is averaged along its own axis; ghosts wall by wall in the order z0, x0, y0, zL, xL, yL -- a free-slip wall
    mirrors the normal component with a sign flip and copies the tangential ones, the pass of a no-slip wall
    (bc[w] == BC_TYPE_NOSLIP; bc None: all free-slip) is skipped as in the reference, so its ghosts keep what they hold.
    The pass of a no-slip wall with a non-zero velocity wallvel[w] = (Uz, Ux, Uy) runs in its slot: -V for the normal component
    and 2 U_c - V for a tangential component c, so that the velocity interpolated onto the wall is U (deliberately
    discontinuous at U = 0, where walls at rest keep the reference's behaviour).
    The pass of a wall with a flow (wallflow[w] not None; wall_flows) runs in its slot too, even for a no-slip wall at rest: the
    normal component becomes 2 Un - V with Un continued constantly into the ghost rim, so that the velocity interpolated onto the
    wall is Un; the tangential components are copied on a free-slip wall and follow 2 U_c - V on a no-slip wall.
    Returns ([gz, gx, gy], [Vz, Vx, Vy])."""
    walls = stokes_walls(bc, "advection_velocity")
    U = wall_velocities(wallvel, walls, "advection_velocity")
    Un = wall_flows(wallflow, nx, "advection_velocity")
    shp = tuple(int(v) + 1 for v in nx)
    vz, vx, vy = newvel
    V = [np.zeros(shp) for _ in range(3)]
    V[0][1:-1, 1:-1, 1:-1] = 0.5 * (vz[1:, :-1, :-1] + vz[:-1, :-1, :-1])
    V[1][1:-1, 1:-1, 1:-1] = 0.5 * (vx[:-1, 1:, :-1] + vx[:-1, :-1, :-1])
    V[2][1:-1, 1:-1, 1:-1] = 0.5 * (vy[:-1, :-1, 1:] + vy[:-1, :-1, :-1])
    g = [np.insert(np.asarray(m, dtype=np.float64), 0, m[0] - (m[1] - m[0])) for m in gridmp]
    for ghost, inner in ((0, 1), (-1, -2)):
        for axis in range(3):
            w = axis + (0 if ghost == 0 else 3)
            moving = walls[w] == BC_TYPE_NOSLIP and (U[w].any() or Un[w] is not None)
            if walls[w] == BC_TYPE_NOSLIP and not moving:
                continue
            for comp in range(3):
                dst = [slice(None)] * 3; src = [slice(None)] * 3
                dst[axis] = ghost; src[axis] = inner
                if comp == axis and Un[w] is not None:
                    V[comp][tuple(dst)] = 2 * np.pad(Un[w], 1, mode="edge") - V[comp][tuple(src)]
                elif comp == axis:
                    V[comp][tuple(dst)] = -V[comp][tuple(src)]
                elif moving:
                    V[comp][tuple(dst)] = 2 * U[w, comp] - V[comp][tuple(src)]
                else:
                    V[comp][tuple(dst)] = V[comp][tuple(src)]
    return g, V


WARM_START_DEFAULT = (3, 2)          # (points, order) of Options3.stokes_warm_start = True: the 2-D step's default
WARM_START_MAX_POINTS = 6            # X0_HIST + 1 of csrc/pl_x0.h


def warm_start_setting(value, who="Options3.stokes_warm_start"):
    """(points, order) of a stokes_warm_start value: False / None -> (0, 0), off; True -> WARM_START_DEFAULT; a (points, order) pair
    is checked by the library's rule (pl3_stokes_set_warm_start): points 2 .. 6, order 1 .. 3, points >= order + 1."""
    if value is None or value is False:
        return (0, 0)
    if value is True:
        return WARM_START_DEFAULT
    try:
        points, order = value
        ok = all(isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)) for v in (points, order))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise Exception("%s: expected False, True or a (points, order) pair of integers, got %r" % (who, value))
    points, order = int(points), int(order)
    if points < 2 or points > WARM_START_MAX_POINTS:
        raise Exception("%s: points = %d must be 2 .. %d" % (who, points, WARM_START_MAX_POINTS))
    if order < 1 or order > 3:
        raise Exception("%s: order = %d must be 1 .. 3" % (who, order))
    if points < order + 1:
        raise Exception("%s: order = %d needs points >= %d, got points = %d" % (who, order, order + 1, points))
    return (points, order)


class Options3:
    """Options of pylamp2.py:37-77 that Simulation3 honours (the 2-D driver's names)."""

    def __init__(self, **kw):
        self.do_heatdiff = True
        self.do_subgrid_heatdiff = True
        self.tdep_rho = True
        self.tdep_eta = True
        self.etamin, self.etamax, self.Tref = 1e17, 1e23, 1623.0
        self.tstep_adv_max = 50e9 * SECINYR; self.tstep_adv_min = 50e-9 * SECINYR
        self.tstep_dif_max = 50e9 * SECINYR; self.tstep_dif_min = 50e-9 * SECINYR
        self.tstep_modifier = 0.67
        self.bcstokes = [BC_TYPE_FREESLIP] * 6
        # beyond the reference: velocities (Uz, Ux, Uy) of the six walls, (6, 3); tangential components of NOSLIP walls only (None: at rest)
        self.bcstokesvel = None
        # beyond the reference: flow through the six walls (wall_flows: per wall None, a scalar or the plane Un of the wall-normal
        # velocity along +axis); needs tracs_fence_enabled = False with marker_deletion = True, and tracdens_min > 0 (None: no flow)
        self.bcstokesflow = None
        # beyond the reference: what enters through an inflow wall (wall_materials: per wall None or {TR_* column: scalar or plane}); the
        # refill's new tracers between the wall and the cell's residents take these values where the wall flow is inward (None: the
        # zero-gradient inflow, every new tracer the mean of its cell)
        self.bcinflow = None
        self.bcheat = [BC_TYPE_FIXTEMP, BC_TYPE_FIXFLOW, BC_TYPE_FIXFLOW, BC_TYPE_FIXTEMP, BC_TYPE_FIXFLOW, BC_TYPE_FIXFLOW]
        self.bcheatvals = [273.0, 0.0, 0.0, 1623.0, 0.0, 0.0]
        # beyond the reference: the heat boundary values as profiles over the walls (wall_heat_values: per wall None, a scalar or the
        # plane over the wall's nodes -- temperatures on a FIXTEMP wall, k dT/dx_a along +a on a FIXFLOW wall); a wall with a plane
        # ignores its entry of bcheatvals (None: every wall takes its entry of bcheatvals)
        self.bcheatprofile = None
        self.stokes_rtol, self.stokes_maxit = DEFAULT_RTOL, DEFAULT_MAXIT
        self.heat_rtol, self.heat_maxit = 1e-12, 2000
        self.grav = None
        # census + refill (pylamp2.py:588-633 with a third axis): a cell below tracdens_min tracers is refilled to tracdens; 0 = off
        self.tracdens, self.tracdens_min = 0, 0
        self.inject_seed = 12345                # seed of the counter-based stream of the new positions
        self.inject_unique_ids = False          # False: the reference's ID rule (pylamp2.py:621-622, repeats IDs); True: max + 1, + 2, ...
        # parts of the 2-D step that do not exist in 3-D yet: anything but these values is rejected by name
        self.tracs_fence_enabled = True
        self.surface_stabilization = False
        # True: step() is one pl3_resident_step call -- every grid field stays on the device, field() downloads on demand
        self.resident = False
        # beyond the reference: cells of the markers by per-axis search, which lets Simulation3 take a rectilinear grid=
        self.marker_search = False
        # the fence-off path of pylamp2.py:563-581: tracs_fence_enabled = False AND marker_deletion = True.  Two switches because the
        # plain rejection of tracs_fence_enabled = False is pinned behaviour: the deletion is opted into by name, and
        # marker_deletion = True with the fence on is rejected too, so that one combination has one meaning
        self.marker_deletion = False
        # beyond the reference: the classical RK4 weights (1, 2, 2, 1) / 6 instead of the reference's (1, 1, 1, 1) / 6, which move a tracer
        # by 2/3 U tstep in a uniform field U.  A flow through the walls wants True: the markers then carry the volume the walls bring in
        self.rk4_classic = False
        # beyond the reference: the Stokes solve starts from the extrapolated history of its solutions (Context3.set_warm_start) instead
        # of the hydrostatic state.  False: off; True: (points, order) = WARM_START_DEFAULT; or a (points, order) pair
        self.stokes_warm_start = False
        # beyond the reference: the viscous dissipation of the Stokes solution heats the material (added to the scattered H before the heat
        # solve; needs do_heatdiff), and / or the step keeps the fields strainrate, stress, dissipation (strain_fields).  Both off: the
        # step is bit for bit what it is without them
        self.shear_heating = False
        self.strain_fields = False
        # beyond the reference: a yield stress limits the viscosity of the Stokes solve, eta_eff = min(eta, max(tau_y / (2 e), floor)) with
        # e the second invariant of the strain rate and tau_y = tau0 + dtau_dz z (Context3.set_yield).  None: off; tau0 [Pa]; or
        # (tau0, dtau_dz).  yield_eta_floor: the floor [Pa s], None = etamin.  Every step then runs a Picard loop of Stokes solves;
        # picard_maxit (1 .. 32) and picard_tol (the change max |ln(eta_new / eta_prev)| at which it stops) are user settings, and these
        # defaults a choice: ten solves bound the cost of a step, 1e-2 is a 1 % change of the viscosity
        self.yield_stress = None
        self.yield_eta_floor = None
        self.picard_maxit, self.picard_tol = 10, 1e-2
        for k, v in kw.items():
            if not hasattr(self, k):
                raise Exception("unknown option " + k)
            setattr(self, k, v)
        warm_start_setting(self.stokes_warm_start)
        yield_setting(self.yield_stress, "Options3.yield_stress")


class Simulation3:
    """The 3-D counterpart of driver.Simulation: tracers stay on the GPU, step() follows the loop of pylamp2.py:290-581 with a
    third axis -- properties, tracer->grid, Stokes, time step, heat, grid->tracer (+ subgrid diffusion), RK4, fence, and the census
    + refill of depleted cells inside the end-of-step sort (Options3.tracdens / tracdens_min / inject_seed / inject_unique_ids;
    refill() does it without a step).  step() reports ninjected, nrefilled (cells) and nempty (cells that held no tracer: their new
    tracers carry NaN fields, as in the reference) and raises before the Stokes solve when a scattered field holds a NaN.  One rank.

    Walls: the Stokes walls are free-slip or no-slip per wall (Options3.bcstokes = [z0, x0, y0, zL, xL, yL]); a no-slip wall may
    move in its own plane (Options3.bcstokesvel, set_wall_velocity).

    Grid: a regular grid unless Options3.marker_search = True, with which grid= may be any rectilinear grid (per axis strictly
    increasing from 0 to L[d]): the marker kernels then find cells by search in the coordinates (the rule is in
    include/pylamp_hip.h at pl3_mic_set_search), while the time-step rules and the subgrid time scale keep the mean spacing.

    Resident step: Options3.resident = True runs the same sequence inside the library with every grid field kept on the device
    (pl3_resident_step; field() then downloads on demand, transfer_stats() counts what crosses the bus).

    Deletion: Options3.tracs_fence_enabled = False together with Options3.marker_deletion = True runs without the fence: a tracer
    that leaves the box (x_d <= 0 or x_d >= L_d) is removed by the next sort, the census and the refill of that sort see the
    survivors, step() / advect() / refill() report nremoved and Context3.tracers_removed() counts them.

    Through-flow: on that path material may flow through the walls (Options3.bcstokesflow, set_wall_flow; wall_flows states the
    format); the net flux must vanish (wall_fluxes).  The outflow is deleted, the cells along an inflow wall are kept filled by the
    refill (tracdens_min > 0 is required), whose new tracers carry the mean of their cell's residents -- a zero-gradient inflow --
    unless the wall has an inflow material.

    Inflow material (Options3.bcinflow, set_inflow_material; wall_materials states the format): the new tracers that lie between
    the wall and every resident of their cell take the wall's values in the columns it names, step() / advect() / refill() report
    them as ninflow, and an inflow cell that ran empty gets finite values in those columns (a scattered column the material leaves
    out is still NaN there and step() raises its NaN error).  A prescribed TR_TMP is a tracer temperature like any other, so with
    heat diffusion on it enters the next step's temperature scatter, and the heat solve of the same step can hold the matching
    patch of the wall hot (next paragraph).

    Heat walls: Options3.bcheatprofile / set_heat_profile give the boundary values of the heat solve as profiles over the walls
    (wall_heat_values states the format); heat_budget() gives the heat flow through the six walls, the storage rate and the source
    of the last step's heat solve.

    RK4: Options3.rk4_classic = True makes the tracers move by U tstep (the reference's RK4 weights, the default, move them by 2/3
    of that).

    Yield stress: Options3.yield_stress = tau0 or (tau0, dtau_dz) limits the viscosity of the Stokes solve, eta_eff = min(eta,
    max(tau_y / (2 e), floor)) (Context3.set_yield), and every step runs a Picard loop of at most Options3.picard_maxit Stokes solves
    until the change of the viscosities is at most Options3.picard_tol (picard_loop); step() reports it as rep["picard"], field()
    knows etas_eff and etan_eff.

    Not built: surface stabilisation, several ranks -- each is rejected with an error that names it."""

    def __init__(self, nx, L, tr_x=None, tr_f=None, options=None, device=0, grid=None):
        self.nx = [int(v) for v in nx]
        self.L = [float(v) for v in L]
        if len(self.nx) != 3 or len(self.L) != 3:
            raise Exception("Simulation3: nx and L need three entries (z, x, y)")
        self.opt = options or Options3()
        o = self.opt
        self.grid = [np.linspace(0, self.L[d], self.nx[d]) for d in range(3)]          # pylamp2.py:90
        if grid is not None and o.marker_search:
            given = [np.array(grid[d], dtype=np.float64).reshape(-1) for d in range(3)]
            for d in range(3):
                c = given[d]
                if c.size != self.nx[d]:
                    raise Exception("Simulation3: grid[%d] has %d coordinates, nx[%d] = %d" % (d, c.size, d, self.nx[d]))
                if not np.all(np.diff(c) > 0):
                    raise Exception("Simulation3: grid[%d] is not strictly increasing" % d)
                if c[0] != 0.0 or abs(c[-1] - self.L[d]) > 1e-12 * self.L[d]:
                    raise Exception("Simulation3: grid[%d] does not span 0..L[%d] (it runs from %r to %r, L = %r)" % (d, d, c[0], c[-1], self.L[d]))
            self.grid = given
        elif grid is not None:
            for d in range(3):
                if not np.allclose(np.asarray(grid[d], dtype=np.float64), np.linspace(0, self.L[d], self.nx[d]), rtol=0, atol=1e-9 * self.L[d]):
                    raise Exception("Simulation3: non-uniform grids are not supported by the 3-D markers unless Options3.marker_search = True")
        self.gridmp = gridmp_of(self.grid)
        if int(o.tracdens) < 0 or int(o.tracdens_min) < 0 or int(o.tracdens_min) > int(o.tracdens):
            raise Exception("Simulation3: tracer injection needs tracdens >= tracdens_min >= 0 (got tracdens = %s, tracdens_min = %s)"
                            % (o.tracdens, o.tracdens_min))
        if not o.tracs_fence_enabled and not o.marker_deletion:
            raise Exception("Simulation3: the fence-off deletion path (tracs_fence_enabled = False) is not supported in 3-D "
                            "unless Options3.marker_deletion = True")
        if o.marker_deletion and o.tracs_fence_enabled:
            raise Exception("Simulation3: Options3.marker_deletion = True needs tracs_fence_enabled = False (with the fence on no "
                            "tracer leaves the box and there is nothing to delete)")
        if o.surface_stabilization:
            raise Exception("Simulation3: surface stabilisation is not supported in 3-D")
        self.shear_heating, self.strain_fields = bool(o.shear_heating), bool(o.strain_fields)
        if self.shear_heating and not o.do_heatdiff:
            raise Exception("Simulation3: Options3.shear_heating = True needs the heat solve, Options3.do_heatdiff = True")
        self.yield_stress = yield_setting(o.yield_stress, "Simulation3: Options3.yield_stress")
        if self.yield_stress is not None:
            if isinstance(o.picard_maxit, (bool, np.bool_)) or not isinstance(o.picard_maxit, (int, np.integer)) or not 1 <= o.picard_maxit <= PICARD_MAXIT_CAP:
                raise Exception("Simulation3: Options3.picard_maxit = %r must be an integer 1 .. %d" % (o.picard_maxit, PICARD_MAXIT_CAP))
            if not float(o.picard_tol) >= 0:
                raise Exception("Simulation3: Options3.picard_tol = %r must be >= 0" % (o.picard_tol,))
        self.bcstokes = stokes_walls(o.bcstokes, "Simulation3: Options3.bcstokes")
        self.bcstokesflow = self._checked_flow(o.bcstokesflow, "Simulation3: Options3.bcstokesflow")
        wall_materials(o.bcinflow, self.nx, "Simulation3: Options3.bcinflow")
        self.bcheatprofile = self._checked_heat_profile(o.bcheatprofile, "Simulation3: Options3.bcheatprofile")
        self.ctx = Context3(self.nx, self.grid, device)
        if self.bcheatprofile is not None:
            self.ctx.set_heat_wall_values(self.bcheatprofile)      # once: the context keeps the planes for both step paths
        self.bcstokesvel = wall_velocities(o.bcstokesvel, self.bcstokes, "Simulation3: Options3.bcstokesvel")
        self.ctx.set_stokes_walls(self.bcstokes)        # the resident step and the device advection velocity read them from the context
        self.ctx.set_wall_velocity(self.bcstokesvel)
        if any(a is not None for a in self.bcstokesflow):
            self.ctx.set_wall_flow(self.bcstokesflow)
        if o.marker_search:
            self.ctx.set_marker_search(True)
        if o.marker_deletion:
            self.ctx.set_marker_deletion(True)
        if o.rk4_classic:
            self.ctx.set_rk4_classic(True)
        self.warm_start = warm_start_setting(o.stokes_warm_start, "Simulation3: Options3.stokes_warm_start")
        if self.warm_start[0]:
            self.ctx.set_warm_start(*self.warm_start)
        if self.yield_stress is not None:
            self.ctx.set_yield(*self.yield_stress, eta_floor=o.etamin if o.yield_eta_floor is None else o.yield_eta_floor)
            self.ctx.set_picard(o.picard_maxit, o.picard_tol)        # (read by the resident step; the staged one runs the same loop below)
        if o.resident and self.shear_heating:
            self.ctx.set_shear_heating(True)
        if o.resident and self.strain_fields:
            self.ctx.set_strain_fields(True)
        self._inflow = False
        if o.bcinflow is not None:
            self.set_inflow_material(o.bcinflow)
        self.it = 0
        self.totaltime = 0.0
        self.last = None
        self.ntrac = 0
        self.fields = {}
        self._newtemp = None
        self._stepped = False                    # resident: the library holds the fields of a step
        if tr_x is not None:
            self.upload(tr_x, tr_f)

    def set_wall_velocity(self, wallvel):
        """New velocities (Uz, Ux, Uy) of the six walls, (6, 3) (None: all at rest), from the next step on; the kinds stay those of
        Options3.bcstokes, so only the tangential components of its NOSLIP walls may be non-zero."""
        v = wall_velocities(wallvel, self.bcstokes, "Simulation3.set_wall_velocity")
        self.ctx.set_wall_velocity(v)
        self.bcstokesvel = v

    def _checked_flow(self, flow, who):
        """wall_flows plus what a flow needs of the markers: the fence would stop the outflow, and the cells along an inflow wall are
        kept filled by the census refill alone."""
        o = self.opt
        fl = wall_flows(flow, self.nx, who)
        if any(a is not None for a in fl):
            if o.tracs_fence_enabled or not o.marker_deletion:
                raise Exception("%s: a flow through the walls needs tracs_fence_enabled = False together with marker_deletion = True "
                                "(the fence would hold the outflowing tracers at the wall)" % who)
            if int(o.tracdens_min) == 0:
                raise Exception("%s: a flow through the walls needs the refill of depleted cells, tracdens >= tracdens_min > 0 (got "
                                "tracdens_min = 0): the cells along an inflow wall would run empty" % who)
        return fl

    def set_wall_flow(self, flow):
        """A new flow through the six walls (wall_flows; None: none) from the next step on.  New tracers of the refilled cells along an
        inflow wall carry the mean of the cell's residents, a zero-gradient inflow, or the wall's material (set_inflow_material)."""
        fl = self._checked_flow(flow, "Simulation3.set_wall_flow")
        self.ctx.set_wall_flow(fl)
        self.bcstokesflow = fl

    def set_inflow_material(self, material):
        """The material of the six walls (wall_materials; None: none) for the refills from now on: new tracers between an inflow wall
        and the residents of their cell take it.  A wall that carries no flow right now may hold one; it waits for set_wall_flow."""
        ms = wall_materials(material, self.nx, "Simulation3.set_inflow_material")
        self.ctx.set_inflow_material(material)
        self._inflow = any(m is not None for m in ms)

    def _checked_heat_profile(self, values, who):
        """wall_heat_values, or None where no wall has a plane; a profile needs the heat solve."""
        V = wall_heat_values(values, self.nx, who)
        if all(a is None for a in V):
            return None
        if not self.opt.do_heatdiff:
            raise Exception("%s: a profile over the heat walls needs the heat solve, Options3.do_heatdiff = True" % who)
        return V

    def set_heat_profile(self, values):
        """New profiles over the six heat walls (wall_heat_values; None: every wall takes its entry of Options3.bcheatvals again) from the next
        step on: a hot patch can move or switch on.  The kinds stay those of Options3.bcheat."""
        V = self._checked_heat_profile(values, "Simulation3.set_heat_profile")
        if V is not None or self.bcheatprofile is not None:
            self.ctx.set_heat_wall_values(V)
        self.bcheatprofile = V

    def heat_budget(self):
        """The heat budget of the last step's heat solve (heat_budget: wall_flow into the box through the six walls, storage, source
        and imbalance, in watts), from the temperature and the coefficients the step left on the device."""
        if not self.opt.do_heatdiff:
            raise Exception("Simulation3.heat_budget: the heat solve is off (Options3.do_heatdiff = False)")
        if self.last is None:
            raise Exception("Simulation3.heat_budget: no step has run yet")
        return _budget(self.ctx, None)

    # -- tracer state ------------------------------------------------------------------------------------------------
    def _lib_call(self, name, *args):
        if self.ctx.nranks_attached():
            raise Exception("Simulation3: several ranks are not supported by the 3-D markers")
        self.ctx.check(getattr(self.ctx.lib, name)(self.ctx.handle(), *args))

    def upload(self, tr_x, tr_f):
        tr_x = _x3(tr_x); tr_f = _lib.f64(tr_f)
        if tr_f.shape != (tr_x.shape[0], NFTRAC):
            raise Exception("tracer arrays must be (n, 3) and (n, %d)" % NFTRAC)
        self._lib_call("pl3_tracers_upload", tr_x.shape[0], _lib.dptr(tr_x), _lib.dptr(tr_f))
        self.ntrac = tr_x.shape[0] - self.ctx.tracers_removed()[0]
        self.reset_stokes_history()              # other tracers, another flow: its solutions are no start for the next solve

    def reset_stokes_history(self):
        """Forget the Stokes solutions kept for the warm start (Options3.stokes_warm_start): the next solve starts cold."""
        self.ctx.clear_history()

    def count(self):
        n = C.c_int64()
        self._lib_call("pl3_tracers_count", C.byref(n))
        self.ntrac = n.value
        return n.value

    def tracers(self):
        """(tr_x, tr_f) in the resident (cell-sorted) order; TR__ID identifies a tracer."""
        n = self.count()
        tr_x = np.empty((n, 3)); tr_f = np.empty((n, NFTRAC))
        self._lib_call("pl3_tracers_download", n, _lib.dptr(tr_x), _lib.dptr(tr_f))
        return tr_x, tr_f

    def tracer_velocity(self):
        """(n, 3) velocities of the last advection, in the order tracers() returns."""
        n = self.count()
        v = np.empty((n, 3))
        self._lib_call("pl3_get_tracer_velocity", n, _lib.dptr(v))
        return v

    def census(self):
        """Tracers per cell, (nz-1, nx-1, ny-1): a by-product of the sort."""
        cnt = np.empty([v - 1 for v in self.nx], dtype=np.int32)
        self._lib_call("pl3_tracers_census", cnt.size, cnt.ctypes.data_as(C.POINTER(C.c_int32)))
        return cnt

    def field(self, name):
        """A grid field of the last step: rho, etas, etan, cp, T, H, mat, kz, kx, ky, velz, velx, vely, pres, temp; with
        Options3.shear_heating or Options3.strain_fields also strainrate, stress, dissipation (H then includes the dissipation if
        shear_heating is on); with Options3.yield_stress also etas_eff, etan_eff, the effective viscosities after the step's Picard loop
        (etas, etan stay the scattered material fields)."""
        if self.opt.resident and name not in self.fields:
            out = np.empty(self.nx)
            self._lib_call("pl3_get_field", name.encode(), _lib.dptr(out))
            self.fields[name] = out                  # cached until the next step
        if name not in self.fields:
            raise Exception("Simulation3.field: no field '%s' (have: %s)" % (name, ", ".join(sorted(self.fields))))
        return self.fields[name]

    def transfer_stats(self, reset=False):
        """Host <-> device copies of this simulation's library calls since the last reset: counts and bytes of those of at least one
        node field (8 nz nx ny bytes) and of the smaller ones."""
        v = (C.c_int64 * 4)()
        self.ctx.check(self.ctx.lib.pl3_transfer_stats(self.ctx.handle(), v, 1 if reset else 0))
        return dict(large=int(v[0]), large_bytes=int(v[1]), small=int(v[2]), small_bytes=int(v[3]))

    def stage_times(self):
        ms = (C.c_double * 4)()
        self._lib_call("pl3_resident_times", ms)
        return dict(scatter=ms[0], gather=ms[1], rk4=ms[2], sort=ms[3])

    # -- the marker stages of a step, one at a time (the same kernels as the module-level functions) ------------------
    def update_properties(self):
        o = self.opt
        self._lib_call("pl3_resident_props", int(o.tdep_rho), int(o.tdep_eta), float(o.Tref), float(o.etamin), float(o.etamax))

    def scatter(self, columns, avgscheme, grid=None):
        """Tracer columns -> the node set `grid` (default: the nodes); returns the list of (nz, nx, ny) arrays."""
        g = [_lib.f64(c) for c in (grid or self.grid)]
        shp = tuple(c.size for c in g)
        nf = len(columns)
        outs = [np.empty(shp) for _ in range(nf)]
        op = (_lib.c_double_p * nf)(*[_lib.dptr(a) for a in outs])
        self._lib_call("pl3_resident_trac2grid", nf, (C.c_int * nf)(*[int(c) for c in columns]), (C.c_int * nf)(*[int(s) for s in avgscheme]),
                       _lib.dptr(g[0]), shp[0], _lib.dptr(g[1]), shp[1], _lib.dptr(g[2]), shp[2], op)
        return outs

    def scatter_fields(self):
        """Properties + the field list of a step: nodes (rho, etas, cp, T, H, mat), cell centres (etan) and the three mixed sets
        of the conductivity (k_d at the midpoints along d and the nodes along the other two axes, cf. pylamp2.py:312-313)."""
        self.update_properties()
        g, mp, f = self.grid, self.gridmp, {}
        A, G = INTERP_AVG_ARITHW, INTERP_AVG_GEOMW
        if self.opt.do_heatdiff:
            f["rho"], f["etas"], f["cp"], f["T"], f["H"], f["mat"] = self.scatter([TR_RHO, TR_ETA, TR_HCP, TR_TMP, TR_IHT, TR_MAT], [A, G, A, A, A, A])
            f["etan"], = self.scatter([TR_ETA], [G], mp)
            f["kz"], = self.scatter([TR_HCD], [A], [mp[0], g[1], g[2]])
            f["kx"], = self.scatter([TR_HCD], [A], [g[0], mp[1], g[2]])
            f["ky"], = self.scatter([TR_HCD], [A], [g[0], g[1], mp[2]])
        else:
            f["rho"], f["etas"] = self.scatter([TR_RHO, TR_ETA], [A, G])
            f["etan"], = self.scatter([TR_ETA], [INTERP_AVG_GEOMETRIC], mp)            # unweighted, as pylamp2.py:322
        return f

    def temp_to_tracers(self, field, absolute, tstep=0.0):
        """Nodal temperature (absolute) or its increment to the tracers; the increment with subgrid diffusion if enabled."""
        self._lib_call("pl3_resident_temp_to_tracers", 1 if absolute else 0, _lib.dptr(_f3(field, self.nx)),
                       0 if absolute or not self.opt.do_subgrid_heatdiff else 1, float(tstep))

    def _refill_args(self, it):
        o = self.opt
        out = (C.c_int64 * 4)()
        return out, (int(o.tracdens), int(o.tracdens_min), int(o.inject_seed) & (2 ** 64 - 1), int(self.it if it is None else it),
                     1 if o.inject_unique_ids else 0, out)

    def _counters(self, out):
        """The four counters of a sort with refill; with Options3.marker_deletion also nremoved, and with an inflow material set also
        ninflow, the new tracers that took a wall's material (without them the dict keeps its four keys: callers compare it whole).
        ntrac follows the first two."""
        c = dict(ninjected=int(out[0]), nrefilled=int(out[1]), nempty=int(out[2]), mincount=int(out[3]))
        gone = self.ctx.tracers_removed()[0]
        if self.opt.marker_deletion:
            c["nremoved"] = gone
        if self._inflow:
            c["ninflow"] = self.ctx.inflow_count()[0]
        self.ntrac += c["ninjected"] - gone
        return c

    def refill(self, it=None):
        """Sort + census + refill of the cells below opt.tracdens_min to opt.tracdens, without advection (a sparse initial set is
        topped up with it).  `it` selects the random stream (default: the step counter).  Returns ninjected, nrefilled (cells),
        nempty (cells without any tracer before the call) and mincount (smallest count before the call); with Options3.marker_deletion
        also nremoved, the tracers the sort removed (the counts are those after the removal); with an inflow material set also ninflow,
        the new tracers that took a wall's material."""
        out, args = self._refill_args(it)
        self._lib_call("pl3_resident_refill", *args)
        return self._counters(out)

    def advect(self, grids, vels, tstep, it=None):
        """RK4 + fence (with Options3.marker_deletion: no fence, the sort removes the tracers outside the box) + the sort by cell with
        the refill in the same pass; returns the counters of refill()."""
        shp = tuple(v + 1 for v in self.nx)
        g = [_lib.f64(c) for c in grids]; V = [_f3(a, shp) for a in vels]
        out, args = self._refill_args(it)
        self._lib_call("pl3_resident_advect", *[_lib.dptr(c) for c in g], *[_lib.dptr(a) for a in V], float(tstep),
                       0 if self.opt.marker_deletion else 1, *args)
        return self._counters(out)

    # -- one time step -----------------------------------------------------------------------------------------------
    _NAN_MESSAGE = ("Simulation3.step: the scattered field '%s' holds NaN at %d nodes - a grid node without any marker in "
                    "reach makes the interpolated fields NaN, and so do tracers injected into a cell without residents "
                    "(their fields are 0/0 as in pylamp2.py:624-629): raise the marker density or enable injection "
                    "(Options3.tracdens / tracdens_min) before cells run empty")

    def _step_resident(self):
        """step() as one library call: the fields stay on the device."""
        o = self.opt
        cfg = _lib.Step3Config()
        for k in ("do_heatdiff", "do_subgrid_heatdiff", "tdep_rho", "tdep_eta", "stokes_maxit", "heat_maxit", "tracdens", "tracdens_min"):
            setattr(cfg, k, int(getattr(o, k)))
        for k in ("etamin", "etamax", "tstep_adv_max", "tstep_adv_min", "tstep_dif_max", "tstep_dif_min", "tstep_modifier", "stokes_rtol",
                  "heat_rtol"):
            setattr(cfg, k, float(getattr(o, k)))
        cfg.tref = float(o.Tref)
        for w in range(6):
            cfg.bcheat[w] = int(o.bcheat[w]); cfg.bcheatvals[w] = float(o.bcheatvals[w])
        cfg.use_grav = 0 if o.grav is None else 1
        for d in range(3):
            cfg.grav[d] = 0.0 if o.grav is None else float(o.grav[d])
        cfg.inject_seed = int(o.inject_seed) & (2 ** 64 - 1)
        cfg.inject_unique_ids = 1 if o.inject_unique_ids else 0
        r = _lib.Step3Report()
        if self.ctx.nranks_attached():
            raise Exception("Simulation3: several ranks are not supported by the 3-D markers")
        rc = self.ctx.lib.pl3_resident_step(self.ctx.handle(), C.byref(cfg), self.it + 1, C.byref(r))
        if rc != 0:
            self.fields = {}
            for name, n in (("rho", r.nan_rho), ("etas", r.nan_etas)):
                if n > 0:
                    raise Exception(self._NAN_MESSAGE % (name, int(n)))
            self.ctx.check(rc)
        self.it += 1
        self.ntrac = int(r.ntrac)
        self.totaltime += r.tstep
        rep = dict(it=self.it, tstep=r.tstep, limiter="H" if r.limiter else "S", stokes=r.stokes.as_dict(),
                   heat=r.heat.as_dict() if o.do_heatdiff else None, ninjected=int(r.ninjected), nrefilled=int(r.nrefilled),
                   nempty=int(r.nempty), mincount=int(r.mincount), nremoved=int(r.nremoved))
        if self._inflow:                         # (the staged step's key order: the counters of the sort, then time and ntrac)
            rep["ninflow"] = self.ctx.inflow_count()[0]
        rep.update(time=self.totaltime, ntrac=self.ntrac)
        if self.warm_start[0]:
            rep["stokes_start"] = self.ctx.history_info()["start"]
        if self.shear_heating or self.strain_fields:
            rep["dissipation_total"] = self.ctx.dissipation_total()
        if self.yield_stress is not None:
            rep["picard"] = self.ctx.picard_report()
        self.fields = {}
        self._stepped = True
        self.last = rep
        return rep

    def step(self):
        o = self.opt
        if o.resident:
            return self._step_resident()
        self.it += 1
        dx = [self.L[d] / (self.nx[d] - 1) for d in range(3)]
        f = self.scatter_fields()
        for name in ("rho", "etas"):
            if np.isnan(f[name]).any():
                self.it -= 1
                raise Exception(self._NAN_MESSAGE % (name, int(np.isnan(f[name]).sum())))
        if o.do_heatdiff:
            if self.it > 1:                      # pylamp2.py:327-331: the walls keep the solved temperature
                nt = self._newtemp
                for d in range(3):
                    for w in (0, -1):
                        s = [slice(None)] * 3; s[d] = w
                        f["T"][tuple(s)] = nt[tuple(s)]
            diffusivity = f["kz"] / (f["rho"] * f["cp"])
            tstep_temp = o.tstep_modifier * np.min(dx) ** 2 / np.max(2 * diffusivity)
            tstep_temp = max(min(tstep_temp, o.tstep_dif_max), o.tstep_dif_min)
        A, _ = makeStokesMatrix(self.nx, self.grid, f["etas"], f["etan"], f["rho"], bc=self.bcstokes, grav=o.grav, ctx=self.ctx,
                                wallvel=self.bcstokesvel)
        x = solve(A, rtol=o.stokes_rtol, maxit=o.stokes_maxit)
        picard = None
        if self.yield_stress is not None:        # the Picard loop of pl3_resident_step
            picard = picard_loop(A, o.picard_maxit, o.picard_tol, rtol=o.stokes_rtol, maxit=o.stokes_maxit)
            x = solution(A)                      # (the last update keeps its Kcont-scaled pressure in step with the operator's new scaling)
            f["etas_eff"], f["etan_eff"] = coefficients(A)
        newvel, pres = x2vp(x, self.nx)
        with np.errstate(divide="ignore"):       # (a fluid at rest: the clamp below takes tstep_adv_max)
            tstep_stokes = o.tstep_modifier * np.min(dx) / max(np.max(v) for v in newvel)
        tstep_stokes = max(min(tstep_stokes, o.tstep_adv_max), o.tstep_adv_min)
        if o.do_heatdiff:
            limiter = "H" if tstep_temp < tstep_stokes else "S"
            tstep = min(tstep_temp, tstep_stokes)
        else:
            tstep, limiter = tstep_stokes, "S"
        rep = dict(it=self.it, tstep=tstep, limiter=limiter, stokes=A.last_stats, heat=None)
        if self.warm_start[0]:
            self.ctx.commit_solution(tstep)      # (as pl3_resident_step does: both paths keep the same history)
        f.update(velz=newvel[0], velx=newvel[1], vely=newvel[2], pres=pres)
        if self.shear_heating or self.strain_fields:
            sf = strain_fields(A)                # (of the solution on the device: the kernel of the resident step)
            dissipation_total = sf.pop("dissipation_total")
            f.update(sf)
            if self.shear_heating:
                f["H"] = f["H"] + f["dissipation"]
        if o.do_heatdiff:
            H, _ = makeDiffusionMatrix(self.nx, self.grid, self.gridmp, f["T"], [f["kz"], f["kx"], f["ky"]], f["cp"], f["rho"], f["H"],
                                       o.bcheat, o.bcheatvals, tstep, ctx=self.ctx)
            newtemp = x2t(solve_heat(H, rtol=o.heat_rtol, maxit=o.heat_maxit), self.nx).copy()
            rep["heat"] = H.last_stats
            if self.it == 1:
                self.temp_to_tracers(newtemp, True)
            else:
                self.temp_to_tracers(newtemp - f["T"], False, tstep)
            self._newtemp = newtemp
            f["temp"] = newtemp
        grids, vels = advection_velocity(newvel, self.gridmp, self.nx, self.bcstokes, self.bcstokesvel, self.bcstokesflow)
        rep.update(self.advect(grids, vels, tstep, self.it))
        rep.setdefault("nremoved", 0)
        self.totaltime += tstep
        rep["time"] = self.totaltime; rep["ntrac"] = self.count()
        if self.warm_start[0]:
            rep["stokes_start"] = self.ctx.history_info()["start"]
        if self.shear_heating or self.strain_fields:
            rep["dissipation_total"] = dissipation_total
        if picard is not None:
            rep["picard"] = picard
        self.fields = f
        self.last = rep
        return rep

    def write_snapshot(self, outdir="out"):
        """griddata.NNNNNN.npz / tracs.NNNNNN.npz with the keys of the 2-D snapshots (pylamp2.py:637-650) plus the third axis."""
        import os
        if self.opt.resident and self._stepped:
            f = {k: self.field(k) for k in ("velz", "velx", "vely", "pres", "rho")}
            if self.opt.do_heatdiff:
                f["temp"] = self.field("temp")
            if self.shear_heating or self.strain_fields:
                f.update({k: self.field(k) for k in STRAIN_FIELDS})
            if self.yield_stress is not None:
                f.update({k: self.field(k) for k in ("etas_eff", "etan_eff")})
        else:
            f = self.fields
        extra = {k: f[k] for k in STRAIN_FIELDS} if self.shear_heating or self.strain_fields else {}
        if self.yield_stress is not None:
            extra.update(etas_eff=f["etas_eff"], etan_eff=f["etan_eff"])
        temp = f["temp"] if "temp" in f else f["velx"] * 0.0
        tr_x, tr_f = self.tracers(); tr_v = self.tracer_velocity()
        os.makedirs(outdir, exist_ok=True)
        np.savez(os.path.join(outdir, "griddata.{:06d}.npz".format(self.it)), gridz=self.grid[0], gridx=self.grid[1], gridy=self.grid[2],
                 velz=f["velz"], velx=f["velx"], vely=f["vely"], pres=f["pres"], rho=f["rho"], temp=temp, tstep=self.it, time=self.totaltime, **extra)
        np.savez(os.path.join(outdir, "tracs.{:06d}.npz".format(self.it)), tr_x=tr_x, tr_f=tr_f, tr_v=tr_v, tstep=self.it, time=self.totaltime)

    def close(self):
        self.ctx.close()


def falling_sphere_tracers(nx, L, rng, per_axis=2, radius=0.15, centre=(0.3, 0.5, 0.5), jitter=0.2):
    """A dense, stiff sphere (3400 kg/m3, 1e22 Pa s) in a lighter, weaker fluid (3300 kg/m3, 1e19 Pa s): the 3-D counterpart of
    the reference's falling-block model (pylamp2.py:172-183).  Tracers sit on a jittered regular lattice of per_axis^3 per
    cell, so that no cell starts empty; radius and centre are fractions of L[0] and of L."""
    ax = []
    for d in range(3):
        m = per_axis * (int(nx[d]) - 1)
        ax.append((np.arange(m) + 0.5) * (float(L[d]) / m))
    Z, X, Y = np.meshgrid(*ax, indexing="ij")
    tr_x = np.stack([Z.ravel(), X.ravel(), Y.ravel()], axis=1)
    n = tr_x.shape[0]
    tr_x += rng.uniform(-jitter, jitter, (n, 3)) * np.array([float(L[d]) / (per_axis * (int(nx[d]) - 1)) for d in range(3)])
    tr_f = np.zeros((n, NFTRAC))
    tr_f[:, TR__ID] = np.arange(n)
    tr_f[:, 6] = 3300; tr_f[:, TR_MAT] = 1; tr_f[:, 10] = 1e19            # TR_RH0, TR_ET0
    r2 = sum((tr_x[:, d] - centre[d] * float(L[d])) ** 2 for d in range(3))
    inside = r2 < (radius * float(L[0])) ** 2
    tr_f[inside, 6] = 3400; tr_f[inside, TR_MAT] = 2; tr_f[inside, 10] = 1e22
    return tr_x, tr_f
