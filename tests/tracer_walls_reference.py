"""TEST INFRASTRUCTURE ONLY -- numpy reference of the tracers' fixed-value walls and wall flux, on top of
oracle/hdg_oracle.py, oracle/tracer_oracle.py, tests/tracer_diffusion_reference.py, tests/buoyancy_reference.py and
tests/viscosity_reference.py, which it imports and does not change.

Per wall side w a tracer is no-flux (the form D of section 19) or held at a fixed value g_w.  On a fixed-value wall edge e of
cell K, n out of the domain:

    D_w(chi, q) = int_e ( chi dn q + q dn chi - eta_b chi q )          l_w(chi; g) = g int_e ( eta_b chi - dn chi )
    eta_b       = (k+1)(k+2)/2 P_K/|K|
    tendency    = M^-1 T(q, P(Q)) + kappa M^-1 ( D q + sum_w D_w q + sum_w l_w(.; g_w) )
    Phi_w       = kappa int_w ( dn q - eta_b (q - g_w) ) ds = kappa l_w(.; 1) . (g_w 1 - q)      (the form against chi = 1)

assembled in the nodal basis of the oracle with its exact edge rule (d.eq_exact).  Sides of the unit square in the order
bottom (y = 0), right (x = 1), top (y = 1), left (x = 0); a general mesh has one side, the whole boundary, at index 0.
Walls are a dict {side: value}; a missing side is no flux."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tracer_diffusion_reference as tdr
from buoyancy_reference import B, _as2d, _kappa

__all__ = ["SIDES", "side_of_edges", "wall_terms", "WallOperator", "imex_with_walls", "implicit_with_walls", "dg_with_walls",
           "euler_at_rest", "integral"]

SIDES = ("bottom", "right", "top", "left")


def side_of_edges(d, general=False):
    """The side index of every boundary edge, in the order of d.ebnd."""
    m = d.mesh
    eb = d.ebnd
    if general:
        return np.zeros(len(eb), dtype=int)
    mid = 0.5 * (m.edge_a[eb] + m.edge_b[eb])
    L = float(np.max(m.edge_b[:, 0]))
    tol = 1e-9 * L
    side = np.full(len(eb), -1)
    side[np.abs(mid[:, 1]) < tol] = 0
    side[np.abs(mid[:, 0] - L) < tol] = 1
    side[np.abs(mid[:, 1] - L) < tol] = 2
    side[np.abs(mid[:, 0]) < tol] = 3
    assert np.all(side >= 0)
    return side


def wall_terms(d, general=False):
    """Per side (four entries; a general mesh fills the first only): (D_w [NP, NP], l_w(.; 1) [NP]) in the nodal basis."""
    m, k = d.mesh, d.k
    eb = d.ebnd
    out = [(np.zeros((d.NP, d.NP)), np.zeros(d.NP)) for _ in range(4)]
    if len(eb) == 0:
        return out
    v = m.cell_vertices
    per = sum(np.linalg.norm(v[:, (i + 1) % 3] - v[:, i], axis=1) for i in range(3))
    ratio = per / (0.5 * m.detJ)
    cells, nb = m.edge_plus[eb], m.edge_normal_plus[eb]
    eta_b = 0.5 * (k + 1) * (k + 2) * ratio[cells]
    val, grad, wl = tdr._edge_tab_p(d, eb, cells)
    dn = np.einsum("mqkd,md->mqk", grad, nb)
    W = (np.einsum("mq,mqi,mqj->mij", wl, val, dn) + np.einsum("mq,mqi,mqj->mij", wl, dn, val)
         - eta_b[:, None, None] * np.einsum("mq,mqi,mqj->mij", wl, val, val))
    lv = eta_b[:, None] * np.einsum("mq,mqi->mi", wl, val) - np.einsum("mq,mqi->mi", wl, dn)
    side = side_of_edges(d, general)
    for i in range(len(eb)):
        Dw, l = out[side[i]]
        Dw[np.ix_(d.dofP[cells[i]], d.dofP[cells[i]])] += W[i]
        l[d.dofP[cells[i]]] += lv[i]
    return out


class WallOperator:
    """Everything of one discretisation: D, the wall terms per side, M; built once, read-only."""

    def __init__(self, d, general=False):
        self.d, self.general = d, general
        self.sides = ("boundary",) if general else SIDES
        self.D = tdr.diffusion_matrix(d)
        self.terms = wall_terms(d, general)
        self.M = d.MP.toarray()
        self.A0 = np.linalg.solve(self.M, self.D)
        for a in [self.D, self.M, self.A0] + [x for t in self.terms for x in t]:
            a.setflags(write=False)

    def _idx(self, walls):
        return [(self.sides.index(s), float(g)) for s, g in (walls or {}).items()]

    def form(self, walls):
        """(D + sum_w D_w, sum_w g_w l_w): the bilinear form and the load, before M^-1"""
        Dw, l = self.D.copy(), np.zeros(self.d.NP)
        for w, g in self._idx(walls):
            Dw = Dw + self.terms[w][0]
            l = l + g * self.terms[w][1]
        return Dw, l

    def minv(self, walls):
        """(A, b): what hdg_apply_tracer_wall_diffusion applies, out = A q + b"""
        if not walls:
            return self.A0, np.zeros(self.d.NP)
        Dw, l = self.form(walls)
        return np.linalg.solve(self.M, Dw), np.linalg.solve(self.M, l)

    def flux(self, walls, kappa, q):
        """Phi_w of the four sides (0 on a no-flux side), positive into the domain"""
        out = np.zeros(4)
        for w, g in self._idx(walls):
            l = self.terms[w][1]
            out[w] = kappa * float(l @ (g - q))
        return out

    def tendency(self, tr, walls, kappa):
        """tend(q [n, NP], u) of n tracers: walls a dict for all or a list of n dicts (None: no flux), kappa scalar or n values"""
        def fn(q, u):
            n = q.shape[0]
            ws = [walls] * n if (walls is None or isinstance(walls, dict)) else list(walls)
            kap = _kappa(kappa, n)
            out = np.empty_like(q)
            for t in range(n):
                out[t] = tr._lu_mp.solve(tr.tracer_form(q[t], u))
                if kap[t] != 0.0:
                    A, b = self.minv(ws[t])
                    out[t] = out[t] + kap[t] * (A @ q[t] + b)
            return out
        return fn


def integral(d, q):
    """int q"""
    return float(np.ones(d.NP) @ (d.MP @ q))


def euler_at_rest(op, walls, kappa, dt, q0, nsteps):
    """Forward Euler at zero velocity: the states q_0 .. q_nsteps"""
    A, b = op.minv(walls)
    qs = [np.array(q0, dtype=float)]
    for _ in range(nsteps):
        qs.append(qs[-1] + dt * kappa * (A @ qs[-1] + b))
    return qs


def imex_with_walls(o, tr, tend, Q0, p0, q0, f_rhs, T_final, beta=0.0, g=(0.0, -1.0), nu=0.0, Avisc=None):
    """OracleHDGIMEX.step (projection method or the monolithic stage solve, as o says) with the tracers carried along by
    tend(q, u) (WallOperator.tendency), the buoyancy B(q^(j)) and nu Avisc Q^(j) in every forcing slot: the loop of
    viscosity_reference.imex_with_viscosity with the tracer tendency handed in."""
    from oracle.hdg_oracle import _solve_singular

    d, dt, s = o.disc, o.dt, o.nstages
    nt = int(np.round(T_final / dt))
    one = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    visc = (lambda Qj: nu * (Avisc @ Qj.ravel()).reshape(-1, 2)) if Avisc is not None and nu != 0.0 else (lambda Qj: 0.0)
    slot = lambda t, Qj, qj: f_rhs(t) + visc(Qj) + B(d, qj, beta, g)
    o.set_initial_condition(Q0, p0)
    for k in range(nt):
        tn = k * dt
        qs = [q.copy()] + [None] * (s - 1)
        o.stage_Q[0], o.stage_p[0], o.stage_l[0] = o.Q.copy(), o.p.copy(), o.lam.copy()
        o.b_rhs[0] = slot(tn + o.c_expl[0] * dt, o.stage_Q[0], qs[0])
        for i in range(1, s):
            o.Qstar[i - 1] = d.project_bdm(o.stage_Q[i - 1])
            adt = o.a_impl[i, i] * dt
            F = d.assemble_f_impl(o.Qstar[i - 1], o.flux)
            ri = o._residual(i)
            if o.use_projection_method:
                lu = spla.splu((d.MQ - adt * F).tocsc())
                for _ in range(o.n_richardson):
                    Qi = o.stage_Q[i].ravel()
                    rhs = ri - d.MQ @ Qi + adt * (F @ Qi + d.G_p @ o.stage_p[i] + d.G_l @ o.stage_l[i])
                    dQ = lu.solve(rhs)
                    o.Q_tent[i] = dQ.reshape(-1, 2)
                    du, dp, dl = d.solve_mixed_poisson(rP=-(1.0 / adt) * (d.Wdiv @ dQ))
                    dp, dl = d.shift_pressure(dp, dl)
                    o.stage_Q[i] = o.stage_Q[i] + o.Q_tent[i] + adt * du.reshape(-1, 2)
                    o.stage_p[i] = o.stage_p[i] + dp
                    o.stage_l[i] = o.stage_l[i] + dl
            else:
                Ktop = sp.bmat([[d.MQ - adt * F, -adt * d.G_p, -adt * d.G_l], [d.Bdiv, d.T, -d.Et], [d.CT.T, d.Et.T, -d.Lm]], format="csc")
                x = _solve_singular(d, Ktop, np.concatenate([ri, np.zeros(d.NP + d.NL)]))
                o.stage_Q[i] = x[: d.NQ].reshape(-1, 2)
                o.stage_p[i] = x[d.NQ: d.NQ + d.NP]
                o.stage_l[i] = x[d.NQ + d.NP:]
            o.stage_p[i], o.stage_l[i] = d.shift_pressure(o.stage_p[i], o.stage_l[i])
            ui = tr.cg_project(o.stage_Q[i])
            acc = qs[0].copy()
            for j in range(i):
                if o.a_expl[i, j] != 0:
                    acc = acc + dt * o.a_expl[i, j] * tend(qs[j], ui)
            qs[i] = acc
            o.b_rhs[i] = slot(tn + o.c_expl[i] * dt, o.stage_Q[i], qs[i])
        qn = qs[0].copy()
        for i in range(s):
            if o.b_expl[i] != 0:
                qn = qn + dt * o.b_expl[i] * tend(qs[i], tr.cg_project(o.stage_Q[i]))
        u, phi, lam = d.solve_mixed_poisson(rQ=o._final_residual())
        o.Q = u.reshape(-1, 2)
        rP, rL = d.pressure_reconstruction_rhs(o.Q, slot(tn + dt, o.Q, qn))
        _, p, lam = d.solve_mixed_poisson(rP=rP, rL=rL)
        o.p, o.lam = d.shift_pressure(p, lam)
        q = qn
    return o.Q, o.p, (q[0] if one else q)


def implicit_with_walls(d, tr, tend, dt, Q0, p0, q0, f_rhs, T_final, flux="upwind"):
    """oracle.tracer_oracle.implicit_with_tracer with the tendency handed in: forward Euler from the fields at the START of
    the step, the velocity projected as tracer_tendency does."""
    from oracle.hdg_oracle import OracleHDGImplicit

    nt = int(np.round(T_final / dt))
    Q = Q0.copy()
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one_tracer = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    one = OracleHDGImplicit(d, dt, flux=flux)
    for k in range(nt):
        dq = dt * tend(q, tr.cg_project(Q))
        Q, p = one.solve(Q, p, lambda t, k=k: f_rhs(k * dt), dt)
        q = q + dq
    return Q, p, (q[0] if one_tracer else q)


def dg_with_walls(d, tr, tend, dt, Q0, p0, q0, f_rhs, nsteps, flux="upwind"):
    """tests/dg_reference.py: dg_step with the tracers, the tendency handed in."""
    from dg_reference import dg_step

    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one_tracer = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    for k in range(nsteps):
        f = np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)
        dq = dt * tend(q, tr.cg_project(Q))
        Q, p = dg_step(d, Q, f, dt, flux)
        q = q + dq
    return Q, p, (q[0] if one_tracer else q)
