"""TEST INFRASTRUCTURE ONLY -- numpy reference of the viscous term, on top of oracle/hdg_oracle.py,
tests/tracer_diffusion_reference.py and tests/buoyancy_reference.py, which it imports and does not change.

nu V(w, u) in the momentum equation, V the symmetric interior-penalty form on [DG_p]^2, p = k + 1, with Nitsche walls:

    V(w, u) = - sum_K int_K grad w : grad u
              + sum_{interior e} int_e ( [w].{dn u} + [u].{dn w} - eta_e [w].[u] )
              + sum_{wall e}     int_e ( (w.n)(n.dn u) + (u.n)(n.dn w) - eta_b (w.n)(u.n) )      normal component: always
              + sum_{wall e}     int_e ( (w.t)(t.dn u) + (u.t)(t.dn w) - eta_b (w.t)(u.t) )      tangential: wall = "no_slip" only
    [v] = v+ - v-,  {g} = (g+ + g-)/2,  dn u = (grad u) n,  n out of the '+' cell (out of the domain on a wall),  t normal to n
    eta_e = (p+1)(p+2)/4 max(P_K+/|K+|, P_K-/|K-|)          eta_b = (p+1)(p+2)/2 P_K/|K|

assembled in the nodal basis of the oracle's velocity space with its exact edge rule (d.eq_exact: degree 4k+7 >= 2p).  The
term is explicit, like the forcing: wherever a loop uses the forcing slot b_rhs[j] it uses b_rhs[j] + B(q^(j)) + nu M^-1 V Q^(j):
  IMEX        slot j < s takes the stage velocity Q_j (slot 0: Q_n), slot s (b_new of the pressure reconstruction) takes Q_{n+1}
  implicit    slot 0 takes Q_n, forward Euler, next to f(t_k)                                  (HDG and DG)"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from buoyancy_reference import B, _as2d, _kappa, _tendency

__all__ = ["WALLS", "penalties", "viscous_matrix", "minv_v", "imex_with_viscosity", "implicit_with_viscosity", "dg_with_viscosity",
           "kinetic_energy", "taylor_green_Qs", "TaylorGreenNS", "l2_error_velocity"]

WALLS = ("free_slip", "no_slip")


def penalties(d):
    """(eta_e of every interior edge in the order of d.eint, eta_b of every boundary edge in the order of d.ebnd)"""
    m, p = d.mesh, d.k + 1
    v = m.cell_vertices
    per = sum(np.linalg.norm(v[:, (i + 1) % 3] - v[:, i], axis=1) for i in range(3))
    ratio = per / (0.5 * m.detJ)
    c0 = 0.25 * (p + 1) * (p + 2)
    return c0 * np.maximum(ratio[m.edge_plus[d.eint]], ratio[m.edge_minus[d.eint]]), 2.0 * c0 * ratio[m.edge_plus[d.ebnd]]


def _edge_tab_u(d, edges, cells, n):
    """Values [m, q, nu], normal derivatives [m, q, nu] along n [m, 2] and weights [m, q] of the DG_{k+1} basis of `cells`."""
    m = d.mesh
    t, w = d.eq_exact
    x = m.edge_a[edges][:, None, :] + t[None, :, None] * (m.edge_b[edges] - m.edge_a[edges])[:, None, :]
    val, grad = d.PU.tabulate(m.ref_coords(cells, x), deriv=1)
    gphys = np.einsum("mrd,mqkr->mqkd", m.Jinv[cells], grad)
    return val, np.einsum("mqkd,md->mqk", gphys, n), w[None, :] * m.edge_len[edges][:, None]


def viscous_matrix(d, wall="free_slip"):
    """V as a dense [NQ, NQ] matrix in the nodal basis (rows and columns d.dofQ): V[i, j] = V(phi_i, phi_j)."""
    assert wall in WALLS
    m, nu, nc = d.mesh, d.nu, d.mesh.ncells
    dofs = np.arange(nc * nu).reshape(nc, nu)
    S = np.zeros((nc * nu, nc * nu))  # one component: the volume and the interior edges
    vol = -np.einsum("cq,cqid,cqjd->cij", d.cwdet, d.cUg, d.cUg)
    for c in range(nc):
        S[np.ix_(dofs[c], dofs[c])] += vol[c]
    eta_e, eta_b = penalties(d)
    e = d.eint
    n = m.edge_normal_plus[e]
    side = []
    for cells, sign in ((m.edge_plus[e], 1.0), (m.edge_minus[e], -1.0)):
        val, dn, wl = _edge_tab_u(d, e, cells, n)
        side.append((cells, sign, val, dn, wl))
    for (ca, sa, va, dna, wl) in side:  # test function on side a
        for (cb, sb, vb, dnb, _) in side:  # trial function on side b
            blk = (0.5 * sa * np.einsum("mq,mqi,mqj->mij", wl, va, dnb) + 0.5 * sb * np.einsum("mq,mqi,mqj->mij", wl, dna, vb)
                   - sa * sb * eta_e[:, None, None] * np.einsum("mq,mqi,mqj->mij", wl, va, vb))
            for i in range(len(e)):
                S[np.ix_(dofs[ca[i]], dofs[cb[i]])] += blk[i]
    V = np.zeros((d.NQ, d.NQ))
    V[0::2, 0::2] = S
    V[1::2, 1::2] = S
    eb = d.ebnd
    if len(eb):
        cells, nb = m.edge_plus[eb], m.edge_normal_plus[eb]
        val, dn, wl = _edge_tab_u(d, eb, cells, nb)
        W = (np.einsum("mq,mqi,mqj->mij", wl, val, dn) + np.einsum("mq,mqi,mqj->mij", wl, dn, val)
             - eta_b[:, None, None] * np.einsum("mq,mqi,mqj->mij", wl, val, val))
        for i in range(len(eb)):
            P = np.outer(nb[i], nb[i]) if wall == "free_slip" else np.eye(2)  # n n^T, plus t t^T with no slip
            for d1 in range(2):
                for d2 in range(2):
                    if P[d1, d2] != 0.0:
                        V[np.ix_(d.dofQ[cells[i], :, d1], d.dofQ[cells[i], :, d2])] += P[d1, d2] * W[i]
    return V


def minv_v(d, wall="free_slip", V=None):
    """M^-1 V, dense: what hdg_apply_viscosity applies to Q.ravel()."""
    V = viscous_matrix(d, wall) if V is None else V
    return np.linalg.solve(d.MQ.toarray(), V)


def _visc(A, nu, Q):
    return nu * (A @ Q.ravel()).reshape(-1, 2)


def imex_with_viscosity(o, A, nu, Q0, p0, f_rhs, T_final, tr=None, q0=None, beta=0.0, g=(0.0, -1.0), kappa=None, Adiff=None,
                        monitor=None):
    """OracleHDGIMEX.step (projection method or the monolithic stage solve, as o says) with nu A Q^(j), A = M^-1 V, in every
    forcing slot; with tr / q0 the tracers are carried along and force the flow as in buoyancy_reference.imex_with_buoyancy.
    Returns (Q, p) or (Q, p, q).  monitor(step, Q, p) is called after every step."""
    from oracle.hdg_oracle import _solve_singular

    d, dt, s = o.disc, o.dt, o.nstages
    nt = int(np.round(T_final / dt))
    tracers = q0 is not None
    q = _as2d(q0).copy() if tracers else None
    kap = _kappa(kappa, q.shape[0]) if tracers else None
    slot = lambda t, Qj, qj: f_rhs(t) + _visc(A, nu, Qj) + (B(d, qj, beta, g) if tracers else 0.0)
    o.set_initial_condition(Q0, p0)
    for k in range(nt):
        tn = k * dt
        qs = [q.copy() if tracers else None] + [None] * (s - 1)
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
            if tracers:
                ui = tr.cg_project(o.stage_Q[i])
                acc = qs[0].copy()
                for j in range(i):
                    if o.a_expl[i, j] != 0:
                        acc = acc + dt * o.a_expl[i, j] * _tendency(tr, Adiff, kap, qs[j], ui)
                qs[i] = acc
            o.b_rhs[i] = slot(tn + o.c_expl[i] * dt, o.stage_Q[i], qs[i])
        if tracers:
            qn = qs[0].copy()
            for i in range(s):
                if o.b_expl[i] != 0:
                    qn = qn + dt * o.b_expl[i] * _tendency(tr, Adiff, kap, qs[i], tr.cg_project(o.stage_Q[i]))
        u, phi, lam = d.solve_mixed_poisson(rQ=o._final_residual())
        o.Q = u.reshape(-1, 2)
        rP, rL = d.pressure_reconstruction_rhs(o.Q, slot(tn + dt, o.Q, qn if tracers else None))
        _, p, lam = d.solve_mixed_poisson(rP=rP, rL=rL)
        o.p, o.lam = d.shift_pressure(p, lam)
        if tracers:
            q = qn
        if monitor is not None:
            monitor(k + 1, o.Q, o.p)
    if tracers:
        return o.Q, o.p, (q[0] if np.asarray(q0).ndim == 1 else q)
    return o.Q, o.p


def implicit_with_viscosity(d, A, nu, dt, Q0, p0, f_rhs, T_final, flux="upwind", use_projection_method=True, monitor=None):
    """OracleHDGImplicit with f(t_k) + nu A Q_n as the forcing of step k (forward Euler)."""
    from oracle.hdg_oracle import OracleHDGImplicit

    nt = int(np.round(T_final / dt))
    Q = Q0.copy()
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one = OracleHDGImplicit(d, dt, flux=flux, use_projection_method=use_projection_method)
    for k in range(nt):
        f = f_rhs(k * dt) + _visc(A, nu, Q)
        Q, p = one.solve(Q, p, lambda t, f=f: f, dt)
        if monitor is not None:
            monitor(k + 1, Q, p)
    return Q, p


def dg_with_viscosity(d, A, nu, dt, Q0, p0, f_rhs, nsteps, flux="upwind"):
    """tests/dg_reference.py: dg_step with f(t_k) + nu A Q_n."""
    from dg_reference import dg_step

    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    for k in range(nsteps):
        f = (np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)) + _visc(A, nu, Q)
        Q, p = dg_step(d, Q, f, dt, flux)
    return Q, p


def kinetic_energy(d, Q):
    return 0.5 * float(Q.ravel() @ (d.MQ @ Q.ravel()))


# ---- the Taylor-Green field Q_s of the oracle: Laplace Q_s = -2 pi^2 Q_s, and Q_s . n = 0, dn (Q_s . t) = 0 on the unit square
def taylor_green_Qs(x, y):
    S = lambda z: np.sin((z - 0.5) * np.pi)
    C = lambda z: np.cos((z - 0.5) * np.pi)
    return -C(x) * S(y), S(x) * C(y)


class TaylorGreenNS:
    """oracle.hdg_oracle.TaylorGreen with the separable forcing of the Navier-Stokes solution: the time factor a(t) of
    Q = a(t) Q_s solves  a' = g(t) + ... , so the forcing is (a'(t) + 2 pi^2 nu a(t)) Q_s."""

    def __init__(self, disc, forcing="exponential", kappa=0.5, viscosity=0.0):
        from oracle.hdg_oracle import TaylorGreen

        self.tg = TaylorGreen(disc, forcing, kappa)
        self.viscosity = viscosity

    def initial_condition(self):
        return self.tg.initial_condition()

    def f_rhs(self, t):
        tg = self.tg
        a = np.exp(-tg.kappa * t) if tg.forcing == "exponential" else 1.0 - tg.kappa * t
        return tg.f_rhs(t) + 2.0 * np.pi ** 2 * self.viscosity * a * tg.Qs

    def solution(self, t):
        return self.tg.solution(t)


def l2_error_velocity(d, Q, amplitude):
    """L2 norm of Q - amplitude Q_s, the exact function under the oracle's cell rule"""
    from oracle.fem import triangle_quadrature

    m = d.mesh
    qp, _ = triangle_quadrature(3 * d.k + 4)
    X = m.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,qr->cqd", m.J, qp)
    Qh = np.einsum("qa,cad->cqd", d.cU, Q.reshape(m.ncells, d.nu, 2))
    ex = np.stack(taylor_green_Qs(X[..., 0], X[..., 1]), axis=-1) * amplitude
    return float(np.sqrt(np.sum(d.cwdet[..., None] * (Qh - ex) ** 2)))
