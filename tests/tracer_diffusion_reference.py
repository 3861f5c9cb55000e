"""TEST INFRASTRUCTURE ONLY -- numpy reference of the tracer diffusion term, on top of
oracle/hdg_oracle.py and oracle/tracer_oracle.py, which it imports and does not change.

The symmetric interior-penalty form on DG_k with no-flux walls (boundary edges carry no term):

    D(chi, q) = - sum_K int_K grad chi . grad q + sum_{interior e} int_e ( [chi]{grad q . n} + [q]{grad chi . n} - eta_e [chi][q] )
    [v] = v+ - v-,  {g} = (g+ + g-)/2,  n = the normal out of the '+' cell
    eta_e = (k+1)(k+2)/4 max(P_K+/|K+|, P_K-/|K-|)            P = perimeter, |K| = area

assembled in the nodal basis of the oracle with its exact edge rule (d.eq_exact: degree 4k+7 >= 2k), the time loops of
imex_with_tracer / implicit_with_tracer with kappa M^-1 D q added to every tracer tendency, and the real-axis stability
limit of an explicit tableau."""
import numpy as np

from oracle.tracer_oracle import _step_with_hook

__all__ = ["penalty", "diffusion_matrix", "minv_d", "imex_with_diffusion", "implicit_with_diffusion", "stability_polynomial",
           "stability_limit", "decay_errors", "decay_case", "dg_with_diffusion", "l2_error"]


def penalty(d):
    """eta_e of every interior edge (order of d.eint): Shahbazi's bound with the full perimeter."""
    m, k = d.mesh, d.k
    v = m.cell_vertices
    per = sum(np.linalg.norm(v[:, (i + 1) % 3] - v[:, i], axis=1) for i in range(3))
    ratio = per / (0.5 * m.detJ)
    e = d.eint
    return 0.25 * (k + 1) * (k + 2) * np.maximum(ratio[m.edge_plus[e]], ratio[m.edge_minus[e]])


def _edge_tab_p(d, edges, cells):
    """Values [m, q, np] and normal-free physical gradients [m, q, np, 2] of the DG_k basis of `cells` on `edges`."""
    m = d.mesh
    t, w = d.eq_exact
    x = m.edge_a[edges][:, None, :] + t[None, :, None] * (m.edge_b[edges] - m.edge_a[edges])[:, None, :]
    xi = m.ref_coords(cells, x)
    val, grad = d.PP.tabulate(xi, deriv=1)
    return val, np.einsum("mrd,mqkr->mqkd", m.Jinv[cells], grad), w[None, :] * m.edge_len[edges][:, None]


def diffusion_matrix(d):
    """D as a dense [NP, NP] matrix in the nodal basis: D[i, j] = D(phi_i, phi_j)."""
    m = d.mesh
    D = np.zeros((d.NP, d.NP))
    vol = -np.einsum("cq,cqid,cqjd->cij", d.cwdet, d.cPg, d.cPg)
    for c in range(m.ncells):
        D[np.ix_(d.dofP[c], d.dofP[c])] += vol[c]
    e = d.eint
    n = m.edge_normal_plus[e]
    eta = penalty(d)
    side = []
    for cells, sign in ((m.edge_plus[e], 1.0), (m.edge_minus[e], -1.0)):
        val, grad, wl = _edge_tab_p(d, e, cells)
        side.append((cells, sign, val, np.einsum("mqkd,md->mqk", grad, n), wl))
    for (ca, sa, va, dna, wl) in side:  # test function chi on side a
        for (cb, sb, vb, dnb, _) in side:  # trial function q on side b
            blk = (0.5 * sa * np.einsum("mq,mqi,mqj->mij", wl, va, dnb) + 0.5 * sb * np.einsum("mq,mqi,mqj->mij", wl, dna, vb)
                   - sa * sb * eta[:, None, None] * np.einsum("mq,mqi,mqj->mij", wl, va, vb))
            for i in range(len(e)):
                D[np.ix_(d.dofP[ca[i]], d.dofP[cb[i]])] += blk[i]
    return D


def minv_d(d, D=None):
    """M^-1 D, dense: what hdg_apply_tracer_diffusion applies."""
    D = diffusion_matrix(d) if D is None else D
    return np.linalg.solve(d.MP.toarray(), D)


def imex_with_diffusion(o, tr, A, kappa, Q0, p0, q0, f_rhs, T_final):
    """oracle.tracer_oracle.imex_with_tracer with kappa A q (A = M^-1 D) added to every tendency M^-1 T(q_j, P(Q_i))."""
    nt = int(np.round(T_final / o.dt))
    o.set_initial_condition(Q0, p0)
    q = q0.copy()
    s = o.nstages
    tend = lambda qj, u: tr._lu_mp.solve(tr.tracer_form(qj, u)) + kappa * (A @ qj)
    for k in range(nt):
        qs = [q.copy()] + [None] * (s - 1)

        def after_stage(i):
            ui = tr.cg_project(o.stage_Q[i])
            acc = qs[0].copy()
            for j in range(i):
                if o.a_expl[i, j] != 0:
                    acc = acc + o.dt * o.a_expl[i, j] * tend(qs[j], ui)
            qs[i] = acc

        _step_with_hook(o, f_rhs, k * o.dt, after_stage)
        qn = qs[0].copy()
        for i in range(s):
            if o.b_expl[i] != 0:
                qn = qn + o.dt * o.b_expl[i] * tend(qs[i], tr.cg_project(o.stage_Q[i]))
        q = qn
    return o.Q, o.p, q


def implicit_with_diffusion(d, tr, A, kappa, dt, Q0, p0, q0, f_rhs, T_final, flux="upwind"):
    """oracle.tracer_oracle.implicit_with_tracer with the extra term."""
    from oracle.hdg_oracle import OracleHDGImplicit

    nt = int(np.round(T_final / dt))
    Q = Q0.copy()
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    q = q0.copy()
    one = OracleHDGImplicit(d, dt, flux=flux)
    for k in range(nt):
        dq = dt * (tr.tracer_tendency(q, Q) + kappa * (A @ q))  # fields at the START of the step
        Q, p = one.solve(Q, p, lambda t, k=k: f_rhs(k * dt), dt)
        q = q + dq
    return Q, p, q


def stability_polynomial(a_expl, b_expl):
    """Coefficients c_0 .. c_s of R(z) = 1 + z b^T (I - z A)^-1 1 = sum_m c_m z^m of an explicit tableau."""
    A = np.asarray(a_expl, dtype=float)
    b = np.asarray(b_expl, dtype=float).reshape(-1)
    A = A.reshape(len(b), len(b))
    c, v = [1.0], np.ones(len(b))
    for _ in range(len(b)):
        c.append(float(b @ v))
        v = A @ v
    return np.array(c)


def stability_limit(a_expl, b_expl):
    """The right end x of the interval [0, x] on which |R(-x)| <= 1: the real-axis stability limit."""
    c = stability_polynomial(a_expl, b_expl)
    p = c * (-1.0) ** np.arange(len(c))  # p(x) = R(-x), ascending
    while len(p) > 1 and p[-1] == 0.0:
        p = p[:-1]
    if len(p) == 1:
        return np.inf
    cand = []
    for shift in (-1.0, 1.0):  # p(x) = 1 (the root x = 0 divided out), p(x) = -1
        r = p.copy()
        r[0] += shift
        if shift < 0:
            r = r[1:]
        cand += [z.real for z in np.atleast_1d(np.roots(r[::-1])) if abs(z.imag) <= 1e-12 * max(1.0, abs(z)) and z.real > 0]
    val = lambda x: abs(np.polyval(p[::-1], x))
    for x in sorted(cand):
        if val(x * (1 + 1e-6)) > 1.0:
            return float(x)
    return np.inf


def dg_with_diffusion(d, tr, A, kappa, dt, Q0, p0, q0, f_rhs, nsteps, flux="upwind"):
    """tests/dg_reference.py: dg_solve with the tracer, and the extra term in its forward-Euler update."""
    from dg_reference import dg_step

    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    q = np.array(q0, dtype=float)
    for k in range(nsteps):
        f = np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)
        dq = dt * (tr.tracer_tendency(q, Q) + kappa * (A @ q))  # fields at the START of the step
        Q, p = dg_step(d, Q, f, dt, flux)
        q = q + dq
    return Q, p, q


DECAY_STEPS = 40


def decay_case(k, nx):
    """kappa, dt, steps of the decay runs, CPU and GPU alike: kappa dt rho(M^-1 D) about 0.5 with rho h^2 about
    250 / 900 / 2200 at k = 1 / 2 / 3 (measured by tests/test_tracer_diffusion_cpu.py), DECAY_STEPS steps."""
    h = 2 * np.pi / nx
    return 1.0, 0.5 * h * h / {1: 250.0, 2: 900.0, 3: 2200.0}[k], DECAY_STEPS


def decay_errors(k, nx, kappa, dt, nsteps):
    """Forward Euler at zero velocity on the periodic square (L = 2 pi) from q0 = sin x sin y: the L2 error against
    exp(-2 kappa T) q0, the final field, the discretisation."""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k, periodic=True, L=2 * np.pi)
    A = minv_d(d)
    q0 = d.interpolate_pressure(lambda x, y: np.sin(x) * np.sin(y))
    q = q0.copy()
    for _ in range(nsteps):
        q = q + dt * kappa * (A @ q)
    return l2_error(d, q, np.exp(-2 * kappa * nsteps * dt)), q, d


def l2_error(d, q, amplitude):
    """L2 norm of q - amplitude sin x sin y, the exact function under the oracle's cell rule (exact to degree 3k+4)."""
    from oracle.fem import triangle_quadrature

    m = d.mesh
    qp, _ = triangle_quadrature(3 * d.k + 4)
    X = m.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,qr->cqd", m.J, qp)
    qh = np.einsum("qa,ca->cq", d.cP, q.reshape(m.ncells, d.np_))
    ex = amplitude * np.sin(X[..., 0]) * np.sin(X[..., 1])
    return float(np.sqrt(np.sum(d.cwdet * (qh - ex) ** 2)))
