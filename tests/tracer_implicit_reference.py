"""TEST INFRASTRUCTURE ONLY -- numpy reference of the implicit tracer diffusion, on top of
tests/tracer_diffusion_reference.py and tests/tracer_walls_reference.py, which it imports and does not change.

The split step: a step transports the tracers with tend(q, u) of kappa = 0 (WallOperator.tendency with kappa 0), and where it
forms its new tracers q~ every tracer with kappa_t != 0 becomes the solution of

    (I - dt kappa_t M^-1 D_w) q = q~ + dt kappa_t M^-1 l_w            (dense solves here)

Held here: the three time loops with the split in that place, the dense solve, and a plain conjugate-gradient iteration in the
M inner product (which is the Euclidean one of the orthonormal modal basis the device works in) with the device's start
x_0 = q~ and its stop |r| <= rtol |b|, for iteration counts."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import tracer_diffusion_reference as tdr
import tracer_walls_reference as twr
from buoyancy_reference import B, _as2d, _kappa

__all__ = ["rho", "system", "solve_dense", "finish", "cg", "imex_split", "implicit_split", "dg_split", "euler_at_rest",
           "explicit_at_rest"]


def rho(op, walls=None):
    """Spectral radius of M^-1 (D + sum_w D_w): the diffusion number of these tests is tau rho"""
    A, _ = op.minv(walls)
    return float(np.max(np.abs(np.linalg.eigvals(A))))


def system(op, walls, tau, q):
    """(A, b) of one tracer: A = I - tau M^-1 D_w, b = q + tau M^-1 l_w"""
    Aw, lw = op.minv(walls)
    return np.eye(op.d.NP) - tau * Aw, q + tau * lw


def solve_dense(op, walls, tau, q):
    A, b = system(op, walls, tau, q)
    return np.linalg.solve(A, b)


def finish(op, walls, kappa, dt):
    """q~ [n, NP] -> q_{n+1}: the solve for every tracer with kappa_t != 0, the others untouched"""
    def fn(q):
        n = q.shape[0]
        ws = [walls] * n if (walls is None or isinstance(walls, dict)) else list(walls)
        kap = _kappa(kappa, n)
        out = q.copy()
        for t in range(n):
            if kap[t] != 0.0:
                out[t] = solve_dense(op, ws[t], dt * kap[t], q[t])
        return out
    return fn


def cg(op, walls, tau, q, rtol=1e-10, maxit=2000):
    """(x, iterations, |r| / |b|): plain CG on A x = b from x_0 = q, norms and products in the M inner product"""
    A, b = system(op, walls, tau, q)
    M = op.M
    dot = lambda u, v: float(u @ (M @ v))
    x = q.copy()
    r = b - A @ x
    p = r.copy()
    rr, bb = dot(r, r), dot(b, b)
    its = 0
    while rr > rtol * rtol * bb and its < maxit:
        y = A @ p
        alpha = rr / dot(p, y)
        x = x + alpha * p
        r = r - alpha * y
        rn = dot(r, r)
        p = r + (rn / rr) * p
        rr = rn
        its += 1
    return x, its, (np.sqrt(rr / bb) if bb > 0 else 0.0)


def imex_split(o, tr, tend, fin, Q0, p0, q0, f_rhs, T_final, beta=0.0, g=(0.0, -1.0), nu=0.0, Avisc=None):
    """tracer_walls_reference.imex_with_walls with q_{n+1} = fin(q~_{n+1}): the stage tracers and the tracer of the pressure
    reconstruction's forcing slot are the transported ones."""
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
        q = fin(qn)
    return o.Q, o.p, (q[0] if one else q)


def implicit_split(d, tr, tend, fin, dt, Q0, p0, q0, f_rhs, T_final, flux="upwind"):
    """tracer_walls_reference.implicit_with_walls with the solve behind the forward-Euler update"""
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
        q = fin(q + dq)
    return Q, p, (q[0] if one_tracer else q)


def dg_split(d, tr, tend, fin, dt, Q0, p0, q0, f_rhs, nsteps, flux="upwind"):
    """tracer_walls_reference.dg_with_walls with the solve behind the forward-Euler update"""
    from dg_reference import dg_step

    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one_tracer = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    for k in range(nsteps):
        f = np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)
        dq = dt * tend(q, tr.cg_project(Q))
        Q, p = dg_step(d, Q, f, dt, flux)
        q = fin(q + dq)
    return Q, p, (q[0] if one_tracer else q)


def euler_at_rest(op, walls, tau, q0, nsteps):
    """Backward Euler at zero velocity: the states q_0 .. q_nsteps"""
    qs = [np.array(q0, dtype=float)]
    for _ in range(nsteps):
        qs.append(solve_dense(op, walls, tau, qs[-1]))
    return qs


def explicit_at_rest(op, a_expl, b_expl, tau, q0, nsteps):
    """The explicit tableau at zero velocity and no-flux walls: q <- R(tau M^-1 D) q with its stability polynomial R"""
    c = tdr.stability_polynomial(a_expl, b_expl)
    qs = [np.array(q0, dtype=float)]
    for _ in range(nsteps):
        acc, v = np.zeros_like(qs[-1]), qs[-1].copy()
        for cm in c:
            acc = acc + cm * v
            v = tau * (op.A0 @ v)
        qs.append(acc)
    return qs
