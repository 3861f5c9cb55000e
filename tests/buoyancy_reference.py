"""TEST INFRASTRUCTURE ONLY -- numpy reference of the Boussinesq buoyancy term, on top of
oracle/hdg_oracle.py, oracle/tracer_oracle.py and tests/tracer_diffusion_reference.py, which it imports and does not change.

    du/dt + (u . grad) u + grad p = f(t) + sum_t beta_t q_t g            g constant, beta_t real

B(q) is the nodal interpolation of sum_t beta_t q_t g into the velocity space [DG_{k+1}]^2 (exact: DG_k is a subspace).  The
term is explicit, like the forcing: wherever a loop uses the forcing slot b_rhs[j] it uses b_rhs[j] + B(q^(j)):
  IMEX        slot j < s takes the stage tracer q_j (slot 0: q_n), slot s (b_new of the pressure reconstruction) takes q_{n+1}
  implicit    slot 0 takes q_n, the tracer at the start of the step, next to f(t_k)          (HDG and DG)
Tracers are a [n_tracers, NP] array (one tracer: [NP] is accepted and returned), kappa a scalar or one value per tracer."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

__all__ = ["embedding", "B", "imex_with_buoyancy", "implicit_with_buoyancy", "dg_with_buoyancy", "potential_energy",
           "kinetic_energy", "integrate_uy_times", "integrate_q_uy", "oracles", "rest_state", "wave_fields", "wave_amplitude",
           "crossing", "wave_run"]


def embedding(d):
    """[nu, np]: the values of the DG_k nodal basis at the DG_{k+1} nodes of the reference cell."""
    return d.PP.tabulate(d.PU.nodes)


def _as2d(q):
    q = np.asarray(q, dtype=float)
    return q.reshape(1, -1) if q.ndim == 1 else q


def B(d, q, beta, g):
    """sum_t beta_t q_t g in the velocity space: [nc * nu, 2] nodal."""
    q = _as2d(q)
    beta = np.broadcast_to(np.asarray(beta, dtype=float).reshape(-1), (q.shape[0],))
    a = np.zeros(q.shape[1])
    for t in range(q.shape[0]):
        if beta[t] != 0.0:  # a passive tracer is not read
            a = a + beta[t] * q[t]
    au = np.einsum("na,ca->cn", embedding(d), a.reshape(d.mesh.ncells, d.np_)).reshape(-1)
    return np.stack([g[0] * au, g[1] * au], axis=-1)


def _tendency(tr, A, kappa, q, u):
    """M^-1 T(q_t, u) + kappa_t A q_t of every tracer; u is continuous already"""
    out = np.empty_like(q)
    for t in range(q.shape[0]):
        out[t] = tr._lu_mp.solve(tr.tracer_form(q[t], u))
        if A is not None and kappa[t] != 0.0:
            out[t] = out[t] + kappa[t] * (A @ q[t])
    return out


def _kappa(kappa, n):
    return np.broadcast_to(np.asarray(0.0 if kappa is None else kappa, dtype=float).reshape(-1), (n,))


def imex_with_buoyancy(o, tr, beta, g, Q0, p0, q0, f_rhs, T_final, kappa=None, A=None, monitor=None):
    """OracleHDGIMEX.step (projection method or the monolithic stage solve, as o says) with the tracers carried along as in
    oracle.tracer_oracle.imex_with_tracer, and the buoyancy in every forcing slot.  monitor(step, Q, p, q) is called after
    every step."""
    from oracle.hdg_oracle import _solve_singular

    d, dt, s = o.disc, o.dt, o.nstages
    nt = int(np.round(T_final / dt))
    one = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    kap = _kappa(kappa, q.shape[0])
    o.set_initial_condition(Q0, p0)
    for k in range(nt):
        tn = k * dt
        qs = [q.copy()] + [None] * (s - 1)
        o.b_rhs[0] = f_rhs(tn + o.c_expl[0] * dt) + B(d, qs[0], beta, g)
        o.stage_Q[0], o.stage_p[0], o.stage_l[0] = o.Q.copy(), o.p.copy(), o.lam.copy()
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
            # the stage tracer (the velocity of stage i for every j, as the reference writes it), then its slot
            ui = tr.cg_project(o.stage_Q[i])
            acc = qs[0].copy()
            for j in range(i):
                if o.a_expl[i, j] != 0:
                    acc = acc + dt * o.a_expl[i, j] * _tendency(tr, A, kap, qs[j], ui)
            qs[i] = acc
            o.b_rhs[i] = f_rhs(tn + o.c_expl[i] * dt) + B(d, qs[i], beta, g)
        qn = qs[0].copy()
        for i in range(s):
            if o.b_expl[i] != 0:
                qn = qn + dt * o.b_expl[i] * _tendency(tr, A, kap, qs[i], tr.cg_project(o.stage_Q[i]))
        u, phi, lam = d.solve_mixed_poisson(rQ=o._final_residual())
        o.Q = u.reshape(-1, 2)
        rP, rL = d.pressure_reconstruction_rhs(o.Q, f_rhs(tn + dt) + B(d, qn, beta, g))
        _, p, lam = d.solve_mixed_poisson(rP=rP, rL=rL)
        o.p, o.lam = d.shift_pressure(p, lam)
        q = qn
        if monitor is not None:
            monitor(k + 1, o.Q, o.p, q[0] if one else q)
    return o.Q, o.p, (q[0] if one else q)


def implicit_with_buoyancy(d, tr, beta, g, dt, Q0, p0, q0, f_rhs, T_final, flux="upwind", use_projection_method=True, kappa=None, A=None):
    """oracle.tracer_oracle.implicit_with_tracer with f(t_k) + B(q_n) as the forcing of step k."""
    from oracle.hdg_oracle import OracleHDGImplicit

    nt = int(np.round(T_final / dt))
    Q = Q0.copy()
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one_tracer = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    kap = _kappa(kappa, q.shape[0])
    one = OracleHDGImplicit(d, dt, flux=flux, use_projection_method=use_projection_method)
    for k in range(nt):
        dq = dt * _tendency(tr, A, kap, q, tr.cg_project(Q))  # fields at the START of the step
        f = f_rhs(k * dt) + B(d, q, beta, g)
        Q, p = one.solve(Q, p, lambda t, f=f: f, dt)
        q = q + dq
    return Q, p, (q[0] if one_tracer else q)


def dg_with_buoyancy(d, tr, beta, g, dt, Q0, p0, q0, f_rhs, nsteps, flux="upwind", kappa=None, A=None):
    """tests/dg_reference.py: dg_step with the tracer and f(t_k) + B(q_n)."""
    from dg_reference import dg_step

    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume
    one_tracer = np.asarray(q0).ndim == 1
    q = _as2d(q0).copy()
    kap = _kappa(kappa, q.shape[0])
    for k in range(nsteps):
        f = (np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)) + B(d, q, beta, g)
        dq = dt * _tendency(tr, A, kap, q, tr.cg_project(Q))
        Q, p = dg_step(d, Q, f, dt, flux)
        q = q + dq
    return Q, p, (q[0] if one_tracer else q)


# ---- integrals under the oracle's cell rule (exact to degree 3k+4)
def _cell_points(d):
    from oracle.fem import triangle_quadrature

    m = d.mesh
    qp, _ = triangle_quadrature(3 * d.k + 4)
    return m.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,qr->cqd", m.J, qp)


def kinetic_energy(d, Q):
    return 0.5 * float(Q.ravel() @ (d.MQ @ Q.ravel()))


def potential_energy(d, q, beta, g):
    """PE = - sum_t beta_t int q_t (g . x)"""
    q = _as2d(q)
    beta = np.broadcast_to(np.asarray(beta, dtype=float).reshape(-1), (q.shape[0],))
    X = _cell_points(d)
    gx = g[0] * X[..., 0] + g[1] * X[..., 1]
    pe = 0.0
    for t in range(q.shape[0]):
        qh = np.einsum("qa,ca->cq", d.cP, q[t].reshape(d.mesh.ncells, d.np_))
        pe -= beta[t] * float(np.sum(d.cwdet * qh * gx))
    return pe


def integrate_uy_times(d, Q, fn):
    """int u_y fn(x, y)"""
    X = _cell_points(d)
    uy = np.einsum("qa,ca->cq", d.cU, Q.reshape(d.mesh.ncells, d.nu, 2)[..., 1])
    return float(np.sum(d.cwdet * uy * fn(X[..., 0], X[..., 1])))


def integrate_q_uy(d, q, Q):
    """int q u_y"""
    qh = np.einsum("qa,ca->cq", d.cP, q.reshape(d.mesh.ncells, d.np_))
    uy = np.einsum("qa,ca->cq", d.cU, Q.reshape(d.mesh.ncells, d.nu, 2)[..., 1])
    return float(np.sum(d.cwdet * qh * uy))


# ---- the set-ups that the CPU tests (on the reference alone) and the GPU tests (engine against reference) share
def oracles(nx, k, **kw):
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    d = orc.HDGDiscretisation(nx, k, **kw)
    return d, TracerOracle(d)


# ---- 1. rest state: the force is the gradient of a continuous P_k potential
REST = {2: (lambda x, y: y, lambda x, y: -0.5 * y * y),
        3: (lambda x, y: y * y - 0.5 * y, lambda x, y: -(y ** 3) / 3.0 + 0.25 * y * y)}
# What the reference shows is NOT rounding level (DESIGN.md section 20 records the figures): the discrete pressure gradient of
# the scheme does not cancel the interpolated force exactly, a velocity of a few per cent of free fall remains, and the
# pressure reconstruction of the IMEX steppers returns a multiple of the potential for a steady gradient forcing (2.01 at
# k = 2, where the same run with the force as a plain user forcing shows both; 3.09 at k = 3), so no slope is asserted there.  The
# bounds: the pressure carries at least 80 % of the force, so max|Q| <= 0.2 T max|beta q g|; the implicit stepper's
# p ~ slope * potential has slope 1 within 10 %.
REST_SLOPE = {"implicit": 1.0}
G_DOWN = (0.0, -1.0)


def rest_state(which, k, nx=3, nsteps=3, dt=0.02):
    """(max|Q| / free fall, slope of the fit p ~ slope * (potential - mean), max|q - q0|, (Q, p, q)) after nsteps of the
    reference from rest"""
    from oracle import hdg_oracle as orc

    d, tr = oracles(nx, k)
    q_fn, phi_fn = REST[k]
    q0 = d.interpolate_pressure(q_fn)
    phi = d.interpolate_pressure(phi_fn)
    phi = phi - float(d.int_p @ phi) / d.mesh.volume
    Q0, p0 = np.zeros((d.mesh.ncells * d.nu, 2)), np.zeros(d.NP)
    zero = lambda t: np.zeros_like(Q0)
    if which == "ssp2":
        Q, p, q = imex_with_buoyancy(orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), tr, 1.0, G_DOWN, Q0, p0, q0, zero, nsteps * dt)
    else:
        Q, p, q = implicit_with_buoyancy(d, tr, 1.0, G_DOWN, dt, Q0, p0, q0, zero, nsteps * dt)
    free_fall = nsteps * dt * np.max(np.abs(q0))
    return np.max(np.abs(Q)) / free_fall, float(phi @ p) / float(phi @ phi), np.max(np.abs(q - q0)), (Q, p, q)


# ---- 2. gravity wave
# N = 1, dt = 0.06: N dt = 0.06, a quarter period of omega = N / sqrt 2 is 2.2214 = 37.02 steps.  The background is centred
# (q = -N^2 (y - 1/2)): the scheme does not balance a hydrostatic state exactly (see the rest state above), and the spurious
# velocity, which grows with max|q| T, has to stay small beside the wave; the amplitude below is orthogonal to it.
WAVE_N, WAVE_DT, WAVE_EPS, WAVE_STEPS = 1.0, 0.06, 1e-2, 40
WAVE_T = np.pi / (2.0 * WAVE_N / np.sqrt(2.0))


def wave_fields(d):
    Q0 = d.interpolate_velocity(lambda x, y: (WAVE_EPS * np.pi * np.sin(np.pi * x) * np.cos(np.pi * y),
                                              -WAVE_EPS * np.pi * np.cos(np.pi * x) * np.sin(np.pi * y)))
    return Q0, np.zeros(d.NP), d.interpolate_pressure(lambda x, y: -WAVE_N ** 2 * (y - 0.5))


def wave_amplitude(d, Q):
    """int u_y d_x(sin pi x sin pi y)"""
    return integrate_uy_times(d, Q, lambda x, y: np.pi * np.cos(np.pi * x) * np.sin(np.pi * y))


def crossing(amps, dt):
    """(the step in which the amplitude changes sign, the time of the crossing by linear interpolation)"""
    a = np.asarray(amps)
    n = int(np.nonzero(a[:-1] * a[1:] <= 0.0)[0][0])
    return n + 1, dt * (n + a[n] / (a[n] - a[n + 1]))


def wave_run(nx, k=2):
    """amplitudes after 0 .. WAVE_STEPS steps of SSP2(3,3,2) on the reference"""
    from oracle import hdg_oracle as orc

    d, tr = oracles(nx, k)
    Q0, p0, q0 = wave_fields(d)
    o = orc.OracleHDGIMEX(d, WAVE_DT, "imex_ssp2_332")
    zero = lambda t: np.zeros_like(Q0)
    amps = [wave_amplitude(d, Q0)]
    Q, p, q = imex_with_buoyancy(o, tr, 1.0, G_DOWN, Q0, p0, q0, zero, WAVE_STEPS * WAVE_DT,
                                 monitor=lambda n, Q, p, q: amps.append(wave_amplitude(d, Q)))
    return amps, (Q.copy(), p.copy(), q.copy()), d
