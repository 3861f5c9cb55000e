"""CPU checker of the implicit DG discretisation (helper of the DG tests, not a test module).

Builds one step of IncompressibleEulerDGImplicit (reference: src/timesteppers/dg_implicit.py:10-136) from the public pieces of
the numpy oracle only (oracle/hdg_oracle.py: HDGDiscretisation.MQ, assemble_f_impl, Wdiv, project_bdm, int_p, mesh.volume;
oracle/tracer_oracle.py for the tracer) and solves it directly:

* dg_implicit.py:48-66   momentum rows  (M - dt F(Q*)) u - dt Wdiv^T phi   (F: the HDG f_impl with alpha = 1, hdg_imex.py:313-331;
                         the pressure terms -phi div w dx + 2 avg(w.n) avg(phi) dS + w.n phi ds are -Wdiv^T phi)
* dg_implicit.py:67-71   continuity rows  dt Wdiv u  (psi div v dx - 2 avg(v.n) avg(psi) dS - v.n psi ds = Wdiv, hdg_imex.py:353-365)
* dg_implicit.py:73      right-hand side  M Q + dt M f,  f at t = k dt (dg_implicit.py:125)
* dg_implicit.py:122     Q* = BDM projection of Q
* dg_implicit.py:126-130 the singular, consistent system (phi = const) is made regular by pinning one pressure dof in place of
                         the redundant last continuity row, solved by sparse LU, and phi is shifted to zero mean
* dg_implicit.py:117-120,131-132  tracer: q^{n+1} = q^n + dt M^-1 T(q^n, P(Q^n)) with the velocity at the start of the step
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def dg_matrix(d, Qstar, dt, flux="upwind"):
    """K = [[M - dt F, -dt Wdiv^T], [dt Wdiv, 0]]  (dg_implicit.py:48-71)."""
    F = d.assemble_f_impl(Qstar, flux)
    return sp.bmat([[d.MQ - dt * F, -dt * d.Wdiv.T], [dt * d.Wdiv, None]], format="csc")


def dg_step(d, Q, f, dt, flux="upwind"):
    """One step from the nodal velocity Q with the nodal forcing f (at the start of the step); returns (Q, p)."""
    Qstar = d.project_bdm(Q)  # dg_implicit.py:122
    K = dg_matrix(d, Qstar, dt, flux)
    rhs = np.concatenate([d.MQ @ Q.ravel() + dt * (d.MQ @ f.ravel()), np.zeros(d.NP)])  # dg_implicit.py:73
    # phi = const is the null space and the continuity rows sum to zero: the last continuity row is redundant (its right-hand
    # side is zero too), so it is replaced by phi_last = 0 -- a sparse nonsingular system with the same solution up to the
    # constant the mean shift removes
    K = K.tolil()
    K[d.NQ + d.NP - 1, :] = 0.0
    K[d.NQ + d.NP - 1, d.NQ + d.NP - 1] = 1.0
    x = spla.splu(K.tocsc()).solve(rhs)
    u, phi = x[: d.NQ], x[d.NQ : d.NQ + d.NP]
    return u.reshape(-1, 2), phi - float(d.int_p @ phi) / d.mesh.volume  # dg_implicit.py:128-130


def dg_solve(d, Q0, p0, f_rhs, dt, nsteps, flux="upwind", q0=None, tracer=None):
    """nsteps steps of IncompressibleEulerDGImplicit.solve (dg_implicit.py:98-136); f_rhs(t) -> nodal forcing or None.
    With q0 (nodal DG_k) and tracer (oracle.tracer_oracle.TracerOracle(d)) returns (Q, p, q), else (Q, p)."""
    Q = np.array(Q0, dtype=float).reshape(-1, 2)
    p = p0 - float(d.int_p @ p0) / d.mesh.volume  # dg_implicit.py:102
    q = None if q0 is None else np.array(q0, dtype=float)
    for k in range(nsteps):
        f = np.zeros_like(Q) if f_rhs is None else np.asarray(f_rhs(k * dt), dtype=float).reshape(-1, 2)
        dq = dt * tracer.tracer_tendency(q, Q) if q is not None else None  # velocity at the START of the step
        Q, p = dg_step(d, Q, f, dt, flux)
        if q is not None:
            q = q + dq
    return (Q, p) if q is None else (Q, p, q)


def avg_trace(d, p):
    """avg(p) on interior edges, p on boundary edges, as nodal DGT_k values: the trace reconstruction of the oracle with
    Q = 0 (its lambda-rows are the incidence sum tau <lambda - p, mu>, i.e. the mean of the sides' traces)."""
    return d.reconstruct_trace(np.zeros((d.NQ // 2, 2)), p)
