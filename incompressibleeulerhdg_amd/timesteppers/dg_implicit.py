"""First-order implicit DG timestepper (reference: src/timesteppers/dg_implicit.py:10-136)."""

from ..auxilliary.utils import Averager
from .common import IncompressibleEuler

__all__ = ["IncompressibleEulerDGImplicit"]


class IncompressibleEulerDGImplicit(IncompressibleEuler):
    """Implicit DG method of Guzman et al. (2016), Section 2.2 (dg_implicit.py:10-14).

    Spaces [DG_{k+1}]^2 x DG_k, no trace; one coupled (u, phi) solve per step (dg_implicit.py:48-82), done on the GPU by
    flexible GMRES (hdg_dg_implicit_step).  The reference hands the system to MUMPS; ``dg_rtol`` / ``dg_restart`` /
    ``dg_maxit`` (engine options) set the outer solve.
    """

    def __init__(self, mesh, degree, dt, flux="upwind", callbacks=None, **engine_options):
        super().__init__(mesh, degree, dt, label="DG Implicit", **engine_options)
        assert flux in ["upwind", "centered"]
        self.flux = flux
        self.alpha = 1  # dg_implicit.py:29
        self.tau = 1  # stabilisation of the mixed Poisson preconditioner of the solve (tau' = tau / dt)
        self.callbacks = [] if callbacks is None else callbacks
        self.niter = Averager()
        # one implicit stage, the stage-0 forcing slot: the handle of IncompressibleEulerHDGImplicit; _V_Q / _V_p / _V_q
        # are DG_{k+1}^2 / DG_k / DG_k as in dg_implicit.py:33-35
        self._create_engine(flux=flux, use_projection_method=False, n_richardson=1, tau=self.tau, alpha_penalty=self.alpha,
                            nstages=1, a_expl=[[0]], a_impl=[[1]], b_expl=[1], b_impl=[1], c_expl=[0])

    def solve(self, Q_initial, p_initial, q_initial, f_rhs, T_final, warmup=False, diagnostics=False, probes=None,
              particles=None, particle_every=1, cfl=None, dt_min=None, dt_max=None, adapt_every=1, max_steps=None,
              checkpoint=None, checkpoint_every=0, restart=None):
        """Propagate the solution to T_final; returns (Q, p).  ``diagnostics``, ``probes``, ``particles``, ``checkpoint``,
        ``checkpoint_every``, ``restart``, ``cfl``, ``dt_min``, ``dt_max``, ``adapt_every``, ``max_steps``: see
        IncompressibleEulerHDGIMEX.solve."""
        return self._solve(Q_initial, p_initial, q_initial, f_rhs, T_final, warmup, diagnostics=diagnostics, probes=probes,
                           particles=particles, particle_every=particle_every, checkpoint=checkpoint,
                           checkpoint_every=checkpoint_every, restart=restart, cfl=cfl, dt_min=dt_min, dt_max=dt_max,
                           adapt_every=adapt_every, max_steps=max_steps)

    def _advance(self, k, f_rhs, tracer):
        self._set_forcing(0, f_rhs, self._time(k))  # dg_implicit.py:125; dg_implicit.py:100-102, p_0 -= mean, is done by hdg_set_state
        self.niter.update(self._engine.dg_implicit_step())
        return (k + 1) * self._dt
