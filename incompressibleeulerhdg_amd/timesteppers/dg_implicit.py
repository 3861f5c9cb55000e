"""First-order implicit DG timestepper (reference: src/timesteppers/dg_implicit.py:10-136)."""

from .. import _lib
from ..auxilliary.logging import PerformanceLog
from ..auxilliary.utils import Averager
from ..mesh import Function
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
              particles=None, particle_every=1):
        """Propagate the solution to T_final; returns (Q, p).  ``diagnostics``, ``probes``, ``particles``: see
        IncompressibleEulerHDGIMEX.solve."""
        eng = self._engine
        tracer = self._init_tracer(q_initial)  # dg_implicit.py:103-109
        nt = self.get_timesteps(T_final, warmup)
        # dg_implicit.py:100-102: p_0 -= mean (hdg_set_state)
        eng.set_state(self._as_nodal_velocity(Q_initial), self._as_nodal_pressure(p_initial))
        profile = None
        self._start_diagnostics(diagnostics, nt)
        self._start_probes(probes, nt)
        self._start_particles(particles, nt, particle_every)
        for callback in self.callbacks:
            callback.reset()
            Q, p, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
            callback(Function(self._V_Q, Q), Function(self._V_p, p), 0, q_tracer=self.q_tracer)
        for k in range(nt):
            with PerformanceLog("timestep"):
                t = k * self._dt  # dg_implicit.py:125
                if f_rhs is None or (isinstance(f_rhs, (int, float)) and f_rhs == 0):
                    eng.set_forcing_scale(0, 0.0)
                elif hasattr(f_rhs, "profile"):
                    if profile is not f_rhs.profile:
                        eng.set_forcing_profile(f_rhs.profile)
                        profile = f_rhs.profile
                    eng.set_forcing_scale(0, f_rhs.scale(t))
                else:
                    eng.set_forcing_nodal(0, self._as_nodal_velocity(f_rhs(t)))
                self.niter.update(eng.dg_implicit_step())
            if self.callbacks:
                Q, p, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
                qt = self._tracer_function() if tracer else None
                for callback in self.callbacks:
                    callback(Function(self._V_Q, Q), Function(self._V_p, p), (k + 1) * self._dt, q_tracer=qt)
        self._finish_diagnostics(diagnostics)
        self._finish_probes(probes)
        self._finish_particles(particles)
        Q, p, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
        if tracer:
            self._tracer_function()
        return Function(self._V_Q, Q, "velocity"), Function(self._V_p, p, "pressure")
