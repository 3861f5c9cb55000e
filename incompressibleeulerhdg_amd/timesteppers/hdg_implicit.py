"""First-order implicit HDG timestepper (reference: src/timesteppers/hdg_implicit.py:10-197)."""

from ..auxilliary.utils import Averager
from .common import IncompressibleEuler

__all__ = ["IncompressibleEulerHDGImplicit"]


class IncompressibleEulerHDGImplicit(IncompressibleEuler):
    """First order in time; Chorin's projection method (hdg_implicit.py:101-150).

    ``n_richardson`` is accepted and ignored so that the reference driver's call shape
    (driver.py:220-228) works.  ``use_projection_method=False`` selects the
    monolithic (u, phi, lambda) solve of hdg_implicit.py:151-186.
    """

    def __init__(self, mesh, degree, dt, flux="upwind", use_projection_method=True, callbacks=None,
                 n_richardson=None, **engine_options):
        # the fully implicit step carries the whole dt as implicit weight (four times SSP2(3,3,2)'s a_ii dt): the spectrum
        # of the tentative-velocity operator is too wide for the Chebyshev iteration to pay at k >= 2 (k = 1 / 2 / 3 at
        # 256^2 / 512^2 / 512^2, ms per step with tent_solver 0 / 1: 5.17 / 4.31, 10.80 / 11.17, 15.64 / 16.08)
        engine_options.setdefault("tent_solver", 1 if degree <= 1 else 0)
        super().__init__(mesh, degree, dt, label="HDG Implicit", **engine_options)
        self.flux = flux
        assert self.flux in ["upwind", "centered"]
        self.use_projection_method = use_projection_method
        self.callbacks = [] if callbacks is None else callbacks
        self.alpha = 1  # hdg_implicit.py:41
        self.tau = 1  # hdg_implicit.py:43
        self.niter_tentative = Averager()
        self.niter_pressure = Averager()
        self._create_engine(flux=flux, use_projection_method=use_projection_method, n_richardson=1, tau=self.tau,
                            alpha_penalty=self.alpha, nstages=1, a_expl=[[0]], a_impl=[[1]], b_expl=[1],
                            b_impl=[1], c_expl=[0])

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
        self._set_forcing(0, f_rhs, self._time(k))  # forcing at the START of the step (hdg_implicit.py:100)
        it_t, it_p = self._engine.implicit_step()
        self.niter_tentative.update(it_t)
        self.niter_pressure.update(it_p)
        return (k + 1) * self._dt
