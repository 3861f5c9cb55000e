"""Common functionality of the timesteppers (reference: src/timesteppers/common.py:15-144).

Same class surface as the reference; the bodies call the HIP engine through the ctypes C-ABI.
"""

import os
import warnings
from abc import ABC, abstractmethod

import numpy as np

from .._lib import DIAGNOSTICS, HDG_STATE_CURRENT, POINT_COLUMNS, Engine, HDGError, step_control, step_proposal
from ..auxilliary.logging import PerformanceLog
from ..mesh import Function, FunctionSpace

__all__ = ["IncompressibleEuler"]


def explicit_stability_limit(a_expl, b_expl):
    """The real-axis stability limit of an explicit tableau: the right end x of the interval [0, x] on which
    |R(-x)| <= 1, R(z) = 1 + z b^T (I - z A)^-1 1 (a polynomial, A being strictly lower triangular).  Forward Euler: 2."""
    b = np.asarray(b_expl, dtype=float).reshape(-1)
    A = np.asarray(a_expl, dtype=float).reshape(len(b), len(b))
    coef, v = [1.0], np.ones(len(b))
    for m in range(len(b)):  # R(-x) = sum_m (-x)^m b^T A^(m-1) 1
        coef.append((-1.0) ** (m + 1) * float(b @ v))
        v = A @ v
    p = np.array(coef)  # ascending powers of x
    while len(p) > 1 and p[-1] == 0.0:
        p = p[:-1]
    if len(p) == 1:
        return float("inf")
    roots = []
    for target in (1.0, -1.0):  # where R(-x) meets 1 (the root x = 0 divided out) and -1
        r = p.copy()
        r[0] -= target
        if target > 0:
            r = r[1:]
        roots += [z.real for z in np.atleast_1d(np.roots(r[::-1])) if abs(z.imag) <= 1e-12 * max(1.0, abs(z)) and z.real > 0]
    for x in sorted(roots):  # the first one behind which |R| has left [0, 1] (a root where it only touches 1 is passed over)
        if abs(np.polyval(p[::-1], x * (1 + 1e-6))) > 1.0:
            return float(x)
    return float("inf")


def warn_if_diffusion_unstable(number, limit, what="tracer diffusion"):
    """The explicit diffusion term is stable while kappa_max dt rho(M^-1 D) <= limit; `number` is built from an upper bound of
    the spectral radius, so exceeding the limit is a warning, not an error."""
    if number > limit:
        warnings.warn(f"{what}: the diffusion number kappa_max dt Lambda = {number:.4g} exceeds the stability limit {limit:.4g} of "
                      "the explicit tableau (Lambda is an upper bound of the spectral radius): the run may blow up; reduce dt "
                      "or the diffusivity", RuntimeWarning, stacklevel=3)


def _stability_polynomial(a_expl, b_expl):
    """Ascending coefficients of R(z) = 1 + z b^T (I - z A)^-1 1 of an explicit tableau"""
    b = np.asarray(b_expl, dtype=float).reshape(-1)
    A = np.asarray(a_expl, dtype=float).reshape(len(b), len(b))
    coef, v = [1.0], np.ones(len(b))
    for _ in range(len(b)):
        coef.append(float(b @ v))
        v = A @ v
    return np.array(coef)


def _imaginary_excess(a_expl, b_expl):
    """Ascending coefficients in Y = y^2 of (|R(iy)|^2 - 1) / Y, a real polynomial; coefficients at rounding level (the order
    conditions cancel the low ones exactly only in exact arithmetic) are set to zero"""
    c = _stability_polynomial(a_expl, b_expl)
    re = np.array([(-1.0) ** (m // 2) * c[m] for m in range(0, len(c), 2)])  # Re R(iy) = sum c_2j (-1)^j Y^j
    im = np.array([(-1.0) ** (m // 2) * c[m] for m in range(1, len(c), 2)])  # Im R(iy) = y sum c_2j+1 (-1)^j Y^j
    g = np.polynomial.polynomial.polymul(re, re)
    g2 = np.concatenate([[0.0], np.polynomial.polynomial.polymul(im, im)]) if len(im) else np.zeros(1)
    n = max(len(g), len(g2))
    g = np.pad(g, (0, n - len(g))) + np.pad(g2, (0, n - len(g2)))
    g[0] -= 1.0
    g[np.abs(g) <= 1e-13] = 0.0
    return g[1:]  # g[0] = R(0)^2 - 1 = 0


def explicit_imaginary_limit(a_expl, b_expl):
    """The imaginary-axis stability limit of an explicit tableau: the largest y up to which |R(iy')| <= 1 for all
    0 <= y' <= y.  0 when |R| exceeds 1 right away (forward Euler, every second-order tableau with |R|^2 = 1 + c y^4 + ...)."""
    e = _imaginary_excess(a_expl, b_expl)
    nz = np.nonzero(e)[0]
    if len(nz) == 0:
        return float("inf")
    if e[nz[0]] > 0:  # the leading term of |R|^2 - 1 is positive
        return 0.0
    roots = [z.real for z in np.atleast_1d(np.roots(e[::-1])) if abs(z.imag) <= 1e-12 * max(1.0, abs(z)) and z.real > 0]
    for Y in sorted(roots):  # the first one behind which |R|^2 - 1 is positive
        if np.polyval(e[::-1], Y * (1 + 1e-6)) > 0:
            return float(np.sqrt(Y))
    return float("inf")


def explicit_imaginary_growth(a_expl, b_expl, y):
    """max over 0 <= y' <= y of |R(iy')| - 1, the growth per step of an undamped oscillation with frequency * dt <= y; 0 up to
    explicit_imaginary_limit."""
    e = _imaginary_excess(a_expl, b_expl)
    Y = float(y) ** 2
    if Y == 0.0 or not np.any(e):
        return 0.0
    g = np.concatenate([[0.0], e])[::-1]  # |R|^2 - 1 as a polynomial in Y = y'^2, highest power first
    inner = [z.real for z in np.atleast_1d(np.roots(np.polyder(g))) if abs(z.imag) <= 1e-12 * max(1.0, abs(z)) and 0 < z.real < Y]
    worst = max(np.polyval(g, Yc) for Yc in [Y] + inner)  # the end of the interval or a local maximum inside it
    return float(np.sqrt(1.0 + max(worst, 0.0)) - 1.0)


def warn_if_rotation_unstable(number, growth, limit, growth_limit):
    """The explicit Coriolis term: `number` = F dt, `growth` = the growth per step at that number, `limit` the imaginary-axis
    limit of the tableau.  Warns when the growth per inertial period exceeds growth_limit, or when a non-zero limit is exceeded."""
    per_period = growth * 2.0 * np.pi / number if number > 0 else 0.0
    if per_period > growth_limit or (limit > 0 and number > limit):
        warnings.warn(f"rotation: at the rotation number F dt = {number:.4g} the explicit tableau (imaginary-axis limit {limit:.4g}) "
                      f"amplifies an inertial oscillation by {per_period:.3g} per inertial period (more than {growth_limit:.3g}); F is an "
                      "upper bound of the spectral radius (the largest |f0 + beta y| on the mesh), and in 2-D the part of the "
                      "force that is a gradient is taken by the pressure, so the flow may grow more slowly; reduce dt",
                      RuntimeWarning, stacklevel=3)


class IncompressibleEuler(ABC):
    """Abstract base class for timesteppers of the incompressible Euler equations.

    The reference constructor builds the 1/h_F facet field, V_BDM and the inverse DOF multiplicity
    (common.py:36-70); here those live inside the engine's operator tables (edge lengths are closed
    form on the structured mesh; the BDM averaging is built into the projection kernel).
    """

    rotation_growth_limit = 0.01  # growth per inertial period above which coriolis= warns: a policy default, not a measurement

    def __init__(self, mesh, degree, dt, label=None, **engine_options):
        self._mesh = mesh
        self.degree = degree
        self._dt = dt
        self._label = label
        # tracer_diffusivity=: kappa of every tracer (a scalar or n_tracers values); None: no call at all
        self._tracer_diffusivity = engine_options.pop("tracer_diffusivity", None)
        # tracer_diffusion=: 'explicit' (the default: no call at all) or 'implicit', the backward-Euler solve at the end of every
        # step
        self._tracer_diffusion = engine_options.pop("tracer_diffusion", "explicit")
        if self._tracer_diffusion not in ("explicit", "implicit"):
            raise ValueError(f"tracer_diffusion must be 'explicit' or 'implicit' (got {self._tracer_diffusion!r})")
        if self._tracer_diffusion == "implicit" and self._tracer_diffusivity is None:
            raise ValueError('tracer_diffusion="implicit" needs tracer_diffusivity=')
        # tracer_walls=: fixed-value walls of the tracers, a dict {side: value} or n_tracers of them;
        # None: no call at all
        self._tracer_walls = engine_options.pop("tracer_walls", None)
        # buoyancy=, gravity=: beta of every tracer (a scalar or n_tracers values) and g of the Boussinesq term + sum_t beta_t q_t g
        # (DESIGN.md section 20); None: no call at all.  Set once the tracers are (Engine.set_buoyancy needs them).
        self._buoyancy = engine_options.pop("buoyancy", None)
        self._gravity = engine_options.pop("gravity", None)
        if self._gravity is not None and self._buoyancy is None:
            raise ValueError("gravity= needs buoyancy=")
        # viscosity=, wall=: nu and the wall mode ('free_slip', 'no_slip') of the explicit viscous term + nu Laplace u (DESIGN.md
        # section 21); None: no call at all
        self._viscosity = engine_options.pop("viscosity", None)
        self._wall = engine_options.pop("wall", None)
        if self._wall is not None and self._viscosity is None:
            raise ValueError("wall= needs viscosity=")
        # wall_velocity=: constant tangential speeds of the no-slip walls, a dict {side: speed} or four values (DESIGN.md section
        # 24); None: no call at all
        self._wall_velocity = engine_options.pop("wall_velocity", None)
        if self._wall_velocity is not None and (self._viscosity is None or self._wall != "no_slip"):
            raise ValueError('wall_velocity= needs viscosity= and wall="no_slip"')
        # coriolis=: f0 or (f0, beta) of the explicit Coriolis term - (f0 + beta y) k x u; None: no call at all
        self._coriolis = engine_options.pop("coriolis", None)
        # drag=, drag_target=, drag_region=: sigma, u_s and the region tags of the explicit damping - sigma (u - u_s) (DESIGN.md
        # section 26), each as Engine.set_drag takes it; drag=None: no call at all
        self._drag = engine_options.pop("drag", None)
        self._drag_target = engine_options.pop("drag_target", None)
        self._drag_region = engine_options.pop("drag_region", None)
        if self._drag is None and (self._drag_target is not None or self._drag_region is not None):
            raise ValueError("drag_target= and drag_region= need drag=")
        self._engine_options = engine_options
        self._engine = None
        # common.py:72-73
        self.domain_volume = float(mesh.volume) if getattr(mesh, "general", False) else float(getattr(mesh, "L", 1.0)) ** 2
        self.diagnostics = None  # solve(..., diagnostics=True): dict of the recorded series
        self.probes = None  # solve(..., probes=xy): dict of the recorded point values
        self.particles = None  # solve(..., particles=xy): dict of the recorded particle positions
        self.step_sizes = None  # solve(..., cfl=C): one row (t, dt, A dt) per step taken
        self.step_decisions = None  # ... and one row (t, A, dt held, dt proposed) per decision of the controller
        self.tracer_diffusion_iterations = None  # tracer_diffusion="implicit": the iteration counts of every step's solve
        self._t_adaptive = None  # the start time of the next step while an adaptive run is under way

    # -- engine and function spaces ------------------------------------------------------------
    def _create_engine(self, **kw):
        if getattr(self._mesh, "general", False):
            # general affine triangulation: per-element geometry (hdg_create_general)
            opts = dict(vertices=self._mesh.vertices, cells=self._mesh.cells, degree=self.degree, dt=self._dt)
        else:
            opts = dict(nx=self._mesh.nx, ny=self._mesh.ny, degree=self.degree, dt=self._dt,
                        periodic=getattr(self._mesh, "periodic", False), length=getattr(self._mesh, "L", 1.0))
        opts.update(kw)
        opts.update(self._engine_options)
        self._engine = Engine(**opts)
        xq, xp = self._engine.node_coordinates()
        k = self.degree
        self._V_Q = FunctionSpace(self._mesh, "DG", k + 1, xq, value_size=2)
        self._V_p = FunctionSpace(self._mesh, "DG", k, xp)
        self._V_q = self._V_p  # tracer space DG_k (hdg_imex.py:68)
        for V in (self._V_Q, self._V_p):
            V._engine = self._engine  # device operations on a Function (vorticity callback)
        self._V_trace = ("DGT", k, self._engine.n_edges * self._engine.n_l)
        self._V = (self._V_Q, self._V_p, self._V_trace)
        if self._tracer_walls is not None:  # before the diffusion number is read: Lambda then counts the wall blocks
            self._engine.set_tracer_walls(self._tracer_walls)
            if self._tracer_diffusivity is None or not np.any(np.asarray(self._tracer_diffusivity, dtype=float) != 0.0):
                warnings.warn("tracer_walls= without a non-zero tracer_diffusivity=: a fixed wall value acts through the "
                              "diffusion term only, so the walls do nothing", RuntimeWarning, stacklevel=3)
        if self._tracer_diffusivity is not None:
            self._engine.set_tracer_diffusivity(self._tracer_diffusivity)
            self.diffusion_limit = explicit_stability_limit(opts["a_expl"], opts["b_expl"])
            if self._tracer_diffusion == "implicit":  # no limit to warn about: the term is solved for
                self._engine.set_tracer_diffusion_mode("implicit")
            else:
                warn_if_diffusion_unstable(self._engine.tracer_diffusion_number()[1], self.diffusion_limit)
        if self._viscosity is not None:  # independent of the tracer check above
            self._engine.set_viscosity(self._viscosity, "free_slip" if self._wall is None else self._wall)
            self.viscosity_limit = explicit_stability_limit(opts["a_expl"], opts["b_expl"])
            warn_if_diffusion_unstable(self._engine.viscosity_number()[1], self.viscosity_limit, what="viscosity")
        if self._wall_velocity is not None:  # behind the viscosity: the wall mode has to be no slip
            self._engine.set_wall_velocity(self._wall_velocity)
        if self._coriolis is not None:  # independent of the tracers and of the viscosity
            f0, beta = (self._coriolis, 0.0) if np.ndim(self._coriolis) == 0 else self._coriolis
            self._engine.set_coriolis(f0, beta)
            number = self._engine.coriolis_number()[1]
            self.rotation_limit = explicit_imaginary_limit(opts["a_expl"], opts["b_expl"])
            self.rotation_growth = explicit_imaginary_growth(opts["a_expl"], opts["b_expl"], number)
            warn_if_rotation_unstable(number, self.rotation_growth, self.rotation_limit, self.rotation_growth_limit)
        if self._drag is not None:  # independent of the other terms
            self.set_drag(self._drag, self._drag_target, self._drag_region)
        return self._engine

    def set_drag(self, sigma, target=None, region=None):
        """Engine.set_drag and the stability report: the spectrum of - M^-1 D is real and non-positive like the viscous one and
        the two add, so (nu Lambda_u + S) dt is held against the real-axis limit of the explicit tableau."""
        eng = self._engine
        eng.set_drag(sigma, target, region)
        s = eng.nstages
        self.drag_limit = explicit_stability_limit(list(eng.cfg.a_expl)[:s * s], list(eng.cfg.b_expl)[:s])
        viscous = eng.viscosity_number()[1] if eng.viscosity()[0] > 0 else 0.0
        warn_if_diffusion_unstable(viscous + eng.drag_number()[1], self.drag_limit, what="drag")

    def _as_nodal_velocity(self, Q):
        """Accept a callable (x, y) -> (ux, uy) [the reference passes UFL expressions], a Function or
        an array."""
        if callable(Q):
            return self._V_Q.interpolate(Q)
        if isinstance(Q, Function):
            return np.asarray(Q.dat.data, dtype=float)
        return np.asarray(Q, dtype=float)

    def _as_nodal_pressure(self, p):
        if callable(p):
            return self._V_p.interpolate(p)
        if isinstance(p, Function):
            return np.asarray(p.dat.data, dtype=float)
        return np.asarray(p, dtype=float)

    # -- reference API -------------------------------------------------------------------------
    def get_timesteps(self, t_final, warmup):
        """Number of timesteps (common.py:75-84)."""
        nt = 1 if warmup else int(np.round(t_final / self._dt))
        assert warmup or (abs(nt * self._dt - t_final) < 1.0e-12)
        return nt

    @property
    def label(self):
        return self._label

    def project_bdm(self, Q):
        """Project a velocity from the DG space to the BDM space (common.py:91-108).

        Returns Q* as a Function on the broken space [P_{k+1}]^2 (same function, continuous normals,
        zero normal component on the boundary)."""
        out = self._engine.project_bdm_nodal(self._as_nodal_velocity(Q))
        return Function(self._V_Q, out, "Q_star")

    def _stack_tracers(self, q_initial, n_tracers):
        """The nodal tracer block of Engine.set_tracer: one field of what _as_nodal_pressure accepts, or -- for an engine
        with n_tracers > 1 -- a list / tuple of exactly n_tracers of them, stacked tracer-major."""
        if n_tracers <= 1:
            return self._as_nodal_pressure(q_initial)
        if not isinstance(q_initial, (list, tuple)) or len(q_initial) != n_tracers:
            got = f"{len(q_initial)} items" if isinstance(q_initial, (list, tuple)) else type(q_initial).__name__
            raise ValueError(f"q_initial must be a list or tuple of {n_tracers} tracer fields (n_tracers = {n_tracers}), got {got}")
        return np.stack([self._as_nodal_pressure(q) for q in q_initial])

    @staticmethod
    def _tracer_names(n_tracers):
        return ["tracer"] if n_tracers <= 1 else [f"tracer_{m}" for m in range(n_tracers)]

    def _init_tracer(self, q_initial):
        """q_initial (expression / array / None, driver.py:340-344; a list of them for several tracers) -> the engine's
        tracer state; returns whether a tracer is advected."""
        if q_initial is None or q_initial is False:
            if self._buoyancy is not None:
                raise ValueError("buoyancy= needs a tracer (q_initial)")
            self._engine.set_tracer(None)
            self.q_tracer, self.q_tracers = None, []
            return False
        self._engine.set_tracer(self._stack_tracers(q_initial, self._engine.n_tracers))
        self._set_buoyancy()
        self._tracer_function()
        return True

    def _set_buoyancy(self):
        """buoyancy= / gravity= of the constructor, once the engine holds its tracers"""
        if self._buoyancy is not None:
            self._engine.set_buoyancy(self._buoyancy, (0.0, -1.0) if self._gravity is None else self._gravity)

    def _tracer_function(self):
        """Fetches the tracers: self.q_tracers (all of them), self.q_tracer (tracer 0); returns what the callbacks are
        given as q_tracer=: the Function of one tracer, the list of several."""
        n = self._engine.n_tracers
        block = self._engine.get_tracer().reshape(n, -1)
        self.q_tracers = [Function(self._V_q, block[m].copy(), name) for m, name in enumerate(self._tracer_names(n))]
        self.q_tracer = self.q_tracers[0]
        return self.q_tracer if n == 1 else self.q_tracers

    # -- flow diagnostics (include/hdg_mi355x.h: hdg_compute_diagnostics) ----------------------
    def compute_diagnostics(self, Q, p, q=None):
        """Energy, enstrophy, divergence, normal jumps, pressure and tracer integrals, maximum speed and CFL number of the
        given fields (what _as_nodal_* accepts; q None: no tracer, the tracer entries are NaN), computed on the device.
        Returns a dict keyed by the names of ``_lib.DIAGNOSTICS``."""
        qn = None if q is None else self._as_nodal_pressure(q)
        vals = self._engine.compute_diagnostics(self._as_nodal_velocity(Q), self._as_nodal_pressure(p), qn)
        return {name: float(v) for name, v in zip(DIAGNOSTICS, vals)}

    # -- stream function (include/hdg_streamfunction.h) ------------------------------------------
    def streamfunction(self, Q=None):
        """The stream function psi in CG_{k+1} of the velocity Q (what _as_nodal_velocity accepts; None: the current state),
        solved on the device and returned on the node set of the velocity space, like the vorticity of AnimationCallback.
        Its attribute ``info`` holds the dict of Engine.streamfunction (iterations, defect, mean flow, extrema)."""
        eng = self._engine
        psi, info = eng.streamfunction(None if Q is None else self._as_nodal_velocity(Q))
        V_psi = FunctionSpace(self._mesh, "CG", self._V_Q.degree, self._V_Q.coordinates)
        out = Function(V_psi, eng.cg_to_broken(psi), "streamfunction")
        out.info = info
        return out

    # -- point values (include/hdg_mi355x.h: hdg_evaluate_points / hdg_set_probes) ------------------
    def evaluate_points(self, xy, Q=None, p=None, q=None):
        """Values of the given fields (what _as_nodal_* accepts, None: NaN) at the points xy (n, 2), computed on the device:
        (values (n, 5) in ``_lib.POINT_COLUMNS`` order, located (n,) bool)."""
        return self._engine.evaluate_points(xy, None if Q is None else self._as_nodal_velocity(Q),
                                            None if p is None else self._as_nodal_pressure(p),
                                            None if q is None else self._as_nodal_pressure(q))

    # -- transfer between runs of different mesh size and degree (include/hdg_transfer.h) ----------
    def state_from(self, other):
        """The current state of the timestepper `other` (another nx and degree on a nested mesh, any stepper family), L2
        projected onto this timestepper's spaces on the device: (Q, p, q) as Functions, fit to be passed as Q_initial,
        p_initial, q_initial of solve.  q is None when `other` advects no tracer (or another number of them), else one
        Function or the list of several, as q_tracer(s) is."""
        eng, src = self._engine, other._engine
        tracers = bool(getattr(src, "_tracer_on", False)) and src.n_tracers == eng.n_tracers
        eng.transfer_from(src, tracers=tracers)
        Q, p = self._functions(*self._current(), self._result_names)
        return Q, p, (self._tracer_function() if tracers else None)

    def difference(self, other):
        """{"Q", "p", "q"}: L2 norms of the differences of the current states of this timestepper and `other`, exact on the
        common refinement of the two meshes (Engine.difference_norms)."""
        return self._engine.difference_norms(other._engine)

    # -- forcing -------------------------------------------------------------------------------
    def _set_forcing(self, slot, f_rhs, t):
        if f_rhs is None or (isinstance(f_rhs, (int, float)) and f_rhs == 0):
            self._engine.set_forcing_scale(slot, 0.0)
        elif hasattr(f_rhs, "profile") and hasattr(f_rhs, "scale"):
            if self._forcing_profile is not f_rhs.profile:
                self._engine.set_forcing_profile(f_rhs.profile)
                self._forcing_profile = f_rhs.profile
            self._engine.set_forcing_scale(slot, f_rhs.scale(t))
        else:
            self._engine.set_forcing_nodal(slot, self._as_nodal_velocity(f_rhs(t)))

    # -- time loop (hdg_imex.py:505-660, hdg_implicit.py:52-197, dg_implicit.py:84-136) -------------------------------
    _callback_names = (None, None)  # names of the velocity and pressure Functions handed to callbacks
    _result_names = ("velocity", "pressure")  # ... and of those solve() returns

    def _begin_solve(self, restarted=False):
        """After the state is set, before the recorders start.  ``restarted``: the state came from a checkpoint and must
        stay what it is (no reconstruction, no reset of the engine's statistics)."""

    def _advance(self, k, f_rhs, tracer):
        """Step k (forcing included); returns the time reached, which the callbacks are given."""
        raise NotImplementedError

    def _end_solve(self):
        """After the recorders have finished, before the final fields are fetched."""

    def _call_back(self, t, tracer):
        """The callbacks after a step that reached the time t"""
        if self.callbacks:
            Q, p = self._current()
            qt = self._tracer_function() if tracer else None
            for callback in self.callbacks:
                callback(*self._functions(Q, p, self._callback_names), t, q_tracer=qt)

    def _note_tracer_solve(self, tracer):
        """tracer_diffusion="implicit": one row of iteration counts (n_tracers,) per step, in self.tracer_diffusion_iterations"""
        if tracer and self.tracer_diffusion_iterations is not None:
            self.tracer_diffusion_iterations.append(self._engine.tracer_diffusion_solve()[0])

    def _time(self, k):
        """The time at which step k starts: k dt at a fixed step size, the running sum of the step sizes in an adaptive run"""
        return k * self._dt if self._t_adaptive is None else self._t_adaptive

    # -- adaptive time step (include/hdg_adaptive_dt.h) ----------------------------------------
    def _step_controller(self, T_final, warmup, checkpoint, restart, cfl, dt_min, dt_max, adapt_every, max_steps):
        """solve(..., cfl=, dt_min=, dt_max=, adapt_every=, max_steps=) checked, before the engine is touched: None without
        cfl= (and for a warm-up run, whose one step is the constructor's), else (every, max_steps, dt_min, dt_max)."""
        if cfl is None:
            for name, v in (("dt_min", dt_min), ("dt_max", dt_max), ("max_steps", max_steps)):
                if v is not None:
                    raise ValueError(f"{name}= needs cfl=")
            if adapt_every != 1:
                raise ValueError("adapt_every= needs cfl=")
            return None
        if not (np.isfinite(cfl) and cfl > 0):
            raise ValueError(f"cfl must be a finite number > 0 (got {cfl})")
        if int(adapt_every) != adapt_every or adapt_every < 1:
            raise ValueError(f"adapt_every must be an integer >= 1 (got {adapt_every})")
        if checkpoint is not None or restart is not None:
            raise ValueError("cfl= does not go with checkpoint= or restart=: a checkpoint carries the step size of the "
                             "constructor in its fingerprint and does not hold the time series of an adaptive run")
        dt_max = self._dt if dt_max is None else dt_max
        dt_min = 0.0 if dt_min is None else dt_min
        if not (np.isfinite(dt_min) and dt_min >= 0) or not (dt_max > 0) or dt_min > dt_max:
            raise ValueError(f"dt_min and dt_max must satisfy 0 <= dt_min <= dt_max, dt_max > 0 (got {dt_min}, {dt_max})")
        if not (np.isfinite(T_final) and T_final > 0):
            raise ValueError(f"cfl= needs a finite T_final > 0 (got {T_final})")
        if max_steps is None:
            max_steps = 10 * int(np.ceil(T_final / self._dt))
        if int(max_steps) != max_steps or max_steps < 1:
            raise ValueError(f"max_steps must be an integer >= 1 (got {max_steps})")
        if warmup:
            return None
        return int(adapt_every), int(max_steps), float(dt_min), float(dt_max)

    def _step_caps(self, rates):
        """The upper limits of dt from the explicit terms, in the order of hdg_step_control.caps: the real-axis limit of the
        tableau over kappa_max Lambda and over nu Lambda_u (plus S while the drag is on: rates[2] is the rate of the whole
        velocity-linear part), its imaginary-axis limit over F (only when that limit is positive); None: no limit."""
        cfg, s = self._engine.cfg, self._engine.nstages  # the tableau the engine steps with: a term may have been switched
        a_expl, b_expl = list(cfg.a_expl)[:s * s], list(cfg.b_expl)[:s]  # on through the engine, not through the constructor
        caps = [None, None, None]
        if rates[1] > 0 or rates[2] > 0:
            real = explicit_stability_limit(a_expl, b_expl)
            caps[0] = real / rates[1] if rates[1] > 0 else None
            caps[1] = real / rates[2] if rates[2] > 0 else None
        if rates[3] > 0:
            imaginary = explicit_imaginary_limit(a_expl, b_expl)
            caps[2] = imaginary / rates[3] if imaginary > 0 else None
        return [None if c is None or not np.isfinite(c) else c for c in caps]

    def _adaptive_loop(self, controller, cfl, f_rhs, tracer, T_final):
        """The time loop with cfl=: the controller decides before the first step and after every `every`-th one, the step
        size changes only when the proposal differs from the one held; returns the number of steps taken."""
        eng = self._engine
        every, max_steps, dt_min, dt_max = controller
        dt0 = self._dt
        rates = eng.step_rates()
        control = step_control(cfl, dt_min=dt_min, dt_max=dt_max, caps=self._step_caps(rates))
        sizes, decisions = [], []
        t, k, A = 0.0, 0, rates[0]
        try:
            while T_final - t > 1.0e-12 * T_final:
                if k == max_steps:
                    raise RuntimeError(f"max_steps = {max_steps} steps taken and the run is at t = {t!r}, short of T_final = {T_final!r}")
                if k % every == 0:
                    if k > 0:
                        A = eng.step_rates()[0]
                    held = eng.get_dt()
                    proposal = step_proposal(control, A, held, t, T_final)
                    decisions.append((t, A, held, proposal))
                    if proposal != held:
                        eng.set_dt(proposal)
                        self._dt = proposal
                self._t_adaptive = t
                with PerformanceLog("timestep"):
                    self._advance(k, f_rhs, tracer)
                self._note_tracer_solve(tracer)
                sizes.append((t, self._dt, A * self._dt))
                t, k = t + self._dt, k + 1
                self._call_back(t, tracer)
        except BaseException:
            self._end_adaptive(sizes, decisions, dt0, failed=True)
            raise
        self._end_adaptive(sizes, decisions, dt0)
        return k

    def _end_adaptive(self, sizes, decisions, dt0, failed=False):
        """The stepper and its engine hold the constructor's step size again.  failed: the loop raised, perhaps inside an open
        step, where the engine refuses a new dt: that refusal must not hide the error that is on its way."""
        self.step_sizes = np.array(sizes, dtype=float).reshape(-1, 3)
        self.step_decisions = np.array(decisions, dtype=float).reshape(-1, 4)
        self._t_adaptive = None
        self._dt = dt0
        try:
            self._engine.set_dt(dt0)
        except HDGError:
            if not failed:
                raise

    def _current(self):
        """The current nodal velocity and pressure"""
        return self._engine.get_field(HDG_STATE_CURRENT, lam=False)[:2]

    def _functions(self, Q, p, names):
        return Function(self._V_Q, Q, names[0]), Function(self._V_p, p, names[1])

    def _rank_path(self, path):
        """The checkpoint file of this rank: PATH on one rank, PATH.<rank> on strips."""
        return path if self._engine.nranks == 1 else f"{path}.{self._engine.rank}"

    def _write_checkpoint(self, path, step, t):
        """The engine's state after `step` steps, written under a temporary name and moved into place: a run that is killed
        never leaves half a file."""
        path = self._rank_path(path)
        blob = self._engine.save_checkpoint(step, t)
        tmp = f"{path}.tmp"
        with open(tmp, "wb") as f:
            f.write(blob)
        os.replace(tmp, path)

    def _restart(self, path, nt, warmup, requests):
        """Load the checkpoint; returns (steps done, time reached, whether a tracer is advected).  A request that disagrees
        with what the saved run had switched on is a ValueError, raised before the engine is touched."""
        eng = self._engine
        if warmup:
            raise ValueError("restart: a warm-up run takes one step from the initial condition; it cannot continue a checkpoint")
        with open(self._rank_path(path), "rb") as f:
            blob = f.read()
        saved = Engine.checkpoint_info(blob)
        for name, make in RECORDERS:
            if make.requested(requests[name]) != saved[name]:
                raise ValueError(f"restart: the checkpoint was written {'with' if saved[name] else 'without'} {name}, "
                                 f"this run asks for it {'on' if make.requested(requests[name]) else 'off'}")
        for name, n in (("probes", saved["n_probes"]), ("particles", saved["n_particles"])):
            if saved[name] and len(np.asarray(requests[name], dtype=float).reshape(-1, 2)) != n:
                raise ValueError(f"restart: the checkpoint records {n} {name}, this run asks for "
                                 f"{len(np.asarray(requests[name], dtype=float).reshape(-1, 2))}")
        if saved["step"] > nt:
            raise ValueError(f"restart: the checkpoint was written after step {saved['step']}, this run ends after step {nt}")
        if self._buoyancy is not None and saved["tracer"]:  # configuration, like the diffusivities: set before the load
            eng.set_tracer(np.zeros(eng.shape_q))
            self._set_buoyancy()
        k0, t0 = eng.load_checkpoint(blob)
        if saved["tracer"]:
            self._tracer_function()
        else:
            self.q_tracer, self.q_tracers = None, []
        return k0, t0, saved["tracer"]

    def _solve(self, Q_initial, p_initial, q_initial, f_rhs, T_final, warmup, checkpoint=None, checkpoint_every=0, restart=None,
               cfl=None, dt_min=None, dt_max=None, adapt_every=1, max_steps=None, **requests):
        """The time loop of every stepper; ``requests``: the per-step outputs asked for, by the names of RECORDERS (each
        class there says what counts as asked for) and ``particle_every``.  Each one asked for leaves its dict in the attribute of its name.

        ``checkpoint=PATH`` writes the engine's state (Engine.save_checkpoint) after every ``checkpoint_every``-th step
        (0: never in between) and after the last one; ``restart=PATH`` continues such a file: the state, the tracers and the
        recorders are the saved ones (the initial-condition arguments are ignored and may be None) and the loop runs from
        the saved step to the end, so the run is the uninterrupted one bit for bit.

        ``cfl=C`` holds the CFL number at C with a step size that changes during the run:
        ``self.step_sizes`` then has one row (t, dt, A dt) per step taken, and the recorders take their times from it."""
        eng = self._engine
        controller = self._step_controller(T_final, warmup, checkpoint, restart, cfl, dt_min, dt_max, adapt_every, max_steps)
        self.step_sizes = self.step_decisions = None
        self.tracer_diffusion_iterations = [] if self._tracer_diffusion == "implicit" else None
        nt = self.get_timesteps(T_final, warmup) if controller is None else controller[1]  # adaptive: the size of the row logs
        if checkpoint is not None and int(checkpoint_every) < 0:
            raise ValueError(f"checkpoint_every must be >= 0 (got {checkpoint_every})")
        self._forcing_profile = None
        k0, t0 = 0, 0
        if restart is None:
            tracer = self._init_tracer(q_initial)
            eng.set_state(self._as_nodal_velocity(Q_initial), self._as_nodal_pressure(p_initial))
        else:
            k0, t0, tracer = self._restart(restart, nt, warmup, requests)
        self._begin_solve(restarted=restart is not None)
        recorders = []
        for name, make in RECORDERS:
            setattr(self, name, None)
            if make.requested(requests[name]):
                recorders.append((name, make(requests[name], self._dt, requests["particle_every"])))
                if restart is None:  # a restored engine goes on recording into the logs the checkpoint holds
                    recorders[-1][1].start(eng, nt)
        for callback in self.callbacks:
            callback.reset()
            callback(*self._functions(*self._current(), self._callback_names), t0,
                     q_tracer=self.q_tracers if len(self.q_tracers) > 1 else self.q_tracer)
        if controller is not None:
            self._adaptive_loop(controller, cfl, f_rhs, tracer, T_final)
        for k in (range(k0, nt) if controller is None else ()):
            with PerformanceLog("timestep"):
                t = self._advance(k, f_rhs, tracer)
            self._note_tracer_solve(tracer)
            if checkpoint is not None and (k + 1 == nt or (checkpoint_every and (k + 1) % int(checkpoint_every) == 0)):
                self._write_checkpoint(checkpoint, k + 1, t)
            self._call_back(t, tracer)
        times = None if self.step_sizes is None else np.append(self.step_sizes[:, 0], self.step_sizes[-1:, :2].sum())
        for name, rec in recorders:
            setattr(self, name, rec.finish(eng, times))
        self._end_solve()
        Q, p = self._current()
        if tracer:
            self._tracer_function()  # the final tracer fields: self.q_tracer(s) (the reference returns (Q, p) only)
        return self._functions(Q, p, self._result_names)

    @abstractmethod
    def solve(self, Q_initial, p_initial, q_initial, f_rhs, T_final, warmup=False, diagnostics=False, probes=None,
              particles=None, particle_every=1, cfl=None, dt_min=None, dt_max=None, adapt_every=1, max_steps=None,
              checkpoint=None, checkpoint_every=0, restart=None):
        """Propagate the solution to T_final; returns the final velocity and pressure (common.py:131-144)."""


# -- per-step outputs: each is switched on for a run of nt steps (row 0: the state as it is, then one row per step) and, when
# the run is over, fetched once into a dict and switched off.  The rows live in the engine's row logs.
class _Diagnostics:
    requested = staticmethod(bool)  # solve(..., diagnostics=True)

    def __init__(self, on, dt, every):
        self.dt = dt

    def start(self, eng, nt):
        eng.set_diagnostics(nt + 1)

    def finish(self, eng, times=None):
        """t and the nine series; times: the time of every row of an adaptive run (None: k dt)"""
        try:
            rows = eng.diagnostics(reset=True)
        finally:
            eng.set_diagnostics(0)
        out = {"t": np.arange(rows.shape[0]) * self.dt if times is None else times[:rows.shape[0]].copy()}
        out.update((name, rows[:, i].copy()) for i, name in enumerate(DIAGNOSTICS))
        return out


class _Probes:
    @staticmethod
    def requested(xy):  # solve(..., probes=xy): an empty point set is one too
        return xy is not None

    def __init__(self, xy, dt, every):
        self.xy, self.dt = np.asarray(xy, dtype=float).reshape(-1, 2), dt

    def start(self, eng, nt):
        eng.set_probes(self.xy, nt + 1)

    def finish(self, eng, times=None):
        """t, xy, u (nt+1, n, 2), p, q, omega (nt+1, n)"""
        try:
            rows = eng.probes(reset=True)
        finally:
            eng.set_probes(None, 0)
        c = {name: i for i, name in enumerate(POINT_COLUMNS)}
        return {"t": np.arange(rows.shape[0]) * self.dt if times is None else times[:rows.shape[0]].copy(), "xy": self.xy.copy(),
                "u": rows[:, :, [c["ux"], c["uy"]]].copy(), "p": rows[:, :, c["p"]].copy(),
                "q": rows[:, :, c["q"]].copy(), "omega": rows[:, :, c["omega"]].copy()}


class _Particles:
    """Seeds (n, 2) advected through every step on the device; nt // every + 1 rows: the seeds and the positions after every
    `every`-th step."""
    requested = staticmethod(_Probes.requested)

    def __init__(self, xy, dt, every):
        self.xy, self.dt, self.every = np.asarray(xy, dtype=float).reshape(-1, 2), dt, int(every)
        if self.every < 1:
            raise ValueError(f"particle_every must be at least 1 (got {every})")

    def start(self, eng, nt):
        eng.set_particles(self.xy, nt // self.every + 1, self.every)

    def finish(self, eng, times=None):
        """t, xy (rows, n, 2), clamped, lost"""
        try:
            rows, counts = eng.particles(reset=True)
        finally:
            eng.set_particles(None, 0)
        return {"t": np.arange(rows.shape[0]) * self.every * self.dt if times is None else times[::self.every][:rows.shape[0]].copy(),
                "xy": rows,
                "clamped": counts["clamped"], "lost": counts["lost"]}


RECORDERS = (("diagnostics", _Diagnostics), ("probes", _Probes), ("particles", _Particles))
