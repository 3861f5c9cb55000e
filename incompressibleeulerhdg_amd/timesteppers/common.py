"""Common functionality of the timesteppers (reference: src/timesteppers/common.py:15-144).

Same class surface as the reference; the bodies call the HIP engine through the ctypes C-ABI.
"""

from abc import ABC, abstractmethod

import numpy as np

from .._lib import DIAGNOSTICS, POINT_COLUMNS, Engine
from ..mesh import Function, FunctionSpace

__all__ = ["IncompressibleEuler"]


class IncompressibleEuler(ABC):
    """Abstract base class for timesteppers of the incompressible Euler equations.

    The reference constructor builds the 1/h_F facet field, V_BDM and the inverse DOF multiplicity
    (common.py:36-70); here those live inside the engine's operator tables (edge lengths are closed
    form on the structured mesh; the BDM averaging is built into the projection kernel).
    """

    def __init__(self, mesh, degree, dt, label=None, **engine_options):
        self._mesh = mesh
        self.degree = degree
        self._dt = dt
        self._label = label
        self._engine_options = engine_options
        self._engine = None
        # common.py:72-73
        self.domain_volume = float(mesh.volume) if getattr(mesh, "general", False) else float(getattr(mesh, "L", 1.0)) ** 2
        self.diagnostics = None  # solve(..., diagnostics=True): dict of the recorded series
        self.probes = None  # solve(..., probes=xy): dict of the recorded point values
        self.particles = None  # solve(..., particles=xy): dict of the recorded particle positions

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
        return self._engine

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

    def _init_tracer(self, q_initial):
        """q_initial (expression / array / None, driver.py:340-344) -> the engine's tracer state; returns whether a
        tracer is advected."""
        if q_initial is None or q_initial is False:
            self._engine.set_tracer(None)
            self.q_tracer = None
            return False
        self._engine.set_tracer(self._as_nodal_pressure(q_initial))
        self.q_tracer = Function(self._V_q, self._engine.get_tracer(), "tracer")
        return True

    def _tracer_function(self):
        self.q_tracer = Function(self._V_q, self._engine.get_tracer(), "tracer")
        return self.q_tracer

    # -- flow diagnostics (include/hdg_mi355x.h: hdg_compute_diagnostics) ----------------------
    def compute_diagnostics(self, Q, p, q=None):
        """Energy, enstrophy, divergence, normal jumps, pressure and tracer integrals, maximum speed and CFL number of the
        given fields (what _as_nodal_* accepts; q None: no tracer, the tracer entries are NaN), computed on the device.
        Returns a dict keyed by the names of ``_lib.DIAGNOSTICS``."""
        qn = None if q is None else self._as_nodal_pressure(q)
        vals = self._engine.compute_diagnostics(self._as_nodal_velocity(Q), self._as_nodal_pressure(p), qn)
        return {name: float(v) for name, v in zip(DIAGNOSTICS, vals)}

    def _start_diagnostics(self, on, nt):
        """Record nt + 1 rows on the device: the current state (row 0) and the state after every step."""
        self.diagnostics = None
        if on:
            self._engine.set_diagnostics(nt + 1)

    def _finish_diagnostics(self, on):
        """Fetch the recorded rows once (self.diagnostics: t and the nine series) and switch recording off."""
        if not on:
            return
        try:
            rows = self._engine.diagnostics(reset=True)
        finally:
            self._engine.set_diagnostics(0)
        self.diagnostics = {"t": np.arange(rows.shape[0]) * self._dt}
        for i, name in enumerate(DIAGNOSTICS):
            self.diagnostics[name] = rows[:, i].copy()

    # -- point values (include/hdg_mi355x.h: hdg_evaluate_points / hdg_set_probes) ------------------
    def evaluate_points(self, xy, Q=None, p=None, q=None):
        """Values of the given fields (what _as_nodal_* accepts, None: NaN) at the points xy (n, 2), computed on the device:
        (values (n, 5) in ``_lib.POINT_COLUMNS`` order, located (n,) bool)."""
        return self._engine.evaluate_points(xy, None if Q is None else self._as_nodal_velocity(Q),
                                            None if p is None else self._as_nodal_pressure(p),
                                            None if q is None else self._as_nodal_pressure(q))

    def _start_probes(self, probes, nt):
        """Record nt + 1 rows of point values on the device: the current state (row 0) and the state after every step."""
        self.probes = None
        if probes is not None:
            self._engine.set_probes(np.asarray(probes, dtype=float).reshape(-1, 2), nt + 1)

    def _finish_probes(self, probes):
        """Fetch the recorded rows once (self.probes: t, xy, u (nt+1, n, 2), p, q, omega (nt+1, n)) and switch recording
        off."""
        if probes is None:
            return
        try:
            rows = self._engine.probes(reset=True)
        finally:
            self._engine.set_probes(None, 0)
        c = {name: i for i, name in enumerate(POINT_COLUMNS)}
        self.probes = {"t": np.arange(rows.shape[0]) * self._dt, "xy": np.asarray(probes, dtype=float).reshape(-1, 2).copy(),
                       "u": rows[:, :, [c["ux"], c["uy"]]].copy(), "p": rows[:, :, c["p"]].copy(),
                       "q": rows[:, :, c["q"]].copy(), "omega": rows[:, :, c["omega"]].copy()}

    # -- Lagrangian particles (include/hdg_mi355x.h: hdg_set_particles) -----------------------------
    def _start_particles(self, particles, nt, every=1):
        """Advect the particles seeded at (n, 2) positions through every step on the device and record nt // every + 1 rows:
        the seeds (row 0) and the positions after every `every`-th step."""
        self.particles = None
        self._particle_every = int(every)
        if particles is not None:
            if self._particle_every < 1:
                raise ValueError(f"particle_every must be at least 1 (got {every})")
            self._engine.set_particles(np.asarray(particles, dtype=float).reshape(-1, 2), nt // self._particle_every + 1,
                                       self._particle_every)

    def _finish_particles(self, particles):
        """Fetch the recorded rows once (self.particles: t, xy (rows, n, 2), clamped, lost) and switch the feature off."""
        if particles is None:
            return
        try:
            rows, counts = self._engine.particles(reset=True)
        finally:
            self._engine.set_particles(None, 0)
        self.particles = {"t": np.arange(rows.shape[0]) * self._particle_every * self._dt, "xy": rows,
                          "clamped": counts["clamped"], "lost": counts["lost"]}

    @abstractmethod
    def solve(self, Q_initial, p_initial, q_initial, f_rhs, T_final, warmup=False, diagnostics=False, probes=None,
              particles=None, particle_every=1):
        """Propagate the solution to T_final; returns the final velocity and pressure (common.py:131-144)."""
