"""Model problems as node-evaluated arrays (reference: src/model_problems.py:10-105).

The manufactured Taylor-Green vortex (model_problems.py:38-105), the Kelvin-Helmholtz instability on the unit disk
(:108-131) and the double-layer shear flow on the periodic square (:134-196).
"""

import numpy as np

from .mesh import Function

__all__ = ["TaylorGreen", "RotatingTaylorGreen", "DraggedTaylorGreen", "CylinderWake", "KelvinHelmholtz", "DoubleLayerShearFlow", "SeparableForcing"]


class SeparableForcing:
    """f(t) = g(t) * profile; callable like the reference's ``f_rhs`` lambdas (model_problems.py:76-79)
    and additionally exposes the factorisation so that the engine never re-uploads the profile."""

    def __init__(self, profile, g):
        self.profile = profile
        self.g = g

    def scale(self, t):
        return float(self.g(t))

    def __call__(self, t):
        return self.scale(t) * self.profile


class TaylorGreen:
    """Taylor-Green vortex with manufactured time dependence (model_problems.py:38-105).

    viscosity: nu of the viscous term.  Laplace Q_s = -2 pi^2 Q_s and Q_s is free-slip on the unit square,
    so a(t) Q_s stays an exact Navier-Stokes solution with the separable forcing a'(t) + 2 pi^2 nu a(t); nu = 0 is exactly the
    Euler problem, the kappa == 0 rule included."""

    def __init__(self, V_Q, V_p, forcing="exponential", kappa=0.5, viscosity=0.0):
        assert forcing in ("exponential", "constant"), "Forcing must be 'constant' or 'exponential'"
        self.V_Q, self.V_p = V_Q, V_p
        self.kappa = kappa
        self.viscosity = viscosity
        self.forcing = forcing
        S = lambda z: np.sin((z - 0.5) * np.pi)
        C = lambda z: np.cos((z - 0.5) * np.pi)
        # model_problems.py:56-65 (the code's p_s, not the README's: SURVEY.md C-10)
        self.Q_stationary = lambda x, y: (-C(x) * S(y), S(x) * C(y))
        self.p_stationary = lambda x, y: (S(x) ** 2 + S(y) ** 2) / 2
        self._Qs = V_Q.interpolate(self.Q_stationary)
        self._ps = V_p.interpolate(self.p_stationary)

    def initial_condition(self):
        return self.Q_stationary, self.p_stationary

    def f_rhs(self):
        """Forcing as a function of time; kappa == 0 is treated as zero forcing."""
        k = self.kappa
        if self.viscosity != 0:
            c = 2.0 * np.pi ** 2 * self.viscosity
            if self.forcing == "exponential":
                return SeparableForcing(self._Qs, lambda t: (-k + c) * np.exp(-k * t))
            return SeparableForcing(self._Qs, lambda t: -k + c * (1.0 - k * t))
        if k == 0:
            return SeparableForcing(self._Qs, lambda t: 0.0)
        if self.forcing == "exponential":
            return SeparableForcing(self._Qs, lambda t: -k * np.exp(-k * t))
        return SeparableForcing(self._Qs, lambda t: -k)

    def solution(self, t, integrate_pressure=None):
        """Interpolant of the stationary fields scaled by the time factors (model_problems.py:87-105)."""
        k = self.kappa
        if self.forcing == "exponential":
            Q = np.exp(-k * t) * self._Qs
            p = np.exp(-2 * k * t) * self._ps
        else:
            Q = (1.0 - k * t) * self._Qs
            p = (1.0 - k * t) ** 2 * self._ps
        if integrate_pressure is not None:
            p = p - integrate_pressure(p)  # model_problems.py:104: no division by the volume
        return Function(self.V_Q, Q, "velocity_exact"), Function(self.V_p, p, "pressure_exact")


class RotatingTaylorGreen(TaylorGreen):
    """The Taylor-Green vortex in a rotating frame: coriolis = (f0, beta) of - f_c k x u, f_c = f0 + beta y.

    The solution is TaylorGreen's: the forcing gains + f_c k x Q, which cancels the term.  With the exponential time factor the
    forcing stays separable, profile (-kappa + 2 pi^2 nu) Q_s + f_c k x Q_s times exp(-kappa t); with forcing="constant" the
    two parts carry different time factors (-kappa + ... and 1 - kappa t), so that combination is refused.  coriolis = (0, 0)
    is TaylorGreen itself."""

    def __init__(self, V_Q, V_p, forcing="exponential", kappa=0.5, viscosity=0.0, coriolis=(0.0, 0.0)):
        f0, beta = (float(coriolis), 0.0) if np.ndim(coriolis) == 0 else (float(coriolis[0]), float(coriolis[1]))
        if (f0 != 0 or beta != 0) and forcing != "exponential":
            raise ValueError("RotatingTaylorGreen: forcing='constant' is not separable with rotation (the two time factors differ)")
        super().__init__(V_Q, V_p, forcing, kappa, viscosity)
        self.coriolis = (f0, beta)

    def f_rhs(self):
        f0, beta = self.coriolis
        if f0 == 0 and beta == 0:
            return super().f_rhs()
        k, c = self.kappa, -self.kappa + 2.0 * np.pi ** 2 * self.viscosity

        def profile(x, y):
            qx, qy = self.Q_stationary(x, y)
            fc = f0 + beta * y
            return c * qx - fc * qy, c * qy + fc * qx  # k x Q = (-Q_y, Q_x)

        return SeparableForcing(self.V_Q.interpolate(profile), lambda t: np.exp(-k * t))


class DraggedTaylorGreen(TaylorGreen):
    """The Taylor-Green vortex under a drag towards rest: drag = sigma(x, y) >= 0 of - sigma u.

    The solution is TaylorGreen's: the forcing gains + sigma Q, which cancels the term.  With the exponential time factor the
    forcing stays separable, profile (-kappa + 2 pi^2 nu + sigma) Q_s times exp(-kappa t); the discrete term matches the profile
    exactly for a sigma that is linear over the square.  With forcing="constant" the two parts carry different time factors, so
    that combination is refused.  drag=None is TaylorGreen itself."""

    def __init__(self, V_Q, V_p, forcing="exponential", kappa=0.5, viscosity=0.0, drag=None):
        if drag is not None and forcing != "exponential":
            raise ValueError("DraggedTaylorGreen: forcing='constant' is not separable with a drag (the two time factors differ)")
        super().__init__(V_Q, V_p, forcing, kappa, viscosity)
        self.drag = (lambda x, y, r=float(drag): r + 0.0 * x) if drag is not None and not callable(drag) else drag

    def f_rhs(self):
        if self.drag is None:
            return super().f_rhs()
        k, c = self.kappa, -self.kappa + 2.0 * np.pi ** 2 * self.viscosity

        def profile(x, y):
            qx, qy = self.Q_stationary(x, y)
            s = self.drag(x, y)
            return (c + s) * qx, (c + s) * qy

        return SeparableForcing(self.V_Q.interpolate(profile), lambda t: np.exp(-k * t))


class CylinderWake:
    """Flow past a disc on the doubly periodic square [0, L]^2 by volume penalisation: a uniform stream
    (U, 0); a disc of radius L / 16 at (L / 4, L / 2) held at rest by sigma = S inside, with a tanh edge one cell (h) wide
    (region 1); a sin^2 fringe over the last eighth in x that drives the flow back to the stream (region 2, u_s = (U, 0)), which
    makes the periodic box an open channel.  sigma, target and region are what Engine.set_drag takes.  No exact solution."""

    def __init__(self, V_Q, V_p, L, h, obstacle_drag, stream=1.0, fringe_drag=None):
        self.V_Q, self.V_p = V_Q, V_p
        self.L, self.h, self.S, self.U = float(L), float(h), float(obstacle_drag), float(stream)
        self.fringe = self.S if fringe_drag is None else float(fringe_drag)
        self.radius, self.centre = self.L / 16.0, (self.L / 4.0, self.L / 2.0)
        self.Q_initial = lambda x, y: (self.U + 0.0 * x, 0.0 * y)
        self.p_initial = lambda x, y: 0.0 * x

    def _disc(self, x, y):
        r = np.hypot(x - self.centre[0], y - self.centre[1])
        return 0.5 * (1.0 - np.tanh((r - self.radius) / (0.5 * self.h)))

    def _fringe(self, x):
        z = (x - 0.875 * self.L) / (0.125 * self.L)
        return np.where(z > 0.0, np.sin(np.pi * np.clip(z, 0.0, 1.0)) ** 2, 0.0)

    def sigma(self, x, y):
        disc = self._disc(x, y)
        return self.S * np.where(disc > 1e-8, disc, 0.0) + self.fringe * self._fringe(x)  # exactly zero away from both

    def target(self, x, y):
        return self.U * (x >= (0.875 - 1e-12) * self.L), 0.0 * y  # the fringe's own edge included: sigma vanishes there, not u_s

    def region(self, x, y):
        return np.where(self._fringe(x) > 0.0, 2, np.where(self._disc(x, y) > 1e-8, 1, 0))

    def coefficients(self, force):
        """(C_D, C_L) from the force on the fluid of region 1, Engine.drag_force()[1]: the body feels the negative"""
        q = 0.5 * self.U ** 2 * 2.0 * self.radius
        return -force[0] / q, -force[1] / q

    def initial_condition(self):
        return self.Q_initial, self.p_initial

    def f_rhs(self):
        """Zero forcing."""
        return None

    def solution(self, t, integrate_pressure=None):
        return None


class KelvinHelmholtz:
    """Kelvin-Helmholtz instability on the circular mesh (model_problems.py:108-131): rigid rotation (-y, x) inside
    r < r_max = 0.5, fluid at rest outside, zero pressure, zero forcing; no exact solution."""

    def __init__(self, V_Q, V_p, r_max=0.5):
        self.V_Q, self.V_p = V_Q, V_p
        self.r_max = r_max
        inside = lambda x, y: x ** 2 + y ** 2 < r_max ** 2  # conditional(x**2 + y**2 < r_max**2, (-y, x), (0, 0))
        self.Q_stationary = lambda x, y: (np.where(inside(x, y), -y, 0.0), np.where(inside(x, y), x, 0.0))
        self.p_stationary = lambda x, y: 0.0 * x

    def initial_condition(self):
        return self.Q_stationary, self.p_stationary

    def f_rhs(self):
        """Zero forcing (model_problems.py:129-131)."""
        return None

    def solution(self, t, integrate_pressure=None):
        return None


class Cavity:
    """A closed box of fluid at rest: zero velocity, zero pressure, zero forcing; what moves it is the
    buoyancy of tracers held at fixed values on the walls (the differentially heated cavity, Rayleigh-Benard convection in a
    box).  No exact solution."""

    def __init__(self, V_Q, V_p):
        self.V_Q, self.V_p = V_Q, V_p
        self.Q_initial = lambda x, y: (0.0 * x, 0.0 * y)
        self.p_initial = lambda x, y: 0.0 * x

    def initial_condition(self):
        return self.Q_initial, self.p_initial

    def f_rhs(self):
        """Zero forcing."""
        return None

    def solution(self, t, integrate_pressure=None):
        return None


class DoubleLayerShearFlow:
    """Double layer shear flow (model_problems.py:134-196; Guzman, Shu, Sequeira, IMA J. Numer. Anal. 37 (2017)) on the
    periodic square [0, 2 pi]^2: two tanh shear layers of width rho perturbed by a vertical velocity of magnitude delta;
    the initial pressure is the 28-term Fourier series of the reference, its coefficients by scipy.integrate.quad."""

    def __init__(self, V_Q, V_p, rho=np.pi / 15, delta=0.05):
        from scipy import integrate

        self.V_Q, self.V_p = V_Q, V_p
        self.rho, self.delta = rho, delta
        self.Q_initial = lambda x, y: (np.where(y <= np.pi, np.tanh((y - np.pi / 2) / rho), np.tanh((1.5 * np.pi - y) / rho)),
                                       delta * np.sin(x))
        kmax = 28  # number of Fourier coefficients (model_problems.py:164)
        coef = []
        for k in range(kmax):
            c = integrate.quad(
                lambda z: np.where(z <= 0.0, 1 - np.tanh((np.pi + 2 * z) / (4 * np.pi * rho)) ** 2,
                                   -1 + np.tanh((np.pi - 2 * z) / (4 * np.pi * rho)) ** 2) / (np.pi ** 2 * rho),
                -np.pi, +np.pi, weight="sin", wvar=2 * k + 1, epsabs=1e-12, epsrel=1e-12)[0]
            coef.append(c / (1 + (2 * k + 1) ** 2))
        self._coef = coef

        def p_initial(x, y):
            acc = 0.0
            for k, c in enumerate(self._coef):
                acc = acc + c * np.sin((2 * k + 1) * (y - np.pi))
            return acc * delta * np.cos(x)

        self.p_initial = p_initial

    def initial_condition(self):
        return self.Q_initial, self.p_initial

    def f_rhs(self):
        """Zero forcing (model_problems.py:194-196)."""
        return None
