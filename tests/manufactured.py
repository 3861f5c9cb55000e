"""Manufactured exact solutions with a NON-vanishing advective tendency (helper of the manufactured-solution tests, not a test
module).

For the Taylor-Green vortex (Q.grad)Q + grad p == 0, so the advective part of the implicit tendency is a pure gradient that the
pressure solve absorbs whatever its weight or sign: a wrong stage weight, a wrong upwind sign or a wrong Q* lag passes every
Taylor-Green test.  The solutions here are divergence-free velocities Q = (d_y psi, -d_x psi) built from a stream function that
is a sum of separable modes with DIFFERENT Laplacian eigenvalues, so the vorticity is not a function of psi alone and
curl((Q.grad)Q) != 0.  The forcing

    f(x, y, t; beta) = d_t Q + beta (Q.grad) Q + grad p

makes (Q, p) the exact solution of d_t Q + beta (Q.grad)Q + grad p = f, div Q = 0; beta = 1 is the Euler equations, other
values characterise schemes that weight the advection wrongly.

Every factor is A trig(w z + phi) with trig in {sin, cos}; all derivatives are written out by hand (numpy only: the GPU machine
need not have sympy).  tests/test_manufactured.py checks them symbolically where sympy is available.

* ``unit_square()``       psi vanishes on the boundary of [0, 1]^2, so Q.n = 0 there; mean-free p
* ``periodic_square(L)``  periodic modes on [0, L]^2 (PeriodicSquareMesh(nx, L=L))
* ``perturbed_square_mesh(nx, a)``  the structured unit-square triangulation with its vertices moved by the smooth map
  x -> x + a sin(2 pi x) sin(2 pi y) (both components), which fixes the boundary: the general-mesh path, same exact solution
  as ``unit_square()``.

Each solution gives point values ``Q(x, y, t)``, ``p(x, y, t)``, ``f(x, y, t, beta)``; callables ``(x, y) -> (u, v)`` for the
product classes (``Q_expr``, ``p_expr``, ``f_rhs``); nodal arrays for the numpy oracle and tests/dg_reference.py
(``nodal_Q``, ``nodal_p``, ``nodal_f_rhs``).
"""
import numpy as np

PI = np.pi


class Trig:
    """A trig(w z + phi); trig in {'sin', 'cos'}.  ``d(z, n)`` is the n-th derivative (n = 0, 1, 2)."""

    def __init__(self, kind, w, amp=1.0, phase=0.0):
        assert kind in ("sin", "cos")
        self.kind, self.w, self.amp, self.phase = kind, float(w), float(amp), float(phase)

    def d(self, z, n=0):
        # sin^(n)(s) = sin(s + n pi/2), cos^(n)(s) = cos(s + n pi/2)
        f = np.sin if self.kind == "sin" else np.cos
        return self.amp * self.w ** n * f(self.w * np.asarray(z, dtype=float) + self.phase + n * PI / 2)

    def sympy(self, z):
        import sympy

        f = sympy.sin if self.kind == "sin" else sympy.cos
        r = self.w / PI  # spatial wavenumbers are rational multiples of pi, time frequencies are not
        w = sympy.Rational(round(r * 64), 64) * sympy.pi if abs(r * 64 - round(r * 64)) < 1e-9 else sympy.nsimplify(self.w)
        return sympy.nsimplify(self.amp) * f(w * z + sympy.nsimplify(self.phase))


class ManufacturedSolution:
    """psi = sum_m T_m(t) X_m(x) Y_m(y),  Q = (d_y psi, -d_x psi),  p = sum_n S_n(t) P_n(x) R_n(y).

    psi_modes / p_modes: lists of (T, X, Y) Trig triples."""

    def __init__(self, name, psi_modes, p_modes, L=1.0, periodic=False):
        self.name, self.psi_modes, self.p_modes, self.L, self.periodic = name, psi_modes, p_modes, float(L), periodic

    # -- point values ------------------------------------------------------------------------------------------------------
    def _grad_Q(self, x, y, t):
        """u, v and their first derivatives (ux, uy, vx, vy)."""
        u = v = ux = uy = vx = vy = 0.0
        for T, X, Y in self.psi_modes:
            c = T.d(t)
            u = u + c * X.d(x) * Y.d(y, 1)
            v = v - c * X.d(x, 1) * Y.d(y)
            ux = ux + c * X.d(x, 1) * Y.d(y, 1)
            uy = uy + c * X.d(x) * Y.d(y, 2)
            vx = vx - c * X.d(x, 2) * Y.d(y)
            vy = vy - c * X.d(x, 1) * Y.d(y, 1)
        return u, v, ux, uy, vx, vy

    def Q(self, x, y, t):
        u, v = self._grad_Q(x, y, t)[:2]
        return u + 0.0 * np.asarray(x), v + 0.0 * np.asarray(x)

    def dQdt(self, x, y, t):
        ut = vt = 0.0
        for T, X, Y in self.psi_modes:
            c = T.d(t, 1)
            ut = ut + c * X.d(x) * Y.d(y, 1)
            vt = vt - c * X.d(x, 1) * Y.d(y)
        return ut, vt

    def advection(self, x, y, t):
        """(Q.grad)Q."""
        u, v, ux, uy, vx, vy = self._grad_Q(x, y, t)
        return u * ux + v * uy, u * vx + v * vy

    def p(self, x, y, t):
        p = 0.0 * np.asarray(x, dtype=float)
        for S, P, R in self.p_modes:
            p = p + S.d(t) * P.d(x) * R.d(y)
        return p

    def grad_p(self, x, y, t):
        px = py = 0.0
        for S, P, R in self.p_modes:
            px = px + S.d(t) * P.d(x, 1) * R.d(y)
            py = py + S.d(t) * P.d(x) * R.d(y, 1)
        return px, py

    def f(self, x, y, t, beta=1.0):
        """d_t Q + beta (Q.grad)Q + grad p."""
        (ut, vt), (ax, ay), (px, py) = self.dQdt(x, y, t), self.advection(x, y, t), self.grad_p(x, y, t)
        return ut + beta * ax + px + 0.0 * np.asarray(x), vt + beta * ay + py + 0.0 * np.asarray(x)

    # -- callables for the product classes (common.py: callables (x, y) -> (u, v) are interpolated at the nodes) ----------
    def Q_expr(self, t):
        return lambda x, y: self.Q(x, y, t)

    def p_expr(self, t):
        return lambda x, y: self.p(x, y, t)

    def f_rhs(self, beta=1.0):
        """t -> (x, y) -> f: the non-separable callable forcing (set_forcing_nodal path of the product)."""
        return lambda t: (lambda x, y: self.f(x, y, t, beta))

    # -- nodal arrays for the numpy oracle (oracle.hdg_oracle.HDGDiscretisation) ---------------------------------------------
    def nodal_Q(self, d, t):
        return d.interpolate_velocity(self.Q_expr(t))

    def nodal_p(self, d, t):
        return d.interpolate_pressure(self.p_expr(t))

    def nodal_f_rhs(self, d, beta=1.0):
        X = d.node_coords(d.PU)
        x, y = X[..., 0], X[..., 1]
        return lambda t: np.stack(self.f(x, y, t, beta), axis=-1).reshape(-1, 2)

    # -- sympy restatement (only for the symbolic checks) ---------------------------------------------------------------------
    def sympy_fields(self):
        """(x, y, t, psi, p) as sympy expressions."""
        import sympy

        x, y, t = sympy.symbols("x y t", real=True)
        psi = sum(T.sympy(t) * X.sympy(x) * Y.sympy(y) for T, X, Y in self.psi_modes)
        p = sum(S.sympy(t) * P.sympy(x) * R.sympy(y) for S, P, R in self.p_modes)
        return x, y, t, psi, p


def unit_square():
    """psi = cos t sin(pi x) sin(pi y) + 1/2 sin(2t + 1) sin(2 pi x) sin(pi y)  (Laplacian eigenvalues 2 pi^2, 5 pi^2),
    p = cos t cos(pi x) cos(pi y) (mean free)."""
    psi = [
        (Trig("cos", 1.0), Trig("sin", PI), Trig("sin", PI)),
        (Trig("sin", 2.0, 0.5, 1.0), Trig("sin", 2 * PI), Trig("sin", PI)),
    ]
    p = [(Trig("cos", 1.0), Trig("cos", PI), Trig("cos", PI))]
    return ManufacturedSolution("unit_square", psi, p)


def periodic_square(L=1.0):
    """psi = cos t sin(kx) sin(ky) + 1/2 sin(2t + 1) cos(2kx) sin(ky),  k = 2 pi / L  (eigenvalues 2 k^2, 5 k^2),
    p = cos t sin(kx) cos(ky) (mean free)."""
    k = 2 * PI / L
    psi = [
        (Trig("cos", 1.0), Trig("sin", k), Trig("sin", k)),
        (Trig("sin", 2.0, 0.5, 1.0), Trig("cos", 2 * k), Trig("sin", k)),
    ]
    p = [(Trig("cos", 1.0), Trig("sin", k), Trig("cos", k))]
    return ManufacturedSolution("periodic_square", psi, p, L=L, periodic=True)


def structured_square(nx):
    """Vertices and cells of the structured nx x nx unit-square triangulation (two triangles per square)."""
    xs = np.linspace(0.0, 1.0, nx + 1)
    X = np.array([(x, y) for y in xs for x in xs])
    vid = lambda i, j: j * (nx + 1) + i
    cells = []
    for j in range(nx):
        for i in range(nx):
            cells.append((vid(i, j), vid(i + 1, j), vid(i, j + 1)))
            cells.append((vid(i + 1, j + 1), vid(i, j + 1), vid(i + 1, j)))
    return X, np.array(cells)


def perturbed_square_mesh(nx, a=0.05):
    """(vertices, cells): the structured triangulation moved by x -> x + a sin(2 pi x) sin(2 pi y) in both components.  The
    map fixes the boundary of [0, 1]^2 (so the domain, and unit_square()'s exact solution, are unchanged) and its Jacobian
    determinant 1 + 2 pi a sin(2 pi (x + y)) stays positive for a < 1 / (2 pi).  Applied at every nx, so the meshes of a
    refinement sequence are images of the same smooth map (asymptotic regime)."""
    X, C = structured_square(nx)
    s = a * np.sin(2 * PI * X[:, 0]) * np.sin(2 * PI * X[:, 1])
    s[np.any((X == 0.0) | (X == 1.0), axis=1)] = 0.0  # sin(2 pi) is not 0 in floating point
    return X + s[:, None], C


def l2_errors_oracle(sol, d, Q, p, t):
    """Oracle L2 errors (driver.py:376-377) of (Q, p) against the nodal interpolant of the exact solution; the exact pressure
    is shifted to the discrete zero mean of the stepper's pressure."""
    pe = sol.nodal_p(d, t)
    pe = pe - float(d.int_p @ pe) / d.mesh.volume
    return d.l2_norm_velocity(Q - sol.nodal_Q(d, t)), d.l2_norm_pressure(p - pe)


# -- oracle runs (numpy oracle / tests/dg_reference.py) shared by the CPU and GPU manufactured-solution tests ------------------
STEPPERS = ("implicit_projection", "implicit_monolithic", "dg", "imex_implicit", "imex_ars2_232", "imex_ars3_443",
            "imex_ssp2_332", "imex_ssp3_433")


def solution_for(mesh):
    return periodic_square() if mesh == "periodic" else unit_square()


def oracle_discretisation(mesh, nx, k):
    """mesh in {'square', 'periodic', 'perturbed'}."""
    from oracle import fem
    from oracle.hdg_oracle import HDGDiscretisation

    if mesh == "square":
        return HDGDiscretisation(nx, k)
    if mesh == "periodic":
        return HDGDiscretisation(nx, k, periodic=True)
    if mesh == "perturbed":
        return HDGDiscretisation(0, k, mesh=fem.TriMesh(*perturbed_square_mesh(nx)))
    raise ValueError(mesh)


def oracle_run(stepper, d, sol, dt, T, beta=1.0, flux="upwind"):
    """(Q, p) at T of `stepper` (one of STEPPERS) on the oracle discretisation d, from the exact solution at t = 0, with the
    forcing for beta."""
    from dg_reference import dg_solve
    from oracle.hdg_oracle import OracleHDGImplicit, OracleHDGIMEX

    Q0, p0, f = sol.nodal_Q(d, 0.0), sol.nodal_p(d, 0.0), sol.nodal_f_rhs(d, beta)
    if stepper.startswith("implicit_"):
        return OracleHDGImplicit(d, dt, flux, stepper == "implicit_projection").solve(Q0, p0, f, T)
    if stepper == "dg":
        return dg_solve(d, Q0, p0, f, dt, int(round(T / dt)), flux)
    return OracleHDGIMEX(d, dt, stepper, flux).solve(Q0, p0, f, T)


def oracle_errors(stepper, mesh, nx, k, dt, T, beta=1.0, flux="upwind", extrapolate=True):
    """L2 errors (velocity, pressure) at T.  extrapolate: of 2 X(dt/2) - X(dt), which removes the first-order time error
    (every stepper here is first order in time, see test_manufactured.py) so that the spatial error is what remains."""
    d, sol = oracle_discretisation(mesh, nx, k), solution_for(mesh)
    Q, p = oracle_run(stepper, d, sol, dt / 2 if extrapolate else dt, T, beta, flux)
    if extrapolate:
        Q1, p1 = oracle_run(stepper, d, sol, dt, T, beta, flux)
        Q, p = 2 * Q - Q1, 2 * p - p1
    return l2_errors_oracle(sol, d, Q, p, T)


def orders(errors):
    """log2 of the ratios of successive errors (rows: meshes or time steps halved; columns: velocity, pressure)."""
    e = np.asarray(errors, dtype=float)
    return np.log2(e[:-1] / e[1:])


def beta_of(fixture_class):
    """The advection weight the reference's _final_residual actually applies: it loops i = 1..s-1, so
    b_impl[0] is never read and the scheme solves d_t Q + beta (Q.grad)Q + grad p = f with beta = sum_{i >= 1} b_impl[i]."""
    vals = [float(v) for v in fixture_class["b_impl"]["values"]]
    return float(np.sum(vals[1:fixture_class["nstages"]]))


def tableau_fixture():
    import json
    import os

    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tableaux_reference.json")) as fh:
        return json.load(fh)["classes"]
