"""Every stepper of the numpy oracle against manufactured solutions whose advective tendency does NOT vanish (tests/manufactured.py).

The Taylor-Green tests cannot see a wrong weight on the implicit stage terms, a wrong sign or scale of the upwind term or a wrong
Q* lag: there (Q.grad)Q is a gradient that the pressure solve absorbs.  Here curl((Q.grad)Q) != 0, so each of these errors moves
the velocity.  What is pinned ("Manufactured solutions with advection"):

* spatial orders of every stepper, both fluxes, with the first-order time error removed by 2 X(dt/2) - X(dt);
* SSP2(3,3,2) as the reference defines it solves d_t Q + beta (Q.grad)Q + grad p = f with beta = sum_{i>=1} b_impl[i] = 2/3
  (SURVEY.md C-2): no convergence for the Euler forcing, convergence for the forcing of the derived beta;
* the time order of every tableau is about one (the advecting velocity Q* is the previous stage's), whatever the design order;
* ARS3(4,4,3) as defined diverges as dt shrinks on a short window.

Windows are the measured orders +- 0.3 (never below k + 1 for the velocity, k for the pressure).  The GPU twin of this file is
tests/test_gpu_manufactured.py; it shares the windows below."""
import numpy as np
import pytest

import manufactured as ms

# spatial orders, T = 1/32, dt = 1/128 extrapolated with dt = 1/256; unit square unless stated.
# key -> (stepper, mesh, k, flux, nx list, measured [velocity, pressure] orders per refinement)
SPATIAL = {
    "implicit_projection_upwind_k1": ("implicit_projection", "square", 1, "upwind", (4, 8, 16), [[2.59, 2.99], [2.80, 1.84]]),
    "implicit_monolithic_centered_k1": ("implicit_monolithic", "square", 1, "centered", (4, 8, 16), [[2.62, 2.70], [2.68, 2.14]]),
    "dg_upwind_k1": ("dg", "square", 1, "upwind", (4, 8, 16), [[2.51, 2.72], [2.83, 2.25]]),
    "dg_upwind_k2": ("dg", "square", 2, "upwind", (4, 8), [[3.90, 3.29]]),
    "imex_implicit_upwind_k1": ("imex_implicit", "square", 1, "upwind", (4, 8, 16), [[2.53, 2.29], [2.81, 1.64]]),
    "imex_ars2_232_upwind_k1": ("imex_ars2_232", "square", 1, "upwind", (4, 8, 16), [[2.51, 2.30], [2.84, 1.71]]),
    "imex_ssp3_433_centered_k1": ("imex_ssp3_433", "square", 1, "centered", (4, 8, 16), [[2.61, 2.10], [2.56, 1.35]]),
    # GPU only (tests/test_gpu_manufactured.py): measured on the oracle once
    "imex_ars2_232_upwind_k2": ("imex_ars2_232", "square", 2, "upwind", (4, 8, 16), [[3.97, 3.54], [3.93, 3.10]]),
    "imex_ars2_232_upwind_k3": ("imex_ars2_232", "square", 3, "upwind", (4, 8), [[4.82, 4.50]]),
    "imex_ars2_232_upwind_k1_perturbed": ("imex_ars2_232", "perturbed", 1, "upwind", (4, 8, 16), [[2.47, 2.42], [2.77, 1.83]]),
}
CPU_SPATIAL = [key for key in SPATIAL if not key.endswith(("_k2", "_k3", "_perturbed")) or key.startswith("dg_")]
T_SPATIAL, DT_SPATIAL = 1.0 / 32, 1.0 / 128
WINDOW = 0.3

# time orders on a fixed mesh (successive differences of dt-halved runs, so the spatial error cancels): CPU nx = 4, k = 1
# key -> (T, numbers of steps, measured velocity orders)
TIME_CPU = {
    "imex_ssp2_332": (0.25, (4, 8, 16, 32), [1.08, 0.95]),
    "imex_ars2_232": (0.25, (4, 8, 16, 32), [1.00, 1.02]),
    "imex_ssp3_433": (0.25, (8, 16, 32, 64), [1.32, 1.31]),
    "imex_implicit": (0.25, (16, 32, 64, 128), [0.74, 0.78]),
}
FIXTURE_CLASS = {
    "imex_implicit": "IncompressibleEulerHDGIMEXImplicit",
    "imex_ars2_232": "IncompressibleEulerHDGIMEXARS2_232",
    "imex_ars3_443": "IncompressibleEulerHDGIMEXARS3_443",
    "imex_ssp2_332": "IncompressibleEulerHDGIMEXSSP2_332",
    "imex_ssp3_433": "IncompressibleEulerHDGIMEXSSP3_433",
}


def check_spatial_orders(errs, k, measured):
    o = ms.orders(errs)
    assert np.all(np.isfinite(o)), errs
    assert np.all(np.abs(o - np.asarray(measured)) <= WINDOW), (o.round(3).tolist(), measured, errs)
    assert np.all(o[:, 0] >= k + 1) and np.all(o[:, 1] >= k), o
    return o


def design_order(label):
    """The last number of the tableau's name, e.g. 'HDG IMEX SSP3(4,3,3)' -> 3; the first-order IMEX-implicit pair -> 1."""
    return int(label.rstrip(")").split(",")[-1]) if "(" in label else 1


# ---------------------------------------------------------------------------------------------------------------------------
# the exact solutions themselves
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["unit_square", "periodic_square"])
def test_exact_solution_symbolically(name):
    sympy = pytest.importorskip("sympy")
    sol = getattr(ms, name)()
    x, y, t, psi, p = sol.sympy_fields()
    beta = sympy.Symbol("beta")
    u, v = sympy.diff(psi, y), -sympy.diff(psi, x)
    assert sympy.simplify(sympy.diff(u, x) + sympy.diff(v, y)) == 0  # div Q = 0
    adv = (u * sympy.diff(u, x) + v * sympy.diff(u, y), u * sympy.diff(v, x) + v * sympy.diff(v, y))
    f = [sympy.diff(c, t) + beta * a + sympy.diff(p, z) for c, a, z in ((u, adv[0], x), (v, adv[1], y))]
    curl_adv = sympy.diff(adv[1], x) - sympy.diff(adv[0], y)
    L = sol.L
    if sol.periodic:
        for e in (u, v, p):  # periodic on [0, L]^2
            assert sympy.simplify(e.subs(x, x + L) - e) == 0 and sympy.simplify(e.subs(y, y + L) - e) == 0
    else:
        for s in (0, L):  # Q.n = 0 on the boundary of the square
            assert sympy.simplify(u.subs(x, s)) == 0 and sympy.simplify(v.subs(y, s)) == 0
    assert sympy.simplify(sympy.integrate(sympy.integrate(p, (x, 0, L)), (y, 0, L))) == 0  # mean-free pressure
    # (Q.grad)Q is not a gradient somewhere in the domain, at several times
    cfun = sympy.lambdify((x, y, t), curl_adv, "numpy")
    rng = np.random.default_rng(7)
    X, Y, Tt = rng.uniform(0, L, 64), rng.uniform(0, L, 64), rng.uniform(0, 1, 64)
    assert np.max(np.abs(cfun(X, Y, Tt))) > 1.0
    # the hand-written numpy values equal the symbolic ones (point values, forcing for several beta)
    num = {"Q": sol.Q(X, Y, Tt), "p": sol.p(X, Y, Tt), "adv": sol.advection(X, Y, Tt)}
    ref = {"Q": (u, v), "p": p, "adv": adv}
    for key, expr in ref.items():
        fn = sympy.lambdify((x, y, t), expr, "numpy")
        assert np.allclose(fn(X, Y, Tt), num[key], rtol=1e-13, atol=1e-12), key
    ffun = sympy.lambdify((x, y, t, beta), f, "numpy")
    for b in (1.0, 2.0 / 3.0, -0.5):
        assert np.allclose(ffun(X, Y, Tt, b), sol.f(X, Y, Tt, b), rtol=1e-13, atol=1e-11), b


@pytest.mark.parametrize("mesh,k", [("square", 1), ("periodic", 2), ("perturbed", 2)])
def test_nodal_arrays_equal_the_symbolic_values(mesh, k):
    sympy = pytest.importorskip("sympy")
    sol = ms.solution_for(mesh)
    d = ms.oracle_discretisation(mesh, 3, k)
    x, y, t, psi, p = sol.sympy_fields()
    fQ = sympy.lambdify((x, y, t), (sympy.diff(psi, y), -sympy.diff(psi, x)), "numpy")
    fp = sympy.lambdify((x, y, t), p, "numpy")
    XQ, XP = d.node_coords(d.PU).reshape(-1, 2), d.node_coords(d.PP).reshape(-1, 2)
    tt = 0.375
    assert np.allclose(sol.nodal_Q(d, tt), np.stack(fQ(XQ[:, 0], XQ[:, 1], tt), -1), rtol=0, atol=1e-12)
    assert np.allclose(sol.nodal_p(d, tt), fp(XP[:, 0], XP[:, 1], tt), rtol=0, atol=1e-12)
    # the forcing array and the callable handed to the product interpolate the same function
    fx = np.stack(sol.f_rhs(0.5)(tt)(XQ[:, 0], XQ[:, 1]), -1)
    assert np.array_equal(sol.nodal_f_rhs(d, 0.5)(tt), fx)


def test_perturbed_mesh_fixes_the_boundary_and_stays_valid():
    X0, C = ms.structured_square(8)
    X, C1 = ms.perturbed_square_mesh(8)
    assert np.array_equal(C, C1)
    bnd = np.any((X0 == 0.0) | (X0 == 1.0), axis=1)
    assert np.array_equal(X[bnd], X0[bnd]) and np.max(np.abs(X - X0)) > 0.03
    v = X[C]
    det = (v[:, 1, 0] - v[:, 0, 0]) * (v[:, 2, 1] - v[:, 0, 1]) - (v[:, 2, 0] - v[:, 0, 0]) * (v[:, 1, 1] - v[:, 0, 1])
    assert np.all(det > 0.3 / 64)


# ---------------------------------------------------------------------------------------------------------------------------
# spatial orders of the oracle
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", CPU_SPATIAL)
def test_oracle_spatial_orders(key):
    stepper, mesh, k, flux, nxs, measured = SPATIAL[key]
    errs = [ms.oracle_errors(stepper, mesh, nx, k, DT_SPATIAL, T_SPATIAL, flux=flux) for nx in nxs]
    check_spatial_orders(errs, k, measured)


def test_time_error_is_removed_by_the_extrapolation():
    """the first-order time error pollutes the finest mesh of the implicit stepper (velocity order 2.80 -> about 1.8 without
    the extrapolation): the extrapolation is needed, and enough"""
    plain = [ms.oracle_errors("implicit_projection", "square", nx, 1, DT_SPATIAL / 2, T_SPATIAL, extrapolate=False)
             for nx in (8, 16)]
    assert ms.orders(plain)[0, 0] < 2.0, plain


# ---------------------------------------------------------------------------------------------------------------------------
# SSP2(3,3,2): beta = sum_{i>=1} b_impl[i]
# ---------------------------------------------------------------------------------------------------------------------------
def ssp2_velocity_errors(mesh, nxs, beta, k=1, T=1.0 / 32, dt=1.0 / 256):
    return [ms.oracle_errors("imex_ssp2_332", mesh, nx, k, dt, T, beta=beta, extrapolate=False)[0] for nx in nxs]


def test_ssp2_332_solves_a_different_equation():
    fx = ms.tableau_fixture()
    beta = ms.beta_of(fx["IncompressibleEulerHDGIMEXSSP2_332"])
    assert abs(beta - 2.0 / 3.0) < 1e-15  # b_impl = [1/3, 1/3, 1/3], b_impl[0] unused
    for name in ("IncompressibleEulerHDGIMEXImplicit", "IncompressibleEulerHDGIMEXARS2_232", "IncompressibleEulerHDGIMEXSSP3_433",
                 "IncompressibleEulerHDGIMEXARS3_443"):
        assert abs(ms.beta_of(fx[name]) - 1.0) < 1e-14, name  # the others weight the advection consistently
    nxs = (4, 8, 16)
    e1 = ssp2_velocity_errors("square", nxs, 1.0)
    eb = ssp2_velocity_errors("square", nxs, beta)
    # Euler forcing: a floor that does not shrink with h (measured 0.083 / 0.071 / 0.071)
    assert min(e1) > 0.06 and e1[2] > 0.95 * e1[1], e1
    # forcing of the derived beta: converges like the consistent schemes (measured 0.042 / 0.0076 / 0.0012, orders 2.5 / 2.7)
    check_velocity = ms.orders(np.stack([eb, eb], -1))[:, 0]
    assert np.all(np.abs(check_velocity - [2.48, 2.68]) <= WINDOW) and eb[2] < 0.02 * e1[2], eb


# ---------------------------------------------------------------------------------------------------------------------------
# time orders
# ---------------------------------------------------------------------------------------------------------------------------
def time_differences(stepper, mesh, nx, k, T, nsteps, run=None):
    """||X(T/n_j) - X(T/n_{j+1})|| for successive n: the spatial error is the same in both runs and cancels."""
    d, sol = ms.oracle_discretisation(mesh, nx, k), ms.solution_for(mesh)
    runs = [ms.oracle_run(stepper, d, sol, T / n, T) for n in nsteps]
    return [(d.l2_norm_velocity(a[0] - b[0]), d.l2_norm_pressure(a[1] - b[1])) for a, b in zip(runs[:-1], runs[1:])]


@pytest.mark.parametrize("stepper", list(TIME_CPU))
def test_oracle_time_orders(stepper):
    T, nsteps, measured = TIME_CPU[stepper]
    o = ms.orders(time_differences(stepper, "square", 4, 1, T, nsteps))[:, 0]
    assert np.all(np.abs(o - measured) <= WINDOW), (o.round(3).tolist(), measured)
    # about one for every tableau: the lagged advecting velocity caps the order whatever the tableau was designed for
    label = ms.tableau_fixture()[FIXTURE_CLASS[stepper]]["label"]
    p = design_order(label)
    assert o[-1] > 0.6, (label, o)
    if p >= 2:
        assert o[-1] < p - 0.5, (label, p, o)


# ---------------------------------------------------------------------------------------------------------------------------
# ARS3(4,4,3) as defined: diverges as dt shrinks (CPU only -- never on the GPU)
# ---------------------------------------------------------------------------------------------------------------------------
def test_ars3_443_diverges_as_dt_shrinks():
    """nx = 4, k = 2, T = 1/4: the difference between successive dt-halved runs GROWS (measured 0.042 / 0.070 / 0.110 for
    n = 2 / 4 / 8 / 16 steps; the error against the exact solution 0.040 / 0.033 / 0.066 / 0.094), where every consistent,
    stable scheme has it shrink.  (At nx = 8, k = 2, T = 1/2 the error reaches 1e6 at 32 steps.)"""
    fx = ms.tableau_fixture()["IncompressibleEulerHDGIMEXARS3_443"]
    assert len(fx["b_impl"]["values"]) == fx["nstages"] + 1  # the six-entry b_impl
    diffs = np.array(time_differences("imex_ars3_443", "square", 4, 2, 0.25, (2, 4, 8, 16)))
    assert diffs[1, 0] > 1.4 * diffs[0, 0] and diffs[2, 0] > 1.4 * diffs[1, 0], diffs
    assert diffs[2, 1] > 3.0 * diffs[1, 1], diffs


def test_ars3_443_short_window_is_stable():
    """the window the GPU test uses (nx = 8, k = 2, T = 1/16, 2 / 4 / 8 steps): the differences shrink and stay small (measured
    0.0016 / 0.0014; the error against the exact solution 0.0024 / 0.0016 / 0.0012)"""
    diffs = np.array(time_differences("imex_ars3_443", "square", 8, 2, 1.0 / 16, (2, 4, 8)))
    assert diffs[1, 0] < diffs[0, 0] < 2e-3, diffs
