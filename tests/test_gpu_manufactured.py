"""The product classes against the manufactured solutions with a non-vanishing advective tendency (tests/manufactured.py): the GPU
twin of tests/test_manufactured.py, with the same windows.

Every run goes through the C-ABI with the non-separable callable forcing, i.e. the set_forcing_nodal path.  Covered: the unit
square at k = 1, 2, 3 (k = 3: k_adv_mfma / k_edge_lift_mfma), the periodic square (wrapped tile kernels), the perturbed square
(general-mesh k_g_* kernels); the HDG implicit stepper in both branches, DG implicit at k = 1 and 2 (k_dg_avg_trace), the IMEX
tableaux fused and, once, per solve.  Where a case also runs on the oracle, the GPU errors equal the oracle's at nx = 4 and 8 to
a relative 1e-6, which ties the GPU to the characterisation.  No run that diverges on the CPU is made here (ARS3 only on the
short window tests/test_manufactured.py shows stable)."""
import numpy as np
import pytest

import manufactured as ms
from test_manufactured import DT_SPATIAL, SPATIAL, T_SPATIAL, WINDOW, check_spatial_orders

pytestmark = pytest.mark.gpu
PARITY = 1e-6

IMEX_CLASS = {
    "imex_implicit": "IncompressibleEulerHDGIMEXImplicit",
    "imex_ars2_232": "IncompressibleEulerHDGIMEXARS2_232",
    "imex_ars3_443": "IncompressibleEulerHDGIMEXARS3_443",
    "imex_ssp2_332": "IncompressibleEulerHDGIMEXSSP2_332",
    "imex_ssp3_433": "IncompressibleEulerHDGIMEXSSP3_433",
}


def product_mesh(mesh, nx):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, TriangleMesh, UnitSquareMesh

    if mesh == "square":
        return UnitSquareMesh(nx, nx)
    if mesh == "periodic":
        return PeriodicSquareMesh(nx, nx, L=1.0)
    return TriangleMesh(*ms.perturbed_square_mesh(nx))


def product_run(stepper, mesh, nx, k, dt, T, beta=1.0, flux="upwind", fused=True):
    """(Q, p, timestepper) at T from the exact solution at t = 0; callables for the initial data and the forcing."""
    from incompressibleeulerhdg_amd import timesteppers as tsm

    sol, pm = ms.solution_for(mesh), product_mesh(mesh, nx)
    args = (sol.Q_expr(0.0), sol.p_expr(0.0), None, sol.f_rhs(beta), T)
    if stepper.startswith("implicit_"):
        ts = tsm.IncompressibleEulerHDGImplicit(pm, k, dt, flux=flux, use_projection_method=stepper == "implicit_projection")
        Q, p = ts.solve(*args)
    elif stepper == "dg":
        ts = tsm.IncompressibleEulerDGImplicit(pm, k, dt, flux=flux)
        Q, p = ts.solve(*args)
    else:
        ts = getattr(tsm, IMEX_CLASS[stepper])(pm, k, dt, flux=flux)
        Q, p = ts.solve(*args, fused=fused)
    return np.array(Q.dat.data), np.array(p.dat.data), ts


def product_errors(ts, sol, Q, p, T):
    eng = ts._engine
    Qe = ts._V_Q.interpolate(sol.Q_expr(T))
    pe = ts._V_p.interpolate(sol.p_expr(T))
    pe = pe - eng.integrate_pressure(pe) / ts.domain_volume
    return eng.l2_norms(Q - Qe, p - pe)


def gpu_errors(stepper, mesh, nx, k, dt, T, beta=1.0, flux="upwind", fused=True, extrapolate=True):
    """the product's counterpart of manufactured.oracle_errors"""
    sol = ms.solution_for(mesh)
    Q, p, ts = product_run(stepper, mesh, nx, k, dt / 2 if extrapolate else dt, T, beta, flux, fused)
    if extrapolate:
        Q1, p1, _ = product_run(stepper, mesh, nx, k, dt, T, beta, flux, fused)
        Q, p = 2 * Q - Q1, 2 * p - p1
    return product_errors(ts, sol, Q, p, T)


def check_parity(gpu, cpu):
    rel = np.abs(np.asarray(gpu) - np.asarray(cpu)) / np.abs(np.asarray(cpu))
    assert np.all(rel < PARITY), (gpu, cpu, rel)


# ---------------------------------------------------------------------------------------------------------------------------
# spatial orders: the windows of tests/test_manufactured.py; parity with the oracle where it runs the same case
# ---------------------------------------------------------------------------------------------------------------------------
GPU_SPATIAL = [
    ("implicit_projection_upwind_k1", True, True),
    ("implicit_monolithic_centered_k1", True, True),
    ("dg_upwind_k1", True, True),
    ("dg_upwind_k2", True, True),
    ("imex_implicit_upwind_k1", True, True),
    ("imex_ars2_232_upwind_k1", False, True),  # the per-solve path once
    ("imex_ssp3_433_centered_k1", True, True),
    ("imex_ars2_232_upwind_k2", True, False),
    ("imex_ars2_232_upwind_k3", True, False),
    ("imex_ars2_232_upwind_k1_perturbed", True, True),
]


@pytest.mark.parametrize("key,fused,parity", GPU_SPATIAL)
def test_gpu_spatial_orders(hip_lib, key, fused, parity):
    stepper, mesh, k, flux, nxs, measured = SPATIAL[key]
    errs = [gpu_errors(stepper, mesh, nx, k, DT_SPATIAL, T_SPATIAL, flux=flux, fused=fused) for nx in nxs]
    print(f"{key}: GPU errors {np.asarray(errs).tolist()} orders {ms.orders(errs).round(3).tolist()}")
    if parity:
        for nx, e in zip(nxs[:2], errs[:2]):
            check_parity(e, ms.oracle_errors(stepper, mesh, nx, k, DT_SPATIAL, T_SPATIAL, flux=flux))
    check_spatial_orders(errs, k, measured)


# periodic square (wrapped tile kernels), GPU only: windows measured on the GPU (T = 1/32, dt = 1/128 extrapolated)
PERIODIC = {
    ("imex_ars2_232", 1): ((8, 16, 32), [[2.49, 2.35], [2.86, 1.85]]),
}


@pytest.mark.parametrize("stepper,k", list(PERIODIC))
def test_gpu_spatial_orders_periodic(hip_lib, stepper, k):
    nxs, measured = PERIODIC[(stepper, k)]
    errs = [gpu_errors(stepper, "periodic", nx, k, DT_SPATIAL, T_SPATIAL) for nx in nxs]
    print(f"periodic {stepper} k={k}: GPU errors {np.asarray(errs).tolist()} orders {ms.orders(errs).round(3).tolist()}")
    check_spatial_orders(errs, k, measured)


# ---------------------------------------------------------------------------------------------------------------------------
# SSP2(3,3,2): beta = sum_{i>=1} b_impl[i] of the fixture
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,nxs", [("square", (4, 8, 16)), ("periodic", (8, 16, 32))])
def test_gpu_ssp2_332_beta(hip_lib, mesh, nxs):
    beta = ms.beta_of(ms.tableau_fixture()["IncompressibleEulerHDGIMEXSSP2_332"])
    T, dt = 1.0 / 32, 1.0 / 256
    e1 = [gpu_errors("imex_ssp2_332", mesh, nx, 1, dt, T, beta=1.0, extrapolate=False)[0] for nx in nxs]
    eb = [gpu_errors("imex_ssp2_332", mesh, nx, 1, dt, T, beta=beta, extrapolate=False)[0] for nx in nxs]
    print(f"SSP2(3,3,2) {mesh}: velocity errors, Euler forcing {e1}, forcing for beta = {beta}: {eb}")
    if mesh == "square":
        for nx, a, b in zip(nxs[:2], e1, eb):
            check_parity([a, b], [ms.oracle_errors("imex_ssp2_332", mesh, nx, 1, dt, T, beta=bt, extrapolate=False)[0]
                                  for bt in (1.0, beta)])
    # Euler forcing: a floor that does not shrink with h; forcing for the derived beta: converges
    assert min(e1) > 0.06 and e1[2] > 0.95 * e1[1], e1
    o = ms.orders(np.stack([eb, eb], -1))[:, 0]
    # measured: square 2.48 / 2.68; periodic 2.60 / 1.66 -- its faster flow shows the first-order time error at nx = 32
    assert o[0] >= 2.0 and o[-1] >= (2.0 if mesh == "square" else 1.4) and eb[2] < 0.02 * e1[2], (eb, o)


# ---------------------------------------------------------------------------------------------------------------------------
# time orders at nx = 8, k = 2 (successive differences of dt-halved runs); ARS3 only on the CPU-stable window
# ---------------------------------------------------------------------------------------------------------------------------
TIME_GPU = {  # T, numbers of steps, measured velocity orders (oracle, same mesh)
    "imex_ssp2_332": (0.25, (4, 8, 16, 32), [1.12, 1.03]),
    "imex_ars2_232": (0.25, (4, 8, 16, 32), [0.96, 0.96]),
    "imex_ssp3_433": (0.25, (4, 8, 16, 32), [1.43, 1.16]),
    "imex_implicit": (0.125, (4, 8, 16, 32), [0.83, 0.93]),
    "imex_ars3_443": (1.0 / 16, (2, 4, 8), [0.11]),
}


@pytest.mark.parametrize("stepper", list(TIME_GPU))
def test_gpu_time_orders(hip_lib, stepper):
    T, nsteps, measured = TIME_GPU[stepper]
    runs = [product_run(stepper, "square", 8, 2, T / n, T) for n in nsteps]
    eng = runs[0][2]._engine
    diffs = [eng.l2_norms(a[0] - b[0], a[1] - b[1]) for a, b in zip(runs[:-1], runs[1:])]
    o = ms.orders(diffs)[:, 0]
    print(f"{stepper}: differences {diffs} velocity orders {o.round(3).tolist()}")
    assert np.all(np.abs(o - measured) <= WINDOW), (o, measured)
    if stepper == "imex_ars3_443":
        sol = ms.solution_for("square")
        errs = [product_errors(ts, sol, Q, p, T)[0] for Q, p, ts in runs]
        assert diffs[1][0] < diffs[0][0] < 2e-3 and max(errs) < 5e-3, (diffs, errs)
