"""The CPU checker of the implicit DG discretisation (tests/dg_reference.py; reference src/timesteppers/dg_implicit.py) and the
parts of the DG surface that need no GPU: the operator identities the engine relies on, convergence of the discretisation on
the Taylor-Green vortex, the class and the driver's argument checks (src/driver.py:203-213)."""
import numpy as np
import pytest

from dg_reference import avg_trace, dg_matrix, dg_solve


def _tg_error(nx, k, dt, nsteps):
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k)
    tg = orc.TaylorGreen(d)
    Q, p = dg_solve(d, *tg.initial_condition(), tg.f_rhs, dt, nsteps)
    Qe, _ = tg.solution(nsteps * dt)
    return d.l2_norm_velocity(Q - Qe)


def test_taylor_green_one_step_converges_with_h():
    # at nx = 32 the first-order time error (dt = 0.04) starts to dominate
    errs = [_tg_error(nx, 1, 0.04, 1) for nx in (8, 16, 32)]
    assert errs[0] > 3 * errs[1] > 3 * errs[2], errs
    assert errs[2] < 2e-4, errs


def test_taylor_green_short_run_converges_with_h():
    errs = [_tg_error(nx, 1, 0.04, 5) for nx in (8, 16)]
    assert errs[1] < 0.6 * errs[0], errs


def test_continuity_rows_are_the_averaged_flux_form():
    """psi div v dx - 2 avg(v.n) avg(psi) dS - v.n psi ds (dg_implicit.py:67-71), assembled here facet by facet, equals the
    engine's weak divergence Wdiv (hdg_imex.py:353-365) on a random field."""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(6, 2)
    m = d.mesh
    v = np.random.default_rng(3).standard_normal((d.NQ // 2, 2))
    vc = v.reshape(m.ncells, d.nu, 2)
    out = d.Bdiv @ v.ravel()
    e = d.eint
    cp, cm, n = m.edge_plus[e], m.edge_minus[e], m.edge_normal_plus[e]
    Up, Pp, _, wl = d.edge_tab(e, cp, d.eq_exact)
    Um, Pm, _, _ = d.edge_tab(e, cm, d.eq_exact)
    vnp = np.einsum("mqa,mad,md->mq", Up, vc[cp], n)  # v+ . n+
    vnm = np.einsum("mqa,mad,md->mq", Um, vc[cm], -n)  # v- . n-
    avg_vn = 0.5 * (vnp + vnm)
    # -2 avg(v.n) avg(psi): avg(psi) = (psi+ + psi-) / 2
    np.add.at(out, d.dofP[cp], -np.einsum("mq,mq,mqa->ma", wl, avg_vn, Pp))
    np.add.at(out, d.dofP[cm], -np.einsum("mq,mq,mqa->ma", wl, avg_vn, Pm))
    e = d.ebnd
    c, n = m.edge_plus[e], m.edge_normal_plus[e]
    Ub, Pb, _, wl = d.edge_tab(e, c, d.eq_exact)
    np.add.at(out, d.dofP[c], -np.einsum("mq,mq,mqa->ma", wl, np.einsum("mqa,mad,md->mq", Ub, vc[c], n), Pb))
    ref = d.Wdiv @ v.ravel()
    assert np.max(np.abs(out - ref)) < 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("periodic", [False, True])
def test_pressure_terms_are_the_hdg_gradient_with_the_averaged_trace(periodic):
    """-dt B^T phi of the momentum rows = -dt g(w; phi, lambda) with lambda = avg(phi) (boundary: phi) -- the identity the
    engine's DG operator is built on (pgrad with the averaged trace)."""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(5, 2, periodic=periodic, L=2 * np.pi if periodic else 1.0)
    phi = np.random.default_rng(4).standard_normal(d.NP)
    g = d.G_p @ phi + d.G_l @ avg_trace(d, phi)
    ref = d.Wdiv.T @ phi
    assert np.max(np.abs(g - ref)) < 1e-12 * np.max(np.abs(ref))


@pytest.mark.parametrize("periodic", [False, True])
def test_constants_are_the_null_space(periodic):
    """Wdiv^T 1 = 0: phi = const is in the right null space and the continuity rows sum to zero."""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(6, 1, periodic=periodic, L=2 * np.pi if periodic else 1.0)
    assert np.max(np.abs(d.Wdiv.T @ np.ones(d.NP))) < 1e-12
    K = dg_matrix(d, d.project_bdm(np.random.default_rng(5).standard_normal((d.NQ // 2, 2))), 0.04)
    assert np.max(np.abs(K @ np.concatenate([np.zeros(d.NQ), np.ones(d.NP)]))) < 1e-12
    assert np.max(np.abs(np.concatenate([np.zeros(d.NQ), np.ones(d.NP)]) @ K)) < 1e-12


def test_dg_class_is_exported():
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEuler, IncompressibleEulerDGImplicit

    assert issubclass(IncompressibleEulerDGImplicit, IncompressibleEuler)


@pytest.mark.parametrize("argv,exc,match", [
    (["--discretisation", "dg", "--timestepper", "implicit", "--use_projection_method"], AssertionError, "projection method"),
    (["--discretisation", "dg", "--timestepper", "imex_ssp2_332"], RuntimeError, "Invalid timestepping method for DG discretisation"),
    (["--discretisation", "conforming", "--timestepper", "implicit"], RuntimeError, "out of scope"),
])
def test_driver_argument_checks(argv, exc, match):
    """driver.py:203-213: these fail before any engine is built."""
    from incompressibleeulerhdg_amd import driver

    with pytest.raises(exc, match=match):
        driver.main(argv + ["--output", ""])
