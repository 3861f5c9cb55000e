"""Tracer wall conditions on the GPU (include/hdg_tracer_walls.h) against tests/tracer_walls_reference.py.

Bounds.  The operator hook: relative 1e-10 (section 19's).  Whole steps: 2e-8, the project's whole-step bound.  L2 errors
against the analytic decay: relative 1e-6.  A member of a batch against the same tracer alone: 1e-12 max|q|.  The flux budget:
ten times the residual the numpy reference leaves in the same identity.  Switched off, everything is bitwise what it is
without the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import ctypes as C
import os
import subprocess
import sys
import uuid
import warnings

import numpy as np
import pytest

import tracer_walls_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL, BOUND = 1e-10, 2e-8, 1e-12
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread (TracerBlock<K>, csrc/hdg_cg.hpp)
_OPS = {}


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _mesh_and_operator(kind, nx, k):
    """The package's mesh and the reference's WallOperator of the same triangulation (built once, read-only)."""
    import manufactured as ms
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, TriangleMesh, UnitDiskMesh, UnitSquareMesh
    from oracle import fem
    from oracle import hdg_oracle as orc

    if kind == "square":
        mesh = UnitSquareMesh(nx, nx)
    elif kind == "periodic":
        return PeriodicSquareMesh(nx, nx, L=2 * np.pi), None
    else:
        mesh = UnitDiskMesh(nx) if kind == "disk" else TriangleMesh(*ms.perturbed_square_mesh(nx))
    if (kind, nx, k) not in _OPS:
        d = orc.HDGDiscretisation(nx, k) if kind == "square" else orc.HDGDiscretisation(0, k, mesh=fem.TriMesh(mesh.vertices, mesh.cells))
        _OPS[kind, nx, k] = ref.WallOperator(d, general=kind != "square")
    return mesh, _OPS[kind, nx, k]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _kappa_for(eng, dt, number=0.35):
    """kappa that puts the diffusion number the engine reports (with the walls that are set) at `number`"""
    return number / (dt * eng.tracer_diffusion_number()[0])


FOUR = {"bottom": 1.0, "right": -0.5, "top": 0.25, "left": 2.0}


# ---- 1. the operator hook
@pytest.mark.parametrize("kind,nx,k", [("square", 3, k) for k in (1, 2, 3, 4)] + [("disk", 1, 2), ("perturbed", 3, 1)])
def test_operator_hook_against_the_reference(hip_lib, kind, nx, k):
    mesh, op = _mesh_and_operator(kind, nx, k)
    eng = _stepper("implicit", mesh, k, 0.01)._engine
    X = op.d.node_coords(op.d.PP).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(23 + k)
    smooth = sum(rng.uniform(-1, 1) * np.sin(2 * np.pi * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    fields = {"smooth": smooth, "broken random": rng.standard_normal(len(x))}
    sets = [{"bottom": 0.7}, {"left": -0.3}, {"top": 1.0, "right": 2.0}, FOUR] if kind == "square" else [{"boundary": 0.7}]
    lam0 = eng.tracer_diffusion_number()[0]
    for walls in sets:
        A, b = op.minv(walls)
        for name, q in fields.items():
            want = A @ q + b
            got = eng.apply_tracer_wall_diffusion(q, walls)
            print(f"{kind} k={k} {sorted(walls)} {name}: {_rel(got, want):.3e}")
            assert _rel(got, want) < HOOK, (walls, name)
        assert eng.tracer_walls() is None  # the hook sets nothing
        assert eng.tracer_diffusion_number()[0] == lam0
        eng.set_tracer_walls(walls)
        lam = eng.tracer_diffusion_number()[0]
        eng.set_tracer_walls(None)
        rho = np.max(np.abs(np.linalg.eigvals(A)))
        print(f"  Lambda {lam:.6g} (no walls {lam0:.6g}), rho {rho:.6g}")
        assert rho <= lam <= 4.0 * rho and lam >= lam0
    # the linear profiles against exact zero, and a constant on a general mesh
    if kind == "square":
        steady = [(1.0 - y, {"bottom": 1.0, "top": 0.0}), (x, {"left": 0.0, "right": 1.0})]
    else:
        steady = [(0.0 * x + 0.7, {"boundary": 0.7})]
    for q, walls in steady:
        A, _ = op.minv(walls)
        got = eng.apply_tracer_wall_diffusion(q, walls)
        print(f"{kind} k={k} steady {sorted(walls)}: {np.max(np.abs(got)):.3e} of {np.max(np.abs(A)):.3e}")
        assert np.max(np.abs(got)) < HOOK * np.max(np.abs(A)) * np.max(np.abs(q))
    # all kinds 0: the plain operator, bit for bit
    q = fields["broken random"]
    assert np.array_equal(eng.apply_tracer_wall_diffusion(q, {}), eng.apply_tracer_diffusion(q))


# ---- 2. whole steps against the reference loop
def _q0(x, y):
    return np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y


def _flow(kind, ts, d):
    """Initial state and forcing, for the package and for the oracle."""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from oracle import hdg_oracle as orc

    if kind == "square":
        mp, tg = TaylorGreen(ts._V_Q, ts._V_p), orc.TaylorGreen(d)
        return mp.initial_condition(), mp.f_rhs(), tg.initial_condition(), tg.f_rhs
    Q0 = lambda x, y: (-y * (1 - x * x - y * y), x * (1 - x * x - y * y))
    p0 = lambda x, y: 0 * x
    return (Q0, p0), None, (d.interpolate_velocity(Q0), d.interpolate_pressure(p0)), lambda t: np.zeros((d.mesh.ncells * d.nu, 2))


WALLS_LR = {"left": 0.5, "right": -0.5}


@pytest.mark.parametrize("which,kind,k,nx", [("ssp2", "square", 1, 6), ("ssp2", "square", 2, 4), ("ars2", "square", 2, 4),
                                             ("implicit", "square", 1, 6), ("dg", "square", 1, 6), ("ssp2", "disk", 2, 1)])
def test_whole_steps_against_the_reference_loop(hip_lib, which, kind, k, nx):
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    mesh, op = _mesh_and_operator(kind, nx, k)
    d = op.d
    walls = WALLS_LR if kind == "square" else {"boundary": 0.5}
    nsteps = 3
    dt = 0.25 * d.mesh.h if kind == "square" else 0.02
    tr = TracerOracle(d)
    paths = (False, True) if which in ("ssp2", "ars2") else (None,)
    want = {}
    for fused in paths:
        ts = _stepper(which, mesh, k, dt)
        ts._engine.set_tracer_walls(walls)
        kappa = _kappa_for(ts._engine, dt)
        ts._engine.set_tracer_diffusivity(kappa)
        number = ts._engine.tracer_diffusion_number()[1]
        assert 0.2 <= number <= 0.5, number
        ic, f, oic, of = _flow(kind, ts, d)
        if not want:  # the reference, with and without the walls: once per case
            for key, w in (("walls", walls), ("none", None)):
                tend = op.tendency(tr, w, kappa)
                oq0 = d.interpolate_pressure(_q0)
                if which == "dg":
                    want[key] = ref.dg_with_walls(d, tr, tend, dt, *oic, oq0, of, nsteps)
                elif which == "implicit":
                    want[key] = ref.implicit_with_walls(d, tr, tend, dt, *oic, oq0, of, nsteps * dt)
                else:
                    o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which])
                    want[key] = ref.imex_with_walls(o, tr, tend, *oic, oq0, of, nsteps * dt)
            # a condition on the reference alone: the case sees the walls
            seen = np.max(np.abs(want["walls"][2] - want["none"][2])) / np.max(np.abs(want["none"][2]))
            print(f"{which} {kind} k={k}: kappa {kappa:.4e}, number {number:.3f}, with / without walls differ by {seen:.3e} max|q|")
            assert seen >= 1e-2
        kw = {} if fused is None else {"fused": fused}
        Q, p = ts.solve(*ic, _q0, f, nsteps * dt, **kw)
        oQ, op_, oq = want["walls"]
        errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op_), _rel(ts.q_tracer.dat.data, oq)
        print(f"  fused={fused}: Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
        assert max(errs) < TOL, (fused, errs)


def test_heated_cavity_with_buoyancy_viscosity_and_two_tracers(hip_lib):
    """From rest: tracer 0 between a warm left and a cold right wall drives the flow; tracer 1 has no wall at all and another
    kappa; no-slip viscosity.  Three fused SSP2 steps at (k, nx) = (2, 4) against the reference loop."""
    import viscosity_reference as vref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    k, nx, nsteps = 2, 4, 3
    mesh, op = _mesh_and_operator("square", nx, k)
    d = op.d
    dt = 0.25 * d.mesh.h
    tr = TracerOracle(d)
    walls = [WALLS_LR, {}]
    probe = _stepper("ssp2", mesh, k, dt, n_tracers=2)._engine
    probe.set_tracer_walls(walls)
    kmax = _kappa_for(probe, dt)
    kappa = [kmax, 0.4 * kmax]
    nu = 0.2 / (dt * _visc_lambda(probe))  # viscous diffusion number 0.2
    ts = _stepper("ssp2", mesh, k, dt, n_tracers=2, tracer_walls=walls, tracer_diffusivity=kappa, buoyancy=[1.0, 0.0],
                  viscosity=nu, wall="no_slip")
    assert ts._engine.tracer_walls() == [WALLS_LR, {}]
    q0 = [lambda x, y: 0.2 * np.sin(np.pi * y) * x, _q0]
    zeroQ, zerop = np.zeros((d.mesh.ncells * d.nu, 2)), np.zeros(d.NP)
    oq0 = np.stack([d.interpolate_pressure(f) for f in q0])
    Av = vref.minv_v(d, "no_slip")
    want = {}
    for key, w in (("walls", walls), ("none", None)):
        o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
        want[key] = ref.imex_with_walls(o, tr, op.tendency(tr, w, kappa), zeroQ, zerop, oq0, lambda t: np.zeros_like(zeroQ), nsteps * dt,
                                        beta=[1.0, 0.0], g=(0.0, -1.0), nu=nu, Avisc=Av)
    seen = np.max(np.abs(want["walls"][2][0] - want["none"][2][0])) / np.max(np.abs(want["none"][2][0]))
    seen_Q = np.max(np.abs(want["walls"][0] - want["none"][0])) / np.max(np.abs(want["none"][0]))
    print(f"cavity: kappa {kappa}, nu {nu:.4e}; with / without walls: q differs by {seen:.3e} max|q|, Q by {seen_Q:.3e} max|Q|")
    assert seen >= 1e-2
    Q, p = ts.solve(lambda x, y: (0 * x, 0 * y), lambda x, y: 0 * x, q0, None, nsteps * dt, fused=True)
    oQ, op_, oq = want["walls"]
    got_q = np.stack([f.dat.data for f in ts.q_tracers])
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op_), _rel(got_q[0], oq[0]), _rel(got_q[1], oq[1])
    print(f"  Q {errs[0]:.3e}, p {errs[1]:.3e}, q0 {errs[2]:.3e}, q1 {errs[3]:.3e}")
    assert max(errs) < TOL, errs


def _visc_lambda(eng):
    eng.set_viscosity(1.0, "no_slip")
    lam = eng.viscosity_number()[0]
    eng.set_viscosity(0.0, "no_slip")
    return lam


# ---- 3. manufactured decay between four cold walls
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("nx", [4, 8])
def test_decay_error_equals_the_reference(hip_lib, k, nx):
    """All four sides at 0, q0 = sin pi x sin pi y, zero velocity, forward Euler (the implicit stepper): the L2 error against
    exp(-2 pi^2 kappa T) q0 equals the reference's to a relative 1e-6."""
    from oracle.fem import triangle_quadrature

    mesh, op = _mesh_and_operator("square", nx, k)
    d = op.d
    walls = {s: 0.0 for s in ref.SIDES}
    nsteps, kappa = 40, 1.0
    dt = 0.2 / (nx * nx) / {1: 250.0, 2: 900.0, 3: 2200.0}[k]  # kappa dt rho about 0.2 to 0.4: rho h^2 of section 19, the walls add to it
    q0 = lambda x, y: np.sin(np.pi * x) * np.sin(np.pi * y)
    amp = np.exp(-2 * np.pi ** 2 * kappa * nsteps * dt)

    def l2(q):
        m = d.mesh
        qp, _ = triangle_quadrature(3 * d.k + 4)
        X = m.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,qr->cqd", m.J, qp)
        qh = np.einsum("qa,ca->cq", d.cP, q.reshape(m.ncells, d.np_))
        return float(np.sqrt(np.sum(d.cwdet * (qh - amp * q0(X[..., 0], X[..., 1])) ** 2)))

    q_ref = ref.euler_at_rest(op, walls, kappa, dt, d.interpolate_pressure(q0), nsteps)[-1]
    err_ref = l2(q_ref)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # Lambda is an upper bound
        ts = _stepper("implicit", mesh, k, dt, tracer_walls=walls, tracer_diffusivity=kappa)
    ts.solve(lambda x, y: (0 * x, 0 * y), lambda x, y: 0 * x, q0, None, nsteps * dt)
    err = l2(ts.q_tracer.dat.data)
    print(f"k={k} nx={nx}: L2 error {err:.10e}, reference {err_ref:.10e}, fields differ by {_rel(ts.q_tracer.dat.data, q_ref):.3e}, "
          f"amplitude {amp:.4f}")
    assert abs(err - err_ref) <= 1e-6 * err_ref
    assert err_ref < 0.2 * amp  # the run does decay as the analytic solution does


# ---- 4. the flux budget
def test_flux_budget_between_a_warm_and_a_cold_wall(hip_lib):
    """Zero velocity, bottom 1 / top 0 from q = 0, 12 forward-Euler steps: the change of int q per step is dt times the sum of
    the wall fluxes of the state before the step.  Bound: ten times the residual of the numpy reference in the same identity."""
    k, nx, nsteps = 2, 4, 12
    mesh, op = _mesh_and_operator("square", nx, k)
    d = op.d
    walls = {"bottom": 1.0, "top": 0.0}
    dt = 0.01
    ts = _stepper("implicit", mesh, k, dt)
    eng = ts._engine
    eng.set_tracer_walls(walls)
    kappa = _kappa_for(eng, dt, 0.45)
    eng.set_tracer_diffusivity(kappa)
    # the reference and its own residual
    qs = ref.euler_at_rest(op, walls, kappa, dt, np.zeros(d.NP), nsteps)
    res_ref = max(abs(ref.integral(d, qs[n + 1]) - ref.integral(d, qs[n]) - dt * np.sum(op.flux(walls, kappa, qs[n]))) for n in range(nsteps))
    scale = max(abs(dt * np.sum(op.flux(walls, kappa, q))) for q in qs)
    zero = lambda x, y: (0 * x, 0 * y)
    q = np.zeros(eng.shape_p)
    eng.set_tracer(q)
    res = worst_flux = 0.0
    for n in range(nsteps):
        flux = eng.tracer_wall_flux()
        assert np.array_equal(flux, eng.tracer_wall_flux())  # two calls: the same bits
        want = op.flux(walls, kappa, qs[n])
        worst_flux = max(worst_flux, np.max(np.abs(flux[0] - want)) / np.max(np.abs(want)))
        assert flux[0, 1] == 0.0 and flux[0, 3] == 0.0  # the no-flux sides
        before = eng.integrate_pressure(q)
        ts.solve(zero, lambda x, y: 0 * x, q, None, dt)
        q = ts.q_tracer.dat.data.copy()
        res = max(res, abs(eng.integrate_pressure(q) - before - dt * float(np.sum(flux))))
    print(f"flux budget: device residual {res:.3e}, reference residual {res_ref:.3e} (dt * flux up to {scale:.3e}); "
          f"flux against the reference functional {worst_flux:.3e}; field {_rel(q, qs[-1]):.3e}")
    assert worst_flux <= HOOK
    assert _rel(q, qs[-1]) < TOL
    assert res <= 10.0 * res_ref
    # the steady profile: kappa in through the warm wall, kappa out through the cold one
    eng.set_tracer(ts._V_p.interpolate(lambda x, y: 1.0 - y))
    flux = eng.tracer_wall_flux()[0]
    print(f"steady profile: bottom {float(flux[0])!r}, top {float(flux[2])!r}, kappa {kappa!r}")
    assert abs(flux[0] - kappa) <= HOOK * kappa and abs(flux[2] + kappa) <= HOOK * kappa


# ---- 5. batches
_ALONE = {}
KAPPA_SHARE = lambda m: 0.0 if m == 1 else (m + 2) / 18.0  # distinct, one zero


def _walls_of(m):
    """distinct walls, including none (m = 2) and a fixed side on a tracer without kappa (m = 1)"""
    if m == 2:
        return {}
    sides = [s for i, s in enumerate(ref.SIDES) if (m + 1) >> i & 1 or i == m % 4]
    return {s: 0.3 * (m + 1) - 0.5 * i for i, s in enumerate(sides)}


def _field(m):
    return lambda x, y: np.sin((1.3 + 0.4 * m) * x + 0.2 * m) * np.cos((1.0 + 0.7 * m) * y) + 0.1 * (m + 1) * x


def _batch_run(k, nx, members, kappas, walls, n_tracers=None):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    dt, nsteps = 0.02, 2
    ts = _stepper("ssp2", UnitSquareMesh(nx, nx), k, dt, **({} if n_tracers is None else {"n_tracers": n_tracers}))
    ts._engine.set_tracer_walls(walls)
    ts._engine.set_tracer_diffusivity(kappas)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    q0 = [_field(m) for m in members]
    ts.solve(*mp.initial_condition(), q0 if n_tracers is not None else q0[0], mp.f_rhs(), nsteps * dt, fused=True)
    return np.stack([f_.dat.data.copy() for f_ in ts.q_tracers]), ts


@pytest.mark.parametrize("k,nx,n", [(1, 6, TB[1] + 1), (2, 5, TB[2] + 1), (3, 4, TB[3] + 1), (2, 5, 16)])
def test_a_batch_with_distinct_walls_equals_its_members(hip_lib, k, nx, n):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    walls = [_walls_of(m) for m in range(n)]
    probe = _stepper("ssp2", UnitSquareMesh(nx, nx), k, 0.02, n_tracers=n)._engine
    probe.set_tracer_walls(walls)
    kmax = _kappa_for(probe, 0.02, 0.45)
    top = max(KAPPA_SHARE(m) for m in range(n))
    kappas = [kmax * KAPPA_SHARE(m) / top for m in range(n)]
    assert len(set(kappas)) == n and kappas.count(0.0) == 1 and walls.count({}) == 1 and walls[1]
    batch, ts = _batch_run(k, nx, tuple(range(n)), kappas, walls, n_tracers=n)
    assert 0.2 <= ts._engine.tracer_diffusion_number()[1] <= 0.5
    worst = 0.0
    for m in range(n):
        key = (k, nx, m, kappas[m])
        if key not in _ALONE:
            _ALONE[key] = _batch_run(k, nx, (m,), kappas[m], walls[m])[0][0]
            _ALONE[key].setflags(write=False)
        alone = _ALONE[key]
        diff = np.max(np.abs(batch[m] - alone)) / np.max(np.abs(alone))
        worst = max(worst, diff)
        assert diff <= BOUND, (m, diff)
    # the comparison is not vacuous: the same tracer without its walls differs far beyond the bound
    plain = _batch_run(k, nx, (0,), kappas[0], None)[0][0]
    assert _rel(batch[0], plain) > 1e-4
    print(f"k={k} n={n}: largest |batch - alone| = {worst:.3e} max|q|")


# ---- 6. nothing changes when it is off; nothing is launched more when it is on
def _three_steps(mode, kappa, walls=WALLS_LR):
    """Fields, iteration counts, launch census, digest and checkpoint blob after three fused steps with one tracer."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_tracer(ts._V_p.interpolate(_q0))
    if kappa:
        eng.set_tracer_diffusivity(kappa)
    if mode == "zeros":
        eng.set_tracer_walls({})
    elif mode == "on_then_zeros":
        eng.set_tracer_walls(walls)
        eng.set_tracer_walls([{}])
    elif mode == "on_then_none":
        eng.set_tracer_walls(walls)
        eng.set_tracer_walls(None)
    elif mode == "on":
        eng.set_tracer_walls(walls)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, q=eng.get_tracer(), its=eng.iteration_stats(), digest=eng.state_digest(),
                blob=bytes(eng.save_checkpoint(3, 0.06)), ts=ts)


@pytest.mark.parametrize("with_kappa", [True, False])
def test_switched_off_nothing_changes_and_switched_on_nothing_is_launched_more(hip_lib, with_kappa):
    probe = _three_steps("unset", None)
    kappa = _kappa_for(probe["ts"]._engine, 0.02) if with_kappa else None
    base = _three_steps("unset", kappa)
    for mode in ("zeros", "on_then_zeros", "on_then_none"):
        r = _three_steps(mode, kappa)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p", "q"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"], mode
        assert r["blob"] == base["blob"], mode
    on = _three_steps("on", kappa)
    assert on["census"] == base["census"]  # the walls add no launch in any class: the other form runs instead
    assert np.array_equal(on["Q"], base["Q"]) and np.array_equal(on["p"], base["p"])  # a passive tracer: the flow does not see it
    if with_kappa:
        assert _rel(on["q"], base["q"]) > 1e-3
        assert b"tracer_wall[0][1]" in on["blob"] and b"tracer_wall[0][3]" in on["blob"] and b"tracer_wall[0][0]" not in on["blob"]
    else:
        assert np.array_equal(on["q"], base["q"])  # walls without kappa do nothing
    assert b"tracer_wall" not in base["blob"]


# ---- 7. checkpoint
def _ck_engine(walls, kappa):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, n_tracers=2)
    eng = ts._engine
    if walls is not None:
        eng.set_tracer_walls(walls)
    eng.set_tracer_diffusivity(kappa)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    return ts, eng, ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0)


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_the_walls(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    walls = [{"bottom": 1.0, "left": -0.5}, {"top": 0.25}]
    probe = _ck_engine(walls, 0.0)[1]
    kmax = _kappa_for(probe, 0.02)
    kappa = [kmax, 0.5 * kmax]
    ts, eng, Q0, p0 = _ck_engine(walls, kappa)
    eng.set_state(Q0, p0)
    eng.reconstruct_trace()
    eng.set_tracer(np.stack([ts._V_p.interpolate(_field(m)) for m in range(2)]))
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"tracer_wall[0][0]" in blob and b"tracer_wall[0][3]" in blob and b"tracer_wall[1][2]" in blob and b"tracer_wall[1][0]" not in blob
    for n in range(2):
        eng.step()
    ts2, eng2, _, _ = _ck_engine(walls, kappa)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    assert np.array_equal(eng2.get_tracer(), eng.get_tracer())
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for other in ([{"bottom": 1.0, "left": -0.25}, {"top": 0.25}], [{"bottom": 1.0}, {"top": 0.25}], [{}, {}], None):
        _, eng3, _, _ = _ck_engine(other, kappa)
        with pytest.raises(_lib.HDGError, match="tracer_wall|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


# ---- 8. errors
def _raw_set(eng, n, kind, value):
    kind = np.ascontiguousarray(kind, dtype=np.int32)
    value = np.ascontiguousarray(value, dtype=np.float64)
    return eng.lib.hdg_set_tracer_walls(eng.h, n, kind.ctypes.data_as(C.POINTER(C.c_int)), value.ctypes.data_as(C.POINTER(C.c_double)))


def test_errors_leave_the_setting_and_the_fields(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, n_tracers=3)
    eng = ts._engine
    good = [{"bottom": 1.0}, {}, {"left": 2.0, "top": 3.0}]
    eng.set_tracer_walls(good)
    eng.set_tracer_diffusivity([1e-3, 0.0, 2e-3])
    eng.set_state(np.zeros(eng.shape_Q), np.zeros(eng.shape_p))
    rng = np.random.default_rng(3)
    q = rng.standard_normal(eng.shape_q)
    eng.set_tracer(q)
    q = eng.get_tracer()  # as the engine holds it (nodal -> modal -> nodal)
    flux = eng.tracer_wall_flux()
    lam = eng.tracer_diffusion_number()

    def unchanged():
        assert eng.tracer_walls() == good
        assert np.array_equal(eng.tracer_wall_flux(), flux) and eng.tracer_diffusion_number() == lam
        assert np.array_equal(eng.get_tracer(), q)

    msg = lambda: eng.lib.hdg_last_error(eng.h).decode()
    for n in (2, 4):  # wrong n
        assert _raw_set(eng, n, np.ones((n, 4)), np.zeros((n, 4))) == -1 and f"{n} row(s) for 3 tracer" in msg()
        unchanged()
    kind = np.zeros((3, 4), dtype=np.int32)
    kind[1, 2] = 2  # a bad kind
    assert _raw_set(eng, 3, kind, np.zeros((3, 4))) == -1 and "tracer 1, side 2 (top)" in msg() and "kind 2" in msg()
    unchanged()
    kind[1, 2] = -1
    assert _raw_set(eng, 3, kind, np.zeros((3, 4))) == -1
    unchanged()
    for x in (float("nan"), float("inf"), float("-inf")):  # not finite on a fixed side: tracer and side are named
        with pytest.raises(_lib.HDGError, match=r"tracer 2, side 1 \(right\).*not finite") as e:
            eng.set_tracer_walls([{}, {}, {"right": x}])
        assert e.value.code == -1
        unchanged()
    value = np.full((3, 4), float("nan"))  # ... but a value on a no-flux side is never read
    value[0, 0], value[2, 2], value[2, 3] = 1.0, 3.0, 2.0
    assert _raw_set(eng, 3, np.array([[1, 0, 0, 0], [0, 0, 0, 0], [0, 0, 1, 1]]), value) == 0  # the same setting as `good`
    unchanged()
    with pytest.raises(_lib.HDGError, match="not finite"):
        eng.apply_tracer_wall_diffusion(np.zeros(eng.shape_p), {"top": float("nan")})
    unchanged()
    # the flux needs a tracer
    eng.set_tracer(None)
    with pytest.raises(_lib.HDGError, match="no tracer is set") as e:
        eng.tracer_wall_flux()
    assert e.value.code == -1
    assert eng.tracer_walls() == good  # independent of the tracers being on
    eng.set_tracer(q)
    q = eng.get_tracer()
    unchanged()
    # while a step is open
    eng.tracer_begin_step()
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.set_tracer_walls(None)
    assert e.value.code == -1 and eng.tracer_walls() == good
    # the periodic square has no walls
    per = _stepper("ssp2", PeriodicSquareMesh(4, 4, L=2 * np.pi), 1, 0.02)._engine
    with pytest.raises(_lib.HDGError, match="periodic square has no walls") as e:
        per.set_tracer_walls({"bottom": 1.0})
    assert e.value.code == -1 and per.tracer_walls() is None
    per.set_tracer_walls({})  # no fixed side: fine
    # a general mesh has one side
    disk = _stepper("implicit", UnitDiskMesh(1), 2, 0.02)._engine
    for w in (1, 2, 3):
        kind = np.zeros((1, 4), dtype=np.int32)
        kind[0, w] = 1
        assert _raw_set(disk, 1, kind, np.zeros((1, 4))) == -1 and "whole boundary, at index 0" in disk.lib.hdg_last_error(disk.h).decode()
    disk.set_tracer_walls({"boundary": 1.0})
    assert disk.tracer_walls() == [{"boundary": 1.0}]


def test_the_stepper_warns_for_walls_without_kappa(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    mesh = UnitSquareMesh(4, 4)
    with pytest.warns(RuntimeWarning, match="the walls do nothing"):
        ts = _stepper("ssp2", mesh, 1, 0.02, tracer_walls={"left": 1.0})
    assert ts._engine.tracer_walls() == [{"left": 1.0}]
    lam0 = _stepper("ssp2", mesh, 1, 0.02)._engine.tracer_diffusion_number()[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ts = _stepper("ssp2", mesh, 1, 0.02, tracer_walls={"left": 1.0}, tracer_diffusivity=1e-3)
        assert _stepper("ssp2", mesh, 1, 0.02)._engine.tracer_walls() is None  # tracer_walls=None: no call at all
    lam = ts._engine.tracer_diffusion_number()[0]
    assert lam >= lam0  # the bound counts the wall blocks; on this mesh the interior rows stay the largest
    with pytest.warns(RuntimeWarning, match="exceeds the stability limit 4.52"):
        _stepper("ssp2", mesh, 1, 0.02, tracer_walls={"left": 1.0}, tracer_diffusivity=5.0 / (0.02 * lam))


def test_a_strip_keeps_its_tracer_error(hip_lib, tmp_path):
    token = "/hdg_tw_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "tracer_walls_strip_worker.py"), str(r), "2", token, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0].decode(errors="replace"))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    assert [pr.returncode for pr in procs] == [0, 0], logs
    for o in outs:
        d = np.load(o)
        assert int(d["code"]) == -1 and "single rank" in str(d["msg"]), (d["code"], d["msg"])
        assert str(d["msg"]) == str(d["tracer_msg"])


# ---- 9. the driver
def test_driver_runs_a_heated_cavity(hip_lib, tmp_path):
    """--problem cavity with the heated-cavity flags at nx = 8: the printed lines, and the final wall flux against the
    reference loop's."""
    import viscosity_reference as vref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    k, nx, dt, nsteps, kappa, nu = 1, 8, 0.01, 3, 0.02, 0.01
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "cavity", "--nx", str(nx), "--degree", str(k),
                        "--dt", repr(dt), "--tfinal", repr(nsteps * dt), "--use_projection_method", "--tracer_advection",
                        "--tracer_diffusivity", repr(kappa), "--viscosity", repr(nu), "--wall", "no_slip", "--buoyancy", "1",
                        "--tracer_wall", "left", "0.5", "--tracer_wall", "right", "-0.5", "--output", ""],
                       cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "model problem = cavity" in r.stdout
    assert "tracer wall = tracer 0: right -0.5, left 0.5" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("tracer wall flux = tracer 0: ")]
    assert len(line) == 1, r.stdout
    got = dict((w.split()[0], float(w.split()[1])) for w in line[0].split(": ", 1)[1].split(", "))
    assert list(got) == list(ref.SIDES) and got["bottom"] == 0.0 and got["top"] == 0.0
    _, op = _mesh_and_operator("square", nx, k)
    d = op.d
    tr = TracerOracle(d)
    o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
    zeroQ = np.zeros((d.mesh.ncells * d.nu, 2))
    _, _, q = ref.imex_with_walls(o, tr, op.tendency(tr, WALLS_LR, kappa), zeroQ, np.zeros(d.NP), np.zeros(d.NP), lambda t: np.zeros_like(zeroQ),
                                  nsteps * dt, beta=1.0, g=(0.0, -1.0), nu=nu, Avisc=vref.minv_v(d, "no_slip"))
    want = op.flux(WALLS_LR, kappa, q)
    print(f"driver: wall flux {got}, reference {want}")
    assert got["left"] > 0.0 > got["right"]  # heat enters at the warm wall and leaves at the cold one
    for w, side in enumerate(ref.SIDES):
        assert abs(got[side] - want[w]) <= TOL * np.max(np.abs(want))
