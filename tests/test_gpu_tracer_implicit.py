"""Implicit tracer diffusion on the GPU (include/hdg_tracer_implicit.h) against
tests/tracer_implicit_reference.py.

Bounds.  The solve hook against the dense solve: 1e-9 max|x| at rtol 1e-12 (the CG error is at most about cond(A) rtol, and
cond(A) <= 1 + tau rho <= 5001 here).  Iteration counts at rtol 1e-10: the reference CG's plus 10 % plus 2.  Whole steps: 2e-8,
the project's whole-step bound.  Batches, restarts and the switched-off engine: bitwise.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import tracer_implicit_reference as ref
import tracer_walls_reference as twr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOOK, TOL = 1e-9, 2e-8
L_PER = 2 * np.pi
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread (TracerBlock<K>, csrc/hdg_cg.hpp)
WALLS_LR = {"left": 0.5, "right": -0.5}
NUMBERS = (0.5, 50.0, 5000.0)
_OPS, _RHO = {}, {}


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _mesh_and_operator(kind, nx, k):
    """The package's mesh and the reference's WallOperator of the same triangulation (built once, read-only)."""
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from oracle import hdg_oracle as orc

    if (kind, nx, k) not in _OPS:
        d = orc.HDGDiscretisation(nx, k, periodic=True, L=L_PER) if kind == "periodic" else orc.HDGDiscretisation(nx, k)
        _OPS[kind, nx, k] = twr.WallOperator(d)
    return (PeriodicSquareMesh(nx, nx, L=L_PER) if kind == "periodic" else UnitSquareMesh(nx, nx)), _OPS[kind, nx, k]


def _rho(kind, nx, k, walls):
    key = (kind, nx, k, tuple(sorted((walls or {}).items())))
    if key not in _RHO:
        _RHO[key] = ref.rho(_OPS[kind, nx, k], walls)
    return _RHO[key]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _fields(op, kind, k):
    X = op.d.node_coords(op.d.PP).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(41 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    return np.stack([smooth, rng.standard_normal(len(x)), x + 2.0 * y - 0.5 * x * y])  # smooth, broken random, a jump across the seam


HOOK_CASES = [("square", 3, None), ("square", 3, WALLS_LR), ("periodic", 4, None)]


# ---- 1. the solve hook against the dense solve
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind,nx,walls", HOOK_CASES, ids=["noflux", "walls", "periodic"])
def test_solve_hook_against_the_dense_solve(hip_lib, kind, nx, walls, k):
    mesh, op = _mesh_and_operator(kind, nx, k)
    eng = _stepper("implicit", mesh, k, 0.01, n_tracers=3)._engine
    if walls:
        eng.set_tracer_walls(walls)
    eng.set_tracer_diffusion_mode("explicit", rtol=1e-12)  # the hook solves in either mode, to the rtol that is set
    q = _fields(op, kind, k)
    rho = _rho(kind, nx, k, walls)
    worst = 0.0
    for number in NUMBERS:
        tau = number / rho
        got, its = eng.solve_tracer_diffusion([tau] * 3, q)
        for t, name in enumerate(("smooth", "broken random", "jump across the seam")):
            want = ref.solve_dense(op, walls, tau, q[t])
            err = _rel(got[t], want)
            worst = max(worst, err)
            print(f"{kind} walls={bool(walls)} k={k} number {number:g} {name}: {its[t]} iterations, {err:.3e} max|x|")
            assert err <= HOOK, (number, name)
        assert np.array_equal(eng.tracer_diffusion_solve()[0], its)
        assert np.all(eng.tracer_diffusion_solve()[1] <= 1e-12)
    # tau = 0: that field is neither read nor written, and counts no iteration
    got, its = eng.solve_tracer_diffusion([0.0, 5.0 / rho, 0.0], q)
    same, none = eng.solve_tracer_diffusion([0.0, 0.0, 0.0], q)  # the hook's own way in and out (nodal -> modal -> nodal), no solve
    assert not none.any() and _rel(same, q) < 1e-13
    assert np.array_equal(got[0], same[0]) and np.array_equal(got[2], same[2]) and its[0] == 0 and its[2] == 0 and its[1] > 0
    print(f"{kind} walls={bool(walls)} k={k}: largest error {worst:.3e} max|x|")


# ---- 2. iteration counts
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind,nx,walls", HOOK_CASES, ids=["noflux", "walls", "periodic"])
def test_iteration_counts_are_those_of_plain_cg(hip_lib, kind, nx, walls, k):
    mesh, op = _mesh_and_operator(kind, nx, k)
    eng = _stepper("implicit", mesh, k, 0.01, n_tracers=3)._engine
    if walls:
        eng.set_tracer_walls(walls)
    eng.set_tracer_diffusion_mode("explicit", rtol=1e-10)
    q = _fields(op, kind, k)
    rho = _rho(kind, nx, k, walls)
    for number in NUMBERS:
        tau = number / rho
        _, its = eng.solve_tracer_diffusion([tau] * 3, q)
        want = [ref.cg(op, walls, tau, q[t], rtol=1e-10)[1] for t in range(3)]
        print(f"{kind} walls={bool(walls)} k={k} number {number:g}: device {its.tolist()}, reference CG {want}")
        for t in range(3):
            assert its[t] <= want[t] + 0.1 * want[t] + 2, (number, t)
            assert its[t] > 0


# ---- 3. whole steps against the reference loop
def _q0(kind):
    if kind == "periodic":
        return lambda x, y: np.sin(x) * np.sin(y) + 0.5 * np.cos(3 * x + y)
    return lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y


def _flow(kind, ts, d):
    """Initial state and forcing, for the package and for the oracle."""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from oracle import hdg_oracle as orc

    if kind == "square":
        mp, tg = TaylorGreen(ts._V_Q, ts._V_p), orc.TaylorGreen(d)
        return mp.initial_condition(), mp.f_rhs(), tg.initial_condition(), tg.f_rhs
    Q0 = lambda x, y: (np.where(y <= np.pi, np.tanh((y - np.pi / 2) / (np.pi / 15)), np.tanh((1.5 * np.pi - y) / (np.pi / 15))), 0.05 * np.sin(x))
    p0 = lambda x, y: 0.015 * np.cos(x) * np.sin(y - np.pi)
    f = lambda t: (lambda x, y: (0.1 * np.cos(y) * np.cos(t), 0.2 * np.sin(x + y)))
    return (Q0, p0), f, (d.interpolate_velocity(Q0), d.interpolate_pressure(p0)), lambda t: d.interpolate_velocity(f(t))


@pytest.mark.parametrize("which,kind,k,nx", [("ssp2", "square", 1, 6), ("ssp2", "square", 2, 4), ("ars2", "square", 2, 4),
                                             ("implicit", "square", 1, 6), ("dg", "square", 1, 6), ("ssp2", "periodic", 1, 6)])
def test_whole_steps_against_the_reference_loop(hip_lib, which, kind, k, nx):
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    mesh, op = _mesh_and_operator(kind, nx, k)
    d = op.d
    nsteps = 3
    dt = 0.25 * d.mesh.h
    kappa = 50.0 / (dt * _rho(kind, nx, k, None))  # diffusion number 50: eleven times the explicit limit of SSP2(3,3,2)
    tr = TracerOracle(d)
    q0 = _q0(kind)
    tend = op.tendency(tr, None, 0.0)  # transport alone
    paths = (False, True) if which in ("ssp2", "ars2") else (None,)
    want = {}
    for fused in paths:
        ts = _stepper(which, mesh, k, dt, tracer_diffusivity=kappa, tracer_diffusion="implicit")
        assert ts._engine.tracer_diffusion_mode() == "implicit"
        ic, f, oic, of = _flow(kind, ts, d)
        if not want:  # the reference, with and without the term: once per case
            for key, fin in (("on", ref.finish(op, None, kappa, dt)), ("off", lambda q: q)):
                oq0 = d.interpolate_pressure(q0)
                if which == "dg":
                    want[key] = ref.dg_split(d, tr, tend, fin, dt, *oic, oq0, of, nsteps)
                elif which == "implicit":
                    want[key] = ref.implicit_split(d, tr, tend, fin, dt, *oic, oq0, of, nsteps * dt)
                else:
                    o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which])
                    want[key] = ref.imex_split(o, tr, tend, fin, *oic, oq0, of, nsteps * dt)
            seen = np.max(np.abs(want["on"][2] - want["off"][2])) / np.max(np.abs(want["off"][2]))
            print(f"{which} {kind} k={k}: kappa {kappa:.4e}, with / without the term differ by {seen:.3e} max|q|")
            assert seen >= 1e-2
        kw = {} if fused is None else {"fused": fused}
        Q, p = ts.solve(*ic, q0, f, nsteps * dt, **kw)
        oQ, op_, oq = want["on"]
        errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op_), _rel(ts.q_tracer.dat.data, oq)
        its = np.asarray(ts.tracer_diffusion_iterations)
        print(f"  fused={fused}: Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}; iterations per step {its.ravel().tolist()}")
        assert max(errs) < TOL, (fused, errs)
        assert its.shape == (nsteps, 1) and np.all(its > 0)


def test_heated_cavity_with_buoyancy_walls_and_viscosity(hip_lib):
    """From rest: tracer 0 between a warm left and a cold right wall drives the flow, tracer 1 has no wall and kappa = 0;
    no-slip viscosity.  Three fused SSP2 steps at (k, nx) = (2, 4): the buoyancy reads the undiffused stage tracers."""
    import viscosity_reference as vref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    k, nx, nsteps = 2, 4, 3
    mesh, op = _mesh_and_operator("square", nx, k)
    d = op.d
    dt = 0.25 * d.mesh.h
    tr = TracerOracle(d)
    walls = [WALLS_LR, {}]
    kappa = [50.0 / (dt * _rho("square", nx, k, WALLS_LR)), 0.0]
    probe = _stepper("ssp2", mesh, k, dt, n_tracers=2)._engine
    probe.set_viscosity(1.0, "no_slip")
    nu = 0.2 / (dt * probe.viscosity_number()[0])  # viscous diffusion number 0.2
    ts = _stepper("ssp2", mesh, k, dt, n_tracers=2, tracer_walls=walls, tracer_diffusivity=kappa, tracer_diffusion="implicit",
                  buoyancy=[1.0, 0.0], viscosity=nu, wall="no_slip")
    q0 = [lambda x, y: 0.2 * np.sin(np.pi * y) * x, _q0("square")]
    zeroQ, zerop = np.zeros((d.mesh.ncells * d.nu, 2)), np.zeros(d.NP)
    oq0 = np.stack([d.interpolate_pressure(f) for f in q0])
    Av = vref.minv_v(d, "no_slip")
    tend = op.tendency(tr, None, 0.0)
    want = {}
    for key, fin in (("on", ref.finish(op, walls, kappa, dt)), ("off", lambda q: q)):
        o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
        want[key] = ref.imex_split(o, tr, tend, fin, zeroQ, zerop, oq0, lambda t: np.zeros_like(zeroQ), nsteps * dt,
                                   beta=[1.0, 0.0], g=(0.0, -1.0), nu=nu, Avisc=Av)
    seen = np.max(np.abs(want["on"][2][0] - want["off"][2][0])) / np.max(np.abs(want["off"][2][0]))
    seen_Q = np.max(np.abs(want["on"][0] - want["off"][0])) / np.max(np.abs(want["off"][0]))
    print(f"cavity: kappa {kappa}, nu {nu:.4e}; with / without the term: q differs by {seen:.3e} max|q|, Q by {seen_Q:.3e} max|Q|")
    assert seen >= 1e-2
    Q, p = ts.solve(lambda x, y: (0 * x, 0 * y), lambda x, y: 0 * x, q0, None, nsteps * dt, fused=True)
    oQ, op_, oq = want["on"]
    got_q = np.stack([f.dat.data for f in ts.q_tracers])
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op_), _rel(got_q[0], oq[0]), _rel(got_q[1], oq[1])
    print(f"  Q {errs[0]:.3e}, p {errs[1]:.3e}, q0 {errs[2]:.3e}, q1 {errs[3]:.3e}")
    assert max(errs) < TOL, errs
    its = np.asarray(ts.tracer_diffusion_iterations)
    assert np.all(its[:, 0] > 0) and not np.any(its[:, 1])


# ---- 4. batches
_ALONE = {}
SHARE = lambda m: 0.0 if m == 1 else (m + 2) / 18.0  # distinct, one zero


def _field(m):
    return lambda x, y: np.sin((1.3 + 0.4 * m) * x + 0.2 * m) * np.cos((1.0 + 0.7 * m) * y) + 0.1 * (m + 1) * x


def _batch_run(k, nx, members, kappas, mode="implicit"):
    """Two fused steps; returns the tracers, (Q, p), the velocity iteration statistics and the solve's iteration counts."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    dt, nsteps = 0.02, 2
    n = len(members)
    ts = _stepper("ssp2", UnitSquareMesh(nx, nx), k, dt, **({} if n == 1 else {"n_tracers": n}))
    eng = ts._engine
    if kappas is not None:
        eng.set_tracer_diffusivity(kappas)
        eng.set_tracer_diffusion_mode(mode)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    q0 = [_field(m) for m in members]
    Q, p = ts.solve(*mp.initial_condition(), q0 if n > 1 else q0[0], mp.f_rhs(), nsteps * dt, fused=True)
    return (np.stack([f_.dat.data.copy() for f_ in ts.q_tracers]), (Q.dat.data.copy(), p.dat.data.copy()), eng.iteration_stats(),
            eng.tracer_diffusion_solve()[0].copy())


@pytest.mark.parametrize("k,nx,n", [(1, 6, TB[1] + 1), (2, 5, TB[2] + 1), (3, 4, TB[3] + 1), (1, 6, 16)])
def test_a_batch_member_is_bitwise_the_same_tracer_alone(hip_lib, k, nx, n):
    _, op = _mesh_and_operator("square", nx, k)
    kmax = 50.0 / (0.02 * _rho("square", nx, k, None))
    top = max(SHARE(m) for m in range(n))
    kappas = [kmax * SHARE(m) / top for m in range(n)]
    assert len(set(kappas)) == n and kappas.count(0.0) == 1
    batch, flow, stats, its = _batch_run(k, nx, tuple(range(n)), kappas)
    plain, flow0, stats0, _ = _batch_run(k, nx, tuple(range(n)), None)  # the engine without any diffusion
    for m in range(n):
        key = (k, nx, m, kappas[m])
        if key not in _ALONE:
            _ALONE[key] = _batch_run(k, nx, (m,), kappas[m])
        alone, _, _, its1 = _ALONE[key]
        assert np.array_equal(batch[m], alone[0]), m
        assert its[m] == its1[0], m
        if kappas[m] == 0.0:
            assert np.array_equal(batch[m], plain[m]) and its[m] == 0
        else:
            assert _rel(batch[m], plain[m]) > 1e-3 and its[m] > 0  # not vacuous: the term is seen
    # passive tracers: the flow and its solvers do not see the term
    assert np.array_equal(flow[0], flow0[0]) and np.array_equal(flow[1], flow0[1])
    assert all(np.array_equal(a, b) for a, b in zip(stats, stats0))
    print(f"k={k} n={n}: iterations {its.tolist()}")


# ---- 5. off is off; the census of the implicit mode
def _three_steps(mode, kappa, rtol=1e-10, maxit=2000):
    """Fields, iteration counts, launch census, digest and checkpoint blob after three fused steps with one tracer."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_tracer(ts._V_p.interpolate(_q0("square")))
    if kappa:
        eng.set_tracer_diffusivity(kappa)
    if mode == "explicit":
        eng.set_tracer_diffusion_mode("explicit")
    elif mode == "implicit_then_explicit":
        eng.set_tracer_diffusion_mode("implicit", rtol=1e-6, max_iterations=7)
        eng.set_tracer_diffusion_mode("explicit")
    elif mode == "implicit":
        eng.set_tracer_diffusion_mode("implicit", rtol=rtol, max_iterations=maxit)
    census, its = [], []
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
        census.append({c: v[0] for c, v in eng.launch_stats(reset=True).items()})
        its.append(int(eng.tracer_diffusion_solve()[0][0]))
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, q=eng.get_tracer(), its=eng.iteration_stats(), digest=eng.state_digest(),
                blob=bytes(eng.save_checkpoint(3, 0.06)), ts=ts, solve_its=its)


def test_off_is_off(hip_lib):
    probe = _three_steps("unset", None)
    kappa = 0.35 / (0.02 * probe["ts"]._engine.tracer_diffusion_number()[0])  # inside the explicit limit
    base = _three_steps("unset", kappa)
    for mode in ("explicit", "implicit_then_explicit"):
        r = _three_steps(mode, kappa)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p", "q"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"] and r["blob"] == base["blob"], mode
        assert r["solve_its"] == [0, 0, 0]
    assert b"tracer_diffusion_mode" not in base["blob"]
    assert _rel(base["q"], probe["q"]) > 1e-3  # the explicit term is there


def test_implicit_census(hip_lib):
    """No k_tracer_diff launch; the launches of the solve are all in `other`: 1 (start) + 3 per pass + 1 (the last check, when
    the passes run out before the host has seen every tracer stop) + 1 (accept), passes = min(iterations + 2, max_iterations)."""
    probe = _three_steps("unset", None)
    kappa = 50.0 / (0.02 * probe["ts"]._engine.tracer_diffusion_number()[0])
    maxit = 2000
    for r in (_three_steps("implicit", kappa, maxit=maxit),):
        assert b"tracer_diffusion_mode" in r["blob"]
        assert np.array_equal(r["Q"], probe["Q"]) and np.array_equal(r["p"], probe["p"])
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], probe["its"]))
        for n in range(3):
            m = r["solve_its"][n]
            assert m > 0
            passes = min(m + 2, maxit)
            added = 1 + 3 * passes + (1 if m + 2 > maxit else 0) + 1
            for c in r["census"][n]:
                assert r["census"][n][c] - probe["census"][n][c] == (added if c == "other" else 0), (n, c)
        print(f"iterations per step {r['solve_its']}, launches of `other` per step "
              f"{[r['census'][n]['other'] for n in range(3)]} (without the term {[probe['census'][n]['other'] for n in range(3)]})")


# ---- 6. the adaptive step
def test_adaptive_step_sizes_are_those_without_the_term(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    k, nx, dt = 1, 6, 0.02
    sizes = {}
    lam = _stepper("ssp2", UnitSquareMesh(nx, nx), k, dt)._engine.tracer_diffusion_number()[0]
    kappa = 4.52 / (0.25 * dt * lam)  # the explicit limit would hold dt at a quarter of the constructor's
    for key, kw in (("none", {}), ("implicit", dict(tracer_diffusivity=kappa, tracer_diffusion="implicit")),
                    ("explicit", dict(tracer_diffusivity=kappa))):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # the explicit run is told that it starts above its limit
            ts = _stepper("ssp2", UnitSquareMesh(nx, nx), k, dt, **kw)
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        ts.solve(*mp.initial_condition(), _q0("square"), mp.f_rhs(), 4 * dt, fused=True, cfl=0.3)
        sizes[key] = np.array(ts.step_sizes)
        rates = ts._engine.step_rates()
        print(key, sizes[key][:, 1].tolist(), rates)
        assert (rates[1] > 0) == (key == "explicit")
    assert np.array_equal(sizes["implicit"], sizes["none"])
    assert sizes["explicit"][:, 1].max() < 0.5 * sizes["none"][:, 1].min()  # not vacuous: the explicit term does cap dt


# ---- 7. restart
def _ck_engine(kappa, mode):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, n_tracers=2)
    eng = ts._engine
    eng.set_tracer_walls([WALLS_LR, {}])
    eng.set_tracer_diffusivity(kappa)
    if mode is not None:
        eng.set_tracer_diffusion_mode(mode)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    return ts, eng, ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0)


def test_restart_continues_bit_for_bit_and_is_bound_to_the_mode(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    lam = _ck_engine(0.0, None)[1].tracer_diffusion_number()[0]
    kappa = [50.0 / (0.02 * lam), 20.0 / (0.02 * lam)]
    ts, eng, Q0, p0 = _ck_engine(kappa, "implicit")
    eng.set_state(Q0, p0)
    eng.reconstruct_trace()
    eng.set_tracer(np.stack([ts._V_p.interpolate(_field(m)) for m in range(2)]))
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"tracer_diffusion_mode" in blob
    for n in range(2):
        eng.step()
    ts2, eng2, _, _ = _ck_engine(kappa, "implicit")
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    assert np.array_equal(eng2.get_tracer(), eng.get_tracer())
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for a, b in zip(eng2.tracer_diffusion_solve(), eng.tracer_diffusion_solve()):
        assert np.array_equal(a, b) and np.all(a > 0)
    for mode in (None, "explicit"):
        _, eng3, _, _ = _ck_engine(kappa, mode)
        with pytest.raises(_lib.HDGError, match="tracer_diffusion_mode|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


# ---- 8. errors
def test_errors(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    eng = ts._engine
    raw = lambda mode, rtol, maxit: eng.lib.hdg_set_tracer_diffusion_mode(eng.h, mode, rtol, maxit)
    msg = lambda: eng.lib.hdg_last_error(eng.h).decode()
    eng.set_tracer_diffusion_mode("implicit", rtol=1e-9, max_iterations=50)
    for mode in (2, -1):
        assert raw(mode, 1e-10, 100) == -1 and "neither 0 (explicit) nor 1 (implicit)" in msg()
    for rtol in (0.0, -1e-10, float("nan"), float("inf")):
        assert raw(1, rtol, 100) == -1 and "rtol" in msg()
    assert raw(1, 1e-10, 0) == -1 and "max_iterations" in msg()
    with pytest.raises(ValueError, match="tracer_diffusion must be one of"):
        eng.set_tracer_diffusion_mode("semi")
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    q0 = ts._V_p.interpolate(_q0("square"))
    eng.set_tracer(q0)
    eng.tracer_begin_step()
    assert raw(0, 1e-10, 100) == -1 and "a step is open" in msg()
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.solve_tracer_diffusion([1.0], q0[None])
    assert e.value.code == -1
    assert eng.tracer_diffusion_mode() == "implicit"  # every refused call changed nothing: checked through the fingerprint below

    # max_iterations = 1 at number 5000: HDG_ERR_NOT_CONVERGED, the step is complete and the tracer is the transported one
    lam = eng.tracer_diffusion_number()[0]
    got = {}
    for key in ("implicit", "none"):
        t2 = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
        e2 = t2._engine
        if key == "implicit":
            e2.set_tracer_diffusivity(5000.0 / (0.02 * lam))
            e2.set_tracer_diffusion_mode("implicit", max_iterations=1)
        e2.set_state(t2._as_nodal_velocity(Q0), t2._as_nodal_pressure(p0))
        e2.reconstruct_trace()
        e2.set_tracer(q0)
        if key == "implicit":
            with pytest.raises(_lib.HDGError, match="did not converge after 1 iteration") as e:
                e2.step()
            assert e.value.code == -3
            its, res = e2.tracer_diffusion_solve()
            assert its[0] == 1 and res[0] > 1e-10
        else:
            e2.step()
        got[key] = (e2.get_tracer(), *t2._current())
    for a, b in zip(got["implicit"], got["none"]):
        assert np.array_equal(a, b)

    # a general mesh: the mode setter and the hook are refused, the explicit term keeps working
    dts = _stepper("implicit", UnitDiskMesh(1), 2, 0.02)
    disk = dts._engine
    for mode in (0, 1):
        assert disk.lib.hdg_set_tracer_diffusion_mode(disk.h, mode, 1e-10, 100) == -5
        assert "general meshes are not supported" in disk.lib.hdg_last_error(disk.h).decode()
    with pytest.raises(_lib.HDGError, match="general meshes") as e:
        disk.solve_tracer_diffusion([1.0], np.zeros((1,) + tuple(disk.shape_p)))
    assert e.value.code == -5
    disk.set_tracer_diffusivity(1e-3)
    assert np.all(np.isfinite(disk.apply_tracer_diffusion(np.ones(disk.shape_p))))
    with pytest.raises(ValueError, match='needs tracer_diffusivity='):
        _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, tracer_diffusion="implicit")

    # a two-rank strip
    token = "/hdg_ti_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "tracer_implicit_strip_worker.py"), str(r), "2", token, outs[r]],
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
        assert int(d["code"]) == -5 and "strip partitions are not supported" in str(d["msg"]), (d["code"], d["msg"])


# ---- 9. the driver
def test_driver_runs_the_implicit_mode(hip_lib, tmp_path):
    cmd = [sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "cavity", "--nx", "8", "--degree", "1", "--dt", "0.01",
           "--tfinal", "0.03", "--use_projection_method", "--tracer_advection", "--tracer_diffusivity", "5.0", "--tracer_diffusion",
           "implicit", "--tracer_wall", "left", "0.5", "--tracer_wall", "right", "-0.5", "--output", ""]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=os.path.dirname(HERE)))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    out = r.stdout
    assert "tracer diffusion = implicit" in out and "exceeds the stability limit" not in out + r.stderr
    line = [l for l in out.splitlines() if l.startswith("tracer diffusion number = ")]
    assert len(line) == 1 and "limit" not in line[0] and float(line[0].split("=")[1]) > 4.52
    line = [l for l in out.splitlines() if l.startswith("tracer diffusion iterations per solve (mean) = ")]
    assert len(line) == 1 and float(line[0].split("=")[1]) > 1.0
