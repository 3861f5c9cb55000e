"""Tracer diffusion on the GPU (include/hdg_tracer_diffusion.h) against tests/tracer_diffusion_reference.py.

Bounds.  The operator hook: relative 1e-10, the bound of the advection hook (tests/test_gpu_tracer.py).  Whole steps: 2e-8, the
project's whole-step bound.  L2 errors against the analytic decay: relative 1e-6 (the rule of DESIGN.md section 3 for
manufactured errors).  A member of a batch against the same tracer alone: 1e-12 max|q| (tests/test_gpu_multi_tracer.py).
Switched off, everything is bitwise what it is without the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid
import warnings

import numpy as np
import pytest

import tracer_diffusion_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL, BOUND = 1e-10, 2e-8, 1e-12
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread (TracerBlock<K>, csrc/hdg_cg.hpp)
L_PER = 2 * np.pi


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _mesh_and_oracle(kind, nx, k):
    """The package's mesh and the oracle's discretisation of the same triangulation."""
    import manufactured as ms
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, TriangleMesh, UnitDiskMesh, UnitSquareMesh
    from oracle import fem
    from oracle import hdg_oracle as orc

    if kind == "square":
        return UnitSquareMesh(nx, nx), orc.HDGDiscretisation(nx, k)
    if kind == "periodic":
        return PeriodicSquareMesh(nx, nx, L=L_PER), orc.HDGDiscretisation(nx, k, periodic=True, L=L_PER)
    pm = UnitDiskMesh(nx) if kind == "disk" else TriangleMesh(*ms.perturbed_square_mesh(nx))
    return pm, orc.HDGDiscretisation(0, k, mesh=fem.TriMesh(pm.vertices, pm.cells))


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _kappa_for(eng, dt, number=0.35):
    """kappa that puts the diffusion number the engine reports at `number` (inside [0.2, 0.5])."""
    return number / (dt * eng.tracer_diffusion_number()[0])


# ---- 1. the operator hook
@pytest.mark.parametrize("kind,nx,k", [("square", 3, k) for k in (1, 2, 3, 4)] + [("periodic", 8, k) for k in (1, 2, 3, 4)] +
                         [("disk", 1, 2), ("perturbed", 3, 1)])
def test_operator_hook_against_the_reference(hip_lib, kind, nx, k):
    mesh, d = _mesh_and_oracle(kind, nx, k)
    eng = _stepper("implicit", mesh, k, 0.01)._engine
    A = ref.minv_d(d)
    X = d.node_coords(d.PP).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(17 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    fields = {"smooth random": smooth, "jump across the seam": x + 2.0 * y - 0.5 * x * y, "broken random": rng.standard_normal(len(x))}
    lam = eng.tracer_diffusion_number()[0]
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    print(f"{kind} k={k}: Lambda {lam:.6g}, rho {rho:.6g}")
    assert rho <= lam <= 4.0 * rho
    for name, q in fields.items():
        want = A @ q
        got = eng.apply_tracer_diffusion(q)
        print(f"  {name}: {_rel(got, want):.3e}")
        assert _rel(got, want) < HOOK, name
    assert np.max(np.abs(eng.apply_tracer_diffusion(np.ones(len(x))))) <= 1e-9 * lam  # constants are in the null space


# ---- 2. whole steps against the reference loop
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

    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps = 3
    dt = 0.25 * d.mesh.h
    tr = TracerOracle(d)
    A = ref.minv_d(d)
    q0 = _q0(kind)
    paths = (False, True) if which in ("ssp2", "ars2") else (None,)
    want = {}
    for fused in paths:
        ts = _stepper(which, mesh, k, dt)
        kappa = _kappa_for(ts._engine, dt)
        ts._engine.set_tracer_diffusivity(kappa)
        number = ts._engine.tracer_diffusion_number()[1]
        assert 0.2 <= number <= 0.5, number
        ic, f, oic, of = _flow(kind, ts, d)
        if not want:  # the reference, with and without kappa: once per case
            for kap in (kappa, 0.0):
                oq0 = d.interpolate_pressure(q0)
                if which == "dg":
                    want[kap] = ref.dg_with_diffusion(d, tr, A, kap, dt, *oic, oq0, of, nsteps)
                elif which == "implicit":
                    want[kap] = ref.implicit_with_diffusion(d, tr, A, kap, dt, *oic, oq0, of, nsteps * dt)
                else:
                    o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which])
                    want[kap] = ref.imex_with_diffusion(o, tr, A, kap, *oic, oq0, of, nsteps * dt)
            # a condition on the reference alone: the diffusion is seen
            seen = np.max(np.abs(want[kappa][2] - want[0.0][2])) / np.max(np.abs(want[0.0][2]))
            print(f"{which} {kind} k={k}: kappa {kappa:.4e}, number {number:.3f}, with / without kappa differ by {seen:.3e} max|q|")
            assert seen >= 1e-3
        kw = {} if fused is None else {"fused": fused}
        Q, p = ts.solve(*ic, q0, f, nsteps * dt, **kw)
        oQ, op, oq = want[kappa]
        errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op), _rel(ts.q_tracer.dat.data, oq)
        print(f"  fused={fused}: Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
        assert max(errs) < TOL, (fused, errs)


# ---- 3. analytic decay
@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("nx", [4, 8])
def test_decay_error_equals_the_reference(hip_lib, k, nx):
    """Zero velocity, periodic square, q0 = sin x sin y, forward Euler (the implicit stepper): the L2 error against
    exp(-2 kappa T) q0 equals the reference's to a relative 1e-6."""
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh

    kappa, dt, nsteps = ref.decay_case(k, nx)
    err_ref, q_ref, d = ref.decay_errors(k, nx, kappa, dt, nsteps)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # Lambda is an upper bound: the number may read above 2 where rho is below
        ts = _stepper("implicit", PeriodicSquareMesh(nx, nx, L=L_PER), k, dt, tracer_diffusivity=kappa)
    zero = lambda x, y: (0 * x, 0 * y)
    ts.solve(zero, lambda x, y: 0 * x, lambda x, y: np.sin(x) * np.sin(y), None, nsteps * dt)
    err = ref.l2_error(d, ts.q_tracer.dat.data, np.exp(-2 * kappa * nsteps * dt))
    print(f"k={k} nx={nx}: L2 error {err:.10e}, reference {err_ref:.10e}, fields differ by {_rel(ts.q_tracer.dat.data, q_ref):.3e}")
    assert abs(err - err_ref) <= 1e-6 * err_ref


# ---- 4. invariants
def test_mass_is_kept_and_variance_falls_between_walls(hip_lib):
    """Zero velocity on the unit square: int q stays to 1e-13 int |q|, 1/2 int q^2 does not increase (no-flux walls)."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    k, nx, dt, nsteps = 2, 5, 0.01, 12
    ts = _stepper("ssp2", UnitSquareMesh(nx, nx), k, dt)
    eng = ts._engine
    eng.set_tracer_diffusivity(_kappa_for(eng, dt, 0.45))
    q0 = lambda x, y: x + np.sin(3 * y) + 0.3 * np.cos(7 * x * y)  # a normal gradient at every wall
    ts.solve(lambda x, y: (0 * x, 0 * y), lambda x, y: 0 * x, q0, None, nsteps * dt, fused=True, diagnostics=True)
    mass, half = ts.diagnostics["tracer_integral"], ts.diagnostics["tracer_half_sq"]
    start = ts._V_p.interpolate(q0)
    mass0, abs0 = eng.integrate_pressure(start), eng.integrate_pressure(np.abs(start))
    print(f"int q: start {mass0!r}, rows deviate by {np.max(np.abs(mass - mass0)):.3e}; half square {half[0]:.6e} -> {half[-1]:.6e}")
    assert len(mass) >= nsteps
    assert np.max(np.abs(mass - mass0)) <= 1e-13 * abs0
    assert np.all(np.diff(half) <= 0.0) and half[-1] < half[0]  # D is negative definite off the constants


# ---- 5. nothing changes when it is off
def _transport_launches_per_step(eng_kw):
    a, b = np.asarray(eng_kw["a_expl"]), np.asarray(eng_kw["b_expl"])
    return int(np.count_nonzero(a) + np.count_nonzero(b))


def _three_steps(mode, kappa=None):
    """Fields, iteration counts and the launch census of the third of three fused steps with one tracer."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_tracer(ts._V_p.interpolate(_q0("square")))
    if mode == "zeros":
        eng.set_tracer_diffusivity(0.0)
    elif mode == "on_then_zeros":
        eng.set_tracer_diffusivity(kappa)
        eng.set_tracer_diffusivity([0.0])
    elif mode == "on_then_none":
        eng.set_tracer_diffusivity(kappa)
        eng.set_tracer_diffusivity(None)
    elif mode == "on":
        eng.set_tracer_diffusivity(kappa)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, q=eng.get_tracer(), its=eng.iteration_stats(), digest=eng.state_digest(), ts=ts)


def test_switched_off_nothing_changes(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    base = _three_steps("unset")
    kappa = _kappa_for(base["ts"]._engine, 0.02)
    for mode in ("zeros", "on_then_zeros", "on_then_none"):
        r = _three_steps(mode, kappa)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p", "q"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"], mode
    # switched on: one more launch per transport launch, in one class only; the flow does not see it
    on = _three_steps("on", kappa)
    other = _lib.Engine.LAUNCH_CLASSES[-1]
    s = 3
    tab = dict(a_expl=base["ts"]._a_expl, b_expl=base["ts"]._b_expl)
    more = {c: on["census"][c] - base["census"][c] for c in base["census"]}
    assert more == {c: (_transport_launches_per_step(tab) if c == other else 0) for c in base["census"]}, (more, s)
    assert np.array_equal(on["Q"], base["Q"]) and np.array_equal(on["p"], base["p"])
    assert all(np.array_equal(a, b) for a, b in zip(on["its"], base["its"]))
    assert _rel(on["q"], base["q"]) > 1e-3


# ---- 6. batches
_ALONE = {}
KAPPA_SHARE = lambda m: 0.0 if m == 1 else (m + 2) / 18.0  # distinct, one zero


def _field(m):
    return lambda x, y: np.sin((1.3 + 0.4 * m) * x + 0.2 * m) * np.cos((1.0 + 0.7 * m) * y) + 0.1 * (m + 1) * x


def _batch_run(kind, k, nx, members, kappas, n_tracers=None):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    dt, nsteps = 0.02, 2
    mesh, _ = _mesh_and_oracle(kind, nx, 1)
    ts = _stepper("ssp2", mesh, k, dt, **({} if n_tracers is None else {"n_tracers": n_tracers}))
    ts._engine.set_tracer_diffusivity(kappas)
    if kind == "square":
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        ic, f = mp.initial_condition(), mp.f_rhs()
    else:
        ic, f = (lambda x, y: (np.sin(y) + 0.3 * np.cos(x), 0.5 * np.sin(x)), lambda x, y: 0 * x), None
    q0 = [_field(m) for m in members]
    ts.solve(*ic, q0 if n_tracers is not None else q0[0], f, nsteps * dt, fused=True)
    return np.stack([f_.dat.data.copy() for f_ in ts.q_tracers]), ts


@pytest.mark.parametrize("kind,k,nx,n", [("square", 1, 6, TB[1] + 1), ("square", 2, 5, TB[2] + 1), ("square", 3, 4, TB[3] + 1),
                                         ("periodic", 2, 8, TB[2] + 1), ("square", 2, 5, 16)])
def test_a_batch_with_distinct_diffusivities_equals_its_members(hip_lib, kind, k, nx, n):
    mesh, _ = _mesh_and_oracle(kind, nx, 1)
    probe = _stepper("ssp2", mesh, k, 0.02)._engine
    kmax = _kappa_for(probe, 0.02, 0.45)
    top = max(KAPPA_SHARE(m) for m in range(n))
    kappas = [kmax * KAPPA_SHARE(m) / top for m in range(n)]  # the largest one sets the diffusion number
    assert len(set(kappas)) == n and kappas.count(0.0) == 1
    batch, ts = _batch_run(kind, k, nx, tuple(range(n)), kappas, n_tracers=n)
    assert 0.2 <= ts._engine.tracer_diffusion_number()[1] <= 0.5
    worst = 0.0
    for m in range(n):
        key = (kind, k, nx, m, kappas[m])
        if key not in _ALONE:
            _ALONE[key] = _batch_run(kind, k, nx, (m,), kappas[m])[0][0]
            _ALONE[key].setflags(write=False)
        alone = _ALONE[key]
        diff = np.max(np.abs(batch[m] - alone)) / np.max(np.abs(alone))
        worst = max(worst, diff)
        assert diff <= BOUND, (m, diff)
    # the comparison is not vacuous: members with different kappa differ far beyond the bound
    plain = _batch_run(kind, k, nx, (0,), 0.0)[0][0]
    assert _rel(batch[0], plain) > 1e-4
    print(f"{kind} k={k} n={n}: largest |batch - alone| = {worst:.3e} max|q|")


# ---- 7. checkpoint
def _ck_engine(kappa):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, n_tracers=2)
    eng = ts._engine
    if kappa is not None:
        eng.set_tracer_diffusivity(kappa)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    return ts, eng, ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0)


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_kappa(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    ts, eng, Q0, p0 = _ck_engine(None)
    kmax = _kappa_for(eng, 0.02)
    kappa = [kmax, 0.5 * kmax]
    eng.set_tracer_diffusivity(kappa)
    eng.set_state(Q0, p0)
    eng.reconstruct_trace()
    eng.set_tracer(np.stack([ts._V_p.interpolate(_field(m)) for m in range(2)]))
    plain_size = len(_ck_engine(None)[1].save_checkpoint(0, 0.0))
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert len(blob) > plain_size  # the fingerprint names the diffusivities
    assert b"tracer_kappa[0]" in blob and b"tracer_kappa[1]" in blob
    assert b"tracer_kappa" not in _ck_engine(0.0)[1].save_checkpoint(0, 0.0)
    for n in range(2):
        eng.step()
    ts2, eng2, _, _ = _ck_engine(kappa)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    assert np.array_equal(eng2.get_tracer(), eng.get_tracer())
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for other in ([kmax, 0.25 * kmax], None, 0.0):
        _, eng3, _, _ = _ck_engine(other)
        with pytest.raises(_lib.HDGError, match="tracer_kappa|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


# ---- 8. errors
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, n_tracers=3)
    eng = ts._engine
    for bad in ([1e-3, 2e-3], [1e-3] * 4):
        with pytest.raises(_lib.HDGError, match=rf"{len(bad)} value\(s\) for 3 tracer") as e:
            eng.set_tracer_diffusivity(bad)
        assert e.value.code == -1
    for x in (-1e-3, float("nan"), float("inf")):
        with pytest.raises(_lib.HDGError, match=r"kappa\[2\]") as e:
            eng.set_tracer_diffusivity([1e-3, 0.0, x])
        assert e.value.code == -1
    assert eng.tracer_diffusion_number()[1] == 0.0  # a refused call leaves the setting
    eng.set_tracer_diffusivity([1e-3, 0.0, 2e-3])
    lam, number = eng.tracer_diffusion_number()
    assert number == 2e-3 * 0.02 * lam
    eng.set_tracer(None)  # independent of the tracers being on
    assert eng.tracer_diffusion_number() == (lam, number)
    # while a step is open
    eng.set_state(np.zeros(eng.shape_Q), np.zeros(eng.shape_p))
    eng.set_tracer(np.zeros(eng.shape_q))
    eng.tracer_begin_step()
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.set_tracer_diffusivity([0.0, 0.0, 0.0])
    assert e.value.code == -1


def test_the_stepper_warns_above_the_limit_only(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    mesh = UnitSquareMesh(4, 4)
    probe = _stepper("ssp2", mesh, 1, 0.02)
    lam = probe._engine.tracer_diffusion_number()[0]
    assert not hasattr(probe, "diffusion_limit")  # tracer_diffusivity=None: no call at all
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ts = _stepper("ssp2", mesh, 1, 0.02, tracer_diffusivity=4.0 / (0.02 * lam))
        assert ts.diffusion_limit == pytest.approx(4.519842099789738, rel=1e-12)
        assert _stepper("implicit", mesh, 1, 0.02, tracer_diffusivity=1.9 / (0.02 * lam)).diffusion_limit == 2.0
        assert _stepper("dg", mesh, 1, 0.02, tracer_diffusivity=1.9 / (0.02 * lam)).diffusion_limit == 2.0
    with pytest.warns(RuntimeWarning, match="exceeds the stability limit 4.52"):
        _stepper("ssp2", mesh, 1, 0.02, tracer_diffusivity=5.0 / (0.02 * lam))
    with pytest.warns(RuntimeWarning, match="exceeds the stability limit 2"):
        _stepper("implicit", mesh, 1, 0.02, tracer_diffusivity=2.1 / (0.02 * lam))


def test_a_strip_keeps_its_tracer_error(hip_lib, tmp_path):
    token = "/hdg_td_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "tracer_diffusion_strip_worker.py"), str(r), "2", token, outs[r]],
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


def test_driver_with_two_diffusivities(hip_lib, tmp_path):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "shear", "--nx", "8", "--degree", "1",
                        "--dt", "0.04", "--tfinal", "0.08", "--tracer_advection", "--tracers", "2", "--tracer_diffusivity", "1e-3", "2e-3",
                        "--output", ""], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "tracer diffusivity = 0.001 0.002" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("tracer diffusion number = ")]
    assert len(line) == 1 and "(limit 4.51984)" in line[0], r.stdout
    assert 0.0 < float(line[0].split("=")[1].split("(")[0]) < 4.5
    assert "tracer_1: integral" in r.stdout
