"""Boussinesq buoyancy on the GPU (include/hdg_buoyancy.h) against tests/buoyancy_reference.py.

Bounds.  The hook: 1e-12 max|f| -- the embedding of DG_k in DG_{k+1} is exact, what remains is the rounding of the nodal <-> modal
conversions.  Whole steps, the rest state and the gravity wave: 2e-8, the project's whole-step bound, for Q, p and every q.
Switched off, everything is bitwise what it is without the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import buoyancy_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL = 1e-12, 2e-8
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread of the transport kernels (TracerBlock<K>, csrc/hdg_cg.hpp)
L_PER = 2 * np.pi
G_TILT = (0.3, -1.0)  # not axis-aligned: both components of the pair are written


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
        kw.setdefault("use_projection_method", True)
        kw.update(n_richardson=2)
    return cls(mesh, k, dt, **kw)


# ---- 1. the hook against the reference
def _betas(n):
    """distinct, beta_1 = 0 when there is a tracer 1"""
    return np.array([0.0 if t == 1 else (-1.0) ** t * (0.5 + 0.25 * t) for t in range(n)]) if n > 1 else np.array([1.7])


@pytest.mark.parametrize("kind,nx,k", [("square", 3, k) for k in (1, 2, 3, 4)] + [("periodic", 4, k) for k in (1, 2, 3, 4)] +
                         [("disk", 1, 2), ("perturbed", 3, 1)])
def test_hook_against_the_reference(hip_lib, kind, nx, k):
    mesh, d = _mesh_and_oracle(kind, nx, k)
    X = d.node_coords(d.PP).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(23 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    fields = [smooth, rng.standard_normal(len(x)), x + 2.0 * y - 0.5 * x * y]  # smooth random, broken random, a jump across the seam
    worst = 0.0
    for n in (1, TB[k] + 1, 16):
        eng = _stepper("ssp2", mesh, k, 0.01, n_tracers=n)._engine
        beta = _betas(n)
        eng.set_tracer(np.zeros(eng.shape_q))
        eng.set_buoyancy(beta, G_TILT)
        got_beta, got_g = eng.buoyancy()
        assert np.array_equal(got_beta, beta) and np.array_equal(got_g, G_TILT)
        for first in range(3 if n == 1 else 1):
            q = np.stack([(1.0 + 0.1 * t) * fields[(first + t) % 3] for t in range(n)])
            want = ref.B(d, q, beta, G_TILT)
            got = eng.apply_buoyancy(q if n > 1 else q[0])
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            worst = max(worst, err)
            assert err <= HOOK, (n, first, err)
        if n > 1:  # a passive tracer is not read: NaN in it leaves f finite, and what it was
            q[1] = np.nan
            assert np.array_equal(eng.apply_buoyancy(q), got)
        eng.set_buoyancy(None)  # off: the hook returns zeros
        assert np.array_equal(eng.apply_buoyancy(q if n > 1 else q[0]), np.zeros(eng.shape_Q))
        eng.close()
    print(f"{kind} nx={nx} k={k}: largest |f - reference| = {worst:.3e} max|f|")


# ---- 2. whole steps against the reference loop
def _q0(kind):
    if kind == "periodic":  # zero mean, and it jumps across the seam in x and in y
        return lambda x, y: 0.3 * (x - np.pi) + 0.15 * (y - np.pi) + 0.2 * np.sin(x) * np.sin(y)
    if kind == "disk":
        return lambda x, y: np.sin(2.0 * x) * np.cos(1.5 * y) + 0.5 * y
    return lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y


def _initial(kind, ts, d):
    """initial velocity and pressure, for the package and for the oracle"""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from oracle import hdg_oracle as orc

    if kind == "square":
        return TaylorGreen(ts._V_Q, ts._V_p).initial_condition(), orc.TaylorGreen(d).initial_condition()
    if kind == "periodic":
        Q0 = lambda x, y: (np.where(y <= np.pi, np.tanh((y - np.pi / 2) / (np.pi / 15)), np.tanh((1.5 * np.pi - y) / (np.pi / 15))), 0.05 * np.sin(x))
        p0 = lambda x, y: 0.015 * np.cos(x) * np.sin(y - np.pi)
    else:
        Q0 = lambda x, y: (-y * (1.0 - x * x - y * y), x * (1.0 - x * x - y * y))
        p0 = lambda x, y: 0.1 * x * y
    return (Q0, p0), (d.interpolate_velocity(Q0), d.interpolate_pressure(p0))


def _forcing(mode, ts, d):
    """a user forcing at the same time, nodal or separable: (the package's f_rhs, the oracle's)"""
    from incompressibleeulerhdg_amd.model_problems import SeparableForcing

    if mode == "nodal":
        f = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))
        return f, lambda t: d.interpolate_velocity(f(t))
    prof = lambda x, y: (0.5 * np.sin(1.5 * x) * np.cos(y), -0.4 * np.cos(x) + 0.2 * y)
    g = lambda t: 1.0 + 0.5 * np.sin(3.0 * t)
    profile = d.interpolate_velocity(prof)
    return SeparableForcing(ts._V_Q.interpolate(prof), g), lambda t: g(t) * profile


CONFIGS = {
    "ssp2-k1": ("ssp2", "square", 1, 6, {}), "ssp2-k2": ("ssp2", "square", 2, 4, {}), "ars2-k2": ("ars2", "square", 2, 4, {}),
    "ssp2-unsplit-k1": ("ssp2", "square", 1, 6, {"use_projection_method": False}),
    "implicit-k1": ("implicit", "square", 1, 6, {}), "dg-k1": ("dg", "square", 1, 6, {}),
    "ssp2-periodic-k1": ("ssp2", "periodic", 1, 6, {}), "ssp2-disk-k2": ("ssp2", "disk", 2, 1, {}),
}
RUNS = [(name, fused) for name in CONFIGS for fused in ((True, False) if name in ("ssp2-k1", "ssp2-k2") else (True,))]
_WANT = {}


def _reference_runs(name, mode, d, tr, dt, nsteps, oic, oq0, of, beta, g, kappa=None, A=None):
    """(with beta, without): once per configuration and forcing, shared by the fused and the per-solve run; read-only"""
    from oracle import hdg_oracle as orc

    if (name, mode) in _WANT:
        return _WANT[name, mode]
    which, _, _, _, kw = CONFIGS[name]
    out = []
    for b in (beta, 0.0 * np.asarray(beta)):
        if which == "dg":
            r = ref.dg_with_buoyancy(d, tr, b, g, dt, *oic, oq0, of, nsteps, kappa=kappa, A=A)
        elif which == "implicit":
            r = ref.implicit_with_buoyancy(d, tr, b, g, dt, *oic, oq0, of, nsteps * dt, kappa=kappa, A=A)
        else:
            o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which],
                                  use_projection_method=kw.get("use_projection_method", True))
            r = ref.imex_with_buoyancy(o, tr, b, g, *oic, oq0, of, nsteps * dt, kappa=kappa, A=A)
        r = tuple(np.array(v) for v in r)
        for v in r:
            v.setflags(write=False)
        out.append(r)
    _WANT[name, mode] = out
    return out


def _compare(tag, ts, got_Q, got_p, want, seen_floor=1e-2):
    (oQ, op, oq), (pQ, _, _) = want
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ))
    qs = np.stack([f_.dat.data for f_ in ts.q_tracers])
    errs = [_rel(got_Q, oQ), _rel(got_p, op)] + [_rel(qs[t], np.atleast_2d(oq)[t]) for t in range(len(qs))]
    print(f"{tag}: with / without beta differ by {seen:.3e} max|Q|; Q {errs[0]:.3e}, p {errs[1]:.3e}, q " +
          " ".join(f"{e:.3e}" for e in errs[2:]))
    assert seen >= seen_floor, "the comparison shows nothing: the reference does not see the buoyancy"
    assert max(errs) < TOL, errs


@pytest.mark.parametrize("mode", ["nodal", "separable"])
@pytest.mark.parametrize("name,fused", RUNS)
def test_whole_steps_against_the_reference_loop(hip_lib, name, fused, mode):
    from oracle.tracer_oracle import TracerOracle

    which, kind, k, nx, kw = CONFIGS[name]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps = 3
    dt = 0.02 if kind == "disk" else 0.25 * d.mesh.h
    beta = 0.8 if kind == "periodic" else 2.0
    ts = _stepper(which, mesh, k, dt, buoyancy=beta, gravity=G_TILT, **kw)
    ic, oic = _initial(kind, ts, d)
    f, of = _forcing(mode, ts, d)
    q0 = _q0(kind)
    want = _reference_runs(name, mode, d, TracerOracle(d), dt, nsteps, oic, d.interpolate_pressure(q0), of, beta, G_TILT)
    Q, p = ts.solve(*ic, q0, f, nsteps * dt, **({"fused": fused} if which in ("ssp2", "ars2") else {}))
    assert np.array_equal(ts._engine.buoyancy()[0], [beta])
    _compare(f"{name} fused={fused} {mode}", ts, Q.dat.data, p.dat.data, want)


def test_two_tracers_of_opposite_beta_and_different_kappa(hip_lib):
    import tracer_diffusion_reference as tdref
    from oracle.tracer_oracle import TracerOracle

    name = "ssp2-k1"
    which, kind, k, nx, kw = CONFIGS[name]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps, dt = 3, 0.25 * d.mesh.h
    beta = np.array([2.0, -1.5])
    ts = _stepper(which, mesh, k, dt, n_tracers=2, buoyancy=beta, gravity=G_TILT)
    k0 = 0.35 / (dt * ts._engine.tracer_diffusion_number()[0])
    kappa = np.array([k0, 0.4 * k0])
    ts._engine.set_tracer_diffusivity(kappa)
    ic, oic = _initial(kind, ts, d)
    f, of = _forcing("nodal", ts, d)
    q0 = [_q0("square"), lambda x, y: np.cos(3.0 * x) * y + 0.3 * np.sin(4.0 * y)]
    oq0 = np.stack([d.interpolate_pressure(fn) for fn in q0])
    want = _reference_runs(name, "two tracers", d, TracerOracle(d), dt, nsteps, oic, oq0, of, beta, G_TILT, kappa=kappa, A=tdref.minv_d(d))
    Q, p = ts.solve(*ic, q0, f, nsteps * dt, fused=True)
    _compare("two tracers", ts, Q.dat.data, p.dat.data, want)


# ---- 3. the rest state and the gravity wave on the device
def _manual(which, mesh, k, dt, Q0, p0, q0, beta, g, n_tracers=1):
    """an engine with the state set by hand (no user forcing), ready to step"""
    ts = _stepper(which, mesh, k, dt, **({"n_tracers": n_tracers} if n_tracers > 1 else {}))
    eng = ts._engine
    eng.set_state(Q0, p0)
    if which in ("ssp2", "ars2"):
        eng.reconstruct_trace()
    eng.set_tracer(q0)
    if beta is not None:
        eng.set_buoyancy(beta, g)
    for slot in range(eng.nstages + 1 if which in ("ssp2", "ars2") else 1):
        eng.set_forcing_scale(slot, 0.0)
    return ts, eng


@pytest.mark.parametrize("which", ["ssp2", "implicit"])
def test_rest_state_equals_the_reference(hip_lib, which):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    k, nx, nsteps, dt = 2, 3, 3, 0.02
    level, slope, _, (oQ, op, oq) = ref.rest_state(which, k, nx=nx, nsteps=nsteps, dt=dt)
    ts = _stepper(which, UnitSquareMesh(nx, nx), k, dt, buoyancy=1.0)
    zero = lambda x, y: (0 * x, 0 * y)
    Q, p = ts.solve(zero, lambda x, y: 0 * x, ref.REST[k][0], None, nsteps * dt, **({"fused": True} if which == "ssp2" else {}))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op), _rel(ts.q_tracer.dat.data, oq)
    print(f"{which}: reference max|Q| {level:.3e} of free fall, p = {slope:.4f} * potential; Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
    assert max(errs) < TOL, errs


def test_gravity_wave_changes_sign_in_the_same_step(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    nx, k = 4, 2
    amps_ref, (oQ, op, oq), d = ref.wave_run(nx, k)
    Q0, p0, q0 = ref.wave_fields(d)
    ts, eng = _manual("ssp2", UnitSquareMesh(nx, nx), k, ref.WAVE_DT, Q0, p0, q0, 1.0, ref.G_DOWN)
    amps = [ref.wave_amplitude(d, Q0)]
    for n in range(ref.WAVE_STEPS):
        eng.step()
        amps.append(ref.wave_amplitude(d, ts._current()[0]))
    Q, p = ts._current()
    step, t = ref.crossing(amps, ref.WAVE_DT)
    step_ref, t_ref = ref.crossing(amps_ref, ref.WAVE_DT)
    errs = _rel(Q, oQ), _rel(p, op), _rel(eng.get_tracer(), oq)
    print(f"sign change in step {step} (reference {step_ref}), t = {t:.8f} (reference {t_ref:.8f}, analytic {ref.WAVE_T:.8f}); "
          f"after {ref.WAVE_STEPS} steps Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
    assert step == step_ref
    assert max(errs) < TOL, errs


# ---- 4. off is off
def _three_steps(mode):
    """Fields, iteration counts, digest and the launch census of the third of three fused steps with two tracers."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, n_tracers=2)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_tracer(np.stack([ts._V_p.interpolate(_q0("square")), ts._V_p.interpolate(_q0("disk"))]))
    if mode == "zeros":
        eng.set_buoyancy(0.0)
    elif mode == "on_then_zeros":
        eng.set_buoyancy([1.0, -2.0], G_TILT)
        eng.set_buoyancy([0.0, 0.0], G_TILT)
    elif mode == "on_then_none":
        eng.set_buoyancy([1.0, -2.0], G_TILT)
        eng.set_buoyancy(None)
    elif mode == "on":
        eng.set_buoyancy([1.0, -2.0], G_TILT)
    elif mode == "on_faintly":
        eng.set_buoyancy([1e-9, -2e-9], G_TILT)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, q=eng.get_tracer(), its=eng.iteration_stats(), digest=eng.state_digest())


def test_switched_off_nothing_changes(hip_lib):
    base = _three_steps("unset")
    for mode in ("zeros", "on_then_zeros", "on_then_none"):
        r = _three_steps(mode)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p", "q"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"], mode
    # switched on.  The solver classes of the census follow the iteration counts, and those follow the flow: the launches the
    # term itself adds are read off a run whose beta is too faint to move an iteration count (asserted), the fields off one
    # whose beta is not
    faint = _three_steps("on_faintly")
    assert all(np.array_equal(a, b) for a, b in zip(faint["its"], base["its"]))
    more = {c: faint["census"][c] - base["census"][c] for c in base["census"] if faint["census"][c] != base["census"][c]}
    print(f"beta != 0: launches per step beyond the passive run: {more}")
    assert set(more) <= {"other", "vector_update", "copy_fill"}, more
    assert more.get("other", 0) == 4  # s + 1 = 4 launches of k_buoyancy per SSP2(3,3,2) step
    assert 0.0 < _rel(faint["Q"], base["Q"]) < 1e-6
    assert _rel(_three_steps("on")["Q"], base["Q"]) > 1e-3


# ---- 5. checkpoint
def _ck_engine(beta, g=G_TILT):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, n_tracers=2)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_tracer(np.stack([ts._V_p.interpolate(_q0("square")), ts._V_p.interpolate(_q0("disk"))]))
    if beta is not None:
        eng.set_buoyancy(beta, g)
    return ts, eng


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_beta_and_g(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    beta = [1.0, -2.0]
    ts, eng = _ck_engine(beta)
    plain = _ck_engine(None)[1].save_checkpoint(0, 0.0)
    assert b"buoyancy_beta" not in plain and b"gravity" not in plain
    assert _ck_engine([0.0, 0.0])[1].save_checkpoint(0, 0.0) == plain  # byte for byte what it was
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"buoyancy_beta[0]" in blob and b"buoyancy_beta[1]" in blob and b"gravity[1]" in blob
    for n in range(2):
        eng.step()
    ts2, eng2 = _ck_engine(beta)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    assert np.array_equal(eng2.get_tracer(), eng.get_tracer())
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for other_beta, other_g in (([1.0, -1.0], G_TILT), (beta, (0.0, -1.0)), (None, G_TILT), ([0.0, 0.0], G_TILT)):
        _, eng3 = _ck_engine(other_beta, other_g)
        with pytest.raises(_lib.HDGError, match="buoyancy_beta|gravity|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


def test_a_stepper_restarts_with_its_buoyancy(hip_lib, tmp_path):
    """solve(..., restart=) of a stepper built with buoyancy=: beta and g are set before the checkpoint is loaded, and the run is
    the uninterrupted one bit for bit"""
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    def run(T, **kw):
        ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, buoyancy=2.0, gravity=G_TILT)
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        Q, p = ts.solve(*mp.initial_condition(), _q0("square"), mp.f_rhs(), T, fused=True, **kw)
        return Q.dat.data.copy(), p.dat.data.copy(), ts.q_tracer.dat.data.copy()

    path = str(tmp_path / "run.ck")
    run(0.04, checkpoint=path)
    whole, resumed = run(0.08), run(0.08, restart=path)
    for a, b in zip(whole, resumed):
        assert np.array_equal(a, b)
    plain = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    mp = TaylorGreen(plain._V_Q, plain._V_p)
    with pytest.raises(_lib.HDGError, match="buoyancy_beta|gravity|fingerprint"):
        plain.solve(*mp.initial_condition(), _q0("square"), mp.f_rhs(), 0.08, fused=True, restart=path)


# ---- 6. errors
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, n_tracers=3)
    eng = ts._engine
    with pytest.raises(_lib.HDGError, match="no tracer is set") as e:
        eng.set_buoyancy([1.0, 0.0, 2.0])
    assert e.value.code == -1
    rng = np.random.default_rng(3)
    Q0, p0, q0 = rng.standard_normal(eng.shape_Q), rng.standard_normal(eng.shape_p), rng.standard_normal(eng.shape_q)
    eng.set_state(Q0, p0)
    eng.set_tracer(q0)
    eng.set_buoyancy([1.0, 0.0, 2.0], G_TILT)

    def untouched():
        beta, g = eng.buoyancy()
        assert np.array_equal(beta, [1.0, 0.0, 2.0]) and np.array_equal(g, G_TILT)  # a refused call leaves the setting ...
        Q, p = ts._current()
        assert np.array_equal(eng.get_tracer(), eng_q) and np.array_equal(Q, eng_Q) and np.array_equal(p, eng_p)  # ... and the fields

    eng_q, (eng_Q, eng_p) = eng.get_tracer(), ts._current()
    for bad in ([1.0, 2.0], [1.0] * 4):
        with pytest.raises(_lib.HDGError, match=rf"{len(bad)} value\(s\) for 3 tracer") as e:
            eng.set_buoyancy(bad)
        assert e.value.code == -1
        untouched()
    for x in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.HDGError, match=r"beta\[2\]") as e:
            eng.set_buoyancy([1.0, 0.0, x])
        assert e.value.code == -1
        with pytest.raises(_lib.HDGError, match=r"g\[1\]") as e:
            eng.set_buoyancy([1.0, 0.0, 2.0], (0.0, x))
        assert e.value.code == -1
        untouched()
    with pytest.raises(ValueError, match="two components"):
        eng.set_buoyancy(1.0, (0.0, -1.0, 0.0))
    eng.tracer_begin_step()  # while a step is open
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.set_buoyancy([0.0, 0.0, 0.0])
    assert e.value.code == -1
    assert np.array_equal(eng.buoyancy()[0], [1.0, 0.0, 2.0])


def test_the_steppers_refuse_buoyancy_without_a_tracer(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    with pytest.raises(ValueError, match="gravity= needs buoyancy="):
        _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, gravity=(0.0, -1.0))
    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, buoyancy=1.0)
    with pytest.raises(ValueError, match="buoyancy= needs a tracer"):
        ts.solve(lambda x, y: (0 * x, 0 * y), lambda x, y: 0 * x, None, None, 0.02)


def test_a_strip_keeps_its_tracer_error(hip_lib, tmp_path):
    token = "/hdg_by_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "buoyancy_strip_worker.py"), str(r), "2", token, outs[r]],
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


# ---- 7. driver
def test_driver_with_two_buoyant_tracers(hip_lib, tmp_path):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "shear", "--nx", "8", "--degree", "1",
                        "--dt", "0.04", "--tfinal", "0.08", "--tracer_advection", "--tracers", "2", "--buoyancy", "1", "-1",
                        "--gravity", "0", "-1", "--output", ""], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "buoyancy = 1.0 -1.0" in r.stdout and "gravity = 0.0 -1.0" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("buoyancy mean force = ")]
    assert len(line) == 1, r.stdout
    fx, fy = (float(v) for v in line[0].split("=")[1].split())
    # the mean of the driver's initial fields sin(2 pi (m+1) x) sin(2 pi (m+1) y), interpolated on this mesh, from the oracle's
    # integral; the printed line carries six digits
    from incompressibleeulerhdg_amd.driver import tracer_initial
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(8, 1, periodic=True, L=L_PER)
    mean = sum(b * float(d.int_p @ d.interpolate_pressure(tracer_initial(m))) for m, b in enumerate((1.0, -1.0))) / d.mesh.volume
    assert abs(mean) > 1e-4  # sin(2 pi x) has no whole period on [0, 2 pi]: the line does say something
    assert fx == 0.0 and fy == pytest.approx(-mean, rel=1e-5)
    assert "tracer_1: integral" in r.stdout
