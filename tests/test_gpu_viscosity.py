"""The viscous term on the GPU (include/hdg_viscosity.h) against tests/viscosity_reference.py.

Bounds.  The hook: relative 1e-10 (section 19's bound for its operator hook: table and conversion rounding against entries of
size Lambda).  Whole steps, strips: 2e-8, the project's whole-step bound, for Q and p.  The manufactured solution's L2 error:
relative 1e-6 against the reference's.  Switched off, everything is bitwise what it is without the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid
import warnings

import numpy as np
import pytest

import viscosity_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL = 1e-10, 2e-8
L_PER = 2 * np.pi
NUMBER = 0.35  # nu dt Lambda_u of the whole-step runs
_A = {}


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


def _minv_v(kind, nx, k, wall, d):
    """M^-1 V of the reference: once per mesh, degree and wall mode; read-only"""
    if (kind, nx, k, wall) not in _A:
        A = ref.minv_v(d, wall)
        A.setflags(write=False)
        _A[kind, nx, k, wall] = A
    return _A[kind, nx, k, wall]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.setdefault("use_projection_method", True)
        kw.update(n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _set_number(eng, dt, wall, number=NUMBER):
    """nu such that the reported viscous diffusion number nu dt Lambda_u is `number`"""
    eng.set_viscosity(1.0, wall)
    nu = number / (dt * eng.viscosity_number()[0])
    eng.set_viscosity(nu, wall)
    assert eng.viscosity() == (nu, wall) and eng.viscosity_number()[1] == pytest.approx(number, rel=1e-12)
    return nu


# ---- 1. the hook against the reference
HOOK_CASES = ([("square", 3, k, w) for k in (1, 2, 3, 4) for w in ref.WALLS] + [("periodic", 4, k, "free_slip") for k in (1, 2, 3, 4)] +
              [("disk", 1, 2, w) for w in ref.WALLS] + [("perturbed", 3, 1, w) for w in ref.WALLS])


@pytest.mark.parametrize("kind,nx,k,wall", HOOK_CASES)
def test_hook_against_the_reference(hip_lib, kind, nx, k, wall):
    mesh, d = _mesh_and_oracle(kind, nx, k)
    A = _minv_v(kind, nx, k, wall, d)
    X = d.node_coords(d.PU).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(31 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = lambda: sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    fields = [np.stack([smooth(), smooth()], axis=-1),               # smooth
              rng.standard_normal((len(x), 2)),                      # broken
              np.stack([x + 2.0 * y - 0.5 * x * y, y * y - x], axis=-1)]  # jumps across the periodic seam
    eng = _stepper("ssp2", mesh, k, 0.01)._engine
    worst = 0.0
    for n, Q in enumerate(fields):
        want = (A @ Q.ravel()).reshape(-1, 2)
        got = eng.apply_viscosity(Q, wall)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        worst = max(worst, err)
        assert err <= HOOK, (n, err)
    lam = eng.viscosity_number()[0]
    assert eng.viscosity() == (0.0, "free_slip")  # the hook and the query set nothing
    eng.set_viscosity(1.0, wall)
    lam = eng.viscosity_number()[0]
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    print(f"{kind} nx={nx} k={k} {wall}: largest |out - reference| = {worst:.3e} max|out|; Lambda_u {lam:.6g}, rho {rho:.6g}")
    assert lam >= rho
    eng.close()


# ---- 2. whole steps against the reference loop
def _initial(kind, d):
    """nodal initial velocity and pressure.  The smooth part is the Taylor-Green field (square), the shear layer (periodic
    square) or a vortex (disk); the broken part makes the viscous term visible within three steps at the number 0.35 (the smooth
    part alone changes by 0.06 % of max|Q| between free-slip walls: measured on the reference)"""
    from oracle import hdg_oracle as orc

    if kind == "square":
        Q0, p0 = orc.TaylorGreen(d).initial_condition()
    elif kind == "periodic":
        Q0 = d.interpolate_velocity(lambda x, y: (np.where(y <= np.pi, np.tanh((y - np.pi / 2) / (np.pi / 15)), np.tanh((1.5 * np.pi - y) / (np.pi / 15))), 0.05 * np.sin(x)))
        p0 = d.interpolate_pressure(lambda x, y: 0.015 * np.cos(x) * np.sin(y - np.pi))
    else:
        Q0 = d.interpolate_velocity(lambda x, y: (-y * (1.0 - x * x - y * y), x * (1.0 - x * x - y * y)))
        p0 = d.interpolate_pressure(lambda x, y: 0.1 * x * y)
    return Q0 + 0.4 * np.random.default_rng(5).standard_normal(Q0.shape), p0


CONFIGS = {
    "ssp2-k1": ("ssp2", "square", 1, 6, {}), "ssp2-k2": ("ssp2", "square", 2, 4, {}), "ars2-k2": ("ars2", "square", 2, 4, {}),
    "ssp2-unsplit-k1": ("ssp2", "square", 1, 6, {"use_projection_method": False}),
    "implicit-k1": ("implicit", "square", 1, 6, {}), "dg-k1": ("dg", "square", 1, 6, {}),
    "ssp2-periodic-k1": ("ssp2", "periodic", 1, 6, {}), "ssp2-disk-k2": ("ssp2", "disk", 2, 1, {}),
}
RUNS = ([(name, fused, wall) for name in ("ssp2-k1", "ssp2-k2") for fused in (True, False) for wall in ref.WALLS] +
        [(name, True, "free_slip") for name in CONFIGS if name not in ("ssp2-k1", "ssp2-k2")])
_WANT = {}


def _reference_runs(key, which, d, A, nu, dt, nsteps, Q0, p0, of, kw):
    """(with nu, without): once per configuration, shared by the fused and the per-solve run; read-only"""
    from oracle import hdg_oracle as orc

    if key in _WANT:
        return _WANT[key]
    out = []
    for v in (nu, 0.0):
        if which == "dg":
            r = ref.dg_with_viscosity(d, A, v, dt, Q0, p0, of, nsteps)
        elif which == "implicit":
            r = ref.implicit_with_viscosity(d, A, v, dt, Q0, p0, of, nsteps * dt)
        else:
            o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which],
                                  use_projection_method=kw.get("use_projection_method", True))
            r = ref.imex_with_viscosity(o, A, v, Q0, p0, of, nsteps * dt)
        r = tuple(np.array(x) for x in r)
        for x in r:
            x.setflags(write=False)
        out.append(r)
    _WANT[key] = out
    return out


@pytest.mark.parametrize("name,fused,wall", RUNS)
def test_whole_steps_against_the_reference_loop(hip_lib, name, fused, wall):
    which, kind, k, nx, kw = CONFIGS[name]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps = 3
    dt = 0.02 if kind == "disk" else 0.25 * d.mesh.h
    ts = _stepper(which, mesh, k, dt, **kw)
    nu = _set_number(ts._engine, dt, wall)
    Q0, p0 = _initial(kind, d)
    f = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))
    of = lambda t: d.interpolate_velocity(f(t))
    (oQ, op), (pQ, _) = _reference_runs((name, wall), which, d, _minv_v(kind, nx, k, wall, d), nu, dt, nsteps, Q0, p0, of, kw)
    Q, p = ts.solve(Q0, p0, None, f, nsteps * dt, **({"fused": fused} if which in ("ssp2", "ars2") else {}))
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"{name} fused={fused} {wall}: nu {nu:.4e}; with / without nu differ by {seen:.3e} max|Q|; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert seen >= 1e-2, "the comparison shows nothing: the reference does not see the viscosity"
    assert max(errs) < TOL, errs


def test_forcing_buoyant_diffusing_tracer_and_viscosity_together(hip_lib):
    import tracer_diffusion_reference as tdref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    which, kind, k, nx, kw = CONFIGS["ssp2-k1"]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps, dt, wall, beta, g = 3, 0.25 * d.mesh.h, "no_slip", 2.0, (0.3, -1.0)
    ts = _stepper(which, mesh, k, dt, buoyancy=beta, gravity=g)
    eng = ts._engine
    nu = _set_number(eng, dt, wall)
    kappa = 0.35 / (dt * eng.tracer_diffusion_number()[0])
    eng.set_tracer_diffusivity(kappa)
    Q0, p0 = _initial(kind, d)
    q0 = lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y
    f = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))
    of = lambda t: d.interpolate_velocity(f(t))
    o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
    oQ, op, oq = ref.imex_with_viscosity(o, _minv_v(kind, nx, k, wall, d), nu, Q0, p0, of, nsteps * dt, tr=TracerOracle(d),
                                         q0=d.interpolate_pressure(q0), beta=beta, g=g, kappa=kappa, Adiff=tdref.minv_d(d))
    # the stage lists of this run carry forcing, buoyancy and viscosity: some exceed the eight terms k_pgrad_terms folds and
    # take the lincomb route (test_route_of_the_stage_residuals_... below reads that off the census)
    Q, p = ts.solve(Q0, p0, q0, f, nsteps * dt, fused=True)
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op), _rel(ts.q_tracer.dat.data, oq)
    print(f"forcing + buoyancy + tracer diffusion + viscosity: Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
    assert max(errs) < TOL, errs


# ---- 3. the manufactured Navier-Stokes Taylor-Green solution
@pytest.mark.parametrize("k,nx", [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_manufactured_taylor_green_error_equals_the_reference(hip_lib, k, nx):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    mesh, d = _mesh_and_oracle("square", nx, k)
    nsteps, dt, kappa = 3, 0.25 * d.mesh.h, 0.5
    probe = _stepper("implicit", mesh, k, dt)._engine
    nu = _set_number(probe, dt, "free_slip")
    probe.close()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # 0.35 is below forward Euler's limit 2: no warning
        ts = _stepper("implicit", mesh, k, dt, viscosity=nu)  # wall defaults to free slip
    assert ts._engine.viscosity() == (nu, "free_slip")
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", kappa, viscosity=nu)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt)
    omp = ref.TaylorGreenNS(d, "exponential", kappa, viscosity=nu)
    oQ, op = ref.implicit_with_viscosity(d, _minv_v("square", nx, k, "free_slip", d), nu, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    amp = np.exp(-kappa * nsteps * dt)
    e_dev, e_ref = ref.l2_error_velocity(d, Q.dat.data, amp), ref.l2_error_velocity(d, oQ, amp)
    print(f"k={k} nx={nx}: nu {nu:.4e}; L2 error device {e_dev:.10e}, reference {e_ref:.10e}; fields differ by {_rel(Q.dat.data, oQ):.3e}")
    assert abs(e_dev - e_ref) <= 1e-6 * e_ref


# ---- 4. kinetic energy of an unforced run: falls in every step on the reference (tests/test_viscosity_cpu.py), so here too
@pytest.mark.parametrize("wall", ref.WALLS)
@pytest.mark.parametrize("which", ["ssp2", "implicit"])
def test_energy_falls_in_every_step(hip_lib, which, wall):
    mesh, d = _mesh_and_oracle("square", 4, 2)
    dt, nsteps = 0.25 * d.mesh.h, 6
    ts = _stepper(which, mesh, 2, dt)
    eng = ts._engine
    _set_number(eng, dt, wall)
    Qs = d.interpolate_velocity(ref.taylor_green_Qs)
    eng.set_state(Qs, np.zeros(eng.shape_p))
    if which == "ssp2":
        eng.reconstruct_trace()
    for slot in range(eng.nstages + 1 if which == "ssp2" else 1):
        eng.set_forcing_scale(slot, 0.0)
    ke = [eng.compute_diagnostics(Qs, np.zeros(eng.shape_p))[0]]
    for n in range(nsteps):
        eng.step() if which == "ssp2" else eng.implicit_step()
        ke.append(eng.compute_diagnostics(*ts._current())[0])
    print(f"{which} {wall}: KE / KE_0 = " + " ".join(f"{x / ke[0]:.6f}" for x in ke))
    assert ke[0] == pytest.approx(ref.kinetic_energy(d, Qs), rel=1e-12)
    assert np.all(np.diff(ke) < 0.0)


# ---- 5. off is off; on, the launches it adds
def _three_steps(mode, wall="no_slip"):
    """Fields, iteration counts, digest, checkpoint blob and the launch census of the third of three fused steps."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if mode == "zero":
        eng.set_viscosity(0.0, wall)
    elif mode == "on_then_zero":
        eng.set_viscosity(1e-3, wall)
        eng.set_viscosity(0.0)
    elif mode == "on":
        eng.set_viscosity(1e-3, wall)
    elif mode == "on_faintly":
        eng.set_viscosity(1e-16, wall)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, its=eng.iteration_stats(), digest=eng.state_digest(), blob=eng.save_checkpoint(3, 0.06))


def test_switched_off_nothing_changes(hip_lib):
    base = _three_steps("unset")
    for mode in ("zero", "on_then_zero"):
        r = _three_steps(mode)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"], mode
        assert r["blob"] == base["blob"] and b"viscosity" not in r["blob"], mode
    # switched on.  The solver classes of the census follow the iteration counts, and those follow the flow: the launches the
    # term itself adds are read off a run whose nu is too faint to move an iteration count (asserted)
    faint = _three_steps("on_faintly")
    assert all(np.array_equal(a, b) for a, b in zip(faint["its"], base["its"]))
    more = {c: faint["census"][c] - base["census"][c] for c in base["census"] if faint["census"][c] != base["census"][c]}
    print(f"nu != 0: launches per step beyond the inviscid run: {more}")
    # s + 1 = 4 launches of k_viscosity per SSP2(3,3,2) step; the sum in front of the pressure reconstruction; nothing else.
    # The stage residuals stay within the eight terms k_pgrad_terms folds (forcing and viscosity, no buoyancy): no lincomb more
    assert more == {"other": 4, "vector_update": 1}, more
    assert b"viscosity" in faint["blob"] and b"viscosity_wall" in faint["blob"]
    assert _rel(_three_steps("on")["Q"], base["Q"]) > 1e-3


def _forced_buoyant_run(nu):
    """launch census and iteration counts of three fused steps with a nodal forcing and a buoyant tracer"""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02, buoyancy=2.0, gravity=(0.3, -1.0))
    eng = ts._engine
    if nu:
        eng.set_viscosity(nu, "no_slip")
    f = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))
    q0 = lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)
    eng.launch_stats(reset=True)
    ts.solve(*TaylorGreen(ts._V_Q, ts._V_p).initial_condition(), q0, f, 0.06, fused=True)
    return {c: v[0] for c, v in eng.launch_stats().items()}, eng.iteration_stats()


def test_route_of_the_stage_residuals_with_forcing_buoyancy_and_viscosity(hip_lib):
    """A nodal forcing, the buoyancy and the viscosity together put up to 4 s terms into a stage list: where the merged list
    exceeds the eight terms k_pgrad_terms folds, lincomb forms the residual (in chunks of eight) and the plain pressure-gradient
    kernel follows.  Both routes are one launch in 'pressure_rhs'; the fallback shows as launches in 'vector_update'."""
    base, its0 = _forced_buoyant_run(0.0)
    faint, its1 = _forced_buoyant_run(1e-16)
    assert all(np.array_equal(a, b) for a, b in zip(its0, its1))
    more = {c: faint[c] - base[c] for c in base if faint[c] != base[c]}
    print(f"forcing + buoyancy, nu != 0: launches in three steps beyond nu = 0: {more}")
    # Per SSP2(3,3,2) step: four launches of k_viscosity.  The reconstruction already sums b_new + B without nu: nu adds a term
    # to that launch, not a launch.  The stage residuals still go through k_pgrad_terms: the longest list, stage 2, has two
    # slots of forcing, buoyancy and viscosity each beside its velocities and stays within eight terms (a fallback would show as
    # two lincomb launches, a list in chunks of eight, in each of the two Richardson passes: four or more per step).  The one
    # launch more is the final residual, which lincomb always forms: its list outgrows one chunk of eight terms
    assert more == {"other": 3 * 4, "vector_update": 3 * 1}, more


# ---- 6. strips: two ranks over shared memory against one rank
def _ranks(nranks, kind, wall, tmp_path):
    token = "/hdg_visc_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"{kind}{nranks}_{r}.npz") for r in range(nranks)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "viscosity_strip_worker.py"), str(r), str(nranks), token, kind, wall, outs[r]],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(nranks)]
    logs = []
    try:
        for pr in procs:
            logs.append(pr.communicate(timeout=300)[0].decode(errors="replace"))
    finally:
        for pr in procs:
            if pr.poll() is None:
                pr.kill()
                pr.wait()
    assert [pr.returncode for pr in procs] == [0] * nranks, [log[-2000:] for log in logs]
    return [dict(np.load(o)) for o in outs]


@pytest.mark.parametrize("kind,wall", [("square", "no_slip"), ("periodic", "free_slip")])
def test_two_strips_match_one_rank(hip_lib, tmp_path, kind, wall):
    parts = _ranks(2, kind, wall, tmp_path)
    single = _ranks(1, kind, wall, tmp_path)[0]
    Q, p = np.concatenate([d["Q"] for d in parts]), np.concatenate([d["p"] for d in parts])
    errs = _rel(Q, single["Q"]), _rel(p, single["p"])
    print(f"{kind} {wall}: two strips against one rank: Q {errs[0]:.3e}, p {errs[1]:.3e}; nu {float(single['nu']):.4e}")
    assert all(float(d["nu"]) == float(single["nu"]) and float(d["number"]) == pytest.approx(NUMBER, rel=1e-12) for d in parts)
    assert max(errs) < TOL, errs


# ---- 7. checkpoint
def _ck_engine(nu, wall="no_slip"):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if nu is not None:
        eng.set_viscosity(nu, wall)
    return ts, eng


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_nu_and_the_wall(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    nu = 1e-3
    ts, eng = _ck_engine(nu)
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"viscosity" in blob and b"viscosity_wall" in blob
    for n in range(2):
        eng.step()
    ts2, eng2 = _ck_engine(nu)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for other_nu, other_wall in ((2e-3, "no_slip"), (nu, "free_slip"), (0.0, "no_slip"), (None, None)):
        _, eng3 = _ck_engine(other_nu, other_wall)
        with pytest.raises(_lib.HDGError, match="viscosity|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


def test_a_stepper_restarts_with_its_viscosity(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    def run(T, **kw):
        ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, viscosity=1e-3, wall="no_slip")
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T, fused=True, **kw)
        return Q.dat.data.copy(), p.dat.data.copy()

    path = str(tmp_path / "run.ck")
    run(0.04, checkpoint=path)
    whole, resumed = run(0.08), run(0.08, restart=path)
    for a, b in zip(whole, resumed):
        assert np.array_equal(a, b)
    plain = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    mp = TaylorGreen(plain._V_Q, plain._V_p)
    with pytest.raises(_lib.HDGError, match="viscosity|fingerprint"):
        plain.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.08, fused=True, restart=path)


# ---- 8. errors, the warning, the driver
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    eng = ts._engine
    rng = np.random.default_rng(3)
    eng.set_state(rng.standard_normal(eng.shape_Q), rng.standard_normal(eng.shape_p))
    eng.set_viscosity(1e-3, "no_slip")
    eng_Q, eng_p = ts._current()

    def untouched():
        assert eng.viscosity() == (1e-3, "no_slip")  # a refused call leaves the setting ...
        Q, p = ts._current()
        assert np.array_equal(Q, eng_Q) and np.array_equal(p, eng_p)  # ... and the fields

    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(_lib.HDGError, match="not a finite value >= 0") as e:
            eng.set_viscosity(bad, "free_slip")
        assert e.value.code == -1
        untouched()
    for bad in (2, -1):
        assert eng.lib.hdg_set_viscosity(eng.h, 1e-3, bad) == -1 and "wall" in eng.lib.hdg_last_error(eng.h).decode()
        assert eng.lib.hdg_apply_viscosity(eng.h, bad, eng_Q.ctypes.data_as(_lib._dp), np.empty(eng.shape_Q).ctypes.data_as(_lib._dp)) == -1
        untouched()
    with pytest.raises(ValueError, match="wall must be one of"):
        eng.set_viscosity(1e-3, "sticky")
    eng.begin_step()  # while a step is open
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.set_viscosity(0.0)
    assert e.value.code == -1
    with pytest.raises(_lib.HDGError, match="a step is open"):
        eng.apply_viscosity(eng_Q)
    assert eng.viscosity() == (1e-3, "no_slip")


@pytest.mark.parametrize("which", ["ssp2", "implicit", "dg"])
def test_the_warning_speaks_above_the_limit_only(hip_lib, which):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    mesh, dt = UnitSquareMesh(4, 4), 0.02
    probe = _stepper(which, mesh, 1, dt)
    lam = probe._engine.viscosity_number()[0]
    limit = {"ssp2": 4.5198, "implicit": 2.0, "dg": 2.0}[which]
    probe._engine.close()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ts = _stepper(which, mesh, 1, dt, viscosity=0.95 * limit / (dt * lam), wall="no_slip")
    assert ts.viscosity_limit == pytest.approx(limit, abs=1e-3) and ts._engine.viscosity()[1] == "no_slip"
    with pytest.warns(RuntimeWarning, match="viscosity: the diffusion number"):
        _stepper(which, mesh, 1, dt, viscosity=1.05 * limit / (dt * lam))
    with pytest.warns(RuntimeWarning) as rec:  # independent of the tracer check: an unstable kappa does not speak for the viscosity
        _stepper(which, mesh, 1, dt, viscosity=0.5 * limit / (dt * lam), tracer_diffusivity=1e3)
    said = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
    assert len(said) == 1 and said[0].startswith("tracer diffusion"), said


def test_driver_with_the_viscous_taylor_green_vortex(hip_lib, tmp_path):
    nx, k, dt, nsteps, nu = 8, 1, 1e-3, 3, 1e-2
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "taylorgreen", "--nx", str(nx), "--degree", str(k),
                        "--dt", repr(dt), "--tfinal", repr(nsteps * dt), "--timestepper", "implicit", "--use_projection_method",
                        "--viscosity", "1e-2", "--wall", "free_slip", "--output", ""], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "viscosity = 0.01" in r.stdout and "wall = free_slip" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("viscous diffusion number = ")]
    assert len(line) == 1 and line[0].endswith("(limit 2)"), r.stdout
    number = float(line[0].split("=")[1].split()[0])
    assert 0.0 < number < 2.0 and "RuntimeWarning" not in r.stderr
    err = float([ln for ln in r.stdout.splitlines() if ln.startswith("velocity error = ")][0].split("=")[1])
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k)
    omp = ref.TaylorGreenNS(d, "exponential", 0.5, viscosity=nu)
    oQ, _ = ref.implicit_with_viscosity(d, _minv_v("square", nx, k, "free_slip", d), nu, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    want = d.l2_norm_velocity(oQ - omp.solution(nsteps * dt)[0])
    print(f"driver: viscous diffusion number {number}, velocity error {err!r}, reference {want!r}")
    assert err == pytest.approx(want, rel=1e-6)
