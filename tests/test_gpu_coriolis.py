"""The Coriolis term on the GPU (include/hdg_coriolis.h) against tests/coriolis_reference.py.

Bounds, the project's: the hook relative 1e-10; whole steps and strips 2e-8 for Q and p; the manufactured solution's L2 error
relative 1e-6 against the reference's.  Switched off, everything is bitwise what it is without the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid
import warnings

import numpy as np
import pytest

import coriolis_reference as ref
import viscosity_reference as vref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL = 1e-10, 2e-8
L_PER = 2 * np.pi
NUMBER = 0.3  # F dt of the whole-step runs
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


def _minv_c(kind, nx, k, f0, beta, d):
    """M^-1 C of the reference: once per mesh, degree and (f0, beta); read-only"""
    key = (kind, nx, k, f0, beta)
    if key not in _A:
        A = ref.minv_c(d, f0, beta)
        A.setflags(write=False)
        _A[key] = A
    return _A[key]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.setdefault("use_projection_method", True)
        kw.update(n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _pair(case, kind, dt, number=NUMBER):
    """(f0, beta) with F dt = number.  'beta0': plain rotation.  'equator': f_c changes sign inside the mesh (unit square: from
    -F at y = 0 to F at y = 1; a general mesh spanning y = -1 .. 1: from -0.4 F to F)."""
    F = number / dt
    if case == "beta0":
        return F, 0.0
    return (-F, 2.0 * F) if kind == "square" else (0.3 * F, 0.7 * F)


# ---- 1. the hook against the reference
SQUARE_PAIRS = [(1.3, 0.0), (0.0, 2.1), (-1.3, 2.6)]  # the third: an equator inside the mesh
HOOK_CASES = ([("square", 3, k, SQUARE_PAIRS) for k in (1, 2, 3, 4)] + [("periodic", 4, k, [(1.3, 0.0)]) for k in (1, 2, 3, 4)] +
              [("disk", 1, 2, [(0.4, 2.1)]), ("perturbed", 3, 1, [(-1.3, 2.6)])])


@pytest.mark.parametrize("kind,nx,k,pairs", HOOK_CASES)
def test_hook_against_the_reference(hip_lib, kind, nx, k, pairs):
    mesh, d = _mesh_and_oracle(kind, nx, k)
    X = d.node_coords(d.PU).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(31 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = lambda: sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    poly = np.stack([1.0 + x - 2.0 * y + (x * y if k > 1 else 0.0) + (y ** k), 0.5 - y + 0.3 * x - (x ** k)], axis=-1)  # degree <= k
    fields = [np.stack([smooth(), smooth()], axis=-1), rng.standard_normal((len(x), 2)), poly]
    eng = _stepper("ssp2", mesh, k, 0.01)._engine
    M = d.MQ
    mnorm = lambda v: float(np.sqrt(v.ravel() @ (M @ v.ravel())))
    worst = work = closed = 0.0
    for f0, beta in pairs:
        A = _minv_c(kind, nx, k, f0, beta, d)
        for n, Q in enumerate(fields):
            want = (A @ Q.ravel()).reshape(-1, 2)
            got = eng.apply_coriolis(Q, f0, beta)
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            worst = max(worst, err)
            assert err <= HOOK, (f0, beta, n, err)
            wk = abs(Q.ravel() @ (M @ got.ravel())) / (mnorm(Q) * mnorm(got))  # the term does no work
            work = max(work, wk)
            assert wk <= HOOK, (f0, beta, n, wk)
        exact = ref.closed_form(f0, beta, x, y, poly)
        cf = np.max(np.abs(eng.apply_coriolis(poly, f0, beta) - exact)) / np.max(np.abs(exact))
        closed = max(closed, cf)
        assert cf <= HOOK, (f0, beta, cf)
        assert eng.coriolis() == (0.0, 0.0) and eng.coriolis_number() == (0.0, 0.0)  # the hook and the query set nothing
    for f0, beta in pairs:
        eng.set_coriolis(f0, beta)
        F, number = eng.coriolis_number()
        rho = np.max(np.abs(np.linalg.eigvals(_minv_c(kind, nx, k, f0, beta, d))))
        assert eng.coriolis() == (f0, beta)
        assert F == pytest.approx(ref.vertex_bound(d, f0, beta), rel=1e-13) and number == pytest.approx(0.01 * F, rel=1e-14)
        assert F >= rho * (1 - 1e-12), (f0, beta, F, rho)
        print(f"{kind} nx={nx} k={k} f0={f0} beta={beta}: F {F:.6g}, rho {rho:.6g}")
    print(f"{kind} nx={nx} k={k}: largest |out - reference| = {worst:.3e} max|out|; against the closed form {closed:.3e}; "
          f"|Q^T M out| {work:.3e} |Q|_M |out|_M")
    eng.close()


# ---- 2. whole steps against the reference loop
def _initial(kind, d):
    """nodal initial velocity and pressure: the Taylor-Green field (square), the shear layer (periodic square) or a vortex
    (disk), plus a broken part, as the viscous term's whole-step runs start"""
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


_forcing = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))

CONFIGS = {
    "ssp2-k1": ("ssp2", "square", 1, 6, {}), "ssp2-k2": ("ssp2", "square", 2, 4, {}), "ars2-k2": ("ars2", "square", 2, 4, {}),
    "ssp2-unsplit-k1": ("ssp2", "square", 1, 6, {"use_projection_method": False}),
    "implicit-k1": ("implicit", "square", 1, 6, {}), "dg-k1": ("dg", "square", 1, 6, {}),
    "ssp2-periodic-k1": ("ssp2", "periodic", 1, 6, {}), "ssp2-disk-k2": ("ssp2", "disk", 2, 1, {}),
}
RUNS = ([(name, fused, case) for name in ("ssp2-k1", "ssp2-k2") for fused in (True, False) for case in ("beta0", "equator")] +
        [(name, True, "beta0" if name == "ssp2-periodic-k1" else "equator") for name in CONFIGS if name not in ("ssp2-k1", "ssp2-k2")])
_WANT = {}


def _reference_runs(key, which, d, A, dt, nsteps, Q0, p0, of, kw):
    """(with rotation, without): once per configuration, shared by the fused and the per-solve run; read-only"""
    from oracle import hdg_oracle as orc

    if key in _WANT:
        return _WANT[key]
    out = []
    for v in (1.0, 0.0):
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


@pytest.mark.parametrize("name,fused,case", RUNS)
def test_whole_steps_against_the_reference_loop(hip_lib, name, fused, case):
    which, kind, k, nx, kw = CONFIGS[name]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps = 3
    dt = 0.02 if kind == "disk" else 0.25 * d.mesh.h
    f0, beta = _pair(case, kind, dt)
    if which in ("implicit", "dg"):  # forward Euler at F dt = 0.3: the warning is expected
        with pytest.warns(RuntimeWarning, match="rotation: at the rotation number"):
            ts = _stepper(which, mesh, k, dt, coriolis=(f0, beta), **kw)
    else:
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # SSP2(3,3,2) below 0.337, ARS2(2,3,2) below sqrt 3: silent
            ts = _stepper(which, mesh, k, dt, coriolis=(f0, beta), **kw)
    assert ts._engine.coriolis() == (f0, beta) and ts._engine.coriolis_number()[1] == pytest.approx(NUMBER, rel=1e-12)
    Q0, p0 = _initial(kind, d)
    of = lambda t: d.interpolate_velocity(_forcing(t))
    (oQ, op), (pQ, pp) = _reference_runs((name, case), which, d, _minv_c(kind, nx, k, f0, beta, d), dt, nsteps, Q0, p0, of, kw)
    Q, p = ts.solve(Q0, p0, None, _forcing, nsteps * dt, **({"fused": fused} if which in ("ssp2", "ars2") else {}))
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ)), np.max(np.abs(op - pp)) / np.max(np.abs(op))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"{name} fused={fused} {case}: f0 {f0:.4g} beta {beta:.4g}; with / without rotation differ by {seen[0]:.3e} max|Q|, "
          f"{seen[1]:.3e} max|p|; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert min(seen) >= 1e-2, "the comparison shows nothing: the reference does not see the rotation"
    assert max(errs) < TOL, errs


def test_forcing_buoyant_diffusing_tracer_viscosity_and_rotation_together(hip_lib):
    """both velocity-linear terms on: k_viscosity writes a slot and k_coriolis accumulates into it"""
    import tracer_diffusion_reference as tdref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    which, kind, k, nx, kw = CONFIGS["ssp2-k1"]
    mesh, d = _mesh_and_oracle(kind, nx, k)
    nsteps, dt, wall, bbeta, g = 3, 0.25 * d.mesh.h, "no_slip", 2.0, (0.3, -1.0)
    f0, beta = _pair("equator", kind, dt)
    ts = _stepper(which, mesh, k, dt, buoyancy=bbeta, gravity=g, coriolis=(f0, beta))
    eng = ts._engine
    eng.set_viscosity(1.0, wall)
    nu = 0.35 / (dt * eng.viscosity_number()[0])
    eng.set_viscosity(nu, wall)
    kappa = 0.35 / (dt * eng.tracer_diffusion_number()[0])
    eng.set_tracer_diffusivity(kappa)
    Q0, p0 = _initial(kind, d)
    q0 = lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y
    of = lambda t: d.interpolate_velocity(_forcing(t))
    A = nu * vref.minv_v(d, wall) + _minv_c(kind, nx, k, f0, beta, d)
    runs = []
    for B in (A, nu * vref.minv_v(d, wall)):
        o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
        runs.append(ref.imex_with_viscosity(o, B, 1.0, Q0, p0, of, nsteps * dt, tr=TracerOracle(d), q0=d.interpolate_pressure(q0),
                                            beta=bbeta, g=g, kappa=kappa, Adiff=tdref.minv_d(d)))
    (oQ, op, oq), (pQ, pp, _) = runs
    Q, p = ts.solve(Q0, p0, q0, _forcing, nsteps * dt, fused=True)
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ)), np.max(np.abs(op - pp)) / np.max(np.abs(op))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op), _rel(ts.q_tracer.dat.data, oq)
    print(f"forcing + buoyancy + tracer diffusion + viscosity + rotation: with / without rotation differ by {seen[0]:.3e} max|Q|, "
          f"{seen[1]:.3e} max|p|; Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
    assert min(seen) >= 1e-2
    assert max(errs) < TOL, errs


# ---- 3. the manufactured rotating Taylor-Green solution
@pytest.mark.parametrize("k,nx", [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_manufactured_rotating_taylor_green_error_equals_the_reference(hip_lib, k, nx):
    from incompressibleeulerhdg_amd.model_problems import RotatingTaylorGreen

    mesh, d = _mesh_and_oracle("square", nx, k)
    nsteps, dt, kappa = 3, 0.25 * d.mesh.h, 0.5
    f0, beta = _pair("equator", "square", dt)
    with pytest.warns(RuntimeWarning, match="rotation: at the rotation number"):
        ts = _stepper("implicit", mesh, k, dt, coriolis=(f0, beta))
    mp = RotatingTaylorGreen(ts._V_Q, ts._V_p, "exponential", kappa, coriolis=(f0, beta))
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt)
    omp = ref.RotatingTaylorGreen(d, kappa, 0.0, (f0, beta))
    oQ, op = ref.implicit_with_viscosity(d, _minv_c("square", nx, k, f0, beta, d), 1.0, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    amp = np.exp(-kappa * nsteps * dt)
    e_dev, e_ref = ref.l2_error_velocity(d, Q.dat.data, amp), ref.l2_error_velocity(d, oQ, amp)
    print(f"k={k} nx={nx}: f0 {f0:.4g} beta {beta:.4g}; L2 error device {e_dev:.10e}, reference {e_ref:.10e}; fields differ by {_rel(Q.dat.data, oQ):.3e}")
    assert abs(e_dev - e_ref) <= 1e-6 * e_ref


# ---- 4. off is off; 5. on, the launches it adds
def _three_steps(mode, nu=0.0):
    """Fields, iteration counts, digest, checkpoint blob and the launch census of the third of three fused steps."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if nu:
        eng.set_viscosity(nu, "no_slip")
    if mode == "zero":
        eng.set_coriolis(0.0, 0.0)
    elif mode == "on_then_zero":
        eng.set_coriolis(1.5, -2.0)
        eng.set_coriolis(0.0)
    elif mode == "on":
        eng.set_coriolis(1.5, -2.0)
    elif mode == "on_faintly":
        eng.set_coriolis(1e-16, -2e-16)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(census=census, Q=Q, p=p, its=eng.iteration_stats(), digest=eng.state_digest(), blob=eng.save_checkpoint(3, 0.06))


def _same(r, base, what):
    assert r["census"] == base["census"], what
    for name in ("Q", "p"):
        assert np.array_equal(r[name], base[name]), (what, name)
    assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), what
    assert r["digest"] == base["digest"], what
    assert r["blob"] == base["blob"] and b"coriolis" not in r["blob"], what


def test_switched_off_nothing_changes_and_switched_on_the_launches_it_adds(hip_lib):
    base = _three_steps("unset")
    for mode in ("zero", "on_then_zero"):
        _same(_three_steps(mode), base, mode)
    # viscosity on, rotation off: bitwise the viscous run
    vbase = _three_steps("unset", nu=1e-3)
    for mode in ("zero", "on_then_zero"):
        _same(_three_steps(mode, nu=1e-3), vbase, "viscous " + mode)
    # switched on, with values too faint to move an iteration count (asserted)
    faint = _three_steps("on_faintly")
    assert all(np.array_equal(a, b) for a, b in zip(faint["its"], base["its"]))
    more = {c: faint["census"][c] - base["census"][c] for c in base["census"] if faint["census"][c] != base["census"][c]}
    print(f"rotation alone: launches per step beyond the plain run: {more}")
    # s + 1 = 4 launches of k_coriolis per SSP2(3,3,2) step; the sum in front of the pressure reconstruction; as section 21
    assert more == {"other": 4, "vector_update": 1}, more
    assert b"coriolis_f0" in faint["blob"] and b"coriolis_beta" in faint["blob"]
    vfaint = _three_steps("on_faintly", nu=1e-3)
    assert all(np.array_equal(a, b) for a, b in zip(vfaint["its"], vbase["its"]))
    more = {c: vfaint["census"][c] - vbase["census"][c] for c in vbase["census"] if vfaint["census"][c] != vbase["census"][c]}
    print(f"rotation beside viscosity: launches per step beyond the viscous run: {more}")
    assert more == {"other": 4}, more  # the accumulating launches; the slot vectors and every sum are the viscous term's
    assert _rel(_three_steps("on")["Q"], base["Q"]) > 1e-3


# ---- 6. strips: two ranks over shared memory against one rank
def _ranks(nranks, kind, tmp_path):
    token = "/hdg_cor_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"{kind}{nranks}_{r}.npz") for r in range(nranks)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "coriolis_strip_worker.py"), str(r), str(nranks), token, kind, outs[r]],
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


@pytest.mark.parametrize("kind", ["square", "periodic"])
def test_two_strips_match_one_rank(hip_lib, tmp_path, kind):
    parts = _ranks(2, kind, tmp_path)
    single = _ranks(1, kind, tmp_path)[0]
    Q, p = np.concatenate([d["Q"] for d in parts]), np.concatenate([d["p"] for d in parts])
    errs = _rel(Q, single["Q"]), _rel(p, single["p"])
    print(f"{kind}: two strips against one rank: Q {errs[0]:.3e}, p {errs[1]:.3e}; f0 {float(single['f0']):.4g}, beta {float(single['beta']):.4g}")
    assert all(float(d["f0"]) == float(single["f0"]) and float(d["beta"]) == float(single["beta"]) and
               float(d["number"]) == pytest.approx(NUMBER, rel=1e-12) for d in parts)
    assert max(errs) < TOL, errs


# ---- 7. checkpoint
def _ck_engine(pair):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if pair is not None:
        eng.set_coriolis(*pair)
    return ts, eng


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_f0_and_beta(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    pair = (1.5, -2.0)
    ts, eng = _ck_engine(pair)
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"coriolis_f0" in blob and b"coriolis_beta" in blob
    for n in range(2):
        eng.step()
    ts2, eng2 = _ck_engine(pair)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    for other in ((1.5, 0.0), (2.5, -2.0), (0.0, 0.0), None):
        _, eng3 = _ck_engine(other)
        with pytest.raises(_lib.HDGError, match="coriolis|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


def test_a_stepper_restarts_with_its_rotation(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import RotatingTaylorGreen, TaylorGreen

    def run(T, **kw):
        ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, coriolis=(2.0, 4.0))
        mp = RotatingTaylorGreen(ts._V_Q, ts._V_p, coriolis=(2.0, 4.0))
        Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T, fused=True, **kw)
        return Q.dat.data.copy(), p.dat.data.copy()

    path = str(tmp_path / "run.ck")
    run(0.04, checkpoint=path)
    whole, resumed = run(0.08), run(0.08, restart=path)
    for a, b in zip(whole, resumed):
        assert np.array_equal(a, b)
    plain = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    mp = TaylorGreen(plain._V_Q, plain._V_p)
    with pytest.raises(_lib.HDGError, match="coriolis|fingerprint"):
        plain.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.08, fused=True, restart=path)


# ---- 8. errors
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    eng = ts._engine
    rng = np.random.default_rng(3)
    eng.set_state(rng.standard_normal(eng.shape_Q), rng.standard_normal(eng.shape_p))
    eng.set_coriolis(1.5, -2.0)
    eng_Q, eng_p = ts._current()

    def untouched(e=eng, tsx=ts, want=(1.5, -2.0), fields=(eng_Q, eng_p)):
        assert e.coriolis() == want  # a refused call leaves the setting ...
        Q, p = tsx._current()
        assert np.array_equal(Q, fields[0]) and np.array_equal(p, fields[1])  # ... and the fields

    for bad in (float("nan"), float("inf"), -float("inf")):
        for args in ((bad, 0.0), (1.0, bad)):
            with pytest.raises(_lib.HDGError, match="not both finite") as e:
                eng.set_coriolis(*args)
            assert e.value.code == -1
            with pytest.raises(_lib.HDGError, match="not both finite"):
                eng.apply_coriolis(eng_Q, *args)
            untouched()
    # beta != 0 on the doubly periodic square: set and hook; f0 alone is fine there
    tp = _stepper("ssp2", PeriodicSquareMesh(4, 4, L=L_PER), 1, 0.02)
    ep = tp._engine
    ep.set_state(rng.standard_normal(ep.shape_Q), rng.standard_normal(ep.shape_p))
    ep.set_coriolis(0.7)
    pQ, pp = tp._current()
    with pytest.raises(_lib.HDGError, match="doubly periodic") as e:
        ep.set_coriolis(0.7, 0.1)
    assert e.value.code == -1
    with pytest.raises(_lib.HDGError, match="doubly periodic"):
        ep.apply_coriolis(pQ, 0.0, 0.1)
    untouched(ep, tp, (0.7, 0.0), (pQ, pp))
    ep.close()
    eng.begin_step()  # while a step is open
    with pytest.raises(_lib.HDGError, match="a step is open") as e:
        eng.set_coriolis(0.0)
    assert e.value.code == -1
    with pytest.raises(_lib.HDGError, match="a step is open"):
        eng.apply_coriolis(eng_Q, 1.0)
    assert eng.coriolis() == (1.5, -2.0)


# ---- 9. the driver
def test_driver_with_the_rotating_taylor_green_vortex(hip_lib, tmp_path):
    nx, k, dt, nsteps = 8, 1, 1e-3, 3
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "taylorgreen", "--nx", str(nx), "--degree", str(k),
                        "--dt", repr(dt), "--tfinal", repr(nsteps * dt), "--timestepper", "implicit", "--use_projection_method",
                        "--coriolis", "2", "4", "--output", ""], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "coriolis = 2.0 4.0" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("rotation number F dt = ")]
    assert len(line) == 1 and "(growth per inertial period " in line[0], r.stdout
    number = float(line[0].split("=")[1].split()[0])
    per_period = float(line[0].split("period")[1].strip(" )"))
    assert number == pytest.approx(6e-3, rel=1e-5)  # F = |2 + 4 * 1|
    assert per_period == pytest.approx((np.sqrt(1 + number ** 2) - 1) * 2 * np.pi / number, rel=1e-4)
    assert "RuntimeWarning" in r.stderr and "rotation" in r.stderr  # forward Euler above 3.2e-3
    err = float([ln for ln in r.stdout.splitlines() if ln.startswith("velocity error = ")][0].split("=")[1])
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k)
    omp = ref.RotatingTaylorGreen(d, 0.5, 0.0, (2.0, 4.0))
    oQ, _ = ref.implicit_with_viscosity(d, _minv_c("square", nx, k, 2.0, 4.0, d), 1.0, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    want = d.l2_norm_velocity(oQ - omp.solution(nsteps * dt)[0])
    print(f"driver: rotation number {number}, velocity error {err!r}, reference {want!r}")
    assert err == pytest.approx(want, rel=1e-6)
