"""The stream function on the GPU (include/hdg_streamfunction.h) against tests/streamfunction_reference.py.

Bounds: 1e-10 relative for the hooks (the project's hook bound); 1e-9 for solves -- the iteration stops at a relative
preconditioned residual of 1e-12 and the preconditioned condition number is a few tens (by the iteration counts of section 27),
so the error of the iterate stays three orders above the stop rule at the most.  The defect is compared relative to itself to
1e-9 beyond the floor of double precision (StreamfunctionReference.defect_floor, the rounding bound of the sums that form
u - curl psi): a well-resolved flow makes the defect as small as 3.5e-8 |u| (Taylor-Green at k = 4, nx = 16), the device and the
twin then differ by 5e-15 |u|, which is 2e-7 of the defect and all that double precision knows of it.
"""
import functools
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import streamfunction_worker as worker
from streamfunction_reference import PSI_K1, PSI_K2, StreamfunctionReference

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
HOOK, SOLVE = 1e-10, 1e-9
L_PER = 2.0


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


@functools.lru_cache(maxsize=None)
def _ref(kind, nx, k):
    return StreamfunctionReference(nx, k, periodic=kind == "periodic", L=L_PER if kind == "periodic" else 1.0)


def _pair(kind, nx, k):
    """(timestepper, engine, reference, ix) with  v_reference[ix] = the vector in the engine's dof order"""
    ts, eng = worker.engine(kind, k, nx)
    ref = _ref(kind, nx, k)
    assert eng.cg_size() == ref.ncg and eng.psi_vertex_count() == ref.nv
    return ts, eng, ref, ref.to_engine(eng.cg_coordinates())


def _zero_sum(rng, n):
    v = rng.standard_normal(n)
    return v - v.mean()


# ---- 1. the hooks against the reference
HOOK_CASES = [("square", 3, k) for k in (1, 2, 3, 4)] + [("periodic", 4, k) for k in (1, 2, 3, 4)] + [("square", 130, 1)]


@pytest.mark.parametrize("kind,nx,k", HOOK_CASES)
def test_hooks_against_the_reference(hip_lib, kind, nx, k):
    _, eng, ref, ix = _pair(kind, nx, k)
    inv = np.empty_like(ix)
    inv[ix] = np.arange(len(ix))  # v_engine[inv] = the vector in the reference's order
    rng = np.random.default_rng(11)
    x, c = rng.standard_normal(ref.ncg), rng.standard_normal(ref.nv)
    errs = {"K": _rel(eng.apply_cg_stiffness(x), (ref.K @ x[inv])[ix]),
            "P": _rel(eng.psi_transfer(c), (ref.P @ c)[ix]),
            "PT": _rel(eng.psi_transfer(x, transpose=True), ref.P.T @ x[inv])}
    # adjointness, constants in the kernel of K, linear functions reproduced at the dof coordinates
    r = rng.standard_normal(ref.ncg)
    lhs, rhs = eng.psi_transfer(r, transpose=True) @ c, r @ eng.psi_transfer(c)
    errs["adjoint"] = abs(lhs - rhs) / (np.linalg.norm(r) * np.linalg.norm(eng.psi_transfer(c)))
    errs["K1"] = np.abs(eng.apply_cg_stiffness(np.ones(ref.ncg))).max() / np.abs(eng.apply_cg_stiffness(x)).max()
    if kind == "square":
        V, X = ref.vertex_coordinates(), eng.cg_coordinates()
        lin = lambda Z: 2.0 * Z[:, 0] - 3.0 * Z[:, 1] + 0.5
        errs["linear"] = _rel(eng.psi_transfer(lin(V)), lin(X))
    else:
        errs["linear"] = _rel(eng.psi_transfer(np.full(ref.nv, 0.7)), np.full(ref.ncg, 0.7))  # (periodic: constants)
    # form 1 of the preconditioner is the diagonal
    errs["jacobi"] = _rel(eng.apply_psi_preconditioner(x, form=1), (x[inv] / ref.K.diagonal())[ix])
    print(f"{kind} nx = {nx} k = {k}: " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
    assert max(errs.values()) < HOOK, errs


# ---- 2. symmetry of the preconditioner (the larger sizes reach the fused legs and the tails of the V-cycle)
@pytest.mark.parametrize("kind,nx", [("square", 8), ("square", 66), ("periodic", 8), ("periodic", 64)])
def test_preconditioner_is_symmetric(hip_lib, kind, nx):
    _, eng = worker.engine(kind, 2, nx)
    rng = np.random.default_rng(12)
    n = eng.cg_size()
    r1, r2 = _zero_sum(rng, n), _zero_sum(rng, n)
    for form in (0, 1):
        z1, z2 = eng.apply_psi_preconditioner(r1, form), eng.apply_psi_preconditioner(r2, form)
        a, b = r1 @ z2, r2 @ z1
        scale = np.sqrt((r1 @ z1) * (r2 @ z2))
        print(f"{kind} nx = {nx} form {form}: (r1, B r2) = {a!r}, (r2, B r1) = {b!r}, |difference| / scale = {abs(a - b) / scale:.2e}")
        assert r1 @ z1 > 0.0 and r2 @ z2 > 0.0
        assert abs(a - b) < HOOK * scale


# ---- 3. exactness: a stream function of the space is recovered
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("nx", [4, 16])
def test_polynomial_stream_function_is_recovered(hip_lib, nx, k):
    ts, eng = worker.engine("square", k, nx)
    fn = PSI_K1 if k == 1 else PSI_K2
    Q = ts._as_nodal_velocity(lambda x, y: fn(x, y)[1])
    X = eng.cg_coordinates()
    exact = fn(X[:, 0], X[:, 1])[0]
    V = X[: (nx + 1) ** 2]  # the vertex dofs come first
    on = (V[:, 0] < 1e-9) | (V[:, 0] > 1 - 1e-9) | (V[:, 1] < 1e-9) | (V[:, 1] > 1 - 1e-9)
    assert on.sum() == 4 * nx
    exact = exact - exact[: (nx + 1) ** 2][on].mean()
    psi, info = eng.streamfunction(Q)
    err = np.abs(psi - exact).max() / np.abs(exact).max()
    print(f"nx = {nx} k = {k}: {info['iterations']} iterations, psi error {err:.2e}, defect / |u| {info['defect'] / info['u_l2']:.2e}")
    assert err < SOLVE
    assert info["defect"] < SOLVE * info["u_l2"]
    assert info["psi_min"] == psi.min() and info["psi_max"] == psi.max()
    assert info["mean_flow_x"] == 0.0 and info["mean_flow_y"] == 0.0


# ---- 4. against the reference: a random velocity and the Taylor-Green state after two steps
SOLVE_CASES = ([(kind, nx, k) for kind in ("square", "periodic") for nx in (4, 16) for k in (1, 2, 3, 4)] +
               [("square", 130, 1), ("square", 66, 2)])


@pytest.mark.parametrize("kind,nx,k", SOLVE_CASES)
def test_solve_against_the_reference(hip_lib, kind, nx, k):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, eng, ref, ix = _pair(kind, nx, k)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q2, _ = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 2 * ts._dt)
    fields = {"random": np.random.default_rng(13).standard_normal(eng.shape_Q), "taylor-green": np.asarray(Q2.dat.data)}
    for name, Q in fields.items():
        psi, info = eng.streamfunction(None if name == "taylor-green" else Q)  # (the stepped state: the engine's own)
        want = ref.solve(Q)
        defect, unorm = ref.defect(Q, want)
        ubar = ref.mean_flow(Q)
        floor = ref.defect_floor(Q, want)  # what double precision leaves of the norm of u - curl psi, twin and device
        errs = {"psi": np.abs(psi - want[ix]).max() / np.abs(want).max(),
                "defect": max(abs(info["defect"] - defect) - floor, 0.0) / defect, "u_l2": abs(info["u_l2"] - unorm) / unorm}
        if kind == "periodic":
            errs["ubar"] = np.abs(np.array([info["mean_flow_x"], info["mean_flow_y"]]) - ubar).max() / max(np.abs(ubar).max(), unorm / ref.L)
        print(f"{kind} nx = {nx} k = {k} {name}: {info['iterations']} iterations, defect / |u| = {defect / unorm:.3e} (device - twin: "
              f"{info['defect'] - defect:.2e}, floor {floor:.2e}), " + ", ".join(f"{n} {e:.2e}" for n, e in errs.items()))
        assert max(errs.values()) < SOLVE, (name, errs)
        assert info["residual"] <= 1e-12 and info["psi_min"] == psi.min() and info["psi_max"] == psi.max()
        gauge = psi[: ref.nv].mean() if kind == "periodic" else (ref.gauge[ix] @ psi)
        assert abs(gauge) < 1e-13 * max(np.abs(psi).max(), 1e-300)


def test_constant_velocity_on_the_periodic_square(hip_lib):
    _, eng = worker.engine("periodic", 2, 8)
    Q = np.tile([0.75, -1.25], (eng.shape_Q[0], 1))
    psi, info = eng.streamfunction(Q)
    print(f"constant velocity: max |psi| = {np.abs(psi).max():.2e}, ubar = ({info['mean_flow_x']!r}, {info['mean_flow_y']!r}), "
          f"defect = {info['defect']:.2e}, {info['iterations']} iterations")
    assert np.abs(psi).max() < 1e-13
    assert abs(info["mean_flow_x"] - 0.75) < 1e-13 and abs(info["mean_flow_y"] + 1.25) < 1e-13
    assert info["defect"] < 1e-13 * info["u_l2"]


# ---- 5. the coarse level works
def test_the_coarse_level_works(hip_lib):
    """conditions, not measurements: the default iterations at nx = 16 are at most 1.25 times those at nx = 8 and at most half
    of those of the diagonal alone (HDG_PSI_JACOBI=1, read when an engine is built: a process of its own) at nx = 16"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "streamfunction_worker.py"), "iterations"],
                       env=dict(os.environ, HDG_PSI_JACOBI="1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert r.returncode == 0, r.stdout.decode()[-2000:]
    jacobi = {tuple(line.split()[:3]): int(line.split()[3]) for line in r.stdout.decode().splitlines() if line.split()[:1] in (["square"], ["periodic"])}
    assert len(jacobi) == len(worker.ITERATION_CASES)
    for kind in ("square", "periodic"):
        for k in (2, 4):
            its = {nx: worker.iterations(kind, k, nx) for nx in (8, 16)}
            jac = jacobi[(kind, str(k), "16")]
            print(f"{kind} k = {k}: default {its[8]} -> {its[16]} iterations, the diagonal alone at nx = 16: {jac}")
            assert its[16] <= 1.25 * its[8]
            assert its[16] <= 0.5 * jac


# ---- 6. determinism and non-interference
def _three_steps(call):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, eng = worker.engine("square", 2, 5)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    out = []
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
        if call and n < 2:
            omega = eng.vorticity()
            out.append(ts.streamfunction())
            assert np.array_equal(eng.vorticity(), omega)  # the scratch vectors are shared, the results are not
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return dict(Q=Q, p=p, its=eng.iteration_stats(), digest=eng.state_digest(), census=census, psi=out)


def test_two_calls_same_bits_and_the_step_path_untouched(hip_lib):
    _, eng = worker.engine("periodic", 3, 6)
    Q = np.random.default_rng(14).standard_normal(eng.shape_Q)
    a, ia = eng.streamfunction(Q)
    eng.vorticity(Q)
    b, ib = eng.streamfunction(Q)
    assert np.array_equal(a, b) and ia == ib
    base, run = _three_steps(False), _three_steps(True)
    assert np.array_equal(run["Q"], base["Q"]) and np.array_equal(run["p"], base["p"])
    assert all(np.array_equal(x, y) for x, y in zip(run["its"], base["its"]))
    assert run["digest"] == base["digest"] and run["census"] == base["census"]
    assert all(psi.name() == "streamfunction" and psi.info["iterations"] > 0 for psi in run["psi"])


# ---- 7. refusals
def test_refusals(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    _, eng = worker.engine("square", 2, 4)
    x = np.zeros(eng.cg_size())
    with pytest.raises(_lib.HDGError, match="rtol") as e:
        eng.streamfunction(rtol=0.0)
    assert e.value.code == -1
    eng.begin_step()  # while a step is open
    for call in (eng.streamfunction, lambda: eng.apply_cg_stiffness(x), lambda: eng.apply_psi_preconditioner(x),
                 lambda: eng.psi_transfer(x, transpose=True), eng.psi_vertex_count):
        with pytest.raises(_lib.HDGError, match="a step is open") as e:
            call()
        assert e.value.code == -1
    # a general mesh
    disk = IncompressibleEulerHDGIMEXSSP2_332(UnitDiskMesh(1), 2, 0.01, use_projection_method=True, n_richardson=2)
    for call in (disk._engine.streamfunction, disk._engine.psi_vertex_count, disk.streamfunction):
        with pytest.raises(_lib.HDGError, match="general meshes") as e:
            call()
        assert e.value.code == -5
    # a strip partition of two ranks
    token = "/hdg_psi_" + uuid.uuid4().hex[:12]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "streamfunction_worker.py"), "strip", str(r), "2", token],
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
    assert [pr.returncode for pr in procs] == [0, 0], [log[-2000:] for log in logs]
    assert all(log.count("refused -5") == 2 for log in logs), logs


# ---- 8. surface
def test_animation_callback_writes_the_stream_function(hip_lib, tmp_path, monkeypatch):
    from incompressibleeulerhdg_amd.auxilliary.callbacks import AnimationCallback
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    monkeypatch.chdir(tmp_path)
    for flag, name in ((True, "with.pvd"), (False, "without.pvd")):
        ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(4, 4), 1, 0.05, use_projection_method=True, n_richardson=2,
                                                callbacks=[AnimationCallback(name, streamfunction=True) if flag else AnimationCallback(name)])
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.05)
    assert 'Name="streamfunction"' in (tmp_path / "with_1.vtu").read_text() and 'Name="vorticity"' in (tmp_path / "with_1.vtu").read_text()
    assert "streamfunction" not in (tmp_path / "without_1.vtu").read_text()
    psi = ts.streamfunction()
    assert psi.name() == "streamfunction" and psi.dat.data.shape == (ts._engine.n_cells * ts._engine.n_u,) and psi.info["iterations"] > 0


def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver"] + args + ["--output", ""], cwd=cwd,
                       env=dict(os.environ, PYTHONPATH=os.path.dirname(HERE)), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    return r.returncode, r.stdout.decode()


def test_driver_prints_the_stream_function(hip_lib, tmp_path):
    import re

    args = ["--problem", "cavity", "--nx", "8", "--degree", "2", "--dt", "0.01", "--tfinal", "0.02", "--use_projection_method",
            "--viscosity", "1e-2", "--wall", "no_slip", "--wall_velocity", "top", "1"]
    rc, plain = _driver(args, tmp_path)
    assert rc == 0 and "stream function" not in plain, plain[-2000:]
    rc, out = _driver(args + ["--streamfunction"], tmp_path)
    assert rc == 0, out[-2000:]
    lines = [line for line in out.splitlines() if line.startswith("stream function:")]
    assert len(lines) == 1 and re.search(r"min = \S+ at \(\S+, \S+\), max = \S+ at \(\S+, \S+\), defect = \S+, iterations = \d+$", lines[0]), lines
    # the flag adds its line and the blank one behind it, nothing else: the rows of the timer table aside (wall-clock times),
    # the output without the flag is the output with it less those two lines
    timed = re.compile(r"^\s*\S+ : +\d+ +\S+ +\S+ +\S+$|^\s*solve time\s+=")
    a, b = plain.splitlines(), out.splitlines()
    at = b.index(lines[0])
    assert b[at + 1] == ""
    del b[at:at + 2]
    assert len(a) == len(b) and any(ln.startswith("state digest") for ln in a)
    differ = [(x, y) for x, y in zip(a, b) if x != y and not (timed.match(x) and timed.match(y) and x.split()[0] == y.split()[0])]
    assert not differ, differ
    # refused before any engine is built
    base = ["--nx", "8", "--degree", "1", "--dt", "0.05", "--tfinal", "0.1", "--use_projection_method", "--streamfunction"]
    for more, word in ((["--gpus", "2"], "--gpus 2"), (["--problem", "kelvinhelmholtz"], "kelvinhelmholtz")):
        rc, out = _driver(base + more, tmp_path)
        assert rc != 0 and "--streamfunction does not support" in out and word in out, out[-2000:]
