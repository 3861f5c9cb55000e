"""Point values on the GPU (hdg_evaluate_points / hdg_set_probes / hdg_get_probes, Function.at, solve(probes=), the driver's
--probes), checked against the numpy checker tests/probe_reference.py, against the recorded state, across steppers, on strips
and through the driver."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import probe_reference as pr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _stepper(kind, k, nx=6, cls=None, **kw):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    mesh = {"square": lambda: UnitSquareMesh(nx, nx), "periodic": lambda: PeriodicSquareMesh(nx, nx, L=2.0),
            "disk": lambda: UnitDiskMesh(3)}[kind]()
    cls = cls or IncompressibleEulerHDGIMEXSSP2_332
    if "use_projection_method" not in kw and "DG" not in cls.__name__:
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, 0.02, **kw), mesh


def _evaluator(ts, mesh, kind, k):
    xq, _ = ts._engine.node_coordinates()
    if kind == "disk":
        return pr.PointEvaluator(k, xq, general=(mesh.vertices, mesh.cells))
    return pr.PointEvaluator(k, xq, square=(mesh.nx, mesh.ny, mesh.L, mesh.periodic))


def _points(kind, mesh, rng):
    if kind == "disk":
        pts = [mesh.vertices, 0.5 * (mesh.vertices[mesh.cells[:, 0]] + mesh.vertices[mesh.cells[:, 1]]),
               0.5 * (mesh.vertices[mesh.cells[:, 1]] + mesh.vertices[mesh.cells[:, 2]])]
        r, th = np.sqrt(rng.random(200)), 2 * np.pi * rng.random(200)
        pts.append(0.999 * np.stack([r * np.cos(th), r * np.sin(th)], axis=1))
        return np.concatenate(pts)
    L, nx = mesh.L, mesh.nx
    h = L / nx
    g = np.arange(nx + 1) * h
    X, Y = np.meshgrid(g, g)
    pts = [np.stack([X.ravel(), Y.ravel()], 1), np.stack([X.ravel() + 0.5 * h, Y.ravel()], 1),
           np.stack([X.ravel(), Y.ravel() + 0.5 * h], 1), np.stack([X.ravel() + 0.5 * h, Y.ravel() + 0.5 * h], 1),
           rng.random((200, 2)) * L]
    xy = np.concatenate(pts)
    if mesh.periodic:
        xy = np.concatenate([xy, rng.random((40, 2)) * 3 * L - L])  # given outside [0, L)
    else:
        xy = xy[(xy[:, 0] <= L) & (xy[:, 1] <= L)]
    return xy


def _rel(a, b):
    """max |a - b| relative to the largest |b| of each column, over the entries that are not NaN in b"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    fin = ~np.isnan(b)
    if not fin.any():
        return 0.0
    scale = np.array([np.max(np.abs(b[fin[:, c], c])) if fin[:, c].any() else 1.0 for c in range(b.shape[1])])
    d = np.where(fin, np.abs(a - b), 0.0) / np.maximum(scale, 1e-300)
    return float(np.max(d)) if np.isnan(a[fin]).sum() == 0 else np.inf


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["square", "periodic", "disk"])
def test_evaluate_points_and_at_agree_with_the_checker(hip_lib, kind, k):
    from incompressibleeulerhdg_amd.mesh import Function

    ts, mesh = _stepper(kind, k)
    eng = ts._engine
    rng = np.random.default_rng(10 * k + len(kind))
    xy = _points(kind, mesh, rng)
    Q = rng.standard_normal(eng.shape_Q)
    p = rng.standard_normal(eng.shape_p)
    q = rng.standard_normal(eng.shape_p)
    ev = _evaluator(ts, mesh, kind, k)
    want, wloc = ev.evaluate(xy, Q, p, q)
    got, loc = eng.evaluate_points(xy, Q, p, q)
    assert np.array_equal(loc, wloc) and loc.all()
    assert _rel(got, want) < 1e-12
    # Function.at: the same values, in Firedrake's shapes
    fu, fp = Function(ts._V_Q, Q), Function(ts._V_p, p)
    assert np.array_equal(fu.at(xy), got[:, 0:2]) and np.array_equal(fp.at(xy), got[:, 2])
    x0, y0 = xy[-1]
    assert fp.at(x0, y0) == got[-1, 2] and fp.at((x0, y0)) == got[-1, 2] and isinstance(fp.at(x0, y0), float)
    assert fu.at([x0, y0]).shape == (2,) and np.array_equal(fu.at([[x0, y0]]), got[-1:, 0:2])
    assert np.array_equal(Function(ts._V_q, q).at(xy[:3]), got[:3, 3])
    # exactness for interpolated polynomials of degree k + 1 (velocity) and k (pressure)
    ux = lambda x, y: 0.3 + x ** (k + 1) - 2 * x * y ** k  # noqa: E731
    uy = lambda x, y: y ** (k + 1) + 0.5 * x ** k * y  # noqa: E731
    curl = lambda x, y: 0.5 * k * x ** (k - 1) * y + 2 * k * x * y ** (k - 1)  # noqa: E731
    pf = lambda x, y: 1.0 - x ** k + x * y ** (k - 1)  # noqa: E731
    Qp = ts._V_Q.interpolate(lambda x, y: (ux(x, y), uy(x, y)))
    pp = ts._V_p.interpolate(pf)
    inside = xy if not mesh.periodic else xy[(xy >= 0).all(1) & (xy < mesh.L).all(1)]
    vals, _ = eng.evaluate_points(inside, Qp, pp)
    x, y = inside.T
    for col, ref in ((0, ux(x, y)), (1, uy(x, y)), (2, pf(x, y)), (4, curl(x, y))):
        assert np.max(np.abs(vals[:, col] - ref)) < 1e-11 * (1 + np.max(np.abs(ref))), col
    assert np.isnan(vals[:, 3]).all()


def test_outside_points(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import Function, PointNotInDomainError
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    for kind, bad in (("square", [1.0 + 1e-9, 0.5]), ("disk", [0.999 * np.cos(0.3), 0.999 * np.sin(0.3)])):
        ts, mesh = _stepper(kind, 1)
        eng = ts._engine
        f = Function(ts._V_p, np.ones(eng.shape_p))
        with pytest.raises(PointNotInDomainError):
            f.at(bad)
        assert f.at([[0.0, 0.0], bad], dont_raise=True)[1] is None
        assert f.at(bad, dont_raise=True) is None
        vals, loc = eng.evaluate_points([[0.0, 0.0], bad], p=np.ones(eng.shape_p))
        assert loc.tolist() == [True, False] and np.isnan(vals[1]).all() and vals[0, 2] == pytest.approx(1.0)
        with pytest.raises(_lib.HDGError, match="point 1") as e:
            eng.set_probes([[0.0, 0.0], bad], 10)
        assert e.value.code == -1
        if kind == "square":
            mp = TaylorGreen(ts._V_Q, ts._V_p)
            ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.02, fused=True)
            assert eng.probes().shape[0] == 0 and ts.probes is None
    with pytest.raises(NotImplementedError):
        from incompressibleeulerhdg_amd.mesh import FunctionSpace

        Function(FunctionSpace(mesh, "CG", 1, np.zeros((3, 2))), np.zeros(3)).at(0.0, 0.0)


STEPPERS = ["imex_fused", "imex_perstep", "implicit", "dg"]


def _run_stepper(which, tracer, probes, diagnostics=False, nx=6, k=2, nt=3):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerDGImplicit, IncompressibleEulerHDGImplicit

    cls = {"implicit": IncompressibleEulerHDGImplicit, "dg": IncompressibleEulerDGImplicit}.get(which)
    ts, mesh = _stepper("square", k, nx=nx, cls=cls)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    q0 = (lambda x, y: np.sin(2 * np.pi * x) * np.cos(np.pi * y)) if tracer else None
    kw = {"fused": which == "imex_fused"} if which.startswith("imex") else {}
    Q0, p0 = mp.initial_condition()
    Q, p = ts.solve(Q0, p0, q0, mp.f_rhs(), nt * ts._dt, probes=probes, diagnostics=diagnostics, **kw)
    lam = eng.get_field(_lib.HDG_STATE_CURRENT, Q=False, p=False)[2]
    its = eng.iteration_stats()
    qf = eng.get_tracer() if tracer else None
    return ts, Q.dat.data.copy(), p.dat.data.copy(), lam.copy(), its, qf, (Q0, p0, q0)


@pytest.mark.parametrize("tracer", [False, True])
@pytest.mark.parametrize("which", STEPPERS)
def test_recording_across_steppers(hip_lib, which, tracer):
    rng = np.random.default_rng(3)
    xy = np.concatenate([rng.random((30, 2)), [[0.5, 0.5], [0.0, 1.0], [1.0, 0.0]]])
    ts, Q, p, lam, its, qf, (Q0, p0, q0) = _run_stepper(which, tracer, xy, diagnostics=True)
    rec = ts.probes
    assert rec["u"].shape == (4, len(xy), 2) and rec["omega"].shape == (4, len(xy)) and rec["t"].shape == (4,)
    assert ts.diagnostics["energy"].shape == (4,)
    eng = ts._engine
    first, _ = eng.evaluate_points(xy, ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0),
                                   ts._V_p.interpolate(q0) if tracer else None)
    last, _ = eng.evaluate_points(xy, Q, p, qf)
    for row, ref in ((0, first), (-1, last)):
        got = np.concatenate([rec["u"][row], rec["p"][row][:, None], rec["q"][row][:, None], rec["omega"][row][:, None]], 1)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        if row == 0:  # hdg_set_state shifts the initial pressure to zero mean: row 0 differs by that constant
            dp = got[:, 2] - ref[:, 2]
            assert np.ptp(dp) <= 1e-13 * np.max(np.abs(ref[:, 2]))
            ref = ref.copy()
            ref[:, 2] += np.mean(dp)
            got[:, 2], ref[:, 2] = 0.0, 0.0
        assert _rel(got, ref) <= 1e-14, row
    assert np.isnan(rec["q"]).all() != tracer
    # recording changes nothing
    _, Q2, p2, lam2, its2, qf2, _ = _run_stepper(which, tracer, None)
    assert np.array_equal(Q, Q2) and np.array_equal(p, p2) and np.array_equal(lam, lam2)
    assert all(np.array_equal(a, b) for a, b in zip(its, its2))
    if tracer:
        assert np.array_equal(qf, qf2)
    if which == "imex_perstep":
        ts_f = _run_stepper("imex_fused", tracer, xy)[0]
        for c in ("u", "p", "q", "omega"):
            assert np.array_equal(ts_f.probes[c], rec[c], equal_nan=True), c


def test_capacity_overflow_reports_dropped_rows(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, _ = _stepper("square", 1)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    eng.set_state(ts._as_nodal_velocity(mp.initial_condition()[0]), ts._as_nodal_pressure(mp.initial_condition()[1]))
    eng.set_probes([[0.25, 0.25], [0.75, 0.5]], 2)
    for _ in range(3):
        eng.step()
    with pytest.raises(_lib.HDGError, match="2 row"):
        eng.probes(reset=False)
    with pytest.raises(_lib.HDGError, match="2 row"):  # reported again, then emptied
        eng.probes(reset=True)
    eng.step()
    assert eng.probes().shape == (1, 2, 5)
    with pytest.raises(_lib.HDGError, match="exceed"):
        eng.set_probes(np.full((1 << 16, 2), 0.5), 1 << 10)
    eng.set_probes(None, 0)


def _strips(nranks, k, nx, nsteps, kind, tmp_path):
    token = "/hdg_probe_" + uuid.uuid4().hex[:12]
    procs, outs = [], []
    for r in range(nranks):
        out = str(tmp_path / f"{kind}{nranks}_{r}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "probe_strip_worker.py"), str(r), str(nranks), token,
                                       str(k), str(nx), str(nsteps), kind, out],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for proc in procs:
            o, _ = proc.communicate(timeout=300)
            logs.append(o.decode(errors="replace"))
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    bad = [r for r, proc in enumerate(procs) if proc.returncode != 0]
    assert not bad, logs[bad[0]][-3000:]
    return [dict(np.load(o)) for o in outs]


@pytest.mark.parametrize("kind", ["square", "periodic"])
def test_strips_match_one_rank(hip_lib, tmp_path, kind):
    k, nx, nsteps = 2, 24, 3
    one = _strips(1, k, nx, nsteps, kind, tmp_path)[0]
    assert one["located"].all()
    for P in (2, 3, 4):
        parts = _strips(P, k, nx, nsteps, kind, tmp_path)
        for d in parts:
            assert np.array_equal(d["vals"], parts[0]["vals"]) and np.array_equal(d["u"], parts[0]["u"])
            assert _rel(d["vals"], one["vals"]) <= 1e-14, P
            assert np.array_equal(d["at_u"], d["vals"][:5, 0:2])
            for c in ("u", "p", "omega"):  # the measure of the other strip tests: relative to the largest value
                assert np.max(np.abs(d[c] - one[c])) < 2e-8 * np.max(np.abs(one[c])), (P, c)
            assert np.isnan(d["q"]).all()


def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("gpus", [1, 2])
def test_driver_probes_match_the_python_api(hip_lib, tmp_path, gpus):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    nx, k, dt, nt = 8, 1, 0.04, 3
    tracer = gpus == 1
    L = 2 * np.pi
    pts = np.array([[0.1, 0.2], [L / 2, L / 2], [3.0, 0.0], [L, L], [1.0, 5.5]])
    (tmp_path / "pts.txt").write_text("# probes\n" + "\n".join(f"{float(x)!r} {float(y)!r}" for x, y in pts) + "\n\n")
    args = ["--problem", "shear", "--nx", str(nx), "--degree", str(k), "--dt", repr(dt), "--tfinal", repr(nt * dt),
            "--output", "", "--probes", "pts.txt", "--probe_output", "p.csv", "--gpus", str(gpus)]
    _driver(args + (["--tracer_advection"] if tracer else []), tmp_path)
    lines = (tmp_path / "p.csv").read_text().strip().splitlines()
    assert lines[0] == "step,t,point,x,y,ux,uy,p,q,omega"
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert rows.shape == ((nt + 1) * len(pts), 10)
    ts = IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(nx, nx, L=L), k, dt, flux="upwind",
                                            use_projection_method=False, n_richardson=2)
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
    q0 = (lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)) if tracer else None
    ts.solve(*mp.initial_condition(), q0, mp.f_rhs(), nt * dt, probes=pts)
    P = ts.probes
    want = np.concatenate([P["u"], P["p"][..., None], P["q"][..., None], P["omega"][..., None]], axis=2).reshape(-1, 5)
    assert np.array_equal(rows[:, 0], np.repeat(np.arange(nt + 1), len(pts)))
    assert np.array_equal(rows[:, 2], np.tile(np.arange(len(pts)), nt + 1))
    assert np.array_equal(np.isnan(rows[:, 5:]), np.isnan(want))
    tol = 0.0 if gpus == 1 else 2e-8
    assert _rel(rows[:, 5:], want) <= tol
    # a point outside the mesh stops the run before the first step, naming the line
    (tmp_path / "bad.txt").write_text("0.1 0.1\n# c\n1e300 nan\n")
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "shear", "--nx", str(nx),
                        "--output", "", "--probes", "bad.txt"], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "bad.txt:3" in r.stderr
