"""Lagrangian particles on the GPU (hdg_set_particles / hdg_get_particles / hdg_advance_particles, solve(particles=), the
driver's --particles): closed forms through the C-ABI, the numpy checker tests/particle_reference.py fed with the fields of the
same run, every stepper, strips and the driver."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import particle_reference as par
import probe_reference as pr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _stepper(kind, k, nx=6, cls=None, dt=0.02, **kw):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    mesh = {"square": lambda: UnitSquareMesh(nx, nx), "periodic": lambda: PeriodicSquareMesh(nx, nx, L=2.0),
            "disk": lambda: UnitDiskMesh(3)}[kind]()
    cls = cls or IncompressibleEulerHDGIMEXSSP2_332
    if "use_projection_method" not in kw and "DG" not in cls.__name__:
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, dt, **kw), mesh


def _set_velocity(ts, u):
    eng = ts._engine
    eng.set_state(ts._V_Q.interpolate(u), np.zeros(eng.shape_p))


# ---- 1. closed form: a rigid rotation is in [P_{k+1}]^2, and one Heun step of it is a linear map
@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["square", "periodic"])
def test_frozen_rotation_is_the_linear_map_of_heun(hip_lib, kind, k):
    ts, mesh = _stepper(kind, k, nx=8)
    eng, L = ts._engine, mesh.L
    c = 0.5 * L
    _set_velocity(ts, lambda x, y: (-(y - c), x - c))
    th = np.linspace(0.0, 2 * np.pi, 13)[:-1] + 0.1
    xy = np.concatenate([c + r * L * np.stack([np.cos(th), np.sin(th)], 1) for r in (0.07, 0.23, 0.41, 0.47)])
    dt, m = 0.05, 160  # 8 rad: more than a revolution through the 8 x 8 cells; the radius grows by (1 + dt^4 / 4)^(m / 2)
    eng.set_particles(xy, 4)
    eng.advance_particles(dt, m)
    rows, counts = eng.particles(reset=False)
    assert rows.shape == (2, len(xy), 2) and np.array_equal(rows[0], xy)
    assert counts == {"clamped": 0, "lost": 0, "dropped": 0}
    J = np.array([[0.0, -1.0], [1.0, 0.0]])
    M = np.linalg.matrix_power(np.eye(2) + dt * J + 0.5 * dt * dt * (J @ J), m)
    want = (xy - c) @ M.T + c
    err = np.max(np.abs(rows[1] - want))
    print(f"{kind} k={k}: max deviation from the linear map {err:.3e} (L = {L})")
    assert np.max(np.abs(want - xy)) > 0.05 * L  # they did move
    assert err <= 1e-12 * L
    # two calls of m / 2 steps: the same trajectory (k1 and X* are rebuilt for the dt of the call), one row each
    eng.set_particles(xy, 4)
    eng.advance_particles(dt, m // 2)
    eng.advance_particles(dt, m // 2)
    rows2, _ = eng.particles()
    assert rows2.shape[0] == 3 and np.array_equal(rows2[2], rows[1])
    eng.set_particles(None, 0)


# ---- 2. seam and boundary
def test_uniform_flow_crosses_the_seam_unwrapped(hip_lib):
    ts, mesh = _stepper("periodic", 2, nx=6)
    eng, L = ts._engine, mesh.L
    _set_velocity(ts, lambda x, y: (1.0 + 0 * x, 0.5 + 0 * x))
    rng = np.random.default_rng(2)
    xy = np.concatenate([rng.random((20, 2)) * L, [[0.0, 0.0], [L, L], [-0.25 * L, 3.5 * L]]])
    dt, m = 0.1, 100  # t = 10: five crossings of the domain in x
    eng.set_particles(xy, 2)
    eng.advance_particles(dt, m)
    rows, counts = eng.particles()
    err = np.max(np.abs(rows[1] - (xy + m * dt * np.array([1.0, 0.5]))))
    print(f"periodic uniform flow: max deviation {err:.3e}")
    assert err <= 1e-12 * L and counts["clamped"] == 0 and counts["lost"] == 0
    eng.set_particles(None, 0)


def test_uniform_flow_stops_on_the_boundary_of_the_unit_square(hip_lib):
    ts, mesh = _stepper("square", 2, nx=6)
    eng, L = ts._engine, mesh.L
    u = np.array([1.0, 0.5])
    _set_velocity(ts, lambda x, y: (u[0] + 0 * x, u[1] + 0 * x))
    xy = np.random.default_rng(4).random((24, 2)) * L
    dt, m = 0.1, 12
    eng.set_particles(xy, 4)
    eng.advance_particles(dt, m)
    rows, counts = eng.particles(reset=False)
    want, nclamp, _ = par.heun(lambda s, X: np.tile(u, (len(X), 1)), xy, dt, m, L=L)
    assert np.isfinite(rows).all() and rows.min() >= 0.0 and rows.max() <= L
    assert (rows[1][:, 0] == L).all()  # every particle has reached x = L by t = 1.2 and stays there
    assert np.max(np.abs(rows[1] - want[-1])) <= 1e-12 * L
    assert counts["clamped"] == nclamp > 0 and counts["lost"] == 0
    eng.advance_particles(dt, 20)  # t = 3.2: the corner
    rows, counts = eng.particles()
    assert np.array_equal(rows[2], np.full_like(xy, L)) and counts["lost"] == 0
    eng.set_particles(None, 0)


def test_a_particle_in_a_non_finite_velocity_is_lost_not_faulted(hip_lib):
    ts, mesh = _stepper("periodic", 1, nx=6)
    eng, L = ts._engine, mesh.L
    h = L / 6
    Q = ts._V_Q.interpolate(lambda x, y: (1.0 + 0 * x, 0 * x))
    xq = eng.node_coordinates()[0]
    Q[(xq[:, 0] > 4 * h) & (xq[:, 0] < 5 * h) & (xq[:, 1] < h)] = np.inf  # the interior nodes of the cells (4, 0)
    eng.set_state(Q, np.zeros(eng.shape_p))
    xy = np.array([[3.5 * h, 0.4 * h], [0.5 * h, 2.5 * h]])
    eng.set_particles(xy, 2)
    eng.advance_particles(0.25 * h, 12)
    rows, counts = eng.particles()
    assert np.isnan(rows[1][0]).all() and counts["lost"] == 1
    assert np.max(np.abs(rows[1][1] - (xy[1] + [3 * h, 0.0]))) <= 1e-12 * L
    eng.set_particles(None, 0)


# ---- 3. in a run: every stepper family, against the checker fed with the fields of the same run
STEPPERS = ["imex_fused", "imex_perstep", "implicit", "dg"]
NT, DT = 5, 0.04


class _KeepVelocity:
    def __init__(self):
        self.fields = []

    def reset(self):
        self.fields = []

    def __call__(self, Q, p, t, q_tracer=None):
        self.fields.append(np.array(Q.dat.data, dtype=float))


def _run_stepper(which, k, particles, every=1, tracer=False, keep=None, nx=6):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerDGImplicit, IncompressibleEulerHDGImplicit

    cls = {"implicit": IncompressibleEulerHDGImplicit, "dg": IncompressibleEulerDGImplicit}.get(which)
    ts, mesh = _stepper("square", k, nx=nx, cls=cls, dt=DT, callbacks=[keep] if keep else None)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    q0 = (lambda x, y: np.sin(2 * np.pi * x) * np.cos(np.pi * y)) if tracer else None
    kw = {"fused": which == "imex_fused"} if which.startswith("imex") else {}
    Q, p = ts.solve(*mp.initial_condition(), q0, mp.f_rhs(), NT * DT, particles=particles, particle_every=every, **kw)
    lam = eng.get_field(_lib.HDG_STATE_CURRENT, Q=False, p=False)[2]
    qf = eng.get_tracer() if tracer else None
    return ts, mesh, (Q.dat.data.copy(), p.dat.data.copy(), lam.copy(), eng.iteration_stats(), qf)


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("which", STEPPERS)
def test_particles_in_a_run_match_the_checker(hip_lib, which, k):
    xy = 0.08 + 0.84 * np.random.default_rng(7).random((24, 2))
    keep = _KeepVelocity()
    ts, mesh, _ = _run_stepper(which, k, xy, keep=keep)
    rec = ts.particles
    assert len(keep.fields) == NT + 1
    assert rec["xy"].shape == (NT + 1, len(xy), 2) and np.array_equal(rec["xy"][0], xy)
    assert np.array_equal(rec["t"], np.arange(NT + 1) * DT) and rec["lost"] == 0
    ev = pr.PointEvaluator(k, ts._engine.node_coordinates()[0], square=(mesh.nx, mesh.ny, mesh.L, False))
    want, nclamp, margins = par.heun_fields(ev, keep.fields, xy, DT)
    # on the checker alone: no evaluation point within rounding of a cell edge, where the two sides may own it differently
    assert margins.min() >= 1e-9, margins.min()
    err = np.max(np.abs(rec["xy"] - want))
    print(f"{which} k={k}: max deviation from the checker {err:.3e}, smallest edge margin {margins.min():.3e} h, "
          f"largest displacement {np.max(np.abs(want[-1] - xy)):.3f}")
    assert err <= 1e-10 * mesh.L
    assert rec["clamped"] == nclamp
    # particle_every = 2: rows 0, 2, 4 of the same trajectory
    ts2, _, _ = _run_stepper(which, k, xy, every=2)
    assert np.array_equal(ts2.particles["xy"], rec["xy"][0::2]) and np.array_equal(ts2.particles["t"], rec["t"][0::2])
    if which == "imex_perstep":  # the fused and the per-solve path: the same rows
        ts_f, _, _ = _run_stepper("imex_fused", k, xy)
        assert np.array_equal(ts_f.particles["xy"], rec["xy"])


def test_set_state_refreshes_the_predictor(hip_lib):
    ts, mesh = _stepper("periodic", 2, nx=6)
    eng = ts._engine
    xy = np.array([[0.3, 0.4], [1.1, 1.7]])
    _set_velocity(ts, lambda x, y: (1.0 + 0 * x, 0 * x))
    eng.set_particles(xy, 3)
    _set_velocity(ts, lambda x, y: (0 * x, -2.0 + 0 * x))  # k1 and X* of the first field must not survive
    eng.advance_particles(0.1, 1)
    rows, _ = eng.particles()
    assert np.max(np.abs(rows[1] - (xy + [0.0, -0.2]))) <= 1e-14
    eng.set_particles(None, 0)


# ---- 4. off means off
@pytest.mark.parametrize("which,tracer", [("imex_fused", False), ("imex_fused", True), ("imex_perstep", False),
                                          ("implicit", False), ("dg", False)])
def test_particles_change_nothing_of_the_flow(hip_lib, which, tracer):
    xy = 0.08 + 0.84 * np.random.default_rng(7).random((24, 2))
    a = _run_stepper(which, 2, xy, tracer=tracer)[2]
    b = _run_stepper(which, 2, None, tracer=tracer)[2]
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert all(np.array_equal(x, y) for x, y in zip(a[3], b[3]))
    if tracer:
        assert np.array_equal(a[4], b[4])


def test_switched_off_a_step_issues_the_launches_it_issued_before(hip_lib):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    def steps(particles):
        """launch census (launches per class) of steps 1, 2, 3; particles on during steps 1 and 2 only"""
        ts, _ = _stepper("square", 2, nx=6)
        eng = ts._engine
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        Q0, p0 = mp.initial_condition()
        eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
        eng.reconstruct_trace()
        out = []
        for n in range(3):
            if particles and n == 0:
                eng.set_particles([[0.3, 0.3], [0.6, 0.7]], 8)
            if particles and n == 2:
                eng.set_particles(None, 0)
            eng.launch_stats(reset=True)
            eng.step()
            out.append({c: v[0] for c, v in eng.launch_stats(reset=True).items()})
        return out

    off, on = steps(False), steps(True)
    assert on[2] == off[2]  # after hdg_set_particles(n = 0): exactly the launches of a run that never had particles
    for n in (0, 1):  # with particles on: one launch more, nothing else
        assert on[n]["other"] == off[n]["other"] + 1
        assert {c: v for c, v in on[n].items() if c != "other"} == {c: v for c, v in off[n].items() if c != "other"}


# ---- 5. strips
def _strips(nranks, k, nx, nsteps, kind, tmp_path):
    """Start the ranks of tests/particle_strip_worker.py under a time limit; a rank that fails ends the test, the others are
    killed and nothing further is started."""
    token = "/hdg_part_" + uuid.uuid4().hex[:12]
    procs, outs = [], []
    for r in range(nranks):
        out = str(tmp_path / f"{kind}{nranks}_{r}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "particle_strip_worker.py"), str(r), str(nranks), token,
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


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("kind", ["square", "periodic"])
def test_strips_hold_the_same_rows_and_match_the_checker(hip_lib, tmp_path, kind, P):
    k, nx, nsteps = 2, 24, 4
    parts = _strips(P, k, nx, nsteps, kind, tmp_path)
    d0 = parts[0]
    L, dt, xy = float(d0["L"]), float(d0["dt"]), d0["xy"]
    assert d0["rows"].shape == (nsteps + 1, len(xy), 2) and int(d0["lost"]) == 0
    for d in parts[1:]:  # every rank holds the same rows, bitwise
        assert np.array_equal(d["rows"], d0["rows"]) and int(d["clamped"]) == int(d0["clamped"])
    # the strips' own fields, assembled (strips concatenate in rank order), through the checker
    fields = [np.concatenate([d["fields"][n] for d in parts]) for n in range(nsteps + 1)]
    ev = pr.PointEvaluator(k, np.concatenate([d["xq"] for d in parts]), square=(nx, nx, L, kind == "periodic"))
    want, nclamp, margins = par.heun_fields(ev, fields, xy, dt)
    assert margins.min() >= 1e-9, margins.min()
    h = L / nx
    rows_crossed = np.floor(want[-1][:, 1] / h) != np.floor(xy[:, 1] / h)
    err = np.max(np.abs(d0["rows"] - want))
    print(f"{kind} P={P}: max deviation from the checker {err:.3e}, smallest margin {margins.min():.3e} h, "
          f"{int(rows_crossed.sum())} particles changed cell row")
    assert err <= 1e-10 * L and int(d0["clamped"]) == nclamp


# ---- 6. errors
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, _ = _stepper("square", 1)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    eng.set_state(ts._as_nodal_velocity(mp.initial_condition()[0]), ts._as_nodal_pressure(mp.initial_condition()[1]))
    with pytest.raises(_lib.HDGError, match="seed 1") as e:
        eng.set_particles([[0.5, 0.5], [1.0 + 1e-9, 0.5]], 4)
    assert e.value.code == -1
    eng.step()
    rows, counts = eng.particles()
    assert rows.shape[0] == 0 and counts == {"clamped": 0, "lost": 0, "dropped": 0}  # recording stayed off
    with pytest.raises(_lib.HDGError, match="none set"):
        eng.advance_particles(0.1, 1)
    eng.set_particles([[0.5, 0.5], [1.0 + 1e-13, -1e-13]], 4)  # within the tolerance: clamped onto the boundary
    assert np.array_equal(eng.particles()[0][0], [[0.5, 0.5], [1.0, 0.0]])
    with pytest.raises(_lib.HDGError, match="exceed") as e:
        eng.set_particles(np.full((1 << 17, 2), 0.5), 1 << 10)
    assert e.value.code == -1
    with pytest.raises(_lib.HDGError, match="record_every"):
        eng.set_particles([[0.5, 0.5]], 4, 0)
    # dropped rows are reported, as hdg_get_probes reports them
    eng.set_particles([[0.25, 0.25], [0.75, 0.5]], 2)
    for _ in range(3):
        eng.step()
    with pytest.raises(_lib.HDGError, match="2 row"):
        eng.particles(reset=False)
    with pytest.raises(_lib.HDGError, match="2 row"):
        eng.particles(reset=True)
    eng.step()
    assert eng.particles()[0].shape == (1, 2, 2)
    eng.set_particles(None, 0)
    # a periodic mesh takes any finite seed, and refuses a non-finite one
    tp, _ = _stepper("periodic", 1)
    with pytest.raises(_lib.HDGError, match="seed 0"):
        tp._engine.set_particles([[np.nan, 0.5]], 4)
    tp._engine.set_particles([[-7.0, 55.0]], 4)
    tp._engine.set_particles(None, 0)
    # general meshes
    td, _ = _stepper("disk", 1)
    with pytest.raises(_lib.HDGError, match="general meshes") as e:
        td._engine.set_particles([[0.0, 0.0]], 4)
    assert e.value.code == -5


# ---- 7. driver
def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def test_driver_particles_on_one_and_two_ranks(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    nx, k, dt, nt = 8, 1, 0.04, 4
    L = 2 * np.pi
    h = L / nx
    # a third of the way into the lower triangle of every second cell: with |u| <= 1.05 the particles move at most
    # 1.05 nt dt = 0.17 = 0.22 h and stay inside their cell, where the velocity is one polynomial
    pts = np.array([[(i + 0.3) * h, (j + 0.3) * h] for j in range(0, nx, 2) for i in range(1, nx, 2)])
    (tmp_path / "seeds.txt").write_text("# seeds\n" + "\n".join(f"{float(x)!r} {float(y)!r}" for x, y in pts) + "\n")
    got = {}
    for gpus in (1, 2):
        wd = tmp_path / f"g{gpus}"
        wd.mkdir()
        out = _driver(["--problem", "shear", "--nx", str(nx), "--degree", str(k), "--dt", repr(dt), "--tfinal", repr(nt * dt),
                       "--output", "", "--particles", str(tmp_path / "seeds.txt"), "--particle_every", "2", "--gpus", str(gpus)],
                      wd)
        assert "particles (3 rows x 16 particles" in out
        assert [f for f in os.listdir(wd) if f.endswith(".npz")] == ["particles.npz"]  # one file, written by rank 0
        got[gpus] = dict(np.load(wd / "particles.npz"))
    a, b = got[1], got[2]
    assert a["xy"].shape == b["xy"].shape == (nt // 2 + 1, len(pts), 2)
    assert np.array_equal(a["t"], [0.0, 2 * dt, 4 * dt]) and np.array_equal(a["t"], b["t"])
    assert np.array_equal(a["xy"][0], pts) and np.array_equal(b["xy"][0], pts)
    assert int(a["lost"]) == int(b["lost"]) == 0 and int(a["clamped"]) == int(b["clamped"]) == 0
    # one rank: the rows of the Python interface, bitwise
    ts = IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(nx, nx, L=L), k, dt, flux="upwind",
                                            use_projection_method=False, n_richardson=2)
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
    ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nt * dt, particles=pts, particle_every=2)
    assert np.array_equal(ts.particles["xy"], a["xy"])
    # two ranks: the velocities of the two partitions differ by the solver tolerances, at most du = 2e-8 max |u| at any point
    # (the measure of the strip tests of tests/test_gpu_probes.py).  Both trajectories stay inside one cell, where u is
    # Lipschitz with a constant of the shear layer's 1 / rho, so they part by at most  T du exp(T / rho)  (Gronwall).
    moved = np.max(np.abs(a["xy"] - pts))
    assert 1e-3 < moved < 0.25 * h
    T, umax = nt * dt, 1.05
    bound = T * 2e-8 * umax * np.exp(T / mp.rho)
    dev = np.max(np.abs(a["xy"] - b["xy"]))
    print(f"driver: 1 and 2 ranks part by {dev:.3e} (bound {bound:.3e}), largest displacement {moved:.3f}")
    assert dev <= bound
    # refused before any rank is started
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "kelvinhelmholtz",
                        "--particles", str(tmp_path / "seeds.txt")], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode != 0 and "--particles does not support --problem kelvinhelmholtz" in r.stderr
