"""Flow diagnostics on the device (hdg_compute_diagnostics / hdg_set_diagnostics / hdg_get_diagnostics, DESIGN.md
section 12): against the CPU reference of tests/diagnostics_reference.py, the recorded series against the fields fetched
step by step, recording on / off, strip partitions, the driver and one physics ordering."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from diagnostics_reference import NAMES, diagnostics
from oracle import fem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SUMS = [c for c in NAMES if c not in ("max_speed", "cfl")]


def _mesh(kind, nx=6, level=3):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    if kind == "square":
        return UnitSquareMesh(nx, nx), fem.Mesh(nx)
    if kind == "periodic":
        return PeriodicSquareMesh(nx, nx, L=2 * np.pi), fem.Mesh(nx, periodic=True, L=2 * np.pi)
    pm = UnitDiskMesh(level)
    return pm, fem.TriMesh(pm.vertices, pm.cells)


def _imex(mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    return IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=kw.pop("projection", True), n_richardson=2, **kw)


def _close(a, b, rel):
    return abs(a - b) <= rel * max(abs(a), abs(b))


CASES = [("square", k) for k in (1, 2, 3, 4)] + [("periodic", k) for k in (1, 2, 3, 4)] + [("disk", k) for k in (1, 2, 3)]


@pytest.mark.parametrize("kind,k", CASES)
def test_compute_matches_reference(hip_lib, kind, k):
    pm, fm = _mesh(kind)
    dt = 0.013
    ts = _imex(pm, k, dt)
    rng = np.random.default_rng(1000 * k + len(kind))
    Q = rng.standard_normal(ts._engine.shape_Q)
    p = rng.standard_normal(ts._engine.shape_p)
    q = rng.standard_normal(ts._engine.shape_p)
    for tracer in (None, q):
        got = ts.compute_diagnostics(Q, p, tracer)
        ref = diagnostics(fm, k, Q, p, q=tracer, dt=dt)
        for c in SUMS:
            if tracer is None and c.startswith("tracer"):
                assert np.isnan(got[c]), c
                continue
            assert _close(got[c], ref[c], 1e-12), (c, got[c], ref[c])
        assert got["max_speed"] == ref["max_speed"]
        # h_K: the engine's L / nx against the reference's vertex differences, which can differ in the last bit
        assert _close(got["cfl"], ref["cfl"], 0.0 if kind == "disk" else 1e-15), (got["cfl"], ref["cfl"])


@pytest.mark.parametrize("kind", ["square", "periodic", "disk"])
def test_bdm_projection_has_no_normal_jumps(hip_lib, kind):
    """project_bdm returns an H(div)-conforming field with u.n = 0 on the boundary: both passes must see every edge."""
    pm, fm = _mesh(kind, nx=8)
    k = 2
    ts = _imex(pm, k, 0.01)
    Q = np.random.default_rng(7).standard_normal(ts._engine.shape_Q)
    p = np.zeros(ts._engine.shape_p)
    raw = ts.compute_diagnostics(Q, p)
    d = ts.compute_diagnostics(ts.project_bdm(Q), p)
    norm = np.sqrt(2 * d["energy"])
    assert raw["jump_l2"] > 0.1 * np.sqrt(2 * raw["energy"])  # the random field does jump
    assert d["jump_l2"] <= 1e-13 * norm, (d["jump_l2"], norm)


def _solve_with_snapshots(ts, args, kw, nt):
    """One solve with diagnostics=True whose callback also fetches the fields: row 0 of the reference is
    compute_diagnostics of the initial fields, row n of the fields fetched after step n (same run: the warm starts the
    engine keeps across solves stay out of the comparison)."""
    from incompressibleeulerhdg_amd import _lib

    eng = ts._engine
    rows = []

    class Snap:
        def reset(self):
            pass

        def __call__(self, Q, p, t, q_tracer=None):
            Qf, pf, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
            rows.append(eng.compute_diagnostics(Qf, pf, eng.get_tracer() if ts.q_tracer is not None else None))

    ts.callbacks = [Snap()]
    ts.solve(*args, diagnostics=True, **kw)
    ts.callbacks = []
    assert len(rows) == nt + 1
    return ts.diagnostics, np.array(rows)


def _compare_series(rec, ref, nt, dt, rel=1e-14):
    assert len(rec["t"]) == nt + 1
    assert np.allclose(rec["t"], np.arange(nt + 1) * dt, rtol=0, atol=1e-15)
    for i, c in enumerate(NAMES):
        a, b = rec[c], ref[:, i]
        if np.all(np.isnan(b)):
            assert np.all(np.isnan(a)), c
            continue
        scale = np.maximum(np.abs(b), 1e-30)
        # divergence, jumps and the (zero-mean) pressure integral are rounding-sized against the fields: their differences
        # (the reference sees the fields after a trip through the nodal values) count against the norm of the field
        if c in ("div_l2", "jump_l2"):
            scale = np.maximum(scale, np.sqrt(2 * ref[:, 0]))
        if c == "p_integral":
            scale = np.maximum(scale, 1.0)
        if c == "tracer_integral":
            scale = np.maximum(scale, np.sqrt(2 * ref[:, 6]))
        err = np.max(np.abs(a - b) / scale)
        assert err <= rel, (c, err, a, b)


FAMILIES = ["imex_fused", "imex_solves", "imex_unsplit", "implicit_projection", "implicit_monolithic", "dg"]


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("tracer", [False, True])
def test_series_matches_fetched_fields(hip_lib, family, tracer):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerDGImplicit, IncompressibleEulerHDGImplicit

    nx, k, nt = 8, 2, 3
    dt = 0.25 / nx
    mesh = UnitSquareMesh(nx, nx)
    if family.startswith("imex"):
        ts = _imex(mesh, k, dt, projection=family != "imex_unsplit")
        kw = {"fused": family == "imex_fused"}
    elif family.startswith("implicit"):
        ts = IncompressibleEulerHDGImplicit(mesh, k, dt, use_projection_method=family == "implicit_projection")
        kw = {}
    else:
        ts = IncompressibleEulerDGImplicit(mesh, k, dt)
        kw = {}
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    q0 = (lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)) if tracer else None
    args = (*mp.initial_condition(), q0, mp.f_rhs(), nt * dt)
    rec, ref = _solve_with_snapshots(ts, args, kw, nt)
    _compare_series(rec, ref, nt, dt)
    ts.solve(*args, **kw)
    assert ts.diagnostics is None  # a solve without diagnostics clears the attribute


def test_run_separable_and_per_step_calls(hip_lib):
    """hdg_run_separable records one row per step; so does hdg_step; capacity overflow is reported at the fetch."""
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    nx, k, nt = 8, 2, 4
    dt = 0.25 / nx
    ts = _imex(UnitSquareMesh(nx, nx), k, dt)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    eng = ts._engine
    Q0, p0 = ts._as_nodal_velocity(mp.initial_condition()[0]), ts._as_nodal_pressure(mp.initial_condition()[1])
    f = mp.f_rhs()
    eng.set_forcing_profile(f.profile)
    scales = np.array([[f.scale(n * dt + c * dt) for c in (0.0, 1.0, 0.5)] + [f.scale((n + 1) * dt)] for n in range(nt)])
    eng.set_state(Q0, p0)
    eng.reconstruct_trace()
    eng.set_diagnostics(nt + 1)
    ref = []
    Q, p, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
    ref.append(eng.compute_diagnostics(Q, p))
    for n in range(nt):
        if n % 2:
            eng.run_separable(scales[n:n + 1])
        else:  # hdg_step with the same forcing
            for sl in range(4):
                eng.set_forcing_scale(sl, scales[n, sl])
            eng.step()
        Q, p, _ = eng.get_field(_lib.HDG_STATE_CURRENT, lam=False)
        ref.append(eng.compute_diagnostics(Q, p))
    rows = eng.diagnostics(reset=True)
    eng.set_diagnostics(0)
    _compare_series({"t": np.arange(nt + 1) * dt, **{c: rows[:, i] for i, c in enumerate(NAMES)}}, np.array(ref), nt, dt)
    # overflow: two rows of capacity, three recorded states -> the fetch reports the dropped row
    eng.set_state(Q0, p0)
    eng.set_diagnostics(2)
    eng.run_separable(scales[:2])
    with pytest.raises(_lib.HDGError, match="dropped"):
        eng.diagnostics()
    eng.set_diagnostics(0)


@pytest.mark.parametrize("fused", [True, False])
def test_recording_changes_nothing(hip_lib, fused):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow

    nx, k, nt = 16, 2, 3
    dt = 0.02
    out = []
    for diag in (False, True):
        ts = _imex(PeriodicSquareMesh(nx, nx, L=2 * np.pi), k, dt)
        mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
        q0 = lambda x, y: np.sin(x) * np.cos(y)  # noqa: E731
        Q, p = ts.solve(*mp.initial_condition(), q0, mp.f_rhs(), nt * dt, fused=fused, diagnostics=diag)
        sums, cnt = ts._engine.iteration_stats()
        out.append((Q.dat.data.copy(), p.dat.data.copy(), ts.q_tracer.dat.data.copy(), sums.copy(), cnt.copy()))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def _run_ranks(nranks, k, nx, nsteps, tmp_path):
    token = "/hdg_diag_" + uuid.uuid4().hex[:12]
    procs, outs = [], []
    for r in range(nranks):
        out = str(tmp_path / f"diag_rank{r}_of{nranks}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "diag_strip_worker.py"), str(r), str(nranks), token,
                                       str(k), str(nx), str(nsteps), out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for pr in procs:
        try:
            o, _ = pr.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o.decode(errors="replace"))
    for r, pr in enumerate(procs):
        assert pr.returncode == 0, f"rank {r} failed:\n{logs[r][-3000:]}"
    return [np.load(o) for o in outs]


@pytest.mark.parametrize("nranks", [2, 4])
def test_strip_partition_series(hip_lib, tmp_path, nranks):
    k, nx, nsteps = 2, 16, 3
    single = _run_ranks(1, k, nx, nsteps, tmp_path)[0]
    parts = _run_ranks(nranks, k, nx, nsteps, tmp_path)
    for d in parts:
        s, r = d["series"], single["series"]
        assert s.shape == r.shape == (nsteps + 1, 9)
        for i, c in enumerate(NAMES):
            if c.startswith("tracer"):
                assert np.all(np.isnan(s[:, i]))
                continue
            # row 0 (the same initial fields) exactly up to summation order; later rows carry the Krylov differences
            # of the ranks' reductions
            # row 0 (the same initial fields): 1e-13, up to summation order.  After a step the strips' fields differ from
            # the single rank's by the Krylov tolerance (tests/test_gpu_multirank.py); divergence, jumps and the zero-mean
            # pressure integral are small against the field, so their differences count against its norm
            unorm = np.sqrt(2 * r[0, 0])
            atol0 = 1e-13 * unorm if c in ("div_l2", "jump_l2", "p_integral") else 0.0
            assert np.allclose(s[0, i], r[0, i], rtol=1e-13, atol=atol0), (c, s[0, i], r[0, i])
            atol = 1e-10 * unorm if c in ("div_l2", "jump_l2", "p_integral") else 0.0
            assert np.allclose(s[1:, i], r[1:, i], rtol=1e-11, atol=atol), (c, s[:, i], r[:, i])
        assert s[0, 7] == r[0, 7] and s[0, 8] == r[0, 8]  # maxima of the same initial state: exact
        assert np.array_equal(d["series"], parts[0]["series"], equal_nan=True)  # every rank holds the global values
        assert np.allclose(d["final"][:5], single["final"][:5], rtol=1e-9)


def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=300, env=dict(os.environ, PYTHONPATH=os.path.dirname(HERE)))
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout.splitlines()


def test_driver_writes_csv(hip_lib, tmp_path):
    import re

    base = ["--nx", "8", "--degree", "1", "--dt", "0.05", "--tfinal", "0.15", "--output", ""]
    plain = _driver(base, tmp_path)
    out = _driver(base + ["--diagnostics", "diag.csv"], tmp_path)
    lines = (tmp_path / "diag.csv").read_text().strip().splitlines()
    assert lines[0] == "step,t," + ",".join(NAMES)
    assert len(lines) == 1 + 4  # nt + 1 rows
    assert [int(ln.split(",")[0]) for ln in lines[1:]] == [0, 1, 2, 3]
    assert "solver events" in out and any("cg_floor_exits" in ln for ln in out)
    assert not any("solver events" in ln or "diagnostics" in ln for ln in plain)
    # the flag only adds its two blocks (each up to the next empty line): every other line is the plain run's, in order
    # (wall-clock rows of the performance log left out)
    timing = re.compile(r":\s+\d+\s+\S+e[-+]\d+\s+\S+e[-+]\d+\s+\S+e[-+]\d+")
    rest, skip = [], False
    for ln in out:
        if ln == "solver events" or ln.startswith("diagnostics ("):
            skip = True
        if not skip:
            rest.append(ln)
        elif ln == "":
            skip = False
    assert [ln for ln in rest if not timing.search(ln)] == [ln for ln in plain if not timing.search(ln)]


def test_shear_flow_upwind_dissipates_faster(hip_lib):
    """Unforced double shear layer at 64^2, k = 2: the upwind flux loses kinetic energy each step faster than the centred one."""
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow

    nx, k, nt, dt = 64, 2, 5, 0.01
    energy = {}
    for flux in ("upwind", "centered"):
        ts = _imex(PeriodicSquareMesh(nx, nx, L=2 * np.pi), k, dt, flux=flux)
        mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nt * dt, fused=True, diagnostics=True)
        energy[flux] = ts.diagnostics["energy"]
    assert energy["upwind"][0] == energy["centered"][0]
    loss_up, loss_c = -np.diff(energy["upwind"]), -np.diff(energy["centered"])
    assert np.all(loss_up > loss_c), (loss_up, loss_c)
