"""Several passive tracers in one engine (hdg_config::n_tracers): a batch of tracers rides one flow, and
every member evolves as it would alone.

Bounds.  A member of a batch and the same field carried alone go through kernels that differ only in how many tracers a
thread owns; per tracer the floating-point operations are the same, so the two agree to a few units of 1e-16 per step
(reassociation by a different instantiation at the very most).  BOUND = 1e-12 max|q| leaves four orders of room over that
and lies nine orders below the per-step change of a tracer (above 1e-3, asserted below): a shared, swapped or skipped
tracer cannot pass.  Against the oracle the bound is that of tests/test_gpu_tracer.py, TOL = 2e-8."""
import os
import re
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BOUND = 1e-12
TOL = 2e-8
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread of the transport kernels (TracerBlock<K>, csrc/hdg_cg.hpp)
STEPPERS = ("imex_fused", "imex_perstep", "implicit", "dg")


def field(m):
    """Initial field of tracer m: smooth, and no member is a multiple of another."""
    return lambda x, y: np.sin((1.3 + 0.4 * m) * x + 0.2 * m) * np.cos((1.0 + 0.7 * m) * y) + 0.1 * (m + 1) * x


def _mesh(kind, nx):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    return {"square": lambda: UnitSquareMesh(nx, nx), "periodic": lambda: PeriodicSquareMesh(nx, nx, L=2.0),
            "disk": lambda: UnitDiskMesh(1)}[kind]()


def _stepper(which, kind, k, nx, dt, **kw):
    from incompressibleeulerhdg_amd.timesteppers import (IncompressibleEulerDGImplicit, IncompressibleEulerHDGImplicit,
                                                         IncompressibleEulerHDGIMEXSSP2_332)

    cls = {"implicit": IncompressibleEulerHDGImplicit, "dg": IncompressibleEulerDGImplicit}.get(which, IncompressibleEulerHDGIMEXSSP2_332)
    if which != "dg":
        kw.update(use_projection_method=True, n_richardson=2)
    return cls(_mesh(kind, nx), k, dt, **kw)


def _initial(ts, kind):
    """Initial state and forcing: Taylor-Green on the unit square, a smooth swirl elsewhere."""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    if kind == "square":
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        return mp.initial_condition(), mp.f_rhs()
    if kind == "periodic":  # side 2: periodic in both directions
        Q0 = lambda x, y: (np.sin(np.pi * y) + 0.3 * np.cos(np.pi * x), 0.5 * np.sin(np.pi * x))
    else:
        Q0 = lambda x, y: (-y * (1 - x * x - y * y), x * (1 - x * x - y * y))
    return (Q0, lambda x, y: 0 * x), None


_RUNS = {}


def run(which, kind, k, nx, nsteps, members, n_tracers=None, **solve_kw):
    """One run with the tracers `members` (indices of field()): the final tracers (len(members), N_p), Q, p, iteration
    statistics, the initial block and the stepper.  Runs are shared between the tests; nothing changes a cached one."""
    key = (which, kind, k, nx, nsteps, tuple(members), n_tracers)
    shared = not solve_kw  # a run with recorders is its caller's own
    if shared and key in _RUNS:
        return _RUNS[key]
    dt = 0.02
    opts = {} if n_tracers is None else {"n_tracers": n_tracers}
    ts = _stepper(which, kind, k, nx, dt, **opts)
    (Q0, p0), f = _initial(ts, kind)
    q0 = [field(m) for m in members]
    if ts._engine.n_tracers == 1:
        q0 = q0[0]
    if which.startswith("imex"):
        solve_kw = dict(solve_kw, fused=which == "imex_fused")
    Q, p = ts.solve(Q0, p0, q0, f, nsteps * dt, **solve_kw)
    start = np.stack([ts._V_p.interpolate(field(m)) for m in members])
    res = dict(q=np.stack([f_.dat.data.copy() for f_ in ts.q_tracers]), Q=Q.dat.data.copy(), p=p.dat.data.copy(),
               its=ts._engine.iteration_stats(), start=start, ts=ts)
    for a in (res["q"], res["Q"], res["p"], res["start"]):
        a.setflags(write=False)
    if shared:
        _RUNS[key] = res
    return res


def check_batch(which, kind, k, nx, nsteps, members):
    """The batch of `members` against every member alone; returns the largest relative difference."""
    batch = run(which, kind, k, nx, nsteps, members, n_tracers=len(members))
    assert batch["q"].shape == batch["start"].shape
    worst = 0.0
    for i, m in enumerate(members):
        alone = run(which, kind, k, nx, nsteps, (m,))
        scale = np.max(np.abs(alone["q"][0]))
        diff = np.max(np.abs(batch["q"][i] - alone["q"][0])) / scale
        moved = np.max(np.abs(alone["q"][0] - alone["start"][0])) / scale
        print(f"{which} {kind} k={k} n={len(members)} tracer {m}: |batch - alone| = {diff:.3e} max|q|, moved {moved:.3e}")
        worst = max(worst, diff)
        assert diff <= BOUND, (m, diff)
        assert moved > 1e-3 * nsteps / 2, (m, moved)  # the tracer moved: a skipped update cannot pass
        # the flow does not see the tracers
        assert np.array_equal(batch["Q"], alone["Q"]) and np.array_equal(batch["p"], alone["p"])
        assert all(np.array_equal(a, b) for a, b in zip(batch["its"], alone["its"]))
    return worst


# ---- 1. a batch equals its members
@pytest.mark.parametrize("which,kind,k,nx", [
    ("imex_fused", "square", 1, 6), ("imex_fused", "square", 2, 5), ("imex_fused", "square", 3, 4), ("imex_fused", "square", 4, 4),
    ("imex_perstep", "square", 2, 5), ("imex_perstep", "square", 3, 4),
    ("implicit", "square", 1, 6), ("implicit", "square", 2, 5), ("dg", "square", 2, 5), ("dg", "square", 3, 4),
    ("imex_fused", "periodic", 2, 8), ("imex_perstep", "periodic", 2, 8), ("implicit", "periodic", 2, 8), ("dg", "periodic", 2, 8),
    ("imex_fused", "disk", 2, 0), ("imex_perstep", "disk", 2, 0), ("implicit", "disk", 2, 0), ("dg", "disk", 2, 0),
])
def test_a_batch_equals_its_members(hip_lib, which, kind, k, nx):
    check_batch(which, kind, k, nx, 2, (0, 1, 2))


# ---- 2. block tails: one more tracer than a thread owns, a short last block behind a full one, and the most there can be
@pytest.mark.parametrize("n", sorted({TB[2] + 1, 5, 7, 16}))
def test_block_tails(hip_lib, n):
    check_batch("imex_fused", "square", 2, 5, 1, tuple(range(n)))


@pytest.mark.parametrize("kind,k,nx", [("square", 1, 6), ("square", 3, 4), ("disk", 2, 0), ("periodic", 2, 8)])
def test_block_tails_of_the_other_blockings(hip_lib, kind, k, nx):
    check_batch("imex_fused", kind, k, nx, 1, tuple(range(TB[k] + 1)))


# ---- 3. linearity: the transport is linear in q for a given u
@pytest.mark.parametrize("kind,k,nx", [("square", 2, 5), ("periodic", 2, 8), ("disk", 2, 0)])
def test_linearity_within_a_batch(hip_lib, kind, k, nx):
    dt, nsteps = 0.02, 2
    ts = _stepper("imex_fused", kind, k, nx, dt, n_tracers=3)
    (Q0, p0), f = _initial(ts, kind)
    a, b = ts._V_p.interpolate(field(0)), ts._V_p.interpolate(field(1))
    ts.solve(Q0, p0, [a, b, 2 * a - 3 * b], f, nsteps * dt, fused=True)
    q = [f_.dat.data for f_ in ts.q_tracers]
    scale = max(np.max(np.abs(x)) for x in q)
    dev = np.max(np.abs(q[2] - (2 * q[0] - 3 * q[1]))) / scale
    print(f"linearity {kind} k={k}: {dev:.3e} max|q|")
    assert dev <= BOUND
    assert np.max(np.abs(q[0] - a)) > 1e-3 * scale


# ---- 4. against the oracle
def _q_oracle(m):
    return lambda x, y: np.sin(2 * np.pi * (m + 1) * x) * np.sin(2 * np.pi * y) + 0.25 * m * y


@pytest.mark.parametrize("k,nx", [(1, 6), (2, 4)])
def test_imex_batch_against_the_oracle(hip_lib, k, nx):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle, imex_with_tracer

    dt, nsteps = 0.25 / nx, 2
    d = orc.HDGDiscretisation(nx, k)
    tr = TracerOracle(d)
    tg = orc.TaylorGreen(d)
    want = []
    for m in range(3):
        o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
        want.append(imex_with_tracer(o, tr, *tg.initial_condition(), d.interpolate_pressure(_q_oracle(m)), tg.f_rhs, nsteps * dt))
    for fused in (False, True):
        ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(nx, nx), k, dt, n_tracers=3)
        mp = TaylorGreen(ts._V_Q, ts._V_p)
        Q, p = ts.solve(*mp.initial_condition(), [_q_oracle(m) for m in range(3)], mp.f_rhs(), nsteps * dt, fused=fused)
        for m, (oQ, op, oq) in enumerate(want):
            assert _rel(Q.dat.data, oQ) < TOL and _rel(p.dat.data, op) < TOL
            err = _rel(ts.q_tracers[m].dat.data, oq)
            print(f"oracle k={k} fused={fused} tracer {m}: {err:.3e}")
            assert err < TOL, (fused, m, err)


def test_implicit_batch_against_the_oracle(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGImplicit
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle, implicit_with_tracer

    k, nx = 1, 6
    dt = 0.25 / nx
    d = orc.HDGDiscretisation(nx, k)
    tg = orc.TaylorGreen(d)
    tr = TracerOracle(d)
    ts = IncompressibleEulerHDGImplicit(UnitSquareMesh(nx, nx), k, dt, n_tracers=3)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), [_q_oracle(m) for m in range(3)], mp.f_rhs(), 3 * dt)
    for m in range(3):
        oQ, op, oq = implicit_with_tracer(d, tr, dt, *tg.initial_condition(), d.interpolate_pressure(_q_oracle(m)), tg.f_rhs, 3 * dt)
        assert _rel(Q.dat.data, oQ) < TOL and _rel(p.dat.data, op) < TOL
        assert _rel(ts.q_tracers[m].dat.data, oq) < TOL, m


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


# ---- 5. nothing else moves
def _census(n_tracers, tracer, off_again=False):
    """Fields after, and the launch census of, the third of three fused steps."""
    ts = _stepper("imex_fused", "square", 2, 5, 0.02, **({} if n_tracers is None else {"n_tracers": n_tracers}))
    eng = ts._engine
    (Q0, p0), f = _initial(ts, "square")
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if tracer:
        block = np.stack([ts._V_p.interpolate(field(m)) for m in range(eng.n_tracers)])
        eng.set_tracer(block[0] if eng.n_tracers == 1 else block)
    if off_again:
        eng.set_tracer(None)
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    return census, Q, p, (eng.get_tracer() if tracer and not off_again else None), eng


def test_one_tracer_is_what_it_was(hip_lib):
    runs = [_census(n, True) for n in (None, 0, 1)]
    for census, Q, p, q, eng in runs:
        assert q.shape == eng.shape_p == (eng.n_cells * eng.n_p,)
        assert census == runs[0][0]
        assert np.array_equal(Q, runs[0][1]) and np.array_equal(p, runs[0][2]) and np.array_equal(q, runs[0][3])
    # a batch issues the launches of one tracer: one projection per stage, one transport launch and one update for all
    many = _census(3, True)
    assert many[3].shape == (3,) + many[4].shape_p
    assert many[0] == runs[0][0]
    assert np.max(np.abs(many[3][0] - runs[0][3])) <= BOUND * np.max(np.abs(runs[0][3]))
    # switched off again, a step runs no tracer launch: the census of an engine that never had one, for one and for several
    never = _census(None, False)
    assert sum(never[0].values()) < sum(runs[0][0].values())
    for n in (None, 3):
        off = _census(n, True, off_again=True)
        assert off[0] == never[0]
        assert np.array_equal(off[1], never[1]) and np.array_equal(off[2], never[2])
        with pytest.raises(Exception, match="no tracer"):
            off[4].get_tracer()


@pytest.mark.parametrize("which", ["imex_fused", "imex_perstep", "implicit"])
def test_recorded_columns_refer_to_tracer_0(hip_lib, which):
    from incompressibleeulerhdg_amd._lib import DIAGNOSTICS

    xy = 0.1 + 0.8 * np.random.default_rng(5).random((7, 2))
    two = run(which, "square", 2, 5, 3, (0, 1), n_tracers=2, diagnostics=True, probes=xy)
    one = run(which, "square", 2, 5, 3, (0,), diagnostics=True, probes=xy)
    for name in DIAGNOSTICS:
        assert np.array_equal(two["ts"].diagnostics[name], one["ts"].diagnostics[name]), name
    assert np.all(np.isfinite(one["ts"].diagnostics["tracer_half_sq"]))
    for name in ("u", "p", "q", "omega"):
        assert np.array_equal(two["ts"].probes[name], one["ts"].probes[name]), name
    assert np.all(np.isfinite(one["ts"].probes["q"])) and np.ptp(one["ts"].probes["q"][:, 0]) > 0


def test_particle_rows_do_not_see_the_tracers(hip_lib):
    xy = 0.1 + 0.8 * np.random.default_rng(6).random((9, 2))
    with_tr = run("imex_fused", "square", 2, 5, 3, (0, 1), n_tracers=2, particles=xy)
    without = _stepper("imex_fused", "square", 2, 5, 0.02)
    (Q0, p0), f = _initial(without, "square")
    without.solve(Q0, p0, None, f, 3 * 0.02, fused=True, particles=xy)
    assert np.array_equal(with_tr["ts"].particles["xy"], without.particles["xy"])
    assert np.max(np.abs(without.particles["xy"][-1] - xy)) > 1e-4


# ---- 6. errors
def test_errors(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh

    disk = UnitDiskMesh(1)
    base = dict(nx=4, degree=1, dt=0.01, nstages=1)
    for bad in (17, -1):
        for extra in ({}, {"vertices": disk.vertices, "cells": disk.cells},
                      {"rank": 0, "nranks": 2, "comm_backend": "shm", "comm_token": "/hdg_mt_" + uuid.uuid4().hex[:12]}):
            with pytest.raises(_lib.HDGError, match=f"n_tracers.*{bad}") as e:
                _lib.Engine(n_tracers=bad, **base, **extra)
            assert e.value.code == -1
    for ok in (0, 1, 16):
        assert _stepper("implicit", "square", 1, 4, 0.02, n_tracers=ok)._engine.n_tracers == max(ok, 1)
    ts = _stepper("imex_fused", "square", 1, 4, 0.02, n_tracers=3)
    eng = ts._engine
    npts = eng.shape_p[0]
    for shape in ((npts,), (2, npts), (3, npts + 1), (3 * npts,)):
        with pytest.raises(ValueError):
            eng.set_tracer(np.zeros(shape))
    with pytest.raises(ValueError):
        _stepper("imex_fused", "square", 1, 4, 0.02)._engine.set_tracer(np.zeros((1, npts)))
    (Q0, p0), f = _initial(ts, "square")
    for q0 in ([field(0), field(1)], [field(m) for m in range(4)], field(0)):
        with pytest.raises(ValueError, match="3 tracer fields"):
            ts.solve(Q0, p0, q0, f, 0.04, fused=True)
    assert eng.iteration_stats()[1].sum() == 0  # ... before any step


def test_a_strip_keeps_its_tracer_error(hip_lib, tmp_path):
    token = "/hdg_mt_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"r{r}.npz") for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "multi_tracer_strip_worker.py"), str(r), "2", token, outs[r]],
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


# ---- 7. driver
def test_driver_with_two_tracers(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332
    from incompressibleeulerhdg_amd.driver import tracer_initial

    nx, k, dt, nt = 8, 1, 0.04, 2
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "shear", "--nx", str(nx), "--degree",
                        str(k), "--dt", repr(dt), "--tfinal", repr(nt * dt), "--tracer_advection", "--tracers", "2", "--animation",
                        "--output", ""], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "number of tracers = 2" in r.stdout
    got = re.findall(r"^tracer_(\d): integral = (\S+), half square integral = (\S+)$", r.stdout, flags=re.M)
    assert [g[0] for g in got] == ["0", "1"]
    ts = IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(nx, nx, L=2 * np.pi), k, dt, flux="upwind", use_projection_method=False,
                                            n_richardson=2, n_tracers=2)
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), [tracer_initial(0), tracer_initial(1)], mp.f_rhs(), nt * dt)
    assert [f.name() for f in ts.q_tracers] == ["tracer_0", "tracer_1"] and ts.q_tracer is ts.q_tracers[0]
    for m in range(2):
        assert float(got[m][1]) == ts._engine.integrate_pressure(ts.q_tracers[m].dat.data)
        assert float(got[m][2]) == ts.compute_diagnostics(Q, p, ts.q_tracers[m])["tracer_half_sq"]
    assert float(got[0][2]) != float(got[1][2])
    vtu = (tmp_path / f"evolution_{nt}.vtu").read_text()
    for name in ('Name="tracer_0"', 'Name="tracer_1"', 'Name="vorticity"'):
        assert name in vtu, name
    assert 'Name="tracer"' not in vtu
