"""Adaptive time step on the GPU (include/hdg_adaptive_dt.h): the advective rate of k_step_rate /
k_g_step_rate against column 8 of the diagnostics and against numpy, hdg_set_dt against reference loops that run the oracle's
steppers through the same list of step sizes, the no-op, controlled runs against the numpy twin of the rule, the recorders'
times, strips, the errors and the driver.

Bounds.  Rates: relative 1e-14 -- definition and nodes are the same, so only the few roundings of dt m / h can differ (a bound
on those roundings, not a measured figure).  Whole steps: TOL = 2e-8 relative to the field's max-norm, the bound
tests/test_gpu_timestep.py, test_gpu_periodic.py, test_gpu_general_mesh.py and test_gpu_dg_implicit.py use for whole steps of
the same steppers against the oracle.  Particles: 1e-10 L, the bound of tests/test_gpu_particles.py."""
import os
import subprocess
import sys
import uuid
import warnings

import numpy as np
import pytest

import adaptive_dt_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RATE, TOL = 1e-14, 2e-8
K, NX, DT0, T_FINAL, CFL, DT_MAX = 2, 8, 0.02, 0.25, 0.3, 0.05  # run (a); the strip worker has the same numbers


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _classes():
    from incompressibleeulerhdg_amd import timesteppers as ts

    return {"imex_ssp2_332": ts.IncompressibleEulerHDGIMEXSSP2_332, "imex_ars2_232": ts.IncompressibleEulerHDGIMEXARS2_232,
            "implicit": ts.IncompressibleEulerHDGImplicit, "dg": ts.IncompressibleEulerDGImplicit}


def _mesh(kind, nx):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    if kind == "square":
        return UnitSquareMesh(nx, nx)
    if kind == "periodic":
        return PeriodicSquareMesh(nx, nx, L=2.0)
    return UnitDiskMesh(1)


def _shortest_edges(mesh, eng):
    """h_K of every cell in the order of the engine's cells"""
    if getattr(mesh, "general", False):
        X = np.asarray(mesh.vertices)[np.asarray(mesh.cells)]
        return np.min(np.linalg.norm(X - np.roll(X, 1, axis=1), axis=2), axis=1)
    return np.full(eng.n_cells, getattr(mesh, "L", 1.0) / mesh.nx)


def _stepper(kind, k, nx=4, dt=0.013, which="imex_ssp2_332", **kw):
    mesh = _mesh(kind, nx)
    if which in ("imex_ssp2_332", "imex_ars2_232"):
        kw = dict(use_projection_method=True, n_richardson=2, **kw)
    return _classes()[which](mesh, k, dt, **kw), mesh


# ---- rates
RATE_CASES = [("square", k) for k in (1, 2, 3, 4)] + [("periodic", 2), ("disk", 1), ("disk", 2), ("disk", 3)]


def _fields(eng, mesh):
    """name -> nodal velocity: random, and the random field with one cell made the largest"""
    rng = np.random.default_rng(5 + eng.n_u)
    base = 0.1 * rng.standard_normal(eng.shape_Q)
    out = {"random": rng.standard_normal(eng.shape_Q), "zero": np.zeros(eng.shape_Q)}
    middle = eng.n_cells // 2 - (eng.n_cells // 2) % 2
    for name, c in (("first", 0), ("last", eng.n_cells - 1), ("middle", middle), ("its_neighbour", middle + 1)):
        Q = base.copy()
        Q[c * eng.n_u:(c + 1) * eng.n_u] *= 60.0
        out[name] = Q
    return out


@pytest.mark.parametrize("kind,k", RATE_CASES)
def test_rate_is_column_8_without_dt(hip_lib, kind, k):
    """A dt against the cfl column of compute_diagnostics of the same nodal values, and against numpy: nodal speeds over the
    nodes of hdg_node_coordinates, the shortest edge.  The largest speed in the first cell, in the last one and in both cells
    of a square in the middle (the two cell shapes); a zero field gives exactly 0."""
    dt = 0.013
    ts, mesh = _stepper(kind, k, dt=dt)
    eng = ts._engine
    h = _shortest_edges(mesh, eng)
    assert eng.get_dt() == dt
    for name, Q in _fields(eng, mesh).items():
        eng.set_state(Q, np.zeros(eng.shape_p))
        Qg, pg, _ = eng.get_field(0)
        A = eng.step_rates()[0]
        col8 = ts.compute_diagnostics(Qg, pg)["cfl"]
        speeds = np.max(np.hypot(Qg[:, 0], Qg[:, 1]).reshape(eng.n_cells, eng.n_u), axis=1)
        want = np.max(speeds / h)
        print(f"{kind} k={k} {name}: A dt {A * dt!r}, column 8 {col8!r}, numpy {want * dt!r}; largest cell {int(np.argmax(speeds / h))}")
        if name == "zero":
            assert A == 0.0 and col8 == 0.0
            continue
        assert abs(A * dt - col8) <= RATE * col8 and abs(A - want) <= RATE * want
        if name != "random":
            middle = eng.n_cells // 2 - (eng.n_cells // 2) % 2
            assert int(np.argmax(speeds / h)) == {"first": 0, "last": eng.n_cells - 1, "middle": middle, "its_neighbour": middle + 1}[name]
    # the rule through the engine is the twin applied to that rate
    from incompressibleeulerhdg_amd import _lib

    got = eng.propose_dt(_lib.step_control(0.3, dt_max=1.0), 0.0, 10.0)
    assert got == ref.propose(A, dt, 0.0, 10.0, 0.3, dt_max=1.0)[1]
    assert eng.get_dt() == dt  # it sets nothing


@pytest.mark.parametrize("kind", ["square", "periodic", "disk"])
def test_one_nan_entry_makes_the_rate_not_finite(hip_lib, kind):
    from incompressibleeulerhdg_amd import _lib

    ts, mesh = _stepper(kind, 2)
    eng = ts._engine
    Q = np.random.default_rng(3).standard_normal(eng.shape_Q)
    for row in (0, len(Q) // 2 + 1, len(Q) - 1):
        bad = Q.copy()
        bad[row, row % 2] = np.nan
        eng.set_state(bad, np.zeros(eng.shape_p))
        assert not np.isfinite(eng.step_rates()[0]), row
        with pytest.raises(_lib.HDGError, match="velocity is not finite") as e:
            eng.propose_dt(_lib.step_control(0.3), 0.0, 1.0)
        assert e.value.code == -3
    bad = Q.copy()
    bad[7, 1] = np.inf
    eng.set_state(bad, np.zeros(eng.shape_p))
    assert not np.isfinite(eng.step_rates()[0])
    eng.set_state(Q, np.zeros(eng.shape_p))
    assert np.isfinite(eng.step_rates()[0]) and eng.step_rates()[0] > 0


def test_the_other_rates_are_the_reports_without_dt(hip_lib):
    """rates[1..3] against the three reports divided by dt (a few roundings: 1e-14), and 0 while a term is off"""
    dt = 0.0125
    ts, _ = _stepper("square", 2, dt=dt, n_tracers=2)
    eng = ts._engine
    assert np.array_equal(eng.step_rates()[1:], [0.0, 0.0, 0.0])
    eng.set_tracer_diffusivity([1e-3, 4e-3])
    eng.set_viscosity(2e-3, "no_slip")
    eng.set_coriolis(3.0, -7.0)
    want = [eng.tracer_diffusion_number()[1] / dt, eng.viscosity_number()[1] / dt, eng.coriolis_number()[1] / dt]
    got = eng.step_rates()[1:]
    print(f"rates {got.tolist()}, reports / dt {want}")
    assert np.all(got > 0) and np.all(np.abs(got - want) <= 1e-14 * np.abs(want))
    assert got[2] == eng.coriolis_number()[0] == 4.0
    eng.set_dt(2 * dt)  # the reports use the new value from then on; the rates do not change
    assert np.array_equal(eng.step_rates()[1:], got)
    now = [eng.tracer_diffusion_number()[1], eng.viscosity_number()[1], eng.coriolis_number()[1]]
    assert np.all(np.abs(np.array(now) - 2 * dt * got) <= 1e-14 * np.array(now))


# ---- set_dt against the reference loops
def _tracer0(x, y):
    return np.sin(2.1 * x + 0.3) * np.cos(1.7 * y)


def _reference(kind, which, k, nx, dts):
    """(Q, p, q) of the reference loop through the step sizes dts with the passive tracer _tracer0 carried along, and the
    initial data / forcing for the stepper"""
    from dg_reference import dg_solve
    from oracle import fem
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    mesh = _mesh(kind, nx)
    if kind == "square":
        d = orc.HDGDiscretisation(nx, k)
        tg = orc.TaylorGreen(d, "exponential", 0.5)
        Q0, p0, f = *tg.initial_condition(), tg.f_rhs
        data = "taylorgreen"
    else:
        d = orc.HDGDiscretisation(nx, k, periodic=True, L=2.0) if kind == "periodic" else \
            orc.HDGDiscretisation(0, k, mesh=fem.TriMesh(mesh.vertices, mesh.cells))
        w = np.pi if kind == "periodic" else 1.3
        u0 = lambda x, y: (np.sin(w * x) * np.cos(w * y) + 0.3, -np.cos(w * x) * np.sin(w * y) + 0.1 * np.sin(w * x))
        pr0 = lambda x, y: 0.2 * np.cos(w * x) * np.cos(w * y)
        force = lambda t: (lambda x, y: (0.1 * np.cos(w * y) * np.cos(t), 0.2 * np.sin(w * (x + y)) * (1 + t)))
        Q0, p0, f = d.interpolate_velocity(u0), d.interpolate_pressure(pr0), lambda t: d.interpolate_velocity(force(t))
        data = (u0, pr0, force)
    tr, q0 = TracerOracle(d), d.interpolate_pressure(_tracer0)
    if which.startswith("imex"):
        o = ref.imex_loop(lambda dt: orc.OracleHDGIMEX(d, dt, which), dts, Q0, p0, f, tracer=tr, q0=q0)
        return (o.Q, o.p, o.q), data
    if which == "implicit":
        step = lambda dt, Q, p, g: orc.OracleHDGImplicit(d, dt).solve(Q, p, g, dt)
    else:
        step = lambda dt, Q, p, g: dg_solve(d, Q, p, g, dt, 1)
    return ref.one_step_loop(step, dts, Q0, p0, f, tracer=tr, q0=q0), data


def _run_with_set_dt(kind, which, k, nx, dt1, dt2, data, fused=False):
    """Two steps at dt1, set_dt(dt2), two more, with the tracer _tracer0 on: through the time loop's own pieces (the forcing
    at the running time).  Returns the stepper and (Q, p, q)."""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, _ = _stepper(kind, k, nx=nx, dt=dt1, which=which)
    eng = ts._engine
    if data == "taylorgreen":
        mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
        (Q0, p0), f = mp.initial_condition(), mp.f_rhs()
    else:
        Q0, p0, f = data
    if which.startswith("imex"):
        ts._fused = fused
    ts._forcing_profile = None
    assert ts._init_tracer(_tracer0)
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    ts._begin_solve()
    t = 0.0
    for n, dt in enumerate((dt1, dt1, dt2, dt2)):
        if dt != eng.get_dt():
            eng.set_dt(dt)
            ts._dt = dt
        ts._t_adaptive = t
        ts._advance(n, f, True)
        t += dt
    assert eng.get_dt() == dt2
    return ts, (*ts._current(), eng.get_tracer())


SET_DT_CASES = [("square", "imex_ssp2_332", k, True) for k in (1, 2, 3)] + [("square", "imex_ssp2_332", 2, False)] + \
    [("square", "imex_ars2_232", k, False) for k in (1, 2, 3)] + [("square", "imex_ars2_232", 2, True)] + \
    [("square", "implicit", 2, False), ("square", "dg", 2, False), ("periodic", "imex_ssp2_332", 2, True),
     ("periodic", "implicit", 2, False), ("disk", "imex_ssp2_332", 2, True), ("disk", "dg", 2, False)]
_REF = {}


@pytest.mark.parametrize("kind,which,k,fused", SET_DT_CASES)
def test_set_dt_between_steps_matches_the_reference_loop(hip_lib, kind, which, k, fused):
    nx = 8
    h = {"square": 1.0 / nx, "periodic": 2.0 / nx, "disk": 0.25}[kind]
    dt1 = 0.25 * h
    dt2 = 0.6 * dt1
    key = (kind, which, k)
    if key not in _REF:  # shared by the fused and the per-solve case; read-only
        _REF[key] = _reference(kind, which, k, nx, (dt1, dt1, dt2, dt2))
        for a in _REF[key][0]:
            a.setflags(write=False)
    (oQ, op, oq), data = _REF[key]
    ts, (Q, p, q) = _run_with_set_dt(kind, which, k, nx, dt1, dt2, data, fused)
    errs = _rel(Q, oQ), _rel(p, op), _rel(q, oq)
    moved = _rel(oq, ts._as_nodal_pressure(_tracer0))
    print(f"{kind} {which} k={k} fused={fused}: Q {errs[0]:.3e}, p {errs[1]:.3e}, tracer {errs[2]:.3e} (it moved by {moved:.2e})")
    assert max(errs) < TOL and moved > 1e-3, errs


@pytest.mark.parametrize("csr", [False, True])
def test_set_dt_on_a_general_mesh_replaces_the_tables_of_the_old_gamma(hip_lib, monkeypatch, csr):
    """The per-stage preconditioner tables of a general mesh are built for one gamma and replaced (the old ones freed) when
    dt changes: the matrix-free lift tables and, under HDG_GENERAL_CSR_LIFT, the assembled block-Jacobi.  Back and forth
    between two step sizes, against the reference loop."""
    if csr:
        monkeypatch.setenv("HDG_GENERAL_CSR_LIFT", "1")
    else:
        monkeypatch.delenv("HDG_GENERAL_CSR_LIFT", raising=False)
    from oracle import fem
    from oracle import hdg_oracle as orc

    k, dt1 = 2, 0.25 * 0.25
    dt2 = 0.6 * dt1
    dts = (dt1, dt2, dt1, dt2)
    key = ("disk-alternating", k)
    if key not in _REF:
        mesh = _mesh("disk", 0)
        d = orc.HDGDiscretisation(0, k, mesh=fem.TriMesh(mesh.vertices, mesh.cells))
        u0 = lambda x, y: (np.sin(1.3 * x) * np.cos(1.3 * y) + 0.3, -np.cos(1.3 * x) * np.sin(1.3 * y))
        o = ref.imex_loop(lambda dt: orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), dts, d.interpolate_velocity(u0), np.zeros(d.NP),
                          lambda t: np.zeros((d.NQ // 2, 2)))
        _REF[key] = (o.Q, o.p, u0)
    oQ, op, u0 = _REF[key]
    ts, _ = _stepper("disk", k, dt=dt1)
    eng = ts._engine
    ts._forcing_profile, ts._fused = None, True
    ts._init_tracer(None)
    eng.set_state(ts._as_nodal_velocity(u0), np.zeros(eng.shape_p))
    ts._begin_solve()
    t = 0.0
    for n, dt in enumerate(dts):
        eng.set_dt(dt)
        ts._dt, ts._t_adaptive = dt, t
        ts._advance(n, None, False)
        t += dt
    Q, p = ts._current()
    errs = _rel(Q, oQ), _rel(p, op)
    print(f"disk, csr lift {csr}, dt back and forth: Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert max(errs) < TOL


@pytest.mark.parametrize("which", ["dg", "implicit_monolithic"])
def test_controlled_run_of_the_steppers_that_key_a_set_by_dt(hip_lib, which):
    """The DG step and the monolithic HDG step build a preconditioner set per tau / dt; set_dt frees the sets of the step sizes
    left behind.  A controlled Taylor-Green run (k = 2, 8 x 8) of each against the reference loop fed its dt sequence."""
    from dg_reference import dg_solve
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from oracle import hdg_oracle as orc

    kw = {"use_projection_method": False} if which == "implicit_monolithic" else {}
    ts, _ = _stepper("square", K, nx=NX, dt=DT0, which="dg" if which == "dg" else "implicit", **kw)
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.15, cfl=CFL, dt_max=DT_MAX)
    sizes = ts.step_sizes
    assert len(set(sizes[:, 1])) > 2 and abs(sizes[:, 1].sum() - 0.15) <= 1e-12 * 0.15
    d = orc.HDGDiscretisation(NX, K)
    tg = orc.TaylorGreen(d, "exponential", 0.5)
    if which == "dg":
        step = lambda dt, Q_, p_, g: dg_solve(d, Q_, p_, g, dt, 1)
    else:
        step = lambda dt, Q_, p_, g: orc.OracleHDGImplicit(d, dt, use_projection_method=False).solve(Q_, p_, g, dt)
    oQ, op, _ = ref.one_step_loop(step, list(sizes[:, 1]), *tg.initial_condition(), tg.f_rhs)
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"{which}: {len(sizes)} steps, {len(set(sizes[:, 1]))} distinct dt; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert max(errs) < TOL


def test_a_second_engine_built_with_the_new_dt_agrees(hip_lib):
    """An engine constructed with dt2 and given the first engine's state after step two (the stage vectors too: they start
    the Richardson iteration) takes the same two steps"""
    nx, k = 8, 2
    dt1 = 0.25 / nx
    dt2 = 0.6 * dt1
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, _ = _stepper("square", k, nx=nx, dt=dt1)
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 2 * dt1, fused=True)
    other, _ = _stepper("square", k, nx=nx, dt=dt2)
    mo = TaylorGreen(other._V_Q, other._V_p, "exponential", 0.5)
    other._forcing_profile, other._fused = None, True
    other._init_tracer(None)
    other._engine.set_state(*ts._current())
    for i in range(ts.nstages):
        Q, p, lam = ts._engine.get_field(i)
        other._engine.set_field(i, Q=Q, p=p, lam=lam)
    ts._engine.set_dt(dt2)
    ts._dt = dt2
    for e, f in ((ts, mp.f_rhs()), (other, mo.f_rhs())):
        e._forcing_profile = None
        t = 2 * dt1
        for n in range(2):
            e._t_adaptive = t
            e._advance(n, f, False)
            t += dt2
    (Q1, p1), (Q2, p2) = ts._current(), other._current()
    errs = _rel(Q1, Q2), _rel(p1, p2)
    print(f"engine with set_dt against an engine built with dt2: Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert max(errs) < TOL


@pytest.mark.parametrize("which", ["imex_ssp2_332", "implicit", "dg"])
def test_set_dt_with_the_value_held_is_a_no_op(hip_lib, which):
    """set_dt(get_dt()) between steps: fields, iteration counts and the state digest are bitwise those of a run without"""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    out = []
    for call in (False, True):
        ts, _ = _stepper("square", 2, nx=8, dt=0.25 / 8, which=which)
        eng = ts._engine
        mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
        ts._forcing_profile, ts._fused = None, False
        ts._init_tracer(None)
        eng.set_state(*(ts._as_nodal_velocity(mp.initial_condition()[0]), ts._as_nodal_pressure(mp.initial_condition()[1])))
        ts._begin_solve()
        for n in range(3):
            if call:
                eng.set_dt(eng.get_dt())
            ts._advance(n, mp.f_rhs(), False)
        its = [a.value for a in (ts._averagers() if which.startswith("imex") else [ts.niter_tentative, ts.niter_pressure] if which == "implicit" else [ts.niter])]
        out.append((eng.get_field(0), its, eng.state_digest(), eng.iteration_stats()))
    (f0, i0, d0, s0), (f1, i1, d1, s1) = out
    assert all(np.array_equal(a, b) for a, b in zip(f0, f1)) and i0 == i1 and tuple(d0) == tuple(d1)
    assert all(np.array_equal(a, b) for a, b in zip(s0, s1))


# ---- controlled runs
class _Keep:
    def __init__(self):
        self.fields, self.t = [], []

    def reset(self):
        self.fields, self.t = [], []

    def __call__(self, Q, p, t, q_tracer=None):
        self.fields.append(np.array(Q.dat.data, dtype=float))
        self.t.append(t)


@pytest.fixture(scope="module")
def run_a(hip_lib):
    """Run (a): Taylor-Green with exponential forcing, k = 2, 8 x 8, cfl = 0.3, with every recorder on"""
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    keep = _Keep()
    ts, mesh = _stepper("square", K, nx=NX, dt=DT0, callbacks=[keep])
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    xy = 0.1 + 0.8 * np.random.default_rng(7).random((12, 2))
    probes = np.array([[0.3, 0.4], [0.71, 0.22]])
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T_FINAL, fused=True, cfl=CFL, dt_max=DT_MAX, diagnostics=True,
                    probes=probes, particles=xy)
    return ts, mesh, keep, xy, Q.dat.data.copy(), p.dat.data.copy()


def test_controlled_run_lands_on_t_final_and_follows_the_twin(run_a):
    ts, mesh, keep, xy, Q, p = run_a
    sizes, dec = ts.step_sizes, ts.step_decisions
    t_end = sizes[-1, 0] + sizes[-1, 1]
    print(f"run (a): {len(sizes)} steps, dt in [{sizes[:, 1].min()!r}, {sizes[:, 1].max()!r}], A dt in [{sizes[:, 2].min():.4f}, {sizes[:, 2].max():.4f}]")
    assert abs(t_end - T_FINAL) <= 1e-12 * T_FINAL and abs(sizes[:, 1].sum() - T_FINAL) <= 1e-12 * T_FINAL
    assert len(dec) == len(sizes) and len(set(sizes[:, 1])) > 2  # the step size did change
    dts, props = ref.replay(dec[:, 1], DT0, T_FINAL, cfl=CFL, dt_max=DT_MAX)
    assert np.array_equal(dts.view(np.uint64), sizes[:, 1].view(np.uint64))  # bit for bit
    assert np.array_equal(props.view(np.uint64), dec[:, 3].view(np.uint64))
    assert np.all(sizes[:-1, 2] <= CFL * (1 + 0.1) * (1 + 1e-12))  # held within the band (the last step lands)
    assert ts._engine.get_dt() == DT0 == ts._dt  # the stepper holds the constructor's dt again


def test_controlled_run_matches_the_reference_loop(run_a):
    from oracle import hdg_oracle as orc

    ts, mesh, keep, xy, Q, p = run_a
    d = orc.HDGDiscretisation(NX, K)
    tg = orc.TaylorGreen(d, "exponential", 0.5)
    o = ref.imex_loop(lambda dt: orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), list(ts.step_sizes[:, 1]), *tg.initial_condition(), tg.f_rhs)
    errs = _rel(Q, o.Q), _rel(p, o.p)
    print(f"run (a) against the reference loop with its dt sequence: Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert max(errs) < TOL


def test_recorders_take_their_times_from_the_step_sizes(run_a):
    import particle_reference as par
    import probe_reference as pr

    ts, mesh, keep, xy, Q, p = run_a
    sizes = ts.step_sizes
    n = len(sizes)
    times = np.concatenate([[0.0], np.cumsum(sizes[:, 1])])
    for rec in (ts.diagnostics, ts.probes, ts.particles):
        assert len(rec["t"]) == n + 1
        assert np.array_equal(rec["t"][:-1], sizes[:, 0]) and np.max(np.abs(rec["t"] - times)) <= 1e-15 * n
    assert np.array_equal(keep.t[1:], list(ts.diagnostics["t"][1:])) and len(keep.fields) == n + 1
    assert ts.probes["u"].shape == (n + 1, 2, 2) and ts.particles["xy"].shape == (n + 1, len(xy), 2)
    # the cfl column was recorded with the dt of the step that ended in the row
    assert np.all(np.isfinite(ts.diagnostics["cfl"]))
    # particles: Heun's method through the run's fields with its dt sequence
    ev = pr.PointEvaluator(K, ts._engine.node_coordinates()[0], square=(mesh.nx, mesh.ny, mesh.L, False))
    X, want = xy.copy(), [xy.copy()]
    for s in range(n):
        rows, _, margins = par.heun_fields(ev, keep.fields[s:s + 2], X, sizes[s, 1])
        assert margins.min() >= 1e-9
        X = rows[-1]
        want.append(X.copy())
    err = np.max(np.abs(ts.particles["xy"] - np.array(want)))
    print(f"particles against the checker with the dt sequence: {err:.3e}")
    assert err <= 1e-10 * mesh.L and ts.particles["lost"] == 0


def _cavity(viscosity=None, dt=0.02, dt_max=None, **kw):
    from incompressibleeulerhdg_amd.model_problems import Cavity

    opts = dict(buoyancy=20.0, gravity=(0.0, -1.0))
    if viscosity is not None:
        opts.update(viscosity=viscosity, wall="no_slip")
    hot = lambda x, y: np.where(x < 0.5, 1.0, 0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)  # neither the constructor nor the run may warn
        ts, mesh = _stepper("square", 2, nx=8, dt=dt, **opts)
        mp = Cavity(ts._V_Q, ts._V_p)
        ts.solve(*mp.initial_condition(), hot, mp.f_rhs(), 0.6, fused=True, cfl=0.3, dt_max=dt_max, **kw)
    return ts


def test_cavity_from_rest_starts_at_dt_max_and_shrinks(hip_lib):
    """(b) from rest A = 0: the first decision returns dt_max; buoyancy sets the fluid going and a later decision shrinks dt;
    every decision is the twin's"""
    dt, dt_max = 0.02, 0.024
    ts = _cavity(dt=dt, dt_max=dt_max)
    dec, sizes = ts.step_decisions, ts.step_sizes
    print(f"cavity: {len(sizes)} steps, dt from {sizes[0, 1]!r} to {sizes[-2, 1]!r}, A from {dec[0, 1]!r} to {dec[-1, 1]!r}")
    assert dec[0, 1] == 0.0 and dec[0, 3] == dt_max and sizes[0, 1] == dt_max
    assert np.any(dec[1:-1, 3] < dec[1:-1, 2])
    for t, A, held, p in dec:
        v, want = ref.propose(A, held, t, 0.6, 0.3, dt_max=dt_max)
        assert v == "ok" and np.float64(want).view(np.uint64) == np.float64(p).view(np.uint64)


def test_viscous_cap_is_the_active_limit_and_nothing_warns(hip_lib):
    """(c) a viscosity large enough that the viscous cap limits the first step: the proposal equals the cap, and neither the
    constructor (whose dt obeys the limit) nor the run raises a diffusion warning"""
    from incompressibleeulerhdg_amd.timesteppers.common import explicit_stability_limit

    dt = 0.02
    probe, _ = _stepper("square", 2, nx=8, dt=dt)
    probe._engine.set_viscosity(1.0, "no_slip")
    lam = probe._engine.viscosity_number()[0]
    limit = explicit_stability_limit(probe._a_expl, probe._b_expl)
    nu = limit / (1.18 * dt * lam)  # the cap limit / (nu Lambda_u) = 1.18 dt: above the band, below grow dt and dt_max
    ts = _cavity(viscosity=nu, dt=dt, dt_max=1.0)
    cap = ts.viscosity_limit / ts._engine.step_rates()[2]
    dec = ts.step_decisions
    print(f"viscous cap {cap!r} (1.18 dt = {1.18 * dt!r}), first proposal {dec[0, 3]!r}")
    assert dec[0, 1] == 0.0 and dec[0, 3] == cap and 1.1 * dt < cap < 1.25 * dt
    assert np.all(ts.step_sizes[:-1, 1] <= cap)
    for t, A, held, p in dec:
        assert ref.propose(A, held, t, 0.6, 0.3, dt_max=1.0, caps=(0.0, cap, 0.0))[1] == p


# ---- strips
def _ranks(nranks, mode, tmp_path):
    token = "/hdg_adt_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"adt_{mode}{nranks}_{r}.npz") for r in range(nranks)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "adaptive_dt_strip_worker.py"), str(r), str(nranks), token, mode, outs[r]],
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


def test_two_strips_get_the_global_rate(hip_lib, tmp_path):
    """The largest speed sits in the top owned row of the lower strip: every rank gets it, and no ghost row enters"""
    parts = _ranks(2, "rates", tmp_path)
    want = max(np.max(d["local"]) for d in parts)
    assert np.max(parts[0]["local"]) > 10 * np.max(parts[1]["local"])
    assert np.array_equal(parts[0]["rates"], parts[1]["rates"])
    assert abs(parts[0]["rates"][0] - want) <= RATE * want


@pytest.mark.parametrize("mode", ["run", "run_periodic"])
@pytest.mark.parametrize("nranks", [2, 4])
def test_strips_take_the_same_steps_as_one_rank(hip_lib, tmp_path, nranks, mode):
    """Two and four SHM strips of the unit and of the doubly periodic 8 x 8 square (8 rows do not divide by three, which the
    engine refuses): one dt sequence on every rank, the fields of the one-rank run under the bound of the strip tests"""
    parts = _ranks(nranks, mode, tmp_path)
    single = _ranks(1, mode, tmp_path)[0]
    assert len(set(single["sizes"][:, 1])) > 2  # the step size did change
    for d in parts[1:]:  # every rank reports the same dt sequence bit for bit
        assert np.array_equal(d["sizes"].view(np.uint64), parts[0]["sizes"].view(np.uint64))
        assert np.array_equal(d["decisions"].view(np.uint64), parts[0]["decisions"].view(np.uint64))
    assert len(parts[0]["sizes"]) == len(single["sizes"])
    Q, p = np.concatenate([d["Q"] for d in parts]), np.concatenate([d["p"] for d in parts])
    errs = _rel(Q, single["Q"]), _rel(p, single["p"]), _rel(parts[0]["sizes"][:, 1], single["sizes"][:, 1])
    print(f"{mode}: {nranks} strips against one rank ({len(single['sizes'])} steps): Q {errs[0]:.3e}, p {errs[1]:.3e}, dt {errs[2]:.3e}")
    assert max(errs) < TOL


# ---- errors
def test_set_dt_refuses_bad_values_and_leaves_the_engine_alone(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    out = []
    for poke in (False, True):
        ts, _ = _stepper("square", 2, nx=4, dt=0.05)
        eng = ts._engine
        mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
        if poke:
            for bad in (0.0, -0.01, float("nan"), float("inf"), -float("inf")):
                with pytest.raises(_lib.HDGError, match="is not a finite value > 0") as e:
                    eng.set_dt(bad)
                assert e.value.code == -1 and eng.get_dt() == 0.05
        Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.1, fused=True)
        out.append((Q.dat.data, p.dat.data, eng.state_digest()))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and tuple(out[0][2]) == tuple(out[1][2])
    eng.begin_step()
    with pytest.raises(_lib.HDGError, match="a step is open"):
        eng.set_dt(0.01)


def test_max_steps_and_dt_min_stop_the_run(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts, _ = _stepper("square", 2, nx=8, dt=DT0)
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    with pytest.raises(RuntimeError, match=r"max_steps = 3 steps taken and the run is at t = 0\.0\d+, short of T_final = 0\.25"):
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T_FINAL, fused=True, cfl=CFL, max_steps=3, diagnostics=True)
    assert len(ts.step_sizes) == 3 and ts._engine.get_dt() == DT0
    with pytest.raises(_lib.HDGError, match="is below dt_min = 0.019") as e:
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T_FINAL, fused=True, cfl=0.05, dt_min=0.019)
    assert e.value.code == -1 and ts._engine.get_dt() == DT0
    with pytest.raises(ValueError, match="cfl= does not go with checkpoint="):
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T_FINAL, cfl=CFL, checkpoint="c.bin")
    # warmup=True takes the one step at the constructor's dt
    ts.solve(*mp.initial_condition(), None, mp.f_rhs(), T_FINAL, fused=True, cfl=CFL, warmup=True)
    assert ts.step_sizes is None


def test_driver_prints_the_summary_line_and_refuses_checkpoints(hip_lib, tmp_path):
    argv = [sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--nx", "8", "--degree", "2", "--dt", "0.02", "--tfinal", "0.25",
            "--use_projection_method", "--fused", "--output", "", "--cfl", "0.5"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(argv + ["--dt_max", "0.05"], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("steps = ")]
    assert len(line) == 1, r.stdout
    import re

    m = re.fullmatch(r"steps = (\d+), dt in \[(\S+), (\S+)\], last dt = (\S+)", line[0])
    assert m, line
    n, lo, hi, last = int(m.group(1)), float(m.group(2)), float(m.group(3)), float(m.group(4))
    assert 0 < lo <= last <= hi <= 0.05 and n >= 5 and "velocity error" in r.stdout
    r = subprocess.run(argv + ["--checkpoint", "c.bin"], cwd=tmp_path, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode != 0 and "--cfl does not go with --checkpoint" in r.stderr and not os.path.exists(tmp_path / "c.bin")
