"""Transfer of a state between engines of different mesh size and degree on the GPU (hdg_transfer_state /
hdg_transfer_difference, Engine.transfer_from / difference_norms, state_from / difference of the timesteppers, the driver's
--start_from), checked against the numpy projection tests/transfer_reference.py, against polynomial exactness, conservation,
the inverse pair injection / restriction, Pythagoras, a twin engine that was given the same fields through set_state, and
through the steppers and the driver.  Unit square and doubly periodic square; every engine has nx <= 32 (the one refusal of a
ratio above 16 needs 2 -> 34).

The periodic square cannot hold the two cases with nx = 2: hdg_create refuses a periodic mesh of fewer than 4 cell rows, a
refusal that stays.  There the two cases assert that refusal, and the pair (4, 4) <-> (32, 1) (ratio 8) runs in their place
in addition to the seven cases that can be built."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import transfer_reference as ref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# (nx, k) -> (nx, k)
CASES = [((4, 1), (8, 1)), ((4, 2), (12, 3)), ((4, 4), (8, 2)), ((12, 2), (4, 2)), ((8, 3), (4, 4)), ((6, 1), (6, 3)),
         ((6, 3), (6, 1)), ((2, 4), (32, 1)), ((32, 1), (2, 4))]
PERIODIC_EXTRA = [((4, 4), (32, 1)), ((32, 1), (4, 4))]
TRACER_CASES = {((4, 2), (12, 3)), ((12, 2), (4, 2))}  # two tracers ride along: one prolongation, one restriction
KINDS = ["square", "periodic"]
LENGTH = {"square": 1.0, "periodic": 2.0}


def _buildable(kind, case):
    return kind == "square" or min(case[0][0], case[1][0]) >= 4


def _params(cases=None, extra=True):
    out = []
    for kind in KINDS:
        for case in (CASES if cases is None else cases) + (PERIODIC_EXTRA if extra and kind == "periodic" and cases is None else []):
            if _buildable(kind, case) and not (kind == "square" and case in PERIODIC_EXTRA):
                out.append(pytest.param(kind, case, id=f"{kind}-{case[0][0]}k{case[0][1]}-{case[1][0]}k{case[1][1]}"))
    return out


def _injective(case):
    """the destination space contains the source: finer or equal nested mesh and a degree at least the source's"""
    (ns, ks), (nd, kd) = case
    return nd >= ns and kd >= ks


def _stepper(kind, nx, k, dt=0.01, cls=None, **kw):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    L = kw.pop("L", LENGTH[kind])
    mesh = UnitSquareMesh(nx, nx) if kind == "square" else PeriodicSquareMesh(nx, nx, L=L)
    return (cls or IncompressibleEulerHDGIMEXSSP2_332)(mesh, k, dt, use_projection_method=True, n_richardson=2, **kw)


def _evaluator(ts, kind):
    eng = ts._engine
    xq, _ = eng.node_coordinates()
    return ref.evaluator(eng.cfg.nx, eng.cfg.degree, L=ts._mesh.L if kind == "periodic" else 1.0, periodic=kind == "periodic", xq=xq)


def _current(eng):
    Q, p, _ = eng.get_field(0, lam=False)
    return Q, p


class _Transfer:
    """One transfer of seeded random broken data, with the reference's answer: built once per (kind, case) and shared by
    the tests below, which only read it."""

    def __init__(self, kind, case):
        (ns, ks), (nd, kd) = case
        self.kind, self.case = kind, case
        self.ntr = 2 if case in TRACER_CASES else 0
        kw = {"n_tracers": 2} if self.ntr else {}
        self.src, self.dst = _stepper(kind, ns, ks, **kw), _stepper(kind, nd, kd, **kw)
        S, D = self.src._engine, self.dst._engine
        rng = np.random.default_rng(1000 * ns + 100 * ks + 10 * nd + kd + (5 if kind == "periodic" else 0))
        S.set_state(rng.standard_normal(S.shape_Q), rng.standard_normal(S.shape_p))
        if self.ntr:
            S.set_tracer(rng.standard_normal(S.shape_q))
        # what the source holds (set_state has removed the pressure mean)
        self.Qs, self.ps = _current(S)
        self.qs = S.get_tracer() if self.ntr else None
        D.transfer_from(S, tracers=bool(self.ntr))
        self.Qd, self.pd = _current(D)
        self.qd = D.get_tracer() if self.ntr else None
        es, ed = _evaluator(self.src, kind), _evaluator(self.dst, kind)
        self.want_Q = ref.project(es, ed, self.Qs, "u")
        self.want_p = ref.project(es, ed, self.ps, "p")
        self.want_q = np.stack([ref.project(es, ed, q, "p") for q in self.qs]) if self.ntr else None


@functools.lru_cache(maxsize=None)
def _transfer(kind, case):
    return _Transfer(kind, case)


# ---- 1. against the reference
@pytest.mark.parametrize("kind,case", _params())
def test_transfer_matches_the_reference_projection(hip_lib, kind, case):
    """Seeded random nodal data, a different polynomial in every cell; rounding bound 1e-11 max|field| (at most 21 * 256
    terms, times the conditioning of nodal <-> modal at k = 4).  Largest deviation seen on the MI355X: see DESIGN.md
    section 18."""
    T = _transfer(kind, case)
    fields = [("Q", T.Qd, T.want_Q), ("p", T.pd, T.want_p)]
    if T.ntr:
        fields += [(f"q{t}", T.qd[t], T.want_q[t]) for t in range(T.ntr)]
    worst = 0.0
    for name, got, want in fields:
        dev = np.max(np.abs(got - want)) / np.max(np.abs(want))
        worst = max(worst, dev)
        print(f"transfer {kind} {case}: {name} deviation {dev:.3e} of max|field|")
    print(f"transfer {kind} {case}: largest deviation {worst:.3e}")
    for name, got, want in fields:
        assert np.max(np.abs(got - want)) <= 1e-11 * np.max(np.abs(want)), name


@pytest.mark.parametrize("case", [c for c in CASES if min(c[0][0], c[1][0]) < 4])
def test_periodic_square_refuses_the_meshes_of_two_cells(hip_lib, case):
    """Why the nx = 2 cases run on the unit square only: the engine refuses the periodic mesh (a refusal that stays)."""
    from incompressibleeulerhdg_amd import _lib

    nx, k = min(case, key=lambda c: c[0])
    with pytest.raises(_lib.HDGError, match="at least 4 cell rows"):
        _stepper("periodic", nx, k)


# ---- 2. polynomial exactness
@pytest.mark.parametrize("kind,case", _params())
def test_polynomials_of_the_common_degree_are_reproduced(hip_lib, kind, case):
    (ns, ks), (nd, kd) = case
    k = min(ks, kd)
    src, dst = _stepper(kind, ns, ks), _stepper(kind, nd, kd)
    ux = lambda x, y: 0.3 + x ** (k + 1) - 2 * x * y ** k + y  # noqa: E731
    uy = lambda x, y: y ** (k + 1) + 0.5 * x ** k * y - x  # noqa: E731
    pf = lambda x, y: 1.0 - x ** k + x * y ** (k - 1) + 0.25 * y  # noqa: E731
    vel = lambda x, y: (ux(x, y), uy(x, y))  # noqa: E731
    src._engine.set_state(src._V_Q.interpolate(vel), src._V_p.interpolate(pf))
    dst._engine.transfer_from(src._engine)
    Qd, pd = _current(dst._engine)
    want_Q, want_p = dst._V_Q.interpolate(vel), dst._V_p.interpolate(pf)
    L = LENGTH[kind]
    want_p0 = want_p - dst._engine.integrate_pressure(want_p) / L ** 2  # the state carries a pressure of zero mean
    assert np.max(np.abs(Qd - want_Q)) <= 1e-12 * np.max(np.abs(want_Q))
    assert np.max(np.abs(pd - want_p0)) <= 1e-12 * np.max(np.abs(want_p))


# ---- 3. conservation
def _velocity_integrals(ts, Q):
    """Integrals of the two components of a nodal velocity: nodal weights of the oracle's basis by quadrature, times h^2"""
    from oracle import fem

    k = ts.degree
    pts, w = fem.triangle_quadrature(k + 1)
    W = w @ fem.PolySpace2D(k + 1).tabulate(pts)
    h = (ts._mesh.L if getattr(ts._mesh, "periodic", False) else 1.0) / ts._mesh.nx
    return h * h * np.einsum("n,cnd->d", W, np.asarray(Q).reshape(-1, len(W), 2))


@pytest.mark.parametrize("kind,case", _params())
def test_integrals_are_conserved(hip_lib, kind, case):
    T = _transfer(kind, case)
    S, D = T.src._engine, T.dst._engine
    L2 = LENGTH[kind] ** 2
    pairs = [("p", S.integrate_pressure(T.ps), D.integrate_pressure(T.pd), np.max(np.abs(T.ps)))]
    if T.ntr:
        pairs += [(f"q{t}", S.integrate_pressure(T.qs[t]), D.integrate_pressure(T.qd[t]), np.max(np.abs(T.qs[t]))) for t in range(T.ntr)]
    before, after = _velocity_integrals(T.src, T.Qs), _velocity_integrals(T.dst, T.Qd)
    pairs += [(f"u{d}", before[d], after[d], np.max(np.abs(T.Qs[:, d]))) for d in range(2)]
    for name, a, b, scale in pairs:
        print(f"conservation {kind} {case}: {name} before {a!r} after {b!r}")
        assert abs(a - b) <= 1e-13 * scale * L2, name


# ---- 4. injection, then restriction, is the identity
@pytest.mark.parametrize("kind,case", _params([c for c in CASES if _injective(c)]))
def test_injection_then_restriction_is_the_identity(hip_lib, kind, case):
    T = _transfer(kind, case)
    (ns, ks), _ = case
    kw = {"n_tracers": 2} if T.ntr else {}
    back = _stepper(kind, ns, ks, **kw)
    back._engine.transfer_from(T.dst._engine, tracers=bool(T.ntr))
    Qb, pb = _current(back._engine)
    assert np.max(np.abs(Qb - T.Qs)) <= 1e-12 * np.max(np.abs(T.Qs))
    assert np.max(np.abs(pb - T.ps)) <= 1e-12 * np.max(np.abs(T.ps))
    if T.ntr:
        assert np.max(np.abs(back._engine.get_tracer() - T.qs)) <= 1e-12 * np.max(np.abs(T.qs))
    # the injected field is the source's field: no difference on the common refinement
    d = T.dst._engine.difference_norms(T.src._engine)
    nQ, np_ = T.src._engine.l2_norms(T.Qs, T.ps)
    assert d["Q"] <= 1e-12 * nQ and d["p"] <= 1e-12 * np_


# ---- 5. difference norms
# the coarser mesh carries the higher degree, the lower degree, and the same mesh with two degrees
DIFF_PAIRS = [((4, 3), (8, 1)), ((4, 1), (12, 2)), ((6, 2), (6, 4)), ((16, 2), (4, 2))]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("pair", DIFF_PAIRS, ids=lambda p: f"{p[0][0]}k{p[0][1]}-{p[1][0]}k{p[1][1]}")
def test_difference_norms_agree_with_quadrature(hip_lib, kind, pair):
    (na, ka), (nb, kb) = pair
    A, B = _stepper(kind, na, ka, n_tracers=2), _stepper(kind, nb, kb, n_tracers=2)
    w = 2 * np.pi / LENGTH[kind]
    fa = (lambda x, y: (np.sin(w * x) * np.cos(w * y), 0.5 * np.cos(2 * w * x) + y), lambda x, y: np.cos(w * (x + y)),
          [lambda x, y: np.sin(w * x), lambda x, y: np.exp(-x) * np.sin(w * y)])
    fb = (lambda x, y: (np.sin(w * x + 0.3) * np.cos(w * y), 0.4 * np.cos(2 * w * x) + y * y), lambda x, y: np.cos(w * (x - 2 * y)),
          [lambda x, y: np.sin(w * x + 0.1), lambda x, y: np.exp(-y) * np.sin(w * x)])
    for ts, (fQ, fp, fq) in ((A, fa), (B, fb)):
        ts._engine.set_state(ts._V_Q.interpolate(fQ), ts._V_p.interpolate(fp))
        ts._engine.set_tracer(np.stack([ts._V_p.interpolate(f) for f in fq]))
    ea, eb = _evaluator(A, kind), _evaluator(B, kind)
    (Qa, pa), (Qb, pb) = _current(A._engine), _current(B._engine)
    qa, qb = A._engine.get_tracer(), B._engine.get_tracer()
    got = A._engine.difference_norms(B._engine)
    want = {"Q": ref.difference_norm(ea, eb, Qa, Qb, "u"), "p": ref.difference_norm(ea, eb, pa, pb, "p"),
            "q": np.array([ref.difference_norm(ea, eb, qa[t], qb[t], "p") for t in range(2)])}
    for name in ("Q", "p", "q"):
        print(f"difference {kind} {pair}: {name} got {got[name]!r} want {want[name]!r}")
        assert np.all(np.abs(got[name] - want[name]) <= 1e-12 * np.abs(want[name])), name
    # symmetric to rounding, and exactly zero against itself
    rev = B._engine.difference_norms(A._engine)
    for name in ("Q", "p", "q"):
        assert np.all(np.abs(rev[name] - got[name]) <= 1e-14 * np.abs(got[name])), name
    same = A._engine.difference_norms(A._engine)
    assert same["Q"] == 0.0 and same["p"] == 0.0 and np.array_equal(same["q"], np.zeros(2))
    assert A.difference(B)["Q"] == got["Q"]  # the timestepper's spelling
    # without tracers on one side there are no tracer norms
    B._engine.set_tracer(None)
    assert A._engine.difference_norms(B._engine)["q"] is None


@pytest.mark.parametrize("kind,case", _params([c for c in CASES + PERIODIC_EXTRA if not _injective(c)], extra=False))
def test_projection_defect_is_orthogonal(hip_lib, kind, case):
    """Pythagoras for every non-injective case: |u_S|^2 = |P u_S|^2 + |u_S - P u_S|^2 to 1e-12 relative, the norms from
    l2_norms and difference_norms."""
    T = _transfer(kind, case)
    S, D = T.src._engine, T.dst._engine
    nQ, np_ = S.l2_norms(T.Qs, T.ps)
    mQ, mp = D.l2_norms(T.Qd, T.pd)
    d = D.difference_norms(S)
    print(f"pythagoras {kind} {case}: Q {nQ ** 2!r} = {mQ ** 2!r} + {d['Q'] ** 2!r};  p {np_ ** 2!r} = {mp ** 2!r} + {d['p'] ** 2!r}")
    assert abs(nQ ** 2 - mQ ** 2 - d["Q"] ** 2) <= 1e-12 * nQ ** 2
    assert abs(np_ ** 2 - mp ** 2 - d["p"] ** 2) <= 1e-12 * np_ ** 2
    if T.ntr:
        for t in range(T.ntr):
            ns_ = S.l2_norms(None, T.qs[t])[1]
            nd_ = D.l2_norms(None, T.qd[t])[1]
            assert abs(ns_ ** 2 - nd_ ** 2 - d["q"][t] ** 2) <= 1e-12 * ns_ ** 2


# ---- 6. the destination behaves as after set_state
@pytest.mark.parametrize("kind", KINDS)
def test_destination_steps_like_a_twin_that_was_given_the_fields(hip_lib, kind):
    (ns, ks), (nd, kd) = (4, 1), (8, 2)
    src = _stepper(kind, ns, ks, n_tracers=2)
    one, twin = _stepper(kind, nd, kd, n_tracers=2), _stepper(kind, nd, kd, n_tracers=2)
    L = LENGTH[kind]
    w = 2 * np.pi / L
    vel = lambda x, y: (np.sin(w * x) * np.cos(w * y), -np.cos(w * x) * np.sin(w * y))  # noqa: E731
    src._engine.set_state(src._V_Q.interpolate(vel), src._V_p.interpolate(lambda x, y: np.cos(w * x) * np.cos(w * y)))
    src._engine.set_tracer(np.stack([src._V_p.interpolate(lambda x, y: np.sin(w * x)), src._V_p.interpolate(lambda x, y: np.cos(w * y))]))
    seeds = np.random.default_rng(11).random((20, 2)) * L
    for ts in (one, twin):  # before the transfer: the predictor is that of the zero field
        ts._engine.set_particles(seeds, 4)
    one._engine.transfer_from(src._engine, tracers=True)
    Q, p = _current(one._engine)
    twin._engine.set_tracer(one._engine.get_tracer())
    twin._engine.set_state(Q, p)
    for ts in (one, twin):
        for i in range(ts._engine.nstages + 1):
            ts._engine.set_forcing_scale(i, 0.0)
        ts._engine.reconstruct_trace()
        ts._engine.step()
    (Q1, p1), (Q2, p2) = _current(one._engine), _current(twin._engine)
    umax = np.max(np.abs(Q2))
    assert np.all(np.isfinite(Q1)) and umax > 0.1
    assert np.max(np.abs(Q1 - Q2)) < 2e-8 * umax and np.max(np.abs(p1 - p2)) < 2e-8 * np.max(np.abs(p2))
    q1, q2 = one._engine.get_tracer(), twin._engine.get_tracer()
    assert np.max(np.abs(q1 - q2)) < 2e-8 * np.max(np.abs(q2))
    (r1, c1), (r2, c2) = one._engine.particles(), twin._engine.particles()
    assert r1.shape == (2, 20, 2) and c1 == c2
    assert np.array_equal(r1[0], r2[0]) and np.max(np.abs(r1[1] - r2[1])) <= 1e-12 * L
    assert np.max(np.abs(r1[1] - r1[0])) > 1e-4 * L  # they did move with the new field


# ---- 7. refusals
def _refused(dst, src, code, match, tracers=False, diff=False):
    from incompressibleeulerhdg_amd import _lib

    before = _current(dst._engine)
    with pytest.raises(_lib.HDGError, match=match) as e:
        if diff:
            dst._engine.difference_norms(src._engine)
        else:
            dst._engine.transfer_from(src._engine, tracers=tracers)
    assert e.value.code == code, (e.value.code, str(e.value))
    after = _current(dst._engine)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])


def test_refusals_name_their_cause_and_leave_the_engines_alone(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    ARG, UNSUPPORTED = -1, -5
    rng = np.random.default_rng(2)
    dst = _stepper("square", 8, 2)
    dst._engine.set_state(rng.standard_normal(dst._engine.shape_Q), rng.standard_normal(dst._engine.shape_p))
    per8 = _stepper("periodic", 8, 2, L=1.0)
    per8._engine.set_state(rng.standard_normal(per8._engine.shape_Q), rng.standard_normal(per8._engine.shape_p))
    _refused(dst, dst, ARG, "dst == src")
    _refused(dst, _stepper("periodic", 4, 1, L=1.0), ARG, "different mesh kind")
    _refused(per8, _stepper("periodic", 4, 1, L=2.0), ARG, "different L")
    _refused(dst, _stepper("square", 6, 1), ARG, "not nested")
    _refused(dst, _stepper("square", 12, 1), ARG, "not nested")
    _refused(_stepper("square", 34, 1), _stepper("square", 2, 1), ARG, "ratio r = 17 > 16")
    # tracers: a source without one, and another number of them
    src = _stepper("square", 4, 1)
    _refused(dst, src, ARG, "tracer mismatch", tracers=True)
    src2 = _stepper("square", 4, 1, n_tracers=2)
    src2._engine.set_tracer(np.zeros(src2._engine.shape_q))
    _refused(dst, src2, ARG, "tracer mismatch", tracers=True)
    # an open step on either side
    for i in range(src._engine.nstages + 1):
        src._engine.set_forcing_scale(i, 0.0)
    src._engine.begin_step()
    _refused(dst, src, ARG, "a step is open")
    _refused(dst, src, ARG, "a step is open", diff=True)
    dst2 = _stepper("square", 8, 1)
    _refused(src, dst2, ARG, "a step is open")
    # general meshes
    disk = IncompressibleEulerHDGIMEXSSP2_332(UnitDiskMesh(1), 1, 0.01, use_projection_method=True, n_richardson=2)
    _refused(dst, disk, UNSUPPORTED, "general meshes")
    _refused(disk, dst, UNSUPPORTED, "general meshes")
    _refused(dst, disk, UNSUPPORTED, "general meshes", diff=True)
    # and a pair that fits still goes through afterwards
    dst._engine.transfer_from(dst2._engine)


def test_refuses_another_device(hip_lib):
    import torch

    if torch.cuda.device_count() < 2:
        pytest.skip("one device: an engine on another device cannot be built")
    _refused(_stepper("square", 8, 1), _stepper("square", 4, 1, device=1), -1, "different device")


def test_refuses_engines_of_several_ranks(hip_lib, tmp_path):
    """A strip engine is HDG_ERR_UNSUPPORTED on either side: two ranks over the shared-memory transport, each offering its
    strip to a one-rank engine."""
    import uuid

    token = "/hdg_xfer_" + uuid.uuid4().hex[:12]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "transfer_strip_worker.py"), str(r), "2", token],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, PYTHONPATH=ROOT))
             for r in range(2)]
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
    for r, proc in enumerate(procs):
        assert proc.returncode == 0 and "refused ok" in logs[r], logs[r][-3000:]


# ---- 8. through the steppers
def test_a_coarse_run_starts_a_finer_run_of_higher_degree(hip_lib):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    L = 2 * np.pi
    coarse = IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(8, 8, L=L), 1, 0.01, use_projection_method=True, n_richardson=2)
    fine = IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(16, 16, L=L), 2, 0.005, use_projection_method=True, n_richardson=2)
    mp = DoubleLayerShearFlow(coarse._V_Q, coarse._V_p)
    coarse.solve(*mp.initial_condition(), None, mp.f_rhs(), 4 * 0.01, fused=True, diagnostics=True)
    Q0, p0, q0 = fine.state_from(coarse)
    assert q0 is None and Q0.dat.data.shape == fine._engine.shape_Q and p0.dat.data.shape == fine._engine.shape_p
    fine.solve(Q0, p0, q0, mp.f_rhs(), 2 * 0.005, fused=True, diagnostics=True)
    e_coarse, e_fine = coarse.diagnostics["energy"][-1], fine.diagnostics["energy"][0]
    print(f"energy: coarse run's last row {e_coarse!r}, fine run's first row {e_fine!r}")
    assert abs(e_fine - e_coarse) <= 1e-12 * e_coarse  # injection preserves the L2 norm
    for name, series in fine.diagnostics.items():
        if name not in ("tracer_integral", "tracer_half_sq"):  # NaN without a tracer
            assert series.shape == (3,) and np.all(np.isfinite(series)), name
    d = fine.difference(coarse)
    assert np.isfinite(d["Q"]) and d["Q"] > 0 and np.isfinite(d["p"]) and d["p"] > 0 and d["q"] is None


def test_state_from_carries_the_tracers(hip_lib):
    coarse, fine = _stepper("periodic", 4, 1, n_tracers=2), _stepper("periodic", 8, 2, n_tracers=2)
    w = np.pi
    coarse._engine.set_state(coarse._V_Q.interpolate(lambda x, y: (np.sin(w * x), np.cos(w * y))), np.zeros(coarse._engine.shape_p))
    coarse._engine.set_tracer(np.stack([coarse._V_p.interpolate(lambda x, y: x + y), coarse._V_p.interpolate(lambda x, y: x - 2 * y)]))
    Q, p, q = fine.state_from(coarse)
    assert isinstance(q, list) and len(q) == 2 and q[0].dat.data.shape == fine._engine.shape_p
    assert np.max(np.abs(q[0].dat.data - fine._V_p.interpolate(lambda x, y: x + y))) <= 1e-12 * 4
    assert np.max(np.abs(q[1].dat.data - fine._V_p.interpolate(lambda x, y: x - 2 * y))) <= 1e-12 * 4


# ---- 9. driver
def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _csv(path):
    lines = open(path).read().strip().splitlines()
    names = lines[0].split(",")
    return names, np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])


def test_driver_starts_from_the_checkpoint_of_a_coarser_run(hip_lib, tmp_path):
    _driver(["--problem", "shear", "--nx", "8", "--degree", "1", "--dt", "0.01", "--tfinal", "0.04", "--output", "",
             "--checkpoint", "ck", "--diagnostics", "d1.csv"], tmp_path)
    out = _driver(["--problem", "shear", "--nx", "16", "--degree", "2", "--dt", "0.005", "--tfinal", "0.01", "--output", "",
                   "--start_from", "ck", "--start_nx", "8", "--start_degree", "1", "--start_dt", "0.01", "--diagnostics", "d2.csv"],
                  tmp_path)
    m = re.search(r"^start: transferred nx = 8, degree = 1, t = (\S+) -> nx = 16, degree = 2$", out, re.M)
    assert m, out[-3000:]
    names, first = _csv(tmp_path / "d1.csv")
    _, second = _csv(tmp_path / "d2.csv")
    assert float(m[1]) == first[-1, names.index("t")] and abs(float(m[1]) - 0.04) < 1e-12
    e = names.index("energy")
    assert second.shape[0] == 3 and second[0, names.index("t")] == 0.0
    assert abs(second[0, e] - first[-1, e]) <= 1e-12 * first[-1, e]
