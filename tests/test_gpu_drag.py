"""The linear drag term on the GPU (include/hdg_drag.h) against tests/drag_reference.py.

Bounds, the project's: the hook and the force relative 1e-10; whole steps and strips 2e-8 for Q and p; the manufactured
solution's L2 error relative 1e-6 against the reference's.  Switched off, everything is bitwise what it is without the feature."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import drag_reference as ref
import viscosity_reference as vref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL = 1e-10, 2e-8
L_PER = 2 * np.pi
NUMBER = 0.3  # S dt of the whole-step runs


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _mesh(kind, nx):
    import manufactured as ms
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, TriangleMesh, UnitDiskMesh, UnitSquareMesh

    if kind == "square":
        return UnitSquareMesh(nx, nx)
    if kind == "periodic":
        return PeriodicSquareMesh(nx, nx, L=L_PER)
    return UnitDiskMesh(nx) if kind == "disk" else TriangleMesh(*ms.perturbed_square_mesh(nx))


def _oracle(kind, nx, k, mesh):
    from oracle import fem
    from oracle import hdg_oracle as orc

    if kind == "square":
        return orc.HDGDiscretisation(nx, k)
    if kind == "periodic":
        return orc.HDGDiscretisation(nx, k, periodic=True, L=L_PER)
    return orc.HDGDiscretisation(0, k, mesh=fem.TriMesh(mesh.vertices, mesh.cells))


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.setdefault("use_projection_method", True)
        kw.update(n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _setting(V, rng, S=1.0, most_zero=True):
    """Random vertex values in [0, S] (broken across cells, the largest equal to S) on a cluster of cells, zero on the others"""
    ctr = V.mean(axis=1)
    lo, hi = ctr.min(axis=0), ctr.max(axis=0)
    z = (ctr - lo) / np.maximum(hi - lo, 1e-300)
    on = (z[:, 0] < 0.45) & (z[:, 1] > 0.3) if most_zero else (z[:, 0] < 0.6)
    sig = rng.uniform(0.0, S, (len(V), 3)) * on[:, None]
    sig[np.nonzero(on)[0][0], 1] = S
    return sig


# ---- 1. the hook and 2. the force against the reference
HOOK_CASES = ([("square", 3, k) for k in (1, 2, 3, 4)] + [("periodic", 4, k) for k in (1, 2, 3, 4)] +
              [("square", 12, 1), ("square", 130, 1), ("disk", 1, 2), ("disk", 2, 1), ("perturbed", 3, 1)])
_CASE = {}


def _case(kind, nx, k):
    """engine, geometry, setting and fields of one mesh: built once, shared by the hook and the force test, read-only"""
    key = (kind, nx, k)
    if key in _CASE:
        return _CASE[key]
    eng = _stepper("ssp2", _mesh(kind, nx), k, 0.01)._engine
    V = eng.cell_vertices()
    X = eng.node_coordinates()[0]
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(41 + k)
    w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)
    smooth = lambda: sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    poly = np.stack([1.0 + x - 2.0 * y + (x * y if k > 1 else 0.0) + (y ** k), 0.5 - y + 0.3 * x - (x ** k)], axis=-1)  # degree <= k
    c = dict(eng=eng, V=V, X=X, areas=ref.cell_areas(V), sig=_setting(V, rng, 1.7),
             target=np.stack([smooth(), smooth()], axis=-1), ptarget=np.stack([0.3 - x + 0.5 * y, 0.1 + 0.2 * x + y], axis=-1),
             fields=[np.stack([smooth(), smooth()], axis=-1), rng.standard_normal((len(x), 2)), poly],
             region=rng.integers(0, 4, len(V)))
    on = np.nonzero(np.any(c["sig"] != 0.0, axis=1))[0]
    assert len(on) >= 4
    c["region"][on] = np.arange(len(on)) % 4  # every region holds a cell that carries a sigma
    c["B"] = ref.blocks(c["sig"], k)
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _CASE[key] = c
    return c


def _nodal_sigma(c):
    """the cellwise linear sigma at the velocity nodes, from the nodes' barycentric coordinates"""
    V, X = c["V"], c["X"].reshape(len(c["V"]), -1, 2)
    J = np.stack([V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]], axis=-1)
    lam = np.einsum("cij,cnj->cni", np.linalg.inv(J), X - V[:, None, 0])
    s = c["sig"]
    return (s[:, None, 0] + (s[:, 1] - s[:, 0])[:, None] * lam[..., 0] + (s[:, 2] - s[:, 0])[:, None] * lam[..., 1]).reshape(-1)


@pytest.mark.parametrize("kind,nx,k", HOOK_CASES)
def test_hook_against_the_reference(hip_lib, kind, nx, k):
    c = _case(kind, nx, k)
    eng, sig, B = c["eng"], c["sig"], c["B"]
    assert np.mean(np.all(sig == 0.0, axis=1)) > 0.5  # sigma = 0 on most cells
    if kind in ("square", "periodic"):  # the vertex order the tables belong to
        from incompressibleeulerhdg_amd.output import _cell_vertices

        assert np.max(np.abs(c["V"] - _cell_vertices(nx, nx, L_PER if kind == "periodic" else 1.0))) < 1e-12
    else:
        mesh = _mesh(kind, nx)
        assert np.array_equal(c["V"], np.asarray(mesh.vertices, dtype=float)[np.asarray(mesh.cells)])
    worst = 0.0
    for n, Q in enumerate(c["fields"]):
        for target in (None, c["target"]):
            want = ref.apply_blocks(B, Q, target)
            got = eng.apply_drag(Q, sig, target)
            err = np.max(np.abs(got - want)) / np.max(np.abs(want))
            worst = max(worst, err)
            assert err <= HOOK, (n, target is None, err)
            # Q^T M out = P: the rate of work of the term, from the force kernels
            P = eng.drag_force_of(Q, sig, target)[:, 2].sum()
            work = ref.mass_dot(k, c["areas"], Q, got)
            assert abs(P - work) <= HOOK * max(abs(work), ref.mass_dot(k, c["areas"], Q, Q) * 1.7), (n, P, work)
            if target is None:
                assert work <= 0.0
    exact = ref.closed_form(_nodal_sigma(c), c["fields"][2], c["ptarget"])
    closed = np.max(np.abs(eng.apply_drag(c["fields"][2], sig, c["ptarget"]) - exact)) / np.max(np.abs(exact))
    assert closed <= HOOK, closed
    assert not eng.drag().any() and eng.drag_number() == (0.0, 0.0)  # the hooks set nothing
    eng.set_drag(sig, c["target"], c["region"])
    S, number = eng.drag_number()
    rho = float(np.max(np.linalg.eigvals(B).real))  # M^-1 D is block diagonal: its spectrum is the blocks'
    assert np.array_equal(eng.drag(), sig) and S == ref.bound(sig) and number == pytest.approx(0.01 * S, rel=1e-14)
    assert S >= rho * (1 - 1e-12) and np.min(np.linalg.eigvals(B).real) >= -1e-12 * S
    eng.set_drag(None)
    assert not eng.drag().any() and eng.drag_number() == (0.0, 0.0)
    print(f"{kind} nx={nx} k={k}: largest |out - reference| = {worst:.3e} max|out|; closed form {closed:.3e}; S {S:.6g}, rho {rho:.6g}")


@pytest.mark.parametrize("kind,nx,k", HOOK_CASES)
def test_force_against_the_reference(hip_lib, kind, nx, k):
    c = _case(kind, nx, k)
    eng, sig = c["eng"], c["sig"]
    three = np.where(c["region"] == 2, 3, c["region"])  # region 2 empty
    worst = 0.0
    for Q in c["fields"][:2]:
        for target in (None, c["target"]):
            for region in (c["region"], three, None):
                want = ref.force_blockwise(sig, k, c["areas"], Q, target, region)
                got = eng.drag_force_of(Q, sig, target, region)
                assert got.shape == (4, 3)
                err = np.max(np.abs(got - want)) / np.max(np.abs(want))
                worst = max(worst, err)
                assert err <= HOOK, err
                assert np.array_equal(got, eng.drag_force_of(Q, sig, target, region))  # fixed-order sums: the same bits
                if region is three:
                    assert not got[2].any() and got[[0, 1, 3]].all()
                if region is c["region"]:
                    assert np.all(np.any(got != 0.0, axis=1))  # all four regions used
            # the sum over the regions is the integral of what the hook returns
            total = ref.integral_blockwise(k, c["areas"], eng.apply_drag(Q, sig, target))
            assert np.max(np.abs(got[:, :2].sum(axis=0) - total)) <= HOOK * np.max(np.abs(want)), (got, total)
    assert not eng.drag().any()
    print(f"{kind} nx={nx} k={k}: largest |F - reference| = {worst:.3e} max|F|")


# ---- 3. whole steps against the reference loop
def _initial(kind, d):
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
_target = lambda x, y: (0.5 + 0.3 * np.sin(2.0 * x), -0.2 + 0.4 * np.cos(y + x))

CONFIGS = {
    "ssp2-k1": ("ssp2", "square", 1, 6, {}), "ssp2-k2": ("ssp2", "square", 2, 4, {}), "ars2-k2": ("ars2", "square", 2, 4, {}),
    "ssp2-unsplit-k1": ("ssp2", "square", 1, 6, {"use_projection_method": False}),
    "implicit-k1": ("implicit", "square", 1, 6, {}), "dg-k1": ("dg", "square", 1, 6, {}),
    "ssp2-periodic-k1": ("ssp2", "periodic", 1, 6, {}), "ssp2-disk-k2": ("ssp2", "disk", 2, 1, {}),
}
RUNS = [(name, fused) for name in ("ssp2-k1", "ssp2-k2") for fused in (True, False)] + [(name, True) for name in CONFIGS if name not in ("ssp2-k1", "ssp2-k2")]
_WANT = {}


def _reference_runs(key, which, d, Ab, dt, nsteps, Q0, p0, of, kw):
    """(with drag, without): once per configuration, shared by the fused and the per-solve run; read-only"""
    from oracle import hdg_oracle as orc

    if key in _WANT:
        return _WANT[key]
    out = []
    for v in (1.0, 0.0):
        if which == "dg":
            r = ref.dg_with_viscosity(d, Ab, v, dt, Q0, p0, of, nsteps)
        elif which == "implicit":
            r = ref.implicit_with_viscosity(d, Ab, v, dt, Q0, p0, of, nsteps * dt)
        else:
            o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which],
                                  use_projection_method=kw.get("use_projection_method", True))
            r = ref.imex_with_viscosity(o, Ab, v, Q0, p0, of, nsteps * dt)
        r = tuple(np.array(x) for x in r)
        for x in r:
            x.setflags(write=False)
        out.append(r)
    _WANT[key] = out
    return out


@pytest.mark.parametrize("name,fused", RUNS)
def test_whole_steps_against_the_reference_loop(hip_lib, name, fused):
    which, kind, k, nx, kw = CONFIGS[name]
    mesh = _mesh(kind, nx)
    d = _oracle(kind, nx, k, mesh)
    nsteps = 3
    dt = 0.02 if kind == "disk" else 0.25 * d.mesh.h
    sig = _setting(d.mesh.cell_vertices, np.random.default_rng(7), NUMBER / dt, most_zero=False)
    ts = _stepper(which, mesh, k, dt, drag=sig, drag_target=_target, **kw)
    assert np.max(np.abs(ts._engine.cell_vertices() - d.mesh.cell_vertices)) < 1e-12
    assert ts._engine.drag_number()[1] == pytest.approx(NUMBER, rel=1e-12)
    Q0, p0 = _initial(kind, d)
    of = lambda t: d.interpolate_velocity(_forcing(t))
    Ab = ref.affine(d, sig, d.interpolate_velocity(_target))
    (oQ, op), (pQ, pp) = _reference_runs(name, which, d, Ab, dt, nsteps, Q0, p0, of, kw)
    Q, p = ts.solve(Q0, p0, None, _forcing, nsteps * dt, **({"fused": fused} if which in ("ssp2", "ars2") else {}))
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"{name} fused={fused}: with / without drag differ by {seen:.3e} max|Q|; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert seen >= 1e-2, "the comparison shows nothing: the reference does not see the drag"
    assert max(errs) < TOL, errs


def test_forcing_buoyant_diffusing_tracer_viscosity_rotation_and_drag_together(hip_lib):
    """all three velocity-linear terms on: k_viscosity writes a slot, k_coriolis and then k_drag (with a target) add to it"""
    import coriolis_reference as cref
    import tracer_diffusion_reference as tdref
    from oracle import hdg_oracle as orc
    from oracle.tracer_oracle import TracerOracle

    which, kind, k, nx, kw = CONFIGS["ssp2-k1"]
    mesh = _mesh(kind, nx)
    d = _oracle(kind, nx, k, mesh)
    nsteps, dt, wall, bbeta, g = 3, 0.25 * d.mesh.h, "no_slip", 2.0, (0.3, -1.0)
    f0, beta = -0.3 / dt, 0.6 / dt
    sig = _setting(d.mesh.cell_vertices, np.random.default_rng(7), NUMBER / dt, most_zero=False)
    ts = _stepper(which, mesh, k, dt, buoyancy=bbeta, gravity=g, coriolis=(f0, beta), drag=sig, drag_target=_target)
    eng = ts._engine
    eng.set_viscosity(1.0, wall)
    nu = 0.35 / (dt * eng.viscosity_number()[0])
    eng.set_viscosity(nu, wall)
    kappa = 0.35 / (dt * eng.tracer_diffusion_number()[0])
    eng.set_tracer_diffusivity(kappa)
    assert eng.step_rates()[2] == pytest.approx(nu * eng.viscosity_number()[0] + NUMBER / dt, rel=1e-14)
    Q0, p0 = _initial(kind, d)
    q0 = lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y) + 0.5 * np.cos(5 * x) * y
    of = lambda t: d.interpolate_velocity(_forcing(t))
    base = nu * vref.minv_v(d, wall) + cref.minv_c(d, f0, beta)
    runs = []
    for B in (ref.affine(d, sig, d.interpolate_velocity(_target), base=base), base):
        o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
        runs.append(ref.imex_with_viscosity(o, B, 1.0, Q0, p0, of, nsteps * dt, tr=TracerOracle(d), q0=d.interpolate_pressure(q0),
                                            beta=bbeta, g=g, kappa=kappa, Adiff=tdref.minv_d(d)))
    (oQ, op, oq), (pQ, pp, _) = runs
    Q, p = ts.solve(Q0, p0, q0, _forcing, nsteps * dt, fused=True)
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op), _rel(ts.q_tracer.dat.data, oq)
    print(f"forcing + buoyancy + tracer diffusion + viscosity + rotation + drag: with / without drag differ by {seen:.3e} max|Q|; "
          f"Q {errs[0]:.3e}, p {errs[1]:.3e}, q {errs[2]:.3e}")
    assert seen >= 1e-2
    assert max(errs) < TOL, errs


# ---- 4. the manufactured dragged Taylor-Green solution
@pytest.mark.parametrize("k,nx", [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_manufactured_dragged_taylor_green_error_equals_the_reference(hip_lib, k, nx):
    from incompressibleeulerhdg_amd.model_problems import DraggedTaylorGreen

    mesh = _mesh("square", nx)
    d = _oracle("square", nx, k, mesh)
    nsteps, dt, kappa = 3, 0.25 * d.mesh.h, 0.5
    S = NUMBER / dt
    sigma = lambda x, y: S * (0.2 + 0.5 * x + 0.3 * y)  # linear over the square, S at (1, 1)
    ts = _stepper("implicit", mesh, k, dt, drag=sigma)
    assert ts._engine.drag_number()[1] == pytest.approx(NUMBER, rel=1e-12)
    mp = DraggedTaylorGreen(ts._V_Q, ts._V_p, "exponential", kappa, drag=sigma)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt)
    omp = ref.DraggedTaylorGreen(d, sigma, kappa)
    V = d.mesh.cell_vertices
    oQ, op = ref.implicit_with_viscosity(d, ref.affine(d, sigma(V[..., 0], V[..., 1])), 1.0, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    amp = np.exp(-kappa * nsteps * dt)
    e_dev, e_ref = ref.l2_error_velocity(d, Q.dat.data, amp), ref.l2_error_velocity(d, oQ, amp)
    print(f"k={k} nx={nx}: S {S:.4g}; L2 error device {e_dev:.10e}, reference {e_ref:.10e}; fields differ by {_rel(Q.dat.data, oQ):.3e}")
    assert abs(e_dev - e_ref) <= 1e-6 * e_ref


# ---- 5. off is off; 6. on, the launches it adds
def _three_steps(mode, nu=0.0, f0=0.0):
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
    if f0:
        eng.set_coriolis(f0, -2.0)
    rates = eng.step_rates()
    sig = np.random.default_rng(2).uniform(0.0, 3.0, (eng.n_cells, 3))
    if mode == "zero":
        eng.set_drag(np.zeros((eng.n_cells, 3)), lambda x, y: (1.0 + x, y))
    elif mode == "on_then_zero":
        eng.set_drag(sig, lambda x, y: (1.0 + x, y), np.ones(eng.n_cells, dtype=int))
        assert eng.step_rates()[2] == rates[2] + sig.max() and np.array_equal(eng.step_rates()[[0, 1, 3]], rates[[0, 1, 3]])
        eng.set_drag(None)
    elif mode == "on":
        eng.set_drag(sig, lambda x, y: (1.0 + x, y))
    elif mode == "on_faintly":
        eng.set_drag(1e-16 * sig, lambda x, y: (1.0 + x, y))
    if mode in ("unset", "zero", "on_then_zero"):
        assert np.array_equal(eng.step_rates(), rates)
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
    assert r["blob"] == base["blob"] and b"drag" not in r["blob"], what


def test_switched_off_nothing_changes_and_switched_on_the_launches_it_adds(hip_lib):
    base = _three_steps("unset")
    for mode in ("zero", "on_then_zero"):
        _same(_three_steps(mode), base, mode)
    # viscosity and rotation on, drag off: bitwise that run
    vbase = _three_steps("unset", nu=1e-3, f0=1.5)
    for mode in ("zero", "on_then_zero"):
        _same(_three_steps(mode, nu=1e-3, f0=1.5), vbase, "viscous rotating " + mode)
    # switched on, with values too faint to move an iteration count (asserted)
    faint = _three_steps("on_faintly")
    assert all(np.array_equal(a, b) for a, b in zip(faint["its"], base["its"]))
    more = {c: faint["census"][c] - base["census"][c] for c in base["census"] if faint["census"][c] != base["census"][c]}
    print(f"drag alone: launches per step beyond the plain run: {more}")
    # s + 1 = 4 launches of k_drag per SSP2(3,3,2) step; the sum in front of the pressure reconstruction; as sections 21, 22
    assert more == {"other": 4, "vector_update": 1}, more
    assert b"drag_sigma_d0" in faint["blob"] and b"drag_target_d1" in faint["blob"] and b"drag_region_d0" in faint["blob"]
    for nu, f0 in ((1e-3, 0.0), (0.0, 1.5), (1e-3, 1.5)):
        vb = vbase if nu and f0 else _three_steps("unset", nu=nu, f0=f0)
        vfaint = _three_steps("on_faintly", nu=nu, f0=f0)
        assert all(np.array_equal(a, b) for a, b in zip(vfaint["its"], vb["its"]))
        more = {c: vfaint["census"][c] - vb["census"][c] for c in vb["census"] if vfaint["census"][c] != vb["census"][c]}
        print(f"drag beside nu = {nu}, f0 = {f0}: launches per step beyond that run: {more}")
        assert more == {"other": 4}, more  # the accumulating launches; the slot vectors and every sum are already there
    assert _rel(_three_steps("on")["Q"], base["Q"]) > 1e-3


# ---- 7. strips: two ranks over shared memory against one rank
def _ranks(nranks, kind, tmp_path):
    token = "/hdg_drag_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"{kind}{nranks}_{r}.npz") for r in range(nranks)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "drag_strip_worker.py"), str(r), str(nranks), token, kind, outs[r]],
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
    ferr = _rel(parts[0]["force"], single["force"])
    print(f"{kind}: two strips against one rank: Q {errs[0]:.3e}, p {errs[1]:.3e}, force {ferr:.3e}; S dt {float(single['number']):.4g}")
    assert np.array_equal(parts[0]["force"], parts[1]["force"]) and np.all(np.any(single["force"] != 0.0, axis=1))
    assert all(float(d["number"]) == pytest.approx(NUMBER, rel=1e-12) for d in parts + [single])
    assert np.array_equal(np.concatenate([d["sigma"] for d in parts]), single["sigma"])
    assert max(errs) < TOL, errs
    assert ferr <= HOOK, ferr


# ---- 8. checkpoint
_CK_SIG = lambda e, scale=1.0: scale * np.random.default_rng(2).uniform(0.0, 3.0, (e.n_cells, 3))
_CK_TGT = lambda x, y: (1.0 + x, y)


def _ck_engine(setting):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    if setting is not None:
        eng.set_drag(*setting(eng))
    return ts, eng


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_the_setting(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    setting = lambda e: (_CK_SIG(e), _CK_TGT)
    ts, eng = _ck_engine(setting)
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"drag_sigma_d0" in blob and b"drag_target_d0" in blob and b"drag_region_d1" in blob
    for n in range(2):
        eng.step()
    ts2, eng2 = _ck_engine(setting)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    others = (lambda e: (_CK_SIG(e, 1.5), _CK_TGT), lambda e: (_CK_SIG(e), lambda x, y: (1.0 + x, 2.0 * y)), lambda e: (_CK_SIG(e), None),
              lambda e: (_CK_SIG(e), _CK_TGT, np.ones(e.n_cells, dtype=int)), lambda e: (np.zeros((e.n_cells, 3)), _CK_TGT), None)
    for other in others:
        _, eng3 = _ck_engine(other)
        with pytest.raises(_lib.HDGError, match="drag|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1


# ---- 9. errors
def test_errors(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    eng = ts._engine
    rng = np.random.default_rng(3)
    eng.set_state(rng.standard_normal(eng.shape_Q), rng.standard_normal(eng.shape_p))
    sig = rng.uniform(0.0, 2.0, (eng.n_cells, 3))
    tgt = rng.standard_normal(eng.shape_Q)
    reg = rng.integers(0, 4, eng.n_cells)
    eng.set_drag(sig, tgt, reg)
    eng_Q, eng_p = ts._current()
    force = eng.drag_force()

    def untouched():
        assert np.array_equal(eng.drag(), sig) and eng.drag_number() == (sig.max(), sig.max() * 0.02)  # the setting ...
        assert np.array_equal(eng.drag_force(), force)  # ... its target and tags ...
        Q, p = ts._current()
        assert np.array_equal(Q, eng_Q) and np.array_equal(p, eng_p)  # ... and the fields

    def bad(a, where, value):
        a = a.copy()
        a[where] = value
        return a

    cases = [((bad(sig, (3, 1), -1e-3), tgt, reg), "sigma"), ((bad(sig, (5, 2), np.nan), tgt, reg), "sigma"),
             ((bad(sig, (0, 0), np.inf), tgt, reg), "sigma"), ((sig, bad(tgt, (7, 1), np.nan), reg), "target"),
             ((sig, tgt, bad(reg, 2, 4)), "region"), ((sig, tgt, bad(reg, 9, -1)), "region")]
    for args, word in cases:
        with pytest.raises(_lib.HDGError, match=word) as e:
            eng.set_drag(*args)
        assert e.value.code == -1
        with pytest.raises(_lib.HDGError, match=word):
            eng.drag_force_of(eng_Q, *args)
        if word != "region":
            with pytest.raises(_lib.HDGError, match=word):
                eng.apply_drag(eng_Q, args[0], args[1])
        untouched()
    eng.begin_step()  # while a step is open
    for call in (lambda: eng.set_drag(None), lambda: eng.apply_drag(eng_Q, sig), lambda: eng.drag_force_of(eng_Q, sig), eng.drag_force):
        with pytest.raises(_lib.HDGError, match="a step is open") as e:
            call()
        assert e.value.code == -1
    assert np.array_equal(eng.drag(), sig)


# ---- 10. the adaptive step
def test_adaptive_step_respects_the_drag_cap(hip_lib):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers.common import explicit_stability_limit

    dt = 0.02
    probe = _stepper("ssp2", _mesh("square", 6), 1, dt)
    limit = explicit_stability_limit(probe._a_expl, probe._b_expl)
    probe._engine.set_viscosity(1.0, "free_slip")
    lam = probe._engine.viscosity_number()[0]
    nu = 0.2 * limit / (dt * lam)
    S = 0.65 * limit / dt  # the cap limit / (nu Lambda_u + S) = dt / 0.85: above the held dt, far below what cfl = 5 asks for
    ts = _stepper("ssp2", _mesh("square", 6), 1, dt, viscosity=nu, drag=S)
    rate = ts._engine.step_rates()[2]
    assert rate == pytest.approx(nu * lam + S, rel=1e-14)
    cap = limit / rate
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 0.2, fused=True, cfl=5.0, dt_max=1.0)
    sizes, dec = ts.step_sizes, ts.step_decisions
    print(f"drag cap {cap!r} (dt / 0.85 = {dt / 0.85!r}); first proposal {dec[0, 3]!r}; {len(sizes)} steps, largest dt {sizes[:, 1].max()!r}")
    assert dec[0, 3] == cap and np.all(sizes[:, 1] <= cap) and np.any(sizes[:, 1] == cap)


# ---- 11. the driver
def _driver(args, tmp_path):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver"] + args + ["--output", ""], cwd=tmp_path,
                       capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r


def test_driver_with_the_dragged_taylor_green_vortex(hip_lib, tmp_path):
    nx, k, dt, nsteps = 8, 1, 1e-3, 3
    r = _driver(["--problem", "taylorgreen", "--nx", str(nx), "--degree", str(k), "--dt", repr(dt), "--tfinal", repr(nsteps * dt),
                 "--timestepper", "implicit", "--use_projection_method", "--drag", "2"], tmp_path)
    assert "drag = 2.0" in r.stdout
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("drag: S = ")]
    assert len(line) == 1 and line[0] == "drag: S = 2, S dt = 0.002", r.stdout
    err = float([ln for ln in r.stdout.splitlines() if ln.startswith("velocity error = ")][0].split("=")[1])
    d = _oracle("square", nx, k, None)
    omp = ref.DraggedTaylorGreen(d, lambda x, y: 2.0 + 0.0 * x, 0.5)
    oQ, _ = ref.implicit_with_viscosity(d, ref.affine(d, np.full((d.mesh.ncells, 3), 2.0)), 1.0, dt, *omp.initial_condition(), omp.f_rhs, nsteps * dt)
    want = d.l2_norm_velocity(oQ - omp.solution(nsteps * dt)[0])
    print(f"driver: velocity error {err!r}, reference {want!r}")
    assert err == pytest.approx(want, rel=1e-6)


def test_driver_with_the_cylinder_wake(hip_lib, tmp_path):
    """the driver's run is the in-process run of the same stepper bit for bit (state digest), and that run is the reference loop's"""
    from incompressibleeulerhdg_amd.model_problems import CylinderWake
    from oracle import hdg_oracle as orc

    nx, k, dt, nsteps, nu = 16, 1, 0.02, 3, 1e-2
    r = _driver(["--problem", "cylinder", "--nx", str(nx), "--degree", str(k), "--dt", repr(dt), "--tfinal", repr(nsteps * dt),
                 "--timestepper", "imex_ssp2_332", "--use_projection_method", "--fused", "--viscosity", repr(nu)], tmp_path)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("drag: S = ")]
    assert len(line) == 1, r.stdout
    S = float([ln for ln in r.stdout.splitlines() if ln.startswith("obstacle drag = ")][0].split("=")[1])
    rows = [ln for ln in r.stdout.splitlines() if ln.startswith("disc: ")]
    assert len(rows) == 1, r.stdout
    cd, cl = float(rows[0].split("C_D =")[1].split(",")[0]), float(rows[0].split("C_L =")[1])
    assert np.isfinite(cd) and np.isfinite(cl) and cd > 0.0
    digest = [ln for ln in r.stdout.splitlines() if ln.startswith("state digest = ")][0].split("=")[1].strip()
    mesh = _mesh("periodic", nx)
    ts = _stepper("ssp2", mesh, k, dt, viscosity=nu, wall="free_slip")
    limit = ts.viscosity_limit
    assert S == pytest.approx((0.5 * limit - ts._engine.viscosity_number()[1]) / dt, rel=1e-12)  # the combined number at half the limit
    mp = CylinderWake(ts._V_Q, ts._V_p, L_PER, L_PER / nx, S)
    ts.set_drag(mp.sigma, mp.target, mp.region)
    assert ts._engine.viscosity_number()[1] + ts._engine.drag_number()[1] == pytest.approx(0.5 * limit, rel=1e-6)
    Q, p = ts.solve(*mp.initial_condition(), None, None, nsteps * dt, fused=True)
    mine = ts._engine.state_digest()
    assert f"{mine[0]:016x}{mine[1]:016x}" == digest
    force = ts._engine.drag_force()
    assert mp.coefficients(force[1])[0] == cd and np.all(force[3] == 0.0) and force[1].any() and force[2].any()
    d = orc.HDGDiscretisation(nx, k, periodic=True, L=L_PER)
    V = d.mesh.cell_vertices
    sig = mp.sigma(V[..., 0], V[..., 1])
    assert np.max(np.abs(ts._engine.drag() - sig)) <= 1e-12 * S
    Ab = ref.affine(d, ts._engine.drag(), d.interpolate_velocity(mp.target), base=nu * vref.minv_v(d, "free_slip"))
    o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
    oQ, op = ref.imex_with_viscosity(o, Ab, 1.0, d.interpolate_velocity(mp.Q_initial), d.interpolate_pressure(mp.p_initial),
                                     lambda t: np.zeros((d.NQ // 2, 2)), nsteps * dt)
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"wake: S {S:.6g}, C_D {cd:.6g}, C_L {cl:.3e}; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert max(errs) < TOL, errs
