"""Moving no-slip walls and the viscous wall force on the GPU (include/hdg_moving_walls.h) against
tests/moving_walls_reference.py.

Bounds.  The two hooks and the force budget: relative 1e-10, section 21's bound for its operator hook (table and conversion
rounding against entries of size Lambda_u).  Whole steps, strips: 2e-8, the project's whole-step bound, for Q and p.  Switched
off, everything is bitwise what a viscous engine computes that never heard of the feature.

Larger meshes (several waves, workgroups and XCD row bands; row padding): tests/test_gpu_stencil_sizes.py runs the hooks there."""
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

import moving_walls_reference as ref
import viscosity_reference as vref

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HOOK, TOL = 1e-10, 2e-8
NUMBER = 0.35  # nu dt Lambda_u of the whole-step runs
SPEEDS = (0.3, -0.7, 1.0, 0.45)
_REF = {}


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _reference(nx, k):
    """(package mesh, discretisation, M^-1 V no slip, M^-1 of the four unit loads, force functionals no slip / free slip) of the
    unit square: once per mesh and degree; read-only"""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from oracle import hdg_oracle as orc

    if (nx, k) not in _REF:
        d = orc.HDGDiscretisation(nx, k)
        A = vref.minv_v(d, "no_slip")
        Mi = np.linalg.solve(d.MQ.toarray(), ref.unit_loads(d).T).T
        fun = {w: ref.force_functionals(d, w) for w in vref.WALLS}
        for a in [A, Mi] + [x for f in fun.values() for x in f]:
            a.setflags(write=False)
        _REF[nx, k] = (d, A, Mi, fun)
    return (UnitSquareMesh(nx, nx),) + _REF[nx, k]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "ars2": tsm.IncompressibleEulerHDGIMEXARS2_232,
           "implicit": tsm.IncompressibleEulerHDGImplicit, "dg": tsm.IncompressibleEulerDGImplicit}[which]
    if which != "dg":
        kw.setdefault("use_projection_method", True)
        kw.update(n_richardson=2)
    return cls(mesh, k, dt, **kw)


def _set_number(eng, dt, number=NUMBER):
    """nu such that the reported viscous diffusion number nu dt Lambda_u is `number`, no-slip walls"""
    eng.set_viscosity(1.0, "no_slip")
    nu = number / (dt * eng.viscosity_number()[0])
    eng.set_viscosity(nu, "no_slip")
    assert eng.viscosity_number()[1] == pytest.approx(number, rel=1e-12)
    return nu


def _fields(d, k):
    X = d.node_coords(d.PU).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    rng = np.random.default_rng(31 + k)
    smooth = lambda: sum(rng.uniform(-1, 1) * np.sin(2 * np.pi * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))
    return {"smooth": np.stack([smooth(), smooth()], axis=-1), "broken": rng.standard_normal((len(x), 2))}


# ---- 1. the hook against the reference
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_hook_against_the_reference(hip_lib, k):
    mesh, d, A, Mi, _ = _reference(3, k)
    Ab = ref.affine(d, SPEEDS, A, Minv_loads=Mi)
    eng = _stepper("ssp2", mesh, k, 0.01)._engine
    for name, Q in _fields(d, k).items():
        want = (Ab @ Q.ravel()).reshape(-1, 2)
        got = eng.apply_moving_walls(Q, SPEEDS)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        load = np.max(np.abs(got - eng.apply_viscosity(Q, "no_slip"))) / np.max(np.abs(want))
        print(f"k={k} {name}: |out - reference| = {err:.3e} max|out|; the load is {load:.3e} of it")
        assert err <= HOOK, (name, err)
        assert load > 1e-3  # the load is no rounding matter
        # a dict names the sides
        assert np.array_equal(eng.apply_moving_walls(Q, dict(zip(ref.SIDES, SPEEDS))), got)
    assert eng.viscosity() == (0.0, "free_slip") and not eng.wall_velocity().any()  # the hook sets nothing
    eng.close()


# ---- 2. the linear shear, without a reference
SHEARS = {"top": lambda x, y: (y, 0 * y), "bottom": lambda x, y: (1 - y, 0 * y), "right": lambda x, y: (0 * x, x), "left": lambda x, y: (0 * x, 1 - x)}


@pytest.mark.parametrize("nx,k", [(3, 1), (3, 2), (3, 3), (3, 4), (80, 1), (80, 2)])
def test_linear_shear_is_annihilated(hip_lib, nx, k):
    """u linear between a wall moving at speed 1 and the resting wall opposite: M^-1 (V u + l) vanishes away from the two
    other walls.  At nx = 80 a row of cells is more than a wave: whole waves hold no wall cell, others mix wall and interior lanes"""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    eng = _stepper("ssp2", UnitSquareMesh(nx, nx), k, 0.01)._engine
    xq = eng.node_coordinates()[0].reshape(-1, 2)
    n_u = (k + 2) * (k + 3) // 2
    cx = xq.reshape(-1, n_u, 2)
    for side, u in SHEARS.items():
        Q = np.stack(u(xq[:, 0], xq[:, 1]), axis=-1)
        ax = 0 if side in ("top", "bottom") else 1
        keep = (cx[:, :, ax].min(axis=1) > 1e-9) & (cx[:, :, ax].max(axis=1) < 1 - 1e-9)
        assert keep.any() and not keep.all()
        out = eng.apply_moving_walls(Q, {side: 1.0}).reshape(-1, n_u, 2)
        plain = eng.apply_viscosity(Q, "no_slip").reshape(-1, n_u, 2)
        scale = np.max(np.abs(plain))
        err = np.max(np.abs(out[keep])) / scale
        print(f"nx={nx} k={k} {side}: |M^-1 (V u + l)| = {err:.3e} max|M^-1 V u| ({scale:.3e})")
        assert np.max(np.abs(plain[keep])) > 0.1 * scale  # without the load the wall cells see the whole mismatch
        assert err <= HOOK, (side, err)
    eng.close()


# ---- 3. all speeds zero: bitwise the plain hook
def test_all_speeds_zero_is_the_viscous_hook_bit_for_bit(hip_lib):
    mesh, d, _, _, _ = _reference(3, 2)
    eng = _stepper("ssp2", mesh, 2, 0.01)._engine
    for Q in _fields(d, 2).values():
        for wall in vref.WALLS:
            plain = eng.apply_viscosity(Q, wall)
            for U in ((0.0, 0.0, 0.0, 0.0), {}, None, (-0.0, 0.0, 0.0, 0.0)):
                assert np.array_equal(eng.apply_moving_walls(Q, U, wall), plain), (wall, U)
    eng.close()


# ---- 4. the force hook
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_force_hook_against_the_reference_and_the_budget(hip_lib, k):
    mesh, d, A, Mi, fun = _reference(3, k)
    eng = _stepper("ssp2", mesh, k, 0.01)._engine
    for name, Q in _fields(d, k).items():
        for wall, U in (("no_slip", SPEEDS), ("free_slip", (0.0, 0.0, 0.0, 0.0))):
            want = ref.wall_force(d, 1.0, U, Q, wall, fun[wall])
            got = eng.wall_force_of(Q, U, wall)
            assert got.shape == (4, 2)
            err = _rel(got, want)
            # the budget on the device: the sum over the sides against the integral of the hook's output
            out = eng.apply_moving_walls(Q, U, wall)
            total = ref.integral(d, out)
            budget = np.max(np.abs(got.sum(axis=0) - total)) / np.max(np.abs(got))
            print(f"k={k} {name} {wall}: force {err:.3e}, budget {budget:.3e} (sum {got.sum(axis=0)}, integral {total})")
            assert err <= HOOK and budget <= HOOK
            assert np.array_equal(eng.wall_force_of(Q, U, wall), got)  # two calls: the same bits
            if wall == "free_slip":  # the normal part only
                assert np.all(got[[0, 2], 0] == 0.0) and np.all(got[[1, 3], 1] == 0.0)
    eng.close()


def test_force_on_a_mesh_of_several_blocks(hip_lib):
    """nx = 150: two workgroups per side, the second one partly filled; the force of the linear shear under a lid is the
    shear stress du/dy = 1 over the lid and the bottom, and the budget closes"""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    nx, k = 150, 1
    eng = _stepper("ssp2", UnitSquareMesh(nx, nx), k, 0.01)._engine
    xq = eng.node_coordinates()[0].reshape(-1, 2)
    Q = np.stack([xq[:, 1], 0 * xq[:, 1]], axis=-1)
    F = eng.wall_force_of(Q, {"top": 1.0})
    print(f"nx={nx}: F = {F.tolist()}")
    # the lid drags the fluid along (+1), the resting bottom holds it back (-1); left and right: u.n = y is not zero there
    assert F[2, 0] == pytest.approx(1.0, rel=1e-10) and F[0, 0] == pytest.approx(-1.0, rel=1e-10)
    assert abs(F[2, 1]) <= 1e-10 and abs(F[0, 1]) <= 1e-10
    assert np.array_equal(eng.wall_force_of(Q, {"top": 1.0}), F)
    eng.close()


# ---- 5. three whole steps against the reference loop
def _initial(start, d):
    """'rest': every bit of velocity is the walls' doing; 'broken': section 21's start, the Taylor-Green field with a broken
    random part"""
    from oracle import hdg_oracle as orc

    if start == "rest":
        return np.zeros((d.NQ // 2, 2)), np.zeros(d.NP)
    Q0, p0 = orc.TaylorGreen(d).initial_condition()
    return Q0 + 0.4 * np.random.default_rng(5).standard_normal(Q0.shape), p0


CONFIGS = {
    "ssp2-k1": ("ssp2", 1, 6, {}), "ssp2-k2": ("ssp2", 2, 4, {}), "ars2-k2": ("ars2", 2, 4, {}),
    "ssp2-unsplit-k1": ("ssp2", 1, 6, {"use_projection_method": False}),
    "implicit-k1": ("implicit", 1, 6, {}), "dg-k1": ("dg", 1, 6, {}),
    "ssp2-coriolis-k1": ("ssp2", 1, 6, {"coriolis": (2.0, 1.5)}),
}
RUNS = ([(name, fused, start) for name in ("ssp2-k1", "ssp2-k2") for fused in (True, False) for start in ("rest", "broken")] +
        [(name, True, start) for name in CONFIGS if name not in ("ssp2-k1", "ssp2-k2") for start in ("rest", "broken")])
_WANT = {}
_FORCING = lambda t: (lambda x, y: (0.4 * np.cos(2.0 * y) * np.cos(t) + 0.1 * x, 0.3 * np.sin(x + y) * (1.0 + t)))


def _reference_runs(key, which, d, A, Mi, nu, dt, nsteps, Q0, p0, of, kw):
    """(with the speeds, without): once per configuration and start, shared by the fused and the per-solve run; read-only"""
    import coriolis_reference as cref
    from oracle import hdg_oracle as orc

    if key in _WANT:
        return _WANT[key]
    out = []
    for U in (SPEEDS, (0.0, 0.0, 0.0, 0.0)):
        Ab = ref.affine(d, U, A, Minv_loads=Mi)
        v = nu
        if "coriolis" in kw:  # the slot vector is shared: nu (A Q + b) + M^-1 C Q
            Ab, v = ref.Affine(nu * Ab.A + cref.minv_c(d, *kw["coriolis"]), nu * Ab.b), 1.0
        if which == "dg":
            r = ref.dg_with_moving_walls(d, Ab, v, dt, Q0, p0, of, nsteps)
        elif which == "implicit":
            r = ref.implicit_with_moving_walls(d, Ab, v, dt, Q0, p0, of, nsteps * dt)
        else:
            o = orc.OracleHDGIMEX(d, dt, {"ssp2": "imex_ssp2_332", "ars2": "imex_ars2_232"}[which],
                                  use_projection_method=kw.get("use_projection_method", True))
            r = ref.imex_with_moving_walls(o, Ab, v, Q0, p0, of, nsteps * dt)
        r = tuple(np.array(x) for x in r)
        for x in r:
            x.setflags(write=False)
        out.append(r)
    _WANT[key] = out
    return out


@pytest.mark.parametrize("name,fused,start", RUNS)
def test_whole_steps_against_the_reference_loop(hip_lib, name, fused, start):
    import warnings

    which, k, nx, kw = CONFIGS[name]
    mesh, d, A, Mi, _ = _reference(nx, k)
    nsteps, dt = 3, 0.25 * d.mesh.h
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)  # the rotation number of the coriolis case is not this test's matter
        ts = _stepper(which, mesh, k, dt, **kw)
    eng = ts._engine
    nu = _set_number(eng, dt)
    eng.set_wall_velocity(SPEEDS)
    assert np.array_equal(eng.wall_velocity(), SPEEDS)
    Q0, p0 = _initial(start, d)
    f = None if start == "rest" else _FORCING
    of = (lambda t: np.zeros_like(Q0)) if start == "rest" else (lambda t: d.interpolate_velocity(_FORCING(t)))
    (oQ, op), (pQ, _) = _reference_runs((name, start), which, d, A, Mi, nu, dt, nsteps, Q0, p0, of, kw)
    Q, p = ts.solve(Q0, p0, None, f, nsteps * dt, **({"fused": fused} if which in ("ssp2", "ars2") else {}))
    seen = np.max(np.abs(oQ - pQ)) / np.max(np.abs(oQ))
    errs = _rel(Q.dat.data, oQ), _rel(p.dat.data, op)
    print(f"{name} fused={fused} {start}: nu {nu:.4e}; with / without U differ by {seen:.3e} max|Q|; Q {errs[0]:.3e}, p {errs[1]:.3e}")
    assert seen >= 1e-2, "the comparison shows nothing: the reference does not see the walls move"
    assert max(errs) < TOL, errs
    # the force of the final state, with the nu, wall mode and speeds that are set
    want = ref.wall_force(d, nu, SPEEDS, oQ)
    G, _ = ref.force_functionals(d)
    slack = nu * np.max(np.abs(G).sum(axis=-1)) * TOL * np.max(np.abs(oQ))  # the functional applied to a field within TOL
    assert np.max(np.abs(eng.wall_force() - want)) <= slack + HOOK * np.max(np.abs(want))
    eng.close()


# ---- 6. spin-up under a lid
def _spin_up_reference(d, A, Mi, nu, dt, nsteps):
    from oracle import hdg_oracle as orc

    Ab = ref.affine(d, {"top": 1.0}, A, Minv_loads=Mi)
    ke, fx = [], []

    def mon(n, Q, p):
        ke.append(vref.kinetic_energy(d, Q))
        fx.append(ref.wall_force(d, nu, {"top": 1.0}, Q)[2, 0])

    zero = np.zeros((d.NQ // 2, 2))
    ref.imex_with_moving_walls(orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), Ab, nu, zero, np.zeros(d.NP), lambda t: zero, nsteps * dt, monitor=mon)
    return np.array(ke), np.array(fx)


def test_spin_up_under_a_lid(hip_lib):
    """from rest with U_top = 1: kinetic energy rises in every step, the drag of the lid is positive and falls as the fluid
    under it picks up speed -- on the reference first, then on the device"""
    mesh, d, A, Mi, _ = _reference(4, 2)
    dt, nsteps = 0.25 * d.mesh.h, 6
    ts = _stepper("ssp2", mesh, 2, dt)
    eng = ts._engine
    nu = _set_number(eng, dt)
    rke, rfx = _spin_up_reference(d, A, Mi, nu, dt, nsteps)
    print("reference: KE " + " ".join(f"{x:.6e}" for x in rke) + "; F_top.e_x " + " ".join(f"{x:.6e}" for x in rfx))
    assert rke[0] > 0.0 and np.all(np.diff(rke) > 0.0) and np.all(rfx > 0.0) and np.all(np.diff(rfx) < 0.0)
    eng.set_wall_velocity({"top": 1.0})
    eng.set_state(np.zeros(eng.shape_Q), np.zeros(eng.shape_p))
    eng.reconstruct_trace()
    for slot in range(eng.nstages + 1):
        eng.set_forcing_scale(slot, 0.0)
    F0 = eng.wall_force()
    # at rest the lid's drag is nu U int_top eta_b, and nothing else acts
    assert F0[2, 0] == pytest.approx(nu * ref.force_functionals(d)[1][2, 0], rel=1e-12) and np.count_nonzero(F0) == 1
    ke, fx = [0.0], [F0[2, 0]]
    for n in range(nsteps):
        eng.step()
        ke.append(eng.compute_diagnostics(*ts._current())[0])
        fx.append(eng.wall_force()[2, 0])
    print("device:    KE " + " ".join(f"{x:.6e}" for x in ke[1:]) + "; F_top.e_x " + " ".join(f"{x:.6e}" for x in fx[1:]))
    assert np.all(np.diff(ke) > 0.0) and np.all(np.array(fx) > 0.0) and np.all(np.diff(fx) < 0.0)
    assert _rel(ke[1:], rke) < 1e-6 and _rel(fx[1:], rfx) < 1e-6
    eng.close()


# ---- 7. off is off; on, no launch more
def _three_steps(mode, nu=1e-3):
    """Fields, iteration counts, digest, checkpoint blob and the launch census of the third of three fused steps of a viscous
    engine with no-slip walls."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_viscosity(nu, "no_slip")
    if mode == "zeros":
        eng.set_wall_velocity((0.0, 0.0, 0.0, 0.0))
    elif mode == "on_then_none":
        eng.set_wall_velocity(SPEEDS)
        eng.set_wall_velocity(None)
    elif mode == "on_then_zeros":
        eng.set_wall_velocity(SPEEDS)
        eng.set_wall_velocity({})
    elif mode == "on":
        eng.set_wall_velocity(SPEEDS)
    elif mode == "on_faintly":
        eng.set_wall_velocity({"top": 1e-16, "left": -1e-16})
    for n in range(3):
        eng.launch_stats(reset=True)
        eng.step()
    census = {c: v[0] for c, v in eng.launch_stats(reset=True).items()}
    Q, p = ts._current()
    r = dict(census=census, Q=Q, p=p, its=eng.iteration_stats(), digest=eng.state_digest(), blob=bytes(eng.save_checkpoint(3, 0.06)))
    eng.launch_stats(reset=True)
    eng.wall_force()
    r["force_census"] = {c: v[0] for c, v in eng.launch_stats(reset=True).items() if v[0]}
    eng.close()
    return r


def test_switched_off_nothing_changes_and_switched_on_nothing_is_launched_more(hip_lib):
    base = _three_steps("unset")
    for mode in ("zeros", "on_then_none", "on_then_zeros"):
        r = _three_steps(mode)
        assert r["census"] == base["census"], mode
        for name in ("Q", "p"):
            assert np.array_equal(r[name], base[name]), (mode, name)
        assert all(np.array_equal(a, b) for a, b in zip(r["its"], base["its"])), mode
        assert r["digest"] == base["digest"], mode
        assert r["blob"] == base["blob"] and b"wall_velocity" not in r["blob"], mode
    # switched on.  The solver classes of the census follow the iteration counts, and those follow the flow: the census is read
    # off a run whose speeds are too faint to move an iteration count (asserted)
    faint = _three_steps("on_faintly")
    assert all(np.array_equal(a, b) for a, b in zip(faint["its"], base["its"]))
    assert faint["census"] == base["census"]  # k_viscosity<K, true> runs instead of the plain kernel: no launch more
    assert b"wall_velocity[2]" in faint["blob"] and b"wall_velocity[3]" in faint["blob"]
    assert b"wall_velocity[0]" not in faint["blob"] and b"wall_velocity[1]" not in faint["blob"]
    assert _rel(_three_steps("on")["Q"], base["Q"]) > 1e-3
    assert base["force_census"] == {"other": 2}  # the force: its two launches, tallied in 'other'


# ---- 8. strips: two ranks over shared memory against one rank
def _ranks(nranks, tmp_path):
    token = "/hdg_mw_" + uuid.uuid4().hex[:12]
    outs = [str(tmp_path / f"mw{nranks}_{r}.npz") for r in range(nranks)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "moving_walls_strip_worker.py"), str(r), str(nranks), token, outs[r]],
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


def test_two_strips_match_one_rank(hip_lib, tmp_path):
    parts = _ranks(2, tmp_path)
    single = _ranks(1, tmp_path)[0]
    Q, p = np.concatenate([d["Q"] for d in parts]), np.concatenate([d["p"] for d in parts])
    errs = _rel(Q, single["Q"]), _rel(p, single["p"])
    ferr = max(_rel(d["F"], single["F"]) for d in parts)
    print(f"two strips against one rank: Q {errs[0]:.3e}, p {errs[1]:.3e}, wall force {ferr:.3e}; F = {single['F'].tolist()}")
    assert all(float(d["nu"]) == float(single["nu"]) and np.array_equal(d["U"], SPEEDS) for d in parts)
    assert np.array_equal(parts[0]["F"], parts[1]["F"])  # every rank returns the sum over the ranks
    assert np.all(single["F"] != 0.0)
    assert max(errs) < TOL, errs
    assert ferr <= HOOK, ferr


# ---- 9. checkpoint
def _ck_engine(U, nu=1e-3):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    ts = _stepper("ssp2", UnitSquareMesh(5, 5), 2, 0.02)
    eng = ts._engine
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q0, p0 = mp.initial_condition()
    eng.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    eng.reconstruct_trace()
    eng.set_viscosity(nu, "no_slip")
    if U is not None:
        eng.set_wall_velocity(U)
    return ts, eng


def test_checkpoint_carries_on_bit_for_bit_and_is_bound_to_the_speeds(hip_lib):
    from incompressibleeulerhdg_amd import _lib

    U = {"top": 1.0, "right": -0.5}
    ts, eng = _ck_engine(U)
    for n in range(2):
        eng.step()
    blob = eng.save_checkpoint(2, 0.04)
    assert b"wall_velocity[1]" in blob and b"wall_velocity[2]" in blob and b"wall_velocity[0]" not in blob and b"wall_velocity[3]" not in blob
    for n in range(2):
        eng.step()
    ts2, eng2 = _ck_engine(U)
    assert eng2.load_checkpoint(blob) == (2, 0.04)
    for n in range(2):
        eng2.step()
    assert eng2.state_digest() == eng.state_digest()
    for a, b in zip(ts2._current(), ts._current()):
        assert np.array_equal(a, b)
    assert np.array_equal(eng2.wall_force(), eng.wall_force())
    for other in ({"top": 1.0, "right": -0.25}, {"top": 1.0}, {"top": 1.0, "right": -0.5, "left": 0.1}, {}, None):
        _, eng3 = _ck_engine(other)
        with pytest.raises(_lib.HDGError, match="wall_velocity|fingerprint") as e:
            eng3.load_checkpoint(blob)
        assert e.value.code == -1
    # and the other way round: a save without speeds does not load into an engine with speeds
    _, plain = _ck_engine(None)
    with pytest.raises(_lib.HDGError, match="wall_velocity|fingerprint"):
        _ck_engine(U)[1].load_checkpoint(plain.save_checkpoint(0, 0.0))


# ---- 10. errors
def test_errors_leave_the_setting_and_the_fields(hip_lib):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02)
    eng = ts._engine
    rng = np.random.default_rng(3)
    eng.set_state(rng.standard_normal(eng.shape_Q), rng.standard_normal(eng.shape_p))
    eng_Q, eng_p = ts._current()
    zeros = np.zeros(4)

    def untouched(U, visc):
        assert np.array_equal(eng.wall_velocity(), U) and eng.viscosity() == visc  # a refused call leaves the setting ...
        Q, p = ts._current()
        assert np.array_equal(Q, eng_Q) and np.array_equal(p, eng_p)  # ... and the fields

    # a non-zero speed while the wall mode is not no slip: never set, and free slip
    for visc in ((0.0, "free_slip"), (1e-3, "free_slip")):
        eng.set_viscosity(*visc)
        with pytest.raises(_lib.HDGError, match="needs no-slip walls") as e:
            eng.set_wall_velocity({"top": 1.0})
        assert e.value.code == -1
        untouched(zeros, visc)
        eng.set_wall_velocity(zeros)  # zeros are fine in any mode
        with pytest.raises(_lib.HDGError, match="needs no-slip walls"):
            eng.apply_moving_walls(eng_Q, {"top": 1.0}, "free_slip")
        with pytest.raises(_lib.HDGError, match="needs no-slip walls"):
            eng.wall_force_of(eng_Q, {"top": 1.0}, "free_slip")
        untouched(zeros, visc)
    eng.set_viscosity(0.0, "no_slip")  # nu = 0 with speeds set is allowed and has no effect
    eng.set_wall_velocity(SPEEDS)
    assert not eng.wall_force().any()
    visc = (1e-3, "no_slip")
    eng.set_viscosity(*visc)
    good = np.array(SPEEDS)
    untouched(good, visc)
    for w, side in enumerate(ref.SIDES):  # not finite: the side is named
        for x in (float("nan"), float("inf"), -float("inf")):
            with pytest.raises(_lib.HDGError, match=rf"side {w} \({side}\).*not finite") as e:
                eng.set_wall_velocity({side: x})
            assert e.value.code == -1
            untouched(good, visc)
    with pytest.raises(_lib.HDGError, match="not finite"):
        eng.apply_moving_walls(eng_Q, {"left": float("nan")})
    # free slip while a speed is non-zero
    for nu in (1e-3, 0.0):
        with pytest.raises(_lib.HDGError, match="a wall velocity is set") as e:
            eng.set_viscosity(nu, "free_slip")
        assert e.value.code == -1
        untouched(good, visc)
    for bad in (2, -1):
        dp = _lib._dp
        assert eng.lib.hdg_apply_moving_walls(eng.h, bad, good.ctypes.data_as(dp), eng_Q.ctypes.data_as(dp), np.empty(eng.shape_Q).ctypes.data_as(dp)) == -1
        assert eng.lib.hdg_apply_wall_force(eng.h, bad, good.ctypes.data_as(dp), eng_Q.ctypes.data_as(dp), np.empty(8).ctypes.data_as(dp)) == -1
    untouched(good, visc)
    with pytest.raises(ValueError, match="unknown wall side"):
        eng.set_wall_velocity({"lid": 1.0})
    F = eng.wall_force()
    eng.begin_step()  # while a step is open
    for call in (lambda: eng.set_wall_velocity(None), lambda: eng.wall_force(), lambda: eng.apply_moving_walls(eng_Q, SPEEDS),
                 lambda: eng.wall_force_of(eng_Q, SPEEDS)):
        with pytest.raises(_lib.HDGError, match="a step is open") as e:
            call()
        assert e.value.code == -1
    assert np.array_equal(eng.wall_velocity(), good)
    assert F.any()
    # the periodic square has no walls
    per = _stepper("ssp2", PeriodicSquareMesh(4, 4, L=2 * np.pi), 1, 0.02)._engine
    per.set_viscosity(1e-3, "no_slip")
    with pytest.raises(_lib.HDGError, match="periodic square has no walls") as e:
        per.set_wall_velocity({"bottom": 1.0})
    assert e.value.code == -1 and not per.wall_velocity().any()
    per.set_wall_velocity(zeros)
    assert not per.wall_force().any()
    # a general mesh: unsupported
    disk = _stepper("implicit", UnitDiskMesh(1), 2, 0.02)._engine
    disk.set_viscosity(1e-3, "no_slip")
    for call in (lambda: disk.set_wall_velocity({"top": 1.0}), lambda: disk.wall_force(),
                 lambda: disk.apply_moving_walls(np.zeros(disk.shape_Q), {"top": 1.0}), lambda: disk.wall_force_of(np.zeros(disk.shape_Q), zeros)):
        with pytest.raises(_lib.HDGError, match="general mesh") as e:
            call()
        assert e.value.code == -5
    disk.set_wall_velocity(zeros)
    assert not disk.wall_velocity().any() and disk.viscosity() == (1e-3, "no_slip")
    Qd = np.random.default_rng(4).standard_normal(disk.shape_Q)
    assert np.array_equal(disk.apply_moving_walls(Qd, zeros), disk.apply_viscosity(Qd, "no_slip"))


def test_the_steppers_take_wall_velocity(hip_lib):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    for which in ("ssp2", "ars2", "implicit", "dg"):
        ts = _stepper(which, UnitSquareMesh(4, 4), 1, 0.02, viscosity=1e-3, wall="no_slip", wall_velocity={"top": 1.0})
        assert np.array_equal(ts._engine.wall_velocity(), [0.0, 0.0, 1.0, 0.0])
        ts._engine.close()
    ts = _stepper("ssp2", UnitSquareMesh(4, 4), 1, 0.02, viscosity=1e-3, wall="no_slip")
    assert not ts._engine.wall_velocity().any()


# ---- 11. the driver
def test_driver_runs_the_lid_driven_cavity(hip_lib, tmp_path):
    """--problem cavity --viscosity 1e-2 --wall no_slip --wall_velocity top 1 at nx = 8 (Re = 100): the printed lines, and the
    final wall force against the reference loop's"""
    from oracle import hdg_oracle as orc

    k, nx, dt, nsteps, nu = 1, 8, 0.002, 3, 1e-2  # the viscous diffusion number is 1.9, below SSP2(3,3,2)'s limit 4.52
    argv = [sys.executable, "-m", "incompressibleeulerhdg_amd.driver", "--problem", "cavity", "--nx", str(nx), "--degree", str(k), "--dt", repr(dt),
            "--tfinal", repr(nsteps * dt), "--use_projection_method", "--viscosity", "1e-2", "--wall", "no_slip", "--output", ""]
    r = subprocess.run(argv + ["--wall_velocity", "top", "1"], cwd=tmp_path, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "model problem = cavity" in r.stdout and "wall = no_slip" in r.stdout and "wall velocity = top 1.0" in r.stdout
    assert "RuntimeWarning" not in r.stderr
    got = {}
    for ln in r.stdout.splitlines():
        if ln.startswith("wall force "):
            side, values = ln[len("wall force "):].split(" = ")
            got[side] = [float(x) for x in values.split()]
    assert list(got) == list(ref.SIDES) and all(len(v) == 2 for v in got.values()), r.stdout
    mesh, d, A, Mi, fun = _reference(nx, k)
    zero = np.zeros((d.NQ // 2, 2))
    oQ, _ = ref.imex_with_moving_walls(orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), ref.affine(d, {"top": 1.0}, A, Minv_loads=Mi), nu,
                                      zero, np.zeros(d.NP), lambda t: zero, nsteps * dt)
    want = ref.wall_force(d, nu, {"top": 1.0}, oQ, functionals=fun["no_slip"])
    G = fun["no_slip"][0]
    slack = nu * np.max(np.abs(G).sum(axis=-1)) * TOL * np.max(np.abs(oQ)) + HOOK * np.max(np.abs(want))
    F = np.array([got[s] for s in ref.SIDES])
    print(f"driver: wall force {F.tolist()}, reference {want.tolist()}")
    assert F[2, 0] > 0.0  # the lid drags the fluid along
    assert np.max(np.abs(F - want)) <= slack
    # without the flag the output carries none of it
    r0 = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r0.returncode == 0 and "wall velocity" not in r0.stdout and "wall force" not in r0.stdout
