"""Implicit tracer diffusion without a GPU: the numpy reference tests/tracer_implicit_reference.py on its
own, the scalar rule of csrc/hdg_tracer_implicit_host.hpp through tests/host/tracer_implicit_scalars_check.cpp (g++ with
AddressSanitizer and UBSan), the C-ABI table against the header, the Python surface and the driver's refusals.

The decay test.  Backward Euler at zero velocity from sin x sin y on the periodic square (L = 2 pi), kappa = 1, T = 1, with 4, 8
and 16 steps.  The error that is proportional to dt is the one of the time discretisation, measured against the solution of
the semi-discrete system at T (the matrix exponential), whose amplitude is e^{-2 kappa T} up to the error of the mesh: its
ratios are asserted in 1.8 .. 2.2 at nx = 4, 8 and k = 1, 2 (measured 1.92 .. 1.99).  Against e^{-2 kappa T} sin x sin y itself the
L2 error has a floor set by the mesh, the error of the semi-discrete solution at T: 0.29 / 0.13 / 0.050 / 0.0044 at (k, nx) =
(1, 4) / (1, 8) / (2, 4) / (2, 8), beside time errors of 0.19 .. 0.03.  So there the same ratio is asserted where that floor lies
below the time errors, at k = 2 (measured 2.18, 1.91 at nx = 4 and 1.94, 2.01 at nx = 8; at k = 1 the figures are 0.85, 0.92 and
1.30, 0.78: the mesh's error, not the scheme's), and at every (k, nx) the error is asserted to lie within the floor plus the
time error."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import scipy.linalg

import tracer_diffusion_reference as tdr
import tracer_implicit_reference as ref
import tracer_walls_reference as twr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CACHE = {}


def operator(kind, nx, k):
    from oracle import hdg_oracle as orc

    if (kind, nx, k) not in _CACHE:
        d = orc.HDGDiscretisation(nx, k, periodic=True, L=2 * np.pi) if kind == "periodic" else orc.HDGDiscretisation(nx, k)
        _CACHE[kind, nx, k] = twr.WallOperator(d)
    return _CACHE[kind, nx, k]


def _xy(op):
    X = op.d.node_coords(op.d.PP).reshape(-1, 2)
    return X[:, 0], X[:, 1]


# ---- the reference alone
@pytest.mark.parametrize("k", [1, 2])
def test_stable_at_diffusion_number_50_where_the_explicit_loop_grows(k):
    from oracle import hdg_oracle as orc

    op = operator("periodic", 4, k)
    d = op.d
    x, y = _xy(op)
    rng = np.random.default_rng(5 + k)
    q0 = np.sin(x) * np.sin(y) + 0.3 * rng.standard_normal(len(x)) + 0.7
    tau = 50.0 / ref.rho(op)  # eleven times the real-axis limit 4.52 of SSP2(3,3,2)
    one = np.ones(d.NP)
    integral = lambda q: float(one @ (op.M @ q))
    half_sq = lambda q: 0.5 * float(q @ (op.M @ q))
    qs = ref.euler_at_rest(op, None, tau, q0, 12)
    scale = float(one @ (op.M @ np.abs(q0)))
    drift = max(abs(integral(q) - integral(q0)) for q in qs)
    energy = [half_sq(q) for q in qs]
    print(f"k={k}: integral drift {drift:.3e} of {scale:.3e}; half square {energy[0]:.6g} -> {energy[-1]:.6g}")
    assert drift <= 1e-13 * scale
    assert all(b < a for a, b in zip(energy, energy[1:]))
    o = orc.OracleHDGIMEX(d, 0.01, "imex_ssp2_332")
    assert 4.5 < tdr.stability_limit(o.a_expl, o.b_expl) < 4.6
    grown = ref.explicit_at_rest(op, o.a_expl, o.b_expl, tau, q0, 12)
    print(f"  explicit tableau at the same number: half square {half_sq(grown[0]):.6g} -> {half_sq(grown[-1]):.6g}")
    assert half_sq(grown[-1]) > 1e6 * half_sq(grown[0])


@pytest.mark.parametrize("k,nx", [(1, 4), (1, 8), (2, 4), (2, 8)])
def test_decay_error_is_proportional_to_dt(k, nx):
    op = operator("periodic", nx, k)
    d = op.d
    x, y = _xy(op)
    q0 = np.sin(x) * np.sin(y)
    kappa, T = 1.0, 1.0
    exact_in_time = scipy.linalg.expm(kappa * T * op.A0) @ q0
    norm = lambda v: float(np.sqrt(v @ (op.M @ v)))
    floor = tdr.l2_error(d, exact_in_time, np.exp(-2 * kappa * T))
    amp = float(q0 @ (op.M @ exact_in_time)) / float(q0 @ (op.M @ q0))
    time_err, full_err = [], []
    for n in (4, 8, 16):
        q = ref.euler_at_rest(op, None, kappa * T / n, q0, n)[-1]
        time_err.append(norm(q - exact_in_time))
        full_err.append(tdr.l2_error(d, q, np.exp(-2 * kappa * T)))
    ratios = [time_err[0] / time_err[1], time_err[1] / time_err[2]]
    print(f"k={k} nx={nx}: amplitude of the semi-discrete solution {amp:.6f} (e^-2 = {np.exp(-2.0):.6f}), mesh floor {floor:.3e}")
    print(f"  time error {time_err}, ratios {ratios}")
    print(f"  error against e^-2 sin x sin y {full_err}, ratios {[full_err[0] / full_err[1], full_err[1] / full_err[2]]}")
    assert all(1.8 <= r <= 2.2 for r in ratios)
    assert 0.0 < amp < 1.0  # printed above: it is e^{-2 kappa T} to the mesh's error (43 % off at k = 1, nx = 4)
    for e, t in zip(full_err, time_err):
        assert e <= (floor + t) * (1 + 1e-12)
    if k == 2:  # the mesh's floor lies at or below the smallest time error: the ratio shows against the analytic solution itself
        assert floor < time_err[-1]
        assert all(1.8 <= r <= 2.2 for r in (full_err[0] / full_err[1], full_err[1] / full_err[2]))


@pytest.mark.parametrize("k", [1, 2])
def test_one_step_at_1e8_conducts_between_the_walls(k):
    """left = 0.5, right = -0.5: the linear profile 0.5 - x is a fixed point of the solve (it lies in the space and the Nitsche
    form is consistent), and the rest of the start is damped by at least 1 / (1 + tau lambda_min), lambda_min the smallest
    eigenvalue of -M^-1 (D + D_w).  The reference's own deviation, times ten, is that bound."""
    op = operator("square", 3, k)
    walls = {"left": 0.5, "right": -0.5}
    x, y = _xy(op)
    linear = 0.5 - x
    A, b = op.minv(walls)
    assert np.max(np.abs(A @ linear + b)) <= 1e-9 * np.max(np.abs(A))
    lam = np.sort(np.real(np.linalg.eigvals(-A)))
    assert lam[0] > 0
    tau = 1e8 / lam[-1]
    q0 = np.sin(2 * np.pi * x) * np.cos(3 * y) + 0.2
    q1 = ref.solve_dense(op, walls, tau, q0)
    norm = lambda v: float(np.sqrt(v @ (op.M @ v)))
    dev, start = norm(q1 - linear), norm(q0 - linear)
    bound = 10.0 * start / (1.0 + tau * lam[0])
    print(f"k={k}: deviation from 0.5 - x after one step {dev:.3e} (start {start:.3e}), bound {bound:.3e}")
    assert dev <= bound
    xc, its, res = ref.cg(op, walls, tau, q0, rtol=1e-12, maxit=5000)  # the reference CG reaches it too
    assert res <= 1e-12 and norm(xc - q1) <= 1e-6 * start


def test_reference_cg_counts_are_those_of_the_design_note():
    """k = 2, random right-hand side, rtol 1e-10 at diffusion numbers 10 / 100 / 1000 on the periodic square: the counts DESIGN.md
    section 28 quotes, to the iterations that another random field and the start x_0 = b instead of 0 move them."""
    for nx, quoted in ((6, (37, 101, 160)),):
        op = operator("periodic", nx, 2)
        rho = ref.rho(op)
        q = np.random.default_rng(1).standard_normal(op.d.NP)
        counts = [ref.cg(op, None, number / rho, q)[1] for number in (10.0, 100.0, 1000.0)]
        print(f"nx={nx}: {counts} (quoted {quoted})")
        for c, w in zip(counts, quoted):
            assert abs(c - w) <= 0.15 * w
        x, its, res = ref.cg(op, None, 100.0 / rho, q)
        assert res <= 1e-10 and np.max(np.abs(x - ref.solve_dense(op, None, 100.0 / rho, q))) <= 1e-7 * np.max(np.abs(x))


# ---- the scalar rule on the host
def test_scalar_rule_on_the_host(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path / "tracer_implicit_scalars_check"
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "tracer_implicit_scalars_check.cpp")], check=True)
    for n, tau, rtol, maxit in ((40, 0.3, 1e-10, 500), (200, 30.0, 1e-10, 500), (200, 3000.0, 1e-12, 2000)):
        r = subprocess.run([str(exe), str(n), repr(tau), repr(rtol), str(maxit)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
        its, itp, err, errp, res, state = r.stdout.splitlines()[0].split()
        print(f"n={n} tau={tau}: rule {its} iterations (error {float(err):.3e}), textbook {itp} ({float(errp):.3e}), residual {float(res):.3e}")
        assert int(state) == 1 and float(res) <= rtol
        assert int(its) <= int(itp) + 0.1 * int(itp) + 2
        assert float(err) <= 10 * (1 + 4 * tau) * rtol * 10.0  # cond(A) rtol max|b|, max|b| < 10
    r = subprocess.run([str(exe), "200", "3000.0", "1e-12", "5"], capture_output=True, text=True)  # out of iterations
    assert r.returncode == 0, r.stdout + r.stderr
    its, _, _, _, res, state = r.stdout.splitlines()[0].split()
    assert int(its) == 5 and int(state) == 2 and float(res) > 1e-12


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_tracer_diffusion_mode": "int hdg_set_tracer_diffusion_mode(hdg_handle* h, int mode, double rtol, int max_iterations);",
    "hdg_get_tracer_diffusion_solve": "int hdg_get_tracer_diffusion_solve(hdg_handle* h, int n, int* its, double* res);",
    "hdg_solve_tracer_diffusion": "int hdg_solve_tracer_diffusion(hdg_handle* h, int n, const double* tau, const double* q_in, double* q_out, int* its);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.TRACER_IMPLICIT_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_tracer_implicit.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include")))
                     if f != "hdg_tracer_implicit.h")
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES and name not in _lib.TRACER_DIFFUSION_SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert _lib.TRACER_IMPLICIT_SIGNATURES["hdg_set_tracer_diffusion_mode"] == [h, C.c_int, C.c_double, C.c_int]
    assert _lib.TRACER_IMPLICIT_SIGNATURES["hdg_get_tracer_diffusion_solve"] == [h, C.c_int, ip, dp]
    assert _lib.TRACER_IMPLICIT_SIGNATURES["hdg_solve_tracer_diffusion"] == [h, C.c_int, dp, dp, dp, ip]
    assert _lib.TRACER_IMPLICIT_HEADER.endswith(os.path.join("include", "hdg_tracer_implicit.h")) and os.path.isfile(_lib.TRACER_IMPLICIT_HEADER)
    assert "tracer_diffusion" not in "".join(name for name, _ in _lib.hdg_config._fields_)
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13
    core = open(os.path.join(ROOT, "include", "hdg_mi355x.h")).read()
    assert re.search(r"#define\s+HDG_N_LAUNCH_CLASSES\s+13\b", core)


class _Lib:
    """Stands in for the library: records the calls of the three entry points."""

    def __init__(self):
        self.calls = []

    def hdg_set_tracer_diffusion_mode(self, h, mode, rtol, maxit):
        self.calls.append(("mode", mode, rtol, maxit))
        return 0

    def hdg_get_tracer_diffusion_solve(self, h, n, its, res):
        np.ctypeslib.as_array(its, (n,))[:] = np.arange(n) + 3
        np.ctypeslib.as_array(res, (n,))[:] = 1e-11 * (np.arange(n) + 1)
        return 0

    def hdg_solve_tracer_diffusion(self, h, n, tau, q_in, q_out, its):
        self.calls.append(("solve", n, np.ctypeslib.as_array(tau, (n,)).copy()))
        np.ctypeslib.as_array(q_out, (n * 6,))[:] = 2.0 * np.ctypeslib.as_array(q_in, (n * 6,))
        np.ctypeslib.as_array(its, (n,))[:] = 7
        return 0


def test_python_surface_on_a_stand_in_engine():
    from incompressibleeulerhdg_amd import _lib

    eng = object.__new__(_lib.Engine)
    eng.lib, eng.h, eng.n_tracers, eng.general, eng.shape_p = _Lib(), None, 2, False, (6,)
    eng._ck = lambda rc: None
    assert eng.tracer_diffusion_mode() == "explicit"
    eng.set_tracer_diffusion_mode("implicit")
    assert eng.lib.calls[-1] == ("mode", 1, 1e-10, 2000) and eng.tracer_diffusion_mode() == "implicit"
    eng.set_tracer_diffusion_mode("explicit", rtol=1e-8, max_iterations=30)
    assert eng.lib.calls[-1] == ("mode", 0, 1e-8, 30) and eng.tracer_diffusion_mode() == "explicit"
    eng.set_tracer_diffusion_mode(1)
    assert eng.lib.calls[-1][1] == 1
    with pytest.raises(ValueError, match="tracer_diffusion must be one of"):
        eng.set_tracer_diffusion_mode("crank-nicolson")
    its, res = eng.tracer_diffusion_solve()
    assert its.tolist() == [3, 4] and res.tolist() == [1e-11, 2e-11]
    q = np.arange(12.0).reshape(2, 6)
    x, its = eng.solve_tracer_diffusion([0.5, 0.0], q)
    assert np.array_equal(x, 2.0 * q) and its.tolist() == [7, 7]
    assert eng.lib.calls[-1][1] == 2 and eng.lib.calls[-1][2].tolist() == [0.5, 0.0]
    with pytest.raises(ValueError, match="expected array of shape"):
        eng.solve_tracer_diffusion([0.5], q)


def test_every_stepper_takes_tracer_diffusion(monkeypatch):
    """"implicit" without tracer_diffusivity= raises; with it the stepper sets the mode and stays silent about the explicit
    limit; "explicit" makes no call at all (stand-in engine: no GPU)."""
    import warnings

    from incompressibleeulerhdg_amd import timesteppers as tsm
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import common

    class Eng:
        n_edges, n_l = 1, 1

        def __init__(self, **kw):
            self.calls = []

        def node_coordinates(self):
            return np.zeros((3, 2)), np.zeros((3, 2))

        def set_tracer_diffusivity(self, k):
            self.calls.append("kappa")

        def set_tracer_diffusion_mode(self, mode):
            self.calls.append(("mode", mode))

        def tracer_diffusion_number(self):
            return 1000.0, 50.0  # far above the explicit limit

        def __getattr__(self, name):
            raise AssertionError(f"unexpected call {name}")

    monkeypatch.setattr(common, "Engine", Eng)
    mesh = UnitSquareMesh(4, 4)
    for cls, kw in ((tsm.IncompressibleEulerHDGIMEXSSP2_332, dict(use_projection_method=True)), (tsm.IncompressibleEulerHDGIMEXARS2_232, {}),
                    (tsm.IncompressibleEulerHDGImplicit, {}), (tsm.IncompressibleEulerDGImplicit, {})):
        with pytest.raises(ValueError, match='needs tracer_diffusivity='):
            cls(mesh, 1, 0.01, tracer_diffusion="implicit", **kw)
        with pytest.raises(ValueError, match="'explicit' or 'implicit'"):
            cls(mesh, 1, 0.01, tracer_diffusivity=1.0, tracer_diffusion="both", **kw)
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            ts = cls(mesh, 1, 0.01, tracer_diffusivity=1.0, tracer_diffusion="implicit", **kw)
        assert ts._engine.calls == ["kappa", ("mode", "implicit")], cls
        with pytest.warns(RuntimeWarning, match="exceeds the stability limit"):
            ts = cls(mesh, 1, 0.01, tracer_diffusivity=1.0, **kw)
        assert ts._engine.calls == ["kappa"] and ts.tracer_diffusion_iterations is None


# ---- driver
def test_driver_refuses_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.tracer_diffusion is None
    driver.check_tracers(args)
    ok = ["--tracer_advection", "--tracer_diffusivity", "1e-3", "--tracer_diffusion", "implicit"]
    driver.check_tracers(driver.build_parser().parse_args(ok))

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    for mode in ("implicit", "explicit"):
        with pytest.raises(RuntimeError, match="--tracer_diffusion needs --tracer_diffusivity"):
            driver.main(["--tracer_advection", "--tracer_diffusion", mode])
    with pytest.raises(RuntimeError, match="general mesh"):
        driver.main(["--problem", "kelvinhelmholtz"] + ok)
    with pytest.raises(RuntimeError, match="--gpus 2"):
        driver.main(["--gpus", "2"] + ok)
    args = driver.build_parser().parse_args(["--gpus", "2"] + ok)
    with pytest.raises(RuntimeError, match="--tracer_diffusion implicit does not support --gpus 2"):
        driver.check_tracers(args)
    with pytest.raises(SystemExit):
        driver.build_parser().parse_args(["--tracer_diffusion", "semi"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(ok)
    several = {}
    args = driver.build_parser().parse_args(ok)
    src = open(driver.__file__).read()
    assert 'several["tracer_diffusion"] = "implicit"' in src and args.tracer_diffusion == "implicit" and not several
