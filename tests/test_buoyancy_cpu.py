"""Boussinesq buoyancy on the CPU: what the numpy reference tests/buoyancy_reference.py shows -- the rest
state, a gravity wave, a heavy blob, linearity in (beta, g) -- the C-ABI table of include/hdg_buoyancy.h and the driver's
--buoyancy / --gravity checks.  No GPU and no built library are needed."""
import os
import re

import numpy as np
import pytest

import buoyancy_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G_DOWN = ref.G_DOWN
_oracles = ref.oracles


# ---- 1. rest state: the force is the gradient of a continuous P_k potential (set-up and comments: buoyancy_reference.py)
@pytest.mark.parametrize("which", ["ssp2", "implicit"])
@pytest.mark.parametrize("k", [2, 3])
def test_rest_state_stays_at_rest_on_the_reference(which, k):
    uQ, slope, eq, _ = ref.rest_state(which, k)
    print(f"{which} k={k}: max|Q| {uQ:.3e} of free fall, p = {slope:.4f} * potential, max|q - q0| {eq:.3e}")
    assert uQ <= 0.2
    if which in ref.REST_SLOPE:
        assert abs(slope - ref.REST_SLOPE[which]) <= 0.1 * ref.REST_SLOPE[which]


# ---- 2. gravity wave (set-up: buoyancy_reference.py)
def test_gravity_wave_crossing_time_converges_on_the_reference():
    times = {}
    for nx in (4, 8):
        step, times[nx] = ref.crossing(ref.wave_run(nx)[0], ref.WAVE_DT)
        print(f"nx={nx}: the amplitude changes sign in step {step}, t = {times[nx]:.6f} (analytic {ref.WAVE_T:.6f})")
    assert abs(times[8] - ref.WAVE_T) < abs(times[4] - ref.WAVE_T)


# ---- 3. heavy blob released from rest
def test_heavy_blob_falls_on_the_reference():
    from oracle import hdg_oracle as orc

    k, nx, dt, nsteps = 2, 6, 0.02, 3
    d, tr = _oracles(nx, k)
    q0 = d.interpolate_pressure(lambda x, y: np.exp(-((x - 0.5) ** 2 + (y - 0.6) ** 2) / 0.02))
    Q0, p0 = np.zeros((d.mesh.ncells * d.nu, 2)), np.zeros(d.NP)
    zero = lambda t: np.zeros_like(Q0)
    Q, p, q = ref.imex_with_buoyancy(orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), tr, 1.0, G_DOWN, Q0, p0, q0, zero, nsteps * dt)
    anomaly = q - float(d.int_p @ q) / d.mesh.volume
    flux = ref.integrate_q_uy(d, anomaly, Q)
    dKE = ref.kinetic_energy(d, Q) - ref.kinetic_energy(d, Q0)
    dPE = ref.potential_energy(d, q, 1.0, G_DOWN) - ref.potential_energy(d, q0, 1.0, G_DOWN)
    print(f"int q' u_y {flux:.6e}, dKE {dKE:.6e}, dPE {dPE:.6e}, dKE / (-dPE) {dKE / -dPE:.4f}")
    assert flux < 0.0 and dKE > 0.0 and dPE < 0.0


# ---- 4. linearity of the reference in (beta, g)
def test_reference_is_linear_in_beta_and_g():
    d, _ = _oracles(3, 2)
    rng = np.random.default_rng(5)
    q = rng.standard_normal((3, d.NP))
    b1, b2 = np.array([1.0, 0.0, -2.5]), np.array([0.5, 3.0, 0.25])
    g1, g2 = np.array([0.3, -1.0]), np.array([-2.0, 0.7])
    f = lambda b, g: ref.B(d, q, b, g)
    scale = np.max(np.abs(f(b1, g1)))
    assert np.max(np.abs(f(b1 + b2, g1) - f(b1, g1) - f(b2, g1))) <= 1e-13 * scale
    assert np.max(np.abs(f(b1, g1 + g2) - f(b1, g1) - f(b1, g2))) <= 1e-13 * scale
    assert np.max(np.abs(f(2.0 * b1, g1) - f(b1, 2.0 * g1))) <= 1e-13 * scale
    assert np.array_equal(f(np.zeros(3), g1), np.zeros_like(f(b1, g1)))
    # a passive tracer is not read, and the embedding reproduces a P_k function at the velocity nodes
    q_nan = q.copy()
    q_nan[1] = np.nan
    assert np.array_equal(f(b1, g1), ref.B(d, q_nan, b1, g1))
    fn = lambda x, y: 1.0 + x - 2.0 * y + x * y - 0.5 * y * y
    got = ref.B(d, d.interpolate_pressure(fn), 1.0, (1.0, 0.0))[:, 0]
    X = d.node_coords(d.PU).reshape(-1, 2)
    assert np.max(np.abs(got - fn(X[:, 0], X[:, 1]))) <= 1e-13


# ---- 5. C-ABI, Python surface, driver
SIGNATURES_IN_C = {
    "hdg_set_buoyancy": "int hdg_set_buoyancy(hdg_handle* h, int n, const double* beta, const double g[2]);",
    "hdg_get_buoyancy": "int hdg_get_buoyancy(hdg_handle* h, int n, double* beta, double g[2]);",
    "hdg_apply_buoyancy": "int hdg_apply_buoyancy(hdg_handle* h, const double* q, double* f);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C
    import inspect

    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd import timesteppers as ts

    assert set(_lib.BUOYANCY_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_buoyancy.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read()
                     for f in ("hdg_mi355x.h", "hdg_checkpoint.h", "hdg_transfer.h", "hdg_tracer_diffusion.h"))
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp = C.c_void_p, C.POINTER(C.c_double)
    assert _lib.BUOYANCY_SIGNATURES["hdg_set_buoyancy"] == [h, C.c_int, dp, dp]
    assert _lib.BUOYANCY_HEADER.endswith(os.path.join("include", "hdg_buoyancy.h")) and os.path.isfile(_lib.BUOYANCY_HEADER)
    for name in ("set_buoyancy", "buoyancy", "apply_buoyancy"):
        assert callable(getattr(_lib.Engine, name))
    assert inspect.signature(_lib.Engine.set_buoyancy).parameters["gravity"].default == (0.0, -1.0)
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13
    assert "buoyancy" not in {f[0] for f in _lib.hdg_config._fields_} and _lib.hdg_config._fields_[-1][0] == "n_tracers"
    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(cls.__init__).parameters.values()), cls


def test_driver_host_mean_of_a_nodal_field():
    """the mean the driver prints: exact for P_k fields, on the structured mesh and on a general one"""
    from incompressibleeulerhdg_amd import driver
    from oracle import hdg_oracle as orc
    from oracle.fem import unit_disk_mesh

    fn = lambda x, y: 1.0 + 2.0 * x - y + 3.0 * x * y
    for d in (orc.HDGDiscretisation(3, 2), orc.HDGDiscretisation(1, 2, mesh=unit_disk_mesh(1))):
        q = d.interpolate_pressure(fn)
        want = float(d.int_p @ q) / d.mesh.volume
        assert driver.nodal_mean(d.node_coords(d.PP).reshape(-1, 2), 2, q) == pytest.approx(want, rel=1e-12)


def test_driver_refuses_bad_buoyancy_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.buoyancy is None and args.gravity is None
    driver.check_tracers(args)
    args = driver.build_parser().parse_args(["--tracer_advection", "--tracers", "2", "--buoyancy", "1", "-1", "--gravity", "0", "-1"])
    assert args.buoyancy == [1.0, -1.0] and args.gravity == [0.0, -1.0]
    driver.check_tracers(args)
    driver.check_tracers(driver.build_parser().parse_args(["--tracer_advection", "--tracers", "3", "--buoyancy", "0.5"]))

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    with pytest.raises(RuntimeError, match="--buoyancy needs --tracer_advection"):
        driver.main(["--buoyancy", "1"])
    with pytest.raises(RuntimeError, match="--gravity needs --buoyancy"):
        driver.main(["--tracer_advection", "--gravity", "0", "-1"])
    for n, vals in ((3, ["1", "2"]), (2, ["1", "2", "3"]), (1, ["1", "2"])):
        with pytest.raises(RuntimeError, match=rf"one value or --tracers = {n} values \(got {len(vals)}\)"):
            driver.main(["--tracer_advection", "--tracers", str(n), "--buoyancy", *vals])
    for bad in ("nan", "inf"):
        with pytest.raises(RuntimeError, match="--buoyancy: value 1 .* is not a finite number"):
            driver.main(["--tracer_advection", "--tracers", "2", "--buoyancy", "1", bad])
        with pytest.raises(RuntimeError, match="--gravity: component 0 .* is not a finite number"):
            driver.main(["--tracer_advection", "--buoyancy", "1", "--gravity", bad, "-1"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(["--tracer_advection", "--tracers", "2", "--buoyancy", "1", "-1", "--gravity", "0", "-1"])
