"""The viscous term on the CPU: the numpy reference of the interior-penalty form with Nitsche walls alone,
the host tables of csrc/hdg_tables.hpp through tests/host/viscosity_check.cpp (g++ with AddressSanitizer and UBSan, no GPU), the
C-ABI table of include/hdg_viscosity.h, the model problem and the driver's --viscosity / --wall checks.  No GPU and no built
library are needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import viscosity_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MESHES = {"square3": dict(nx=3), "periodic4": dict(nx=4, periodic=True, L=2 * np.pi)}
_CACHE = {}


def reference(kind, k, wall="free_slip"):
    """(discretisation, V, M^-1 V) of a mesh of MESHES or the level-1 disk; built once, read-only."""
    from oracle import hdg_oracle as orc
    from oracle.fem import unit_disk_mesh

    if (kind, k, wall) not in _CACHE:
        d = orc.HDGDiscretisation(1, k, mesh=unit_disk_mesh(1)) if kind == "disk" else orc.HDGDiscretisation(degree=k, **MESHES[kind])
        V = ref.viscous_matrix(d, wall)
        A = ref.minv_v(d, wall, V)
        V.setflags(write=False)
        A.setflags(write=False)
        _CACHE[kind, k, wall] = (d, V, A)
    return _CACHE[kind, k, wall]


# (mesh, degree, wall mode, dimension of the null space): between walls nothing survives in either mode (the normal component
# vanishes on all four sides, which a constant cannot), on the periodic square the two constant fields do; on the disk a
# free-slip wall leaves the rigid rotation's gradient non-zero, so nothing survives there either
CASES = ([("square3", k, w, 0) for k in (1, 2, 3, 4) for w in ref.WALLS] + [("periodic4", k, "free_slip", 2) for k in (1, 2, 3, 4)] +
         [("disk", 2, w, 0) for w in ref.WALLS])


@pytest.mark.parametrize("kind,k,wall,null", CASES)
def test_reference_is_symmetric_negative_semidefinite_with_the_right_null_space(kind, k, wall, null):
    d, V, _ = reference(kind, k, wall)
    scale = np.max(np.abs(V))
    assert np.max(np.abs(V - V.T)) <= 1e-12 * scale
    ev = np.linalg.eigvalsh(0.5 * (V + V.T))
    assert ev.max() <= 1e-12 * scale  # no positive eigenvalue
    assert ev.min() < -1.0
    assert np.sum(ev > -1e-9 * scale) == null
    if null:  # the two constant fields
        for comp in range(2):
            c = np.zeros(d.NQ)
            c[comp::2] = 1.0
            assert np.max(np.abs(V @ c)) <= 1e-12 * scale


def test_no_slip_only_adds_the_tangential_wall_terms():
    """the two wall modes differ on the wall cells alone (the Nitsche terms by themselves are indefinite: only the whole form
    is negative semidefinite, which the test above checks in both modes)"""
    d, Vf, _ = reference("square3", 2, "free_slip")
    _, Vn, _ = reference("square3", 2, "no_slip")
    diff = Vn - Vf
    assert np.max(np.abs(diff)) > 1.0
    m = d.mesh
    wall_cells = set(m.edge_plus[d.ebnd])
    rows = {int(r) // (2 * d.nu) for r in np.nonzero(np.abs(diff).sum(axis=1))[0]}
    assert rows and rows <= wall_cells


def _consistency(k, nx):
    """|| M^-1 V I(Q_s) + 2 pi^2 I(Q_s) ||_L2 on the unit square, free slip: Q_s satisfies both wall conditions"""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k)
    Qs = d.interpolate_velocity(ref.taylor_green_Qs)
    r = (ref.minv_v(d) @ Qs.ravel() + 2 * np.pi ** 2 * Qs.ravel())
    return float(np.sqrt(r @ (d.MQ @ r)))


@pytest.mark.parametrize("k", [1, 2])
def test_reference_is_consistent_with_the_laplacian(k):
    errs = [_consistency(k, nx) for nx in (4, 8)]
    print(f"k={k}: ||M^-1 V Q_s + 2 pi^2 Q_s|| {errs[0]:.4e} -> {errs[1]:.4e}, ratio {errs[0] / errs[1]:.2f}")
    assert errs[1] < errs[0]


DECAY_NU = 0.05


def decay(k, nx, wall="free_slip", nsteps=None, monitor=None):
    """Unforced Q_s on the unit square with the implicit stepper at nu dt rho about 0.5 (rho h^2 about 1000 / 2400 at k = 1 / 2,
    measured below); T = 0.02: (L2 error against exp(-2 pi^2 nu T) Q_s, nu dt rho, the final Q, the discretisation)"""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(nx, k)
    A = ref.minv_v(d, wall)
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    n = int(np.ceil(0.02 * DECAY_NU * rho / 0.5)) if nsteps is None else nsteps
    dt = 0.02 / n
    Qs = d.interpolate_velocity(ref.taylor_green_Qs)
    zero = lambda t: np.zeros_like(Qs)
    Q, p = ref.implicit_with_viscosity(d, A, DECAY_NU, dt, Qs, np.zeros(d.NP), zero, n * dt, monitor=monitor)
    return ref.l2_error_velocity(d, Q, np.exp(-2 * np.pi ** 2 * DECAY_NU * n * dt)), DECAY_NU * dt * rho, Q, d


@pytest.mark.parametrize("k", [1, 2])
def test_reference_decay_converges(k):
    """the steady Taylor-Green field is an Euler solution (its advection is a gradient), so with viscosity and no forcing it
    decays like exp(-2 pi^2 nu t)"""
    e4, n4, _, _ = decay(k, 4)
    e8, n8, _, _ = decay(k, 8)
    print(f"k={k}: nu dt rho {n4:.3f} / {n8:.3f}; L2 errors {e4:.4e} -> {e8:.4e}, ratio {e4 / e8:.2f}")
    assert 0.3 < n4 <= 0.5 + 1e-12 and 0.3 < n8 <= 0.5 + 1e-12
    assert e8 < e4


def energy_series(which, wall, nsteps=6):
    """kinetic energy after 0 .. nsteps steps of an unforced reference run from Q_s (unit square, k = 2, nx = 4, the number
    nu dt Lambda-free: nu dt rho = 0.35)"""
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(4, 2)
    A = ref.minv_v(d, wall)
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    dt = 0.25 * d.mesh.h
    nu = 0.35 / (dt * rho)
    Qs = d.interpolate_velocity(ref.taylor_green_Qs)
    zero = lambda t: np.zeros_like(Qs)
    ke = [ref.kinetic_energy(d, Qs)]
    mon = lambda n, Q, p: ke.append(ref.kinetic_energy(d, Q))
    if which == "ssp2":
        ref.imex_with_viscosity(orc.OracleHDGIMEX(d, dt, "imex_ssp2_332"), A, nu, Qs, np.zeros(d.NP), zero, nsteps * dt, monitor=mon)
    else:
        ref.implicit_with_viscosity(d, A, nu, dt, Qs, np.zeros(d.NP), zero, nsteps * dt, monitor=mon)
    return np.array(ke)


@pytest.mark.parametrize("wall", ref.WALLS)
@pytest.mark.parametrize("which", ["ssp2", "implicit"])
def test_reference_energy_falls_in_every_step(which, wall):
    ke = energy_series(which, wall)
    print(f"{which} {wall}: KE / KE_0 = " + " ".join(f"{x / ke[0]:.6f}" for x in ke))
    assert np.all(np.diff(ke) < 0.0)


@pytest.mark.parametrize("kind,wall", [("square3", "free_slip"), ("square3", "no_slip"), ("periodic4", "free_slip")])
@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_host_tables_assemble_the_reference_operator(tmp_path, kind, wall, k):
    """Vol / Own / Nbr / Wall of ViscosityTables, assembled over the mesh as the kernel walks it and mapped to the nodal basis,
    against the reference M^-1 V entry by entry at 1e-11 max|entry|; Lambda_u >= the spectral radius numpy computes."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = _host_program(tmp_path.parent)
    m = MESHES[kind]
    out = tmp_path / "op.bin"
    r = subprocess.run([str(exe), str(k), str(m["nx"]), "1" if m.get("periodic") else "0", repr(float(m.get("L", 1.0))),
                        "1" if wall == "no_slip" else "0", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    raw = np.fromfile(out)
    lam, n = raw[0], int(raw[1])
    got = raw[2:].reshape(n, n)
    _, _, A = reference(kind, k, wall)
    assert got.shape == A.shape
    dev = np.max(np.abs(got - A)) / np.max(np.abs(A))
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    print(f"{kind} {wall} k={k}: deviation {dev:.3e} max|entry|, rho {rho:.6g}, Lambda_u {lam:.6g}, rho h^2 {rho * (m.get('L', 1.0) / m['nx']) ** 2:.0f}")
    assert dev <= 1e-11
    assert lam >= rho


_EXE = {}


def _host_program(where):
    if "exe" not in _EXE:
        exe = where / "viscosity_check"
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "viscosity_check.cpp")], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


def test_general_assembly_header_compiles_alone(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "hdg_general.hpp"\nint main() { return hdg::ViscosityTables(2, 0.5).lambda > 0 && &hdg::assemble_viscosity ? 0 : 1; }\n')
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-address", "-I", csrc, str(tu), "-o", str(tmp_path / "tu"), "-lpthread"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_viscosity": "int hdg_set_viscosity(hdg_handle* h, double nu, int wall);",
    "hdg_get_viscosity": "int hdg_get_viscosity(hdg_handle* h, double* nu, int* wall, double out2[2]);",
    "hdg_apply_viscosity": "int hdg_apply_viscosity(hdg_handle* h, int wall, const double* Q, double* out);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C
    import inspect

    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd import timesteppers as ts

    assert set(_lib.VISCOSITY_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_viscosity.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read()
                     for f in ("hdg_mi355x.h", "hdg_checkpoint.h", "hdg_transfer.h", "hdg_tracer_diffusion.h", "hdg_buoyancy.h"))
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp = C.c_void_p, C.POINTER(C.c_double)
    assert _lib.VISCOSITY_SIGNATURES["hdg_set_viscosity"] == [h, C.c_double, C.c_int]
    assert _lib.VISCOSITY_SIGNATURES["hdg_apply_viscosity"] == [h, C.c_int, dp, dp]
    assert _lib.VISCOSITY_HEADER.endswith(os.path.join("include", "hdg_viscosity.h")) and os.path.isfile(_lib.VISCOSITY_HEADER)
    for name in ("set_viscosity", "viscosity", "viscosity_number", "apply_viscosity"):
        assert callable(getattr(_lib.Engine, name))
    assert inspect.signature(_lib.Engine.set_viscosity).parameters["wall"].default == "free_slip"
    assert inspect.signature(_lib.Engine.apply_viscosity).parameters["wall"].default == "free_slip"
    assert _lib.WALL_MODES == {"free_slip": 0, "no_slip": 1}
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13
    assert "viscosity" not in {f[0] for f in _lib.hdg_config._fields_} and _lib.hdg_config._fields_[-1][0] == "n_tracers"
    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(cls.__init__).parameters.values()), cls
    with pytest.raises(ValueError, match="wall must be one of"):
        _lib.wall_code("sticky")


def test_the_steppers_refuse_wall_without_viscosity():
    from incompressibleeulerhdg_amd import timesteppers as ts
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        with pytest.raises(ValueError, match="wall= needs viscosity="):
            cls(UnitSquareMesh(4, 4), 1, 0.02, wall="no_slip")


# ---- model problem
def test_taylor_green_without_viscosity_is_what_it_was():
    import inspect

    from incompressibleeulerhdg_amd.mesh import FunctionSpace, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from oracle import hdg_oracle as orc

    assert list(inspect.signature(TaylorGreen.__init__).parameters)[-1] == "viscosity"
    assert inspect.signature(TaylorGreen.__init__).parameters["viscosity"].default == 0.0
    d = orc.HDGDiscretisation(3, 1)
    mesh = UnitSquareMesh(3, 3)
    V_Q = FunctionSpace(mesh, "DG", 2, d.node_coords(d.PU).reshape(-1, 2), value_size=2)
    V_p = FunctionSpace(mesh, "DG", 1, d.node_coords(d.PP).reshape(-1, 2))
    for forcing in ("exponential", "constant"):
        for kappa in (0.5, 0.0):
            old, new = TaylorGreen(V_Q, V_p, forcing=forcing, kappa=kappa), TaylorGreen(V_Q, V_p, forcing=forcing, kappa=kappa, viscosity=0.0)
            vis = TaylorGreen(V_Q, V_p, forcing=forcing, kappa=kappa, viscosity=0.01)
            want = ref.TaylorGreenNS(d, forcing, kappa, viscosity=0.01)
            for t in (0.0, 0.3):
                assert np.array_equal(old.f_rhs()(t), new.f_rhs()(t)) and old.f_rhs().scale(t) == new.f_rhs().scale(t)
                assert np.allclose(vis.f_rhs()(t), want.f_rhs(t), rtol=0, atol=1e-14)
                for a, b, c in zip(old.solution(t), new.solution(t), vis.solution(t)):
                    assert np.array_equal(a.dat.data, b.dat.data) and np.array_equal(a.dat.data, c.dat.data)


# ---- driver
def test_driver_refuses_bad_viscosity_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.viscosity is None and args.wall is None
    driver.check_viscosity(args)
    args = driver.build_parser().parse_args(["--viscosity", "1e-2", "--wall", "no_slip"])
    assert args.viscosity == 1e-2 and args.wall == "no_slip"
    driver.check_viscosity(args)

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    with pytest.raises(RuntimeError, match="--wall needs --viscosity"):
        driver.main(["--wall", "no_slip"])
    for bad in ("-0.001", "nan", "inf"):
        with pytest.raises(RuntimeError, match="--viscosity .* is not a finite number >= 0"):
            driver.main(["--viscosity", bad])
    with pytest.raises(SystemExit):
        driver.main(["--viscosity", "1e-2", "--wall", "sticky"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(["--viscosity", "1e-2", "--wall", "free_slip"])
