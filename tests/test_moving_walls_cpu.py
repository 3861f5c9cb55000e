"""Moving no-slip walls and the wall force on the CPU: the numpy reference alone (the linear shear, the
force budget, the sign), the host tables of csrc/hdg_tables.hpp through tests/host/moving_walls_check.cpp (g++ with
AddressSanitizer and UBSan, no GPU), the C-ABI table of include/hdg_moving_walls.h, the Python surface and the refusals of the
steppers and the driver.  No GPU and no built library are needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import moving_walls_reference as ref
import viscosity_reference as vref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SPEEDS = (0.3, -0.7, 1.0, 0.45)
_CACHE = {}


def reference(k, nx=3):
    """(discretisation, M^-1 V with no slip, M^-1 of the four unit loads) of the unit square; built once, read-only."""
    from oracle import hdg_oracle as orc

    if (k, nx) not in _CACHE:
        d = orc.HDGDiscretisation(nx, k)
        A = vref.minv_v(d, "no_slip")
        Mi = np.linalg.solve(d.MQ.toarray(), ref.unit_loads(d).T).T
        A.setflags(write=False)
        Mi.setflags(write=False)
        _CACHE[k, nx] = (d, A, Mi)
    return _CACHE[k, nx]


# the exact solution of Stokes flow between a moving and a resting wall, per side: (side, u(x, y))
SHEARS = {"top": lambda x, y: (y, 0 * y), "bottom": lambda x, y: (1 - y, 0 * y), "right": lambda x, y: (0 * x, x), "left": lambda x, y: (0 * x, 1 - x)}


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("side", ref.SIDES)
def test_reference_annihilates_the_linear_shear(k, side):
    """u linear between the moving wall (speed 1) and the resting one opposite: M^-1 (V u + l) vanishes on the cells that do
    not touch the two other walls (where u does not satisfy no slip); without the load it does not"""
    d, A, Mi = reference(k)
    X = d.node_coords(d.PU).reshape(-1, 2)
    u = np.stack(SHEARS[side](X[:, 0], X[:, 1]), axis=-1)
    cv = d.mesh.cell_vertices
    ax = 0 if side in ("top", "bottom") else 1  # the two other walls are the ends of this axis
    keep = (cv[:, :, ax].min(axis=1) > 1e-9) & (cv[:, :, ax].max(axis=1) < 1 - 1e-9)
    assert keep.any() and not keep.all()
    with_load = (ref.affine(d, {side: 1.0}, A, Minv_loads=Mi) @ u.ravel()).reshape(d.mesh.ncells, -1, 2)
    without = (A @ u.ravel()).reshape(d.mesh.ncells, -1, 2)
    r, r0 = np.max(np.abs(with_load[keep])), np.max(np.abs(without[keep]))
    print(f"k={k} {side}: |M^-1 (V u + l)| = {r:.3e}, without the load {r0:.3e}, relative {r / r0:.1e}")
    assert r0 > 1e3
    assert r <= 1e-12 * r0  # rounding of entries of size Lambda_u (the issue measured 6e-15)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_reference_force_budget(k):
    """sum_w F_w = int M^-1 (V u + l(U)) dx for a broken random u, in both wall modes"""
    d, A, Mi = reference(k)
    u = np.random.default_rng(1).standard_normal((d.NQ // 2, 2))
    total = ref.integral(d, ref.affine(d, SPEEDS, A, Minv_loads=Mi) @ u.ravel())
    F = ref.wall_force(d, 1.0, SPEEDS, u)
    err = np.max(np.abs(F.sum(axis=0) - total)) / np.max(np.abs(total))
    free = ref.integral(d, vref.minv_v(d, "free_slip") @ u.ravel())
    Ff = ref.wall_force(d, 1.0, (0, 0, 0, 0), u, "free_slip")
    errf = np.max(np.abs(Ff.sum(axis=0) - free)) / np.max(np.abs(free))
    print(f"k={k}: budget no slip {err:.3e}, free slip {errf:.3e}")
    assert err <= 1e-13 and errf <= 1e-13
    # free slip: the normal part only
    assert np.all(Ff[[0, 2], 0] == 0.0) and np.all(Ff[[1, 3], 1] == 0.0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_reference_sign(k):
    """from rest a lid with U_top > 0 accelerates the top cells in +x, and F_top . e_x > 0"""
    d, A, Mi = reference(k)
    acc = (ref.affine(d, {"top": 1.0}, A, Minv_loads=Mi) @ np.zeros(d.NQ)).reshape(d.mesh.ncells, -1, 2)
    M = d.MQ.toarray()
    mean = (M @ acc.ravel()).reshape(d.mesh.ncells, -1, 2).sum(axis=1)  # int over each cell
    top = d.mesh.cell_vertices[:, :, 1].max(axis=1) > 1 - 1e-9
    touching = np.array([np.sum(np.abs(v[:, 1] - 1.0) < 1e-9) == 2 for v in d.mesh.cell_vertices])  # an edge on the lid
    assert touching.sum() == 3 and np.all(mean[touching, 0] > 0.0)
    assert np.all(mean[~top] == 0.0) and np.all(mean[:, 1] == 0.0)
    F = ref.wall_force(d, 1.0, {"top": 1.0}, np.zeros((d.NQ // 2, 2)))
    assert F[2, 0] > 0.0 and np.count_nonzero(F) == 1


# ---- host tables
_EXE = {}


def _host_program(where):
    if "exe" not in _EXE:
        exe = where / "moving_walls_check"
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "moving_walls_check.cpp")], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_host_load_vectors_are_the_reference_load(tmp_path, k):
    """lvec = - Wall coef(1) and packed_moving() = packed() + the four vectors (the program's own checks); the vectors placed
    as k_viscosity<., true> places them and mapped to the nodal basis against the reference's M^-1 l at 1e-11 max|entry|"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = _host_program(tmp_path.parent)
    out = tmp_path / "load.bin"
    r = subprocess.run([str(exe), str(k), "3", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    raw = np.fromfile(out)
    d, _, Mi = reference(k)
    n, wone = int(raw[0]), raw[1]
    assert n == d.NQ
    got = raw[2:].reshape(4, n)
    dev = np.max(np.abs(got - Mi)) / np.max(np.abs(Mi))
    _, g0 = ref.force_functionals(d)
    print(f"k={k}: load vectors deviate by {dev:.3e} max|entry|; wone {wone!r}")
    assert dev <= 1e-11
    # int_w eta_b over a side of three cells, on the tangential component only
    for w in range(4):
        assert g0[w, ref.TANGENTIAL[w]] == pytest.approx(3 * wone, rel=1e-13) and g0[w, 1 - ref.TANGENTIAL[w]] == 0.0


def test_packed_is_what_the_viscous_kernel_reads():
    """packed() keeps its nine blocks per shape in its order; the new members stand behind it (source check: the host program
    above compares the values)"""
    src = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_tables.hpp")).read()
    body = src[src.index("struct ViscosityTables"):src.index("struct CoriolisTables")]
    packed = body[body.index("dvec packed() const"):body.index("// device layout with moving walls")]
    assert "static constexpr int NBLK = 9;" in body
    assert re.sub(r"\s+", " ", packed).startswith(
        "dvec packed() const { dvec out; auto put = [&](const dvec& B) { for (int m = 0; m < nu; m++) for (int r = 0; r < nu; r++) "
        "out.push_back(B[(size_t)r * nu + m]); }; for (int s = 0; s < 2; s++) { put(Vol[s]); for (int e = 0; e < 3; e++) put(Own[s][e]); "
        "for (int e = 0; e < 3; e++) put(Nbr[s][e]); put(Wall[s][0]); put(Wall[s][2]); } return out; }")
    assert "lvec" not in packed and "dvec out = packed();" in body


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_wall_velocity": "int hdg_set_wall_velocity(hdg_handle* h, const double U[4]);",
    "hdg_get_wall_velocity": "int hdg_get_wall_velocity(hdg_handle* h, double U[4]);",
    "hdg_get_wall_force": "int hdg_get_wall_force(hdg_handle* h, double F[8]);",
    "hdg_apply_moving_walls": "int hdg_apply_moving_walls(hdg_handle* h, int wall, const double U[4], const double* Q, double* out);",
    "hdg_apply_wall_force": "int hdg_apply_wall_force(hdg_handle* h, int wall, const double U[4], const double* Q, double F[8]);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C
    import inspect

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.MOVING_WALL_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_moving_walls.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include")))
                     if f != "hdg_moving_walls.h")
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp = C.c_void_p, C.POINTER(C.c_double)
    assert _lib.MOVING_WALL_SIGNATURES["hdg_set_wall_velocity"] == [h, dp]
    assert _lib.MOVING_WALL_SIGNATURES["hdg_get_wall_force"] == [h, dp]
    assert _lib.MOVING_WALL_SIGNATURES["hdg_apply_moving_walls"] == [h, C.c_int, dp, dp, dp]
    assert _lib.MOVING_WALL_SIGNATURES["hdg_apply_wall_force"] == [h, C.c_int, dp, dp, dp]
    assert _lib.MOVING_WALL_HEADER.endswith(os.path.join("include", "hdg_moving_walls.h")) and os.path.isfile(_lib.MOVING_WALL_HEADER)
    for name in ("set_wall_velocity", "wall_velocity", "wall_force", "apply_moving_walls", "wall_force_of"):
        assert callable(getattr(_lib.Engine, name))
    assert inspect.signature(_lib.Engine.apply_moving_walls).parameters["wall"].default == "no_slip"
    assert inspect.signature(_lib.Engine.wall_force_of).parameters["wall"].default == "no_slip"
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13
    assert not any("wall" in f[0] for f in _lib.hdg_config._fields_) and _lib.hdg_config._fields_[-1][0] == "n_tracers"


def test_wall_velocity_array():
    from incompressibleeulerhdg_amd import _lib

    assert np.array_equal(_lib.wall_velocity_array({"top": 1.0}), [0.0, 0.0, 1.0, 0.0])
    assert np.array_equal(_lib.wall_velocity_array({"left": -2, "bottom": 0.5}), [0.5, 0.0, 0.0, -2.0])
    assert np.array_equal(_lib.wall_velocity_array(SPEEDS), SPEEDS)
    assert _lib.wall_velocity_array(np.array(SPEEDS, dtype=np.float32)).dtype == np.float64
    with pytest.raises(ValueError, match="unknown wall side 'lid'"):
        _lib.wall_velocity_array({"lid": 1.0})
    with pytest.raises(ValueError, match="four values"):
        _lib.wall_velocity_array([1.0, 2.0])


def test_the_steppers_refuse_wall_velocity_without_no_slip_viscosity():
    from incompressibleeulerhdg_amd import timesteppers as ts
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGIMEXARS2_232, ts.IncompressibleEulerHDGImplicit,
                ts.IncompressibleEulerDGImplicit):
        for kw in ({}, {"viscosity": 1e-2}, {"viscosity": 1e-2, "wall": "free_slip"}):
            with pytest.raises(ValueError, match='wall_velocity= needs viscosity= and wall="no_slip"'):
                cls(UnitSquareMesh(4, 4), 1, 0.02, wall_velocity={"top": 1.0}, **kw)


# ---- driver
def test_driver_refuses_bad_wall_velocity_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.wall_velocity is None and driver.wall_velocity(args) is None
    ok = ["--problem", "cavity", "--viscosity", "1e-2", "--wall", "no_slip", "--wall_velocity", "top", "1", "--wall_velocity", "left", "-0.5"]
    assert driver.wall_velocity(driver.build_parser().parse_args(ok)) == {"top": 1.0, "left": -0.5}

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    for argv in (["--wall_velocity", "top", "1"], ["--viscosity", "1e-2", "--wall_velocity", "top", "1"],
                 ["--viscosity", "1e-2", "--wall", "free_slip", "--wall_velocity", "top", "1"]):
        with pytest.raises(RuntimeError, match="--wall_velocity needs --viscosity and --wall no_slip"):
            driver.main(argv)
    visc = ["--viscosity", "1e-2", "--wall", "no_slip"]
    with pytest.raises(RuntimeError, match="--wall_velocity: the doubly periodic square of --problem shear has no walls"):
        driver.main(["--problem", "shear"] + visc + ["--wall_velocity", "top", "1"])
    with pytest.raises(RuntimeError, match="--wall_velocity: the disk of --problem kelvinhelmholtz is a general mesh"):
        driver.main(["--problem", "kelvinhelmholtz"] + visc + ["--wall_velocity", "top", "1"])
    with pytest.raises(RuntimeError, match="--wall_velocity: unknown side 'lid'"):
        driver.main(visc + ["--wall_velocity", "lid", "1"])
    for bad in ("nan", "inf", "fast"):
        with pytest.raises(RuntimeError, match=f"--wall_velocity top: speed {bad} is not a finite number"):
            driver.main(visc + ["--wall_velocity", "top", bad])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(ok)
