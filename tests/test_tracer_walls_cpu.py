"""Tracer wall conditions on the CPU: the numpy reference of the Nitsche wall terms alone, the host
tables of csrc/hdg_tables.hpp through tests/host/tracer_walls_check.cpp (g++ with AddressSanitizer and UBSan, no GPU), the
C-ABI table of include/hdg_tracer_walls.h, the Python surface on a stand-in engine, the Cavity problem and the driver's
--tracer_wall checks.  No GPU and no built library are needed."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import tracer_walls_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_CACHE = {}


def operator(kind, k):
    """The WallOperator of the 3x3 unit square or the level-1 disk; built once, read-only."""
    from oracle import hdg_oracle as orc
    from oracle.fem import unit_disk_mesh

    if (kind, k) not in _CACHE:
        d = orc.HDGDiscretisation(1, k, mesh=unit_disk_mesh(1)) if kind == "disk" else orc.HDGDiscretisation(3, k)
        _CACHE[kind, k] = ref.WallOperator(d, general=kind == "disk")
    return _CACHE[kind, k]


CASES = [("square3", k) for k in (1, 2, 3, 4)] + [("disk", 2)]


def _xy(op):
    X = op.d.node_coords(op.d.PP).reshape(-1, 2)
    return X[:, 0], X[:, 1]


@pytest.mark.parametrize("kind,k", CASES)
def test_reference_is_symmetric_negative_definite_with_a_fixed_side(kind, k):
    op = operator(kind, k)
    scale = np.max(np.abs(op.D))
    sets = [{"boundary": 1.0}] if kind == "disk" else [{"bottom": 1.0}, {"left": 0.3}, {"top": 1.0, "right": 2.0},
                                                         {"bottom": 1.0, "right": 2.0, "top": 3.0, "left": 4.0}]
    for walls in sets:
        Dw, l = op.form(walls)
        assert np.max(np.abs(Dw - Dw.T)) <= 1e-12 * scale, walls
        ev = np.linalg.eigvalsh(0.5 * (Dw + Dw.T))
        assert ev.max() < 0.0, walls  # no positive eigenvalue ...
        assert ev.max() < -1e-9 * scale, walls  # ... and a trivial null space: the constants are gone
        assert np.any(l != 0.0)
    ev0 = np.linalg.eigvalsh(0.5 * (op.D + op.D.T))
    assert np.sum(ev0 > -1e-9 * scale) == 1  # without a fixed side the constants stay


@pytest.mark.parametrize("kind,k", CASES)
def test_linear_profiles_are_steady_and_a_side_mix_up_is_seen(kind, k):
    op = operator(kind, k)
    x, y = _xy(op)
    scale = np.max(np.abs(op.D))
    if kind == "disk":
        cases = [(0.0 * x + 0.7, {"boundary": 0.7}, {"boundary": -0.7})]
    else:
        cases = [(1.0 - y, {"bottom": 1.0, "top": 0.0}, {"bottom": 0.0, "top": 1.0}),
                 (x, {"left": 0.0, "right": 1.0}, {"left": 1.0, "right": 0.0})]
    for q, walls, swapped in cases:
        Dw, l = op.form(walls)
        res = np.max(np.abs(Dw @ q + l))
        print(f"{kind} k={k} {walls}: residual {res:.3e} of {scale * np.max(np.abs(q)):.3e}")
        assert res <= 1e-10 * scale * np.max(np.abs(q))
        Ds, ls = op.form(swapped)
        assert np.max(np.abs(Ds @ q + ls)) > 1e-3 * scale * np.max(np.abs(q))  # the test sees which side is which
        flux = op.flux(walls, 1.0, q)
        if kind != "disk":  # the steady profile carries the flux kappa in at the warm side and out at the cold one
            hot, cold = [op.sides.index(s) for s, g in walls.items() if g == 1.0][0], [op.sides.index(s) for s, g in walls.items() if g == 0.0][0]
            assert abs(flux[hot] - 1.0) <= 1e-10 * scale and abs(flux[cold] + 1.0) <= 1e-10 * scale, flux


@pytest.mark.parametrize("kind,k", CASES)
def test_the_flux_is_the_form_against_one(kind, k):
    op = operator(kind, k)
    rng = np.random.default_rng(5 + k)
    q = rng.standard_normal(op.d.NP)  # broken
    walls = {"boundary": 0.4} if kind == "disk" else {"bottom": 1.0, "right": -0.5, "left": 0.25}
    Dw, l = op.form(walls)
    lhs = float(np.ones(op.d.NP) @ (Dw @ q + l))
    rhs = float(np.sum(op.flux(walls, 1.0, q)))
    scale = np.max(np.abs(op.D)) * np.max(np.abs(q))
    print(f"{kind} k={k}: 1^T (D q + D_w q + l) = {lhs!r}, sum of the fluxes {rhs!r}")
    assert abs(lhs - rhs) <= 1e-10 * scale
    A, b = op.minv(walls)  # and through M^-1: d/dt int q = the sum of the fluxes
    assert abs(ref.integral(op.d, A @ q + b) - rhs) <= 1e-10 * scale
    assert np.all(op.flux(walls, 1.0, q)[[op.sides.index(s) for s in op.sides if s not in walls]] == 0.0)


# ---- host tables
_EXE = {}


def _host_program(where):
    if "exe" not in _EXE:
        exe = where / "tracer_walls_check"
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "tracer_walls_check.cpp")], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


ALL_SUBSETS = list(range(1, 16))
CHOSEN = [0b0001, 0b1000, 0b0110, 0b1111]  # bottom; left; right + top; all four
MASKS = [(1, m) for m in ALL_SUBSETS] + [(k, m) for k in (2, 3, 4) for m in CHOSEN]


@pytest.mark.parametrize("k,mask", MASKS)
def test_host_tables_assemble_the_reference(tmp_path, k, mask):
    """Vol / Own / Nbr / Wall / wvec assembled over the 3x3 unit square as the kernel walks it, mapped to the nodal basis,
    against the reference entry by entry at 1e-11 max|entry|: the operator, the load vector and the flux functional of every
    fixed side; Lambda >= the spectral radius numpy computes."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = _host_program(tmp_path.parent)
    out = tmp_path / "op.bin"
    r = subprocess.run([str(exe), str(k), "3", str(mask), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    raw = np.fromfile(out)
    lam, n, wone = raw[0], int(raw[1]), raw[2]
    got = raw[3:3 + n * n].reshape(n, n)
    loads = raw[3 + n * n:3 + n * n + 4 * n].reshape(4, n)
    funs = raw[3 + n * n + 4 * n:].reshape(4, n)
    op = operator("square3", k)
    walls = {ref.SIDES[w]: 1.0 for w in range(4) if mask >> w & 1}
    A, _ = op.minv(walls)
    assert got.shape == A.shape
    dev = np.max(np.abs(got - A)) / np.max(np.abs(A))
    worst_l = worst_f = 0.0
    ncells_side = 3
    for w in range(4):
        if not mask >> w & 1:
            assert not loads[w].any() and not funs[w].any()
            continue
        l = op.terms[w][1]
        b = np.linalg.solve(op.M, l)  # the device adds M^-1 l
        worst_l = max(worst_l, np.max(np.abs(loads[w] - b)) / np.max(np.abs(b)))
        worst_f = max(worst_f, np.max(np.abs(funs[w] + l)) / np.max(np.abs(l)))  # the functional on q is - l
        assert abs(wone * ncells_side - float(l @ np.ones(n))) <= 1e-11 * wone * ncells_side  # its constant: g int_w eta_b
    rho = np.max(np.abs(np.linalg.eigvals(A)))
    print(f"k={k} mask={mask:04b}: operator {dev:.3e}, load {worst_l:.3e}, functional {worst_f:.3e} max|entry|; rho {rho:.6g}, Lambda {lam:.6g}")
    assert dev <= 1e-11 and worst_l <= 1e-11 and worst_f <= 1e-11
    assert lam >= rho
    assert lam <= 4.0 * rho  # an upper bound worth reporting


def test_general_assembly_header_compiles_alone_with_the_wall_arguments(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc")
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "hdg_general.hpp"\n'
                  "int main() {\n  const hdg::TracerDiffusionTables D(2, 0.5);\n  const bool all[4] = {true, true, true, true}, none[4] = {false, false, false, false};\n"
                  "  auto f = static_cast<hdg::Csr (*)(const hdg::GeneralTables&, const hdg::GMesh&, double&, std::vector<double>*, double*)>(&hdg::assemble_tracer_diffusion);\n"
                  "  return f != nullptr && D.lambda_walls(none) == D.lambda && D.lambda_walls(all) >= D.lambda && (int)D.packed_walls().size() == 2 * hdg::TracerDiffusionTables::wall_stride(D.np) ? 0 : 1;\n}\n")
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc, str(tu), "-o", str(tmp_path / "tu"), "-lpthread"], check=True)
    assert subprocess.run([str(tmp_path / "tu")]).returncode == 0


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_tracer_walls": "int hdg_set_tracer_walls(hdg_handle* h, int n, const int* kind, const double* value);",
    "hdg_get_tracer_wall_flux": "int hdg_get_tracer_wall_flux(hdg_handle* h, int n, double* flux);",
    "hdg_apply_tracer_wall_diffusion": "int hdg_apply_tracer_wall_diffusion(hdg_handle* h, const int kind[4], const double value[4], const double* q, double* out);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.TRACER_WALL_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_tracer_walls.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include"))) if f != "hdg_tracer_walls.h")
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES and name not in _lib.TRACER_DIFFUSION_SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert _lib.TRACER_WALL_SIGNATURES["hdg_set_tracer_walls"] == [h, C.c_int, ip, dp]
    assert _lib.TRACER_WALL_SIGNATURES["hdg_get_tracer_wall_flux"] == [h, C.c_int, dp]
    assert _lib.TRACER_WALL_SIGNATURES["hdg_apply_tracer_wall_diffusion"] == [h, ip, dp, dp, dp]
    assert _lib.TRACER_WALL_HEADER.endswith(os.path.join("include", "hdg_tracer_walls.h")) and os.path.isfile(_lib.TRACER_WALL_HEADER)
    assert _lib.WALL_SIDES == ref.SIDES
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13


class _Lib:
    """Stands in for the library: records the calls of the three entry points."""

    def __init__(self):
        self.calls = []

    def hdg_set_tracer_walls(self, h, n, kind, value):
        self.calls.append(("set", n, None if kind is None else np.ctypeslib.as_array(kind, (n * 4,)).copy(),
                           None if value is None else np.ctypeslib.as_array(value, (n * 4,)).copy()))
        return 0

    def hdg_get_tracer_wall_flux(self, h, n, flux):
        np.ctypeslib.as_array(flux, (n * 4,))[:] = np.arange(n * 4)
        return 0

    def hdg_apply_tracer_wall_diffusion(self, h, kind, value, q, out):
        self.calls.append(("apply", np.ctypeslib.as_array(kind, (4,)).copy(), np.ctypeslib.as_array(value, (4,)).copy()))
        np.ctypeslib.as_array(out, (6,))[:] = 2.0 * np.ctypeslib.as_array(q, (6,))
        return 0


def _stand_in(n_tracers, general=False):
    from incompressibleeulerhdg_amd import _lib

    eng = object.__new__(_lib.Engine)
    eng.lib, eng.h, eng.n_tracers, eng.general, eng.shape_p = _Lib(), None, n_tracers, general, (6,)
    eng._ck = lambda rc: None
    return eng


def test_python_surface_on_a_stand_in_engine():
    eng = _stand_in(2)
    assert eng.tracer_walls() is None
    eng.set_tracer_walls({"left": 0.5, "right": -0.5})  # one dict: every tracer
    _, n, kind, value = eng.lib.calls[-1]
    assert n == 2 and kind.tolist() == [0, 1, 0, 1] * 2 and value.tolist() == [0.0, -0.5, 0.0, 0.5] * 2
    assert eng.tracer_walls() == [{"right": -0.5, "left": 0.5}] * 2
    eng.set_tracer_walls([{"bottom": 1.0}, {}])  # a list: one dict per tracer, a missing side is no flux
    _, n, kind, value = eng.lib.calls[-1]
    assert kind.tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and value[0] == 1.0
    assert eng.tracer_walls() == [{"bottom": 1.0}, {}]
    eng.set_tracer_walls([{}, {}])  # no fixed side at all: off
    assert eng.tracer_walls() is None
    eng.set_tracer_walls({"top": 2.0})
    eng.set_tracer_walls(None)
    assert eng.lib.calls[-1] == ("set", 0, None, None) and eng.tracer_walls() is None
    for bad in ({"boundary": 1.0}, {"north": 1.0}):
        with pytest.raises(ValueError, match="unknown wall side"):
            eng.set_tracer_walls(bad)
    with pytest.raises(ValueError, match="sequence of 2 dicts"):
        eng.set_tracer_walls([{"top": 1.0}])
    assert eng.tracer_wall_flux().tolist() == [[0.0, 1.0, 2.0, 3.0], [4.0, 5.0, 6.0, 7.0]]
    out = eng.apply_tracer_wall_diffusion(np.arange(6.0), {"top": 3.0})
    assert out.tolist() == (2.0 * np.arange(6.0)).tolist()
    assert eng.lib.calls[-1][1].tolist() == [0, 0, 1, 0] and eng.lib.calls[-1][2].tolist() == [0.0, 0.0, 3.0, 0.0]
    gen = _stand_in(1, general=True)
    gen.set_tracer_walls({"boundary": 0.25})
    assert gen.lib.calls[-1][2].tolist() == [1, 0, 0, 0] and gen.tracer_walls() == [{"boundary": 0.25}]
    with pytest.raises(ValueError, match="unknown wall side 'left'"):  # a structured side name on a general mesh
        gen.set_tracer_walls({"left": 1.0})


def test_every_stepper_takes_tracer_walls():
    import inspect

    from incompressibleeulerhdg_amd import timesteppers as ts
    from incompressibleeulerhdg_amd.timesteppers import common

    src = inspect.getsource(common.IncompressibleEuler)
    assert 'engine_options.pop("tracer_walls", None)' in src
    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(cls.__init__).parameters.values()), cls


def test_cavity_is_fluid_at_rest():
    from incompressibleeulerhdg_amd.model_problems import Cavity

    mp = Cavity("V_Q", "V_p")
    Q0, p0 = mp.initial_condition()
    x, y = np.linspace(0, 1, 5), np.linspace(0, 1, 5) ** 2
    ux, uy = Q0(x, y)
    assert np.shape(ux) == x.shape and not np.any(ux) and not np.any(uy) and not np.any(p0(x, y))
    assert mp.f_rhs() is None and mp.solution(0.3) is None and (mp.V_Q, mp.V_p) == ("V_Q", "V_p")


# ---- driver
def test_driver_refuses_bad_walls_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.tracer_wall is None and driver.tracer_walls(args) is None
    driver.check_tracers(args)
    ok = ["--problem", "cavity", "--tracer_advection", "--tracer_diffusivity", "1e-3", "--tracer_wall", "left", "0.5", "--tracer_wall", "right", "-0.5"]
    args = driver.build_parser().parse_args(ok)
    driver.check_tracers(args)
    assert driver.tracer_walls(args) == [{"left": 0.5, "right": -0.5}]
    args = driver.build_parser().parse_args(["--tracer_advection", "--tracers", "3", "--tracer_wall", "bottom", "1", "--tracer_wall", "top", "2", "1"])
    assert driver.tracer_walls(args) == [{"bottom": 1.0}, {"bottom": 1.0, "top": 2.0}, {"bottom": 1.0}]
    args = driver.build_parser().parse_args(["--problem", "kelvinhelmholtz", "--tracer_advection", "--tracer_wall", "boundary", "1"])
    assert driver.tracer_walls(args) == [{"boundary": 1.0}]

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    with pytest.raises(RuntimeError, match="--tracer_wall needs --tracer_advection"):
        driver.main(["--tracer_wall", "left", "1"])
    with pytest.raises(RuntimeError, match="unknown side 'north'"):
        driver.main(["--tracer_advection", "--tracer_wall", "north", "1"])
    for bad in ("nan", "inf", "warm"):
        with pytest.raises(RuntimeError, match="is not a finite number"):
            driver.main(["--tracer_advection", "--tracer_wall", "left", bad])
    for t in ("2", "-1", "x"):
        with pytest.raises(RuntimeError, match=r"is not in 0 \.\. 1"):
            driver.main(["--tracer_advection", "--tracers", "2", "--tracer_wall", "left", "1", t])
    with pytest.raises(RuntimeError, match="SIDE VALUE"):
        driver.main(["--tracer_advection", "--tracer_wall", "left"])
    with pytest.raises(RuntimeError, match="--problem shear has no walls"):
        driver.main(["--problem", "shear", "--tracer_advection", "--tracer_wall", "left", "1"])
    with pytest.raises(RuntimeError, match="unknown side 'left' for --problem kelvinhelmholtz"):
        driver.main(["--problem", "kelvinhelmholtz", "--tracer_advection", "--tracer_wall", "left", "1"])
    with pytest.raises(RuntimeError, match="unknown side 'boundary'"):
        driver.main(["--tracer_advection", "--tracer_wall", "boundary", "1"])
    with pytest.raises(RuntimeError, match="--gpus 2 does not support --tracer_advection"):
        driver.main(["--gpus", "2", "--tracer_advection", "--tracer_wall", "left", "1"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(ok)


def test_walls_without_diffusivity_warn(monkeypatch):
    """The stepper warns that walls without kappa do nothing; with kappa it is silent (stand-in engine: no GPU)."""
    from incompressibleeulerhdg_amd.timesteppers import common

    class Eng:
        n_edges, n_l = 1, 1

        def __init__(self, **kw):
            self.calls = []

        def node_coordinates(self):
            return np.zeros((3, 2)), np.zeros((3, 2))

        def set_tracer_walls(self, w):
            self.calls.append("walls")

        def set_tracer_diffusivity(self, k):
            self.calls.append("kappa")

        def tracer_diffusion_number(self):
            self.calls.append("number")
            return 1.0, 0.1

    class Stepper(common.IncompressibleEuler):
        solve = None

    monkeypatch.setattr(common, "Engine", Eng)
    monkeypatch.setattr(common, "FunctionSpace", lambda *a, **k: type("V", (), {})())
    Stepper.__abstractmethods__ = frozenset()
    mesh = type("M", (), {"nx": 2, "ny": 2})()
    tab = dict(a_expl=[[0.0]], b_expl=[1.0])
    for kappa in (None, 0.0, [0.0, 0.0]):
        with pytest.warns(RuntimeWarning, match="the walls do nothing"):
            Stepper(mesh, 1, 0.1, tracer_walls={"left": 1.0}, tracer_diffusivity=kappa)._create_engine(**tab)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ts = Stepper(mesh, 1, 0.1, tracer_walls={"left": 1.0}, tracer_diffusivity=1e-3)
        eng = ts._create_engine(**tab)
        assert eng.calls == ["walls", "kappa", "number"]  # the walls first: the number then counts the wall blocks
        assert Stepper(mesh, 1, 0.1)._create_engine(**tab).calls == []  # tracer_walls=None: no call at all
