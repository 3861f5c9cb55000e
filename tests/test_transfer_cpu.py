"""Transfer between nested meshes on the CPU: the host tables (csrc/hdg_transfer.hpp through tests/host/transfer_check.cpp, g++
plain and with AddressSanitizer and UBSan), the numpy reference projection the GPU tests compare with, the C-ABI table of
include/hdg_transfer.h and the driver's --start_from options.  No GPU and no built library are needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import transfer_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_children_classes_and_tables(tmp_path, sanitize):
    """The stand-alone program over csrc/hdg_transfer.hpp alone, for r in {1, 2, 3, 16} and all pairs of degrees 1 .. 5: r^2
    children whose areas sum to the parent's and whose class map is their own geometry, Parseval whenever the fine degree
    is at least the coarse one, constants go to constants only, the scalar table is the leading block of the velocity
    table, upper-parent classes are the reflections of the lower-parent ones; 1e-15 absolute."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "transfer_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", str(exe),
                    os.path.join(HERE, "host", "transfer_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    worst = float(re.search(r"worst deviation (\S+)", r.stdout)[1])
    assert worst <= 1e-15


def test_transfer_header_compiles_alone_and_has_no_hip_behind_it(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc")
    text = open(os.path.join(csrc, "hdg_transfer.hpp")).read()
    assert "hip" not in text.split("#pragma once")[1].split("namespace hdg")[0]
    assert re.findall(r'#include "(\w+\.hpp)"', text) == ["hdg_tables.hpp"]
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "hdg_transfer.hpp"\n')
    subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-c", str(tu), "-o", str(tmp_path / "tu.o")], check=True)


def poly(deg, seed):
    """A global polynomial of total degree deg with seeded coefficients of size one: (x, y) -> values."""
    rng = np.random.default_rng(seed)
    coef = {(a, b): rng.uniform(-1, 1) for a in range(deg + 1) for b in range(deg + 1 - a)}
    return lambda x, y: sum(c * x ** a * y ** b for (a, b), c in coef.items())


@pytest.mark.parametrize("periodic", [False, True])
@pytest.mark.parametrize("src,dst", [((2, 1), (6, 1)), ((6, 2), (2, 3)), ((3, 3), (3, 1)), ((2, 4), (4, 2)), ((4, 1), (2, 4))])
def test_reference_reproduces_global_polynomials(src, dst, periodic):
    """The helper's own test: a global polynomial of degree <= min(k) (velocity: + 1) lies in both spaces, so its projection
    is itself -- to 1e-13 in both directions, prolongation, restriction and a change of degree."""
    L = 2.0 if periodic else 1.0
    for (a, b) in ((src, dst), (dst, src)):
        ea, eb = ref.evaluator(*a, L=L, periodic=periodic), ref.evaluator(*b, L=L, periodic=periodic)
        k = min(a[1], b[1])
        for which, deg in (("u", k + 1), ("p", k)):
            f = poly(deg, 7 * deg + a[0])
            xa, xb = ref.nodes(ea, which), ref.nodes(eb, which)
            got = ref.project(ea, eb, f(xa[:, 0], xa[:, 1]), which)
            want = f(xb[:, 0], xb[:, 1])
            assert np.max(np.abs(got - want)) <= 1e-13 * np.max(np.abs(want)), (a, b, which)
            assert ref.difference_norm(ea, eb, f(xa[:, 0], xa[:, 1]), want, which) <= 1e-13 * L * np.max(np.abs(want))


def test_reference_projection_is_orthogonal_and_keeps_means():
    """A restriction of broken random data: the defect is orthogonal to the coarse space (Pythagoras in the helper's own
    norms) and the integral of every component is kept."""
    rng = np.random.default_rng(3)
    fine, coarse = ref.evaluator(6, 2), ref.evaluator(2, 1)
    Q = rng.standard_normal((2 * 36 * fine.nu, 2))
    P = ref.project(fine, coarse, Q, "u")
    zero_f, zero_c = np.zeros_like(Q), np.zeros_like(P)
    n2 = ref.difference_norm(fine, coarse, Q, zero_c, "u") ** 2
    p2 = ref.difference_norm(coarse, fine, P, zero_f, "u") ** 2
    d2 = ref.difference_norm(fine, coarse, Q, P, "u") ** 2
    assert abs(n2 - p2 - d2) <= 1e-12 * n2


SIGNATURES_IN_C = {
    "hdg_transfer_state": "int hdg_transfer_state(hdg_handle* dst, const hdg_handle* src, int with_tracers);",
    "hdg_transfer_difference": "int hdg_transfer_difference(hdg_handle* a, hdg_handle* b, double* norm_Q, double* norm_p, double* norm_q);",
}


def test_c_abi_declares_the_transfer_entry_points_in_their_own_header():
    import ctypes as C

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.TRANSFER_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_transfer.h")).read()
    others = open(os.path.join(ROOT, "include", "hdg_mi355x.h")).read() + open(os.path.join(ROOT, "include", "hdg_checkpoint.h")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header, name
        assert name not in others and name not in _lib.SIGNATURES and name not in _lib.CHECKPOINT_SIGNATURES, name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp = C.c_void_p, C.POINTER(C.c_double)
    assert _lib.TRANSFER_SIGNATURES["hdg_transfer_state"] == [h, h, C.c_int]
    assert _lib.TRANSFER_SIGNATURES["hdg_transfer_difference"] == [h, h, dp, dp, dp]
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name in SIGNATURES_IN_C:
        assert re.search(rf"^int {name}\(", engine, re.M), name
    # the library is rebuilt when the new header changes
    assert _lib.TRANSFER_HEADER.endswith(os.path.join("include", "hdg_transfer.h")) and os.path.isfile(_lib.TRANSFER_HEADER)
    # the Python surface
    for name in ("transfer_from", "difference_norms"):
        assert callable(getattr(_lib.Engine, name))
    from incompressibleeulerhdg_amd.timesteppers.common import IncompressibleEuler

    for name in ("state_from", "difference"):
        assert callable(getattr(IncompressibleEuler, name))


def test_solve_signature_is_unchanged():
    import inspect

    from incompressibleeulerhdg_amd import timesteppers as ts

    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        p = list(inspect.signature(cls.solve).parameters)
        assert p[:7] == ["self", "Q_initial", "p_initial", "q_initial", "f_rhs", "T_final", "warmup"], cls
        assert p[-3:] == ["checkpoint", "checkpoint_every", "restart"], cls


def test_driver_parses_start_from_and_refuses_before_any_engine(tmp_path, monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert (args.start_from, args.start_nx, args.start_degree, args.start_dt) == (None, None, None, None)
    driver.check_start_from(args)
    there = tmp_path / "ck.bin"
    there.write_bytes(b"x")
    args = driver.build_parser().parse_args(["--problem", "shear", "--nx", "16", "--start_from", str(there), "--start_nx", "8",
                                             "--start_degree", "1", "--start_dt", "0.02"])
    assert (args.start_from, args.start_nx, args.start_degree, args.start_dt) == (str(there), 8, 1, 0.02)
    driver.check_start_from(args)  # the plain case is accepted
    driver.check_start_from(driver.build_parser().parse_args(["--problem", "shear", "--nx", "4", "--start_from", str(there),
                                                              "--start_nx", "64"]))  # restriction, r = 16

    # nothing below may start a rank or build an engine
    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    base = ["--problem", "shear", "--nx", "16", "--start_from", str(there)]
    with pytest.raises(RuntimeError, match="--start_from does not go with --problem taylorgreen"):
        driver.main(["--nx", "16", "--start_from", str(there)])
    with pytest.raises(RuntimeError, match="--start_from does not go with --problem kelvinhelmholtz"):
        driver.main(["--problem", "kelvinhelmholtz", "--start_from", str(there)])
    with pytest.raises(RuntimeError, match="--start_from does not go with --gpus 2"):
        driver.main(base + ["--gpus", "2"])
    with pytest.raises(RuntimeError, match="--start_from does not go with --restart"):
        driver.main(base + ["--restart", str(there)])
    with pytest.raises(RuntimeError, match="--start_from does not go with --warmup"):
        driver.main(base + ["--warmup"])
    with pytest.raises(RuntimeError, match="--start_from does not go with --test_pressure_solver"):
        driver.main(base + ["--test_pressure_solver"])
    with pytest.raises(RuntimeError, match=r"--start_from: no checkpoint file .*missing\.bin"):
        driver.main(["--problem", "shear", "--nx", "16", "--start_from", str(tmp_path / "missing.bin")])
    for nx0 in ("6", "24", "0", "512"):  # no integer ratio, or a ratio beyond 16
        with pytest.raises(RuntimeError, match=rf"--start_nx {nx0} and --nx 16 are not nested"):
            driver.main(base + ["--start_nx", nx0])
    with pytest.raises(RuntimeError, match="--start_nx needs --start_from"):
        driver.main(["--problem", "shear", "--start_nx", "8"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(base + ["--start_nx", "8", "--start_degree", "1"])
