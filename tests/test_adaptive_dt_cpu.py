"""Adaptive time step on the CPU: the rule of csrc/hdg_step_control.hpp through
tests/host/step_control_check.cpp (g++ with AddressSanitizer and UBSan, no GPU) against the numpy twin bit for bit, the C-ABI
table of include/hdg_adaptive_dt.h, the Python surface, and the refusals of solve and of the driver.  No GPU and no built library
are needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import adaptive_dt_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    """The lines of the host program: (twelve inputs, verdict, proposal)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("step_control") / "step_control_check"
    subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "step_control_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == f"{len(lines) - 1} cases"
    rows = []
    for ln in lines[:-1]:
        left, right = ln.split(" -> ")
        verdict, p = right.split()
        rows.append(([float.fromhex(w) if w not in ("nan", "-nan", "inf") else float(w.lstrip("-")) for w in left.split()], verdict, p))
    return rows


def _bits(x):
    return np.float64(x).view(np.uint64)


def test_the_twin_reproduces_every_proposal_of_the_host_rule_bit_for_bit(table):
    seen = set()
    for inputs, verdict, word in table:
        cfl, dt_min, dt_max, grow, band, c0, c1, c2, A, dt, t, tf = inputs
        v, p = ref.propose(A, dt, t, tf, cfl, dt_min, dt_max, grow, band, (c0, c1, c2))
        assert v == verdict, (inputs, v, verdict)
        if "nan" in word:
            assert np.isnan(p), inputs
        else:
            assert _bits(p) == _bits(float.fromhex(word)), (inputs, p, word)
        seen.add(verdict)
    assert seen == {"ok", "below_min", "not_finite", "bad_control"}


def test_the_table_covers_the_branches_of_the_rule(table):
    """What the cases are there for, stated on the printed values themselves"""
    rows = {tuple(i): (v, float.fromhex(w) if "nan" not in w else float("nan")) for i, v, w in table}
    dt, b1 = 0.01, 1.0 + 0.1
    get = lambda *i: rows[tuple(float(x) for x in i)]
    inf, nan = float("inf"), float("nan")
    assert get(0.3, 0, 0, 0, 0, 0, 0, 0, 0.0, dt, 0, 1) == ("ok", 1.25 * dt)  # A = 0: cfl / A = inf, the growth limit decides
    assert get(0.3, 0, 0.02, 0, 0, 0, 0, 0, 0.0, 0.019, 0, 1) == ("ok", 0.019)  # A = 0 and dt_max inside the band: dt stays
    assert get(0.3, 0, 0, 0, 0, 0, 0, 0, 1e-300, dt, 0, 1) == ("ok", 1.25 * dt)
    assert get(0.3, 0, 0, 0, 0, 0, 0, 0, 4.9e-324, dt, 0, 1) == ("ok", 1.25 * dt)  # cfl / A overflows to inf
    for A in (inf, -1.0):
        assert get(0.3, 0, 0, 0, 0, 0, 0, 0, A, dt, 0, 1)[0] == "not_finite"
    assert [v for i, (v, p) in rows.items() if np.isnan(i[8])] == ["not_finite"]
    assert get(0.3, 0, 0, 0, 0, 0, 0, 0, 70.0, dt, 0, 1) == ("ok", 0.3 / 70.0)
    assert get(0.3, 0, 0, 0, 0, 0, 0, 0, 25.0, dt, 0, 1) == ("ok", 0.3 / 25.0)
    assert get(0.3, 0, 0, 2.0, 0, 0, 0, 0, 3.0, dt, 0, 1) == ("ok", 2.0 * dt)
    # the band: [dt, (1 + band) dt] keeps dt, one double outside does not
    assert get(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0, 1) == ("ok", dt)
    assert get(0.3, 0, np.nextafter(dt, 0), 0, 0, 0, 0, 0, 1.0, dt, 0, 1) == ("ok", np.nextafter(dt, 0))
    assert get(0.3, 0, b1 * dt, 0, 0, 0, 0, 0, 1.0, dt, 0, 1) == ("ok", dt)
    assert get(0.3, 0, np.nextafter(b1 * dt, 1), 0, 0, 0, 0, 0, 1.0, dt, 0, 1) == ("ok", np.nextafter(b1 * dt, 1))
    assert get(0.3, 0, 0.0105, 0, 0.01, 0, 0, 0, 1.0, dt, 0, 1) == ("ok", 0.0105)
    # caps and dt_max in turn
    for caps in ((0.004, 0.005, 0.006), (0.005, 0.004, 0.006), (0.006, 0.005, 0.004)):
        assert get(0.3, 0, 1.0, 0, 0, *caps, 1.0, dt, 0, 1) == ("ok", 0.004)
    assert get(0.3, 0, 0.003, 0, 0, 0.006, 0.005, 0.004, 1.0, dt, 0, 1) == ("ok", 0.003)
    assert get(0.3, 0, 1.0, 0, 0, inf, 0.0121, inf, 1.0, dt, 0, 1) == ("ok", 0.0121)
    # dt_min
    assert get(0.3, 0.005, 0, 0, 0, 0, 0, 0, 100.0, dt, 0, 1) == ("below_min", 0.003)
    assert get(0.3, 0.003, 0, 0, 0, 0, 0, 0, 100.0, dt, 0, 1) == ("ok", 0.003)
    assert get(0.3, 0.005, 0, 0, 0, 0, 0, 0, 1.0, dt, 0.999, 1) == ("ok", 1.0 - 0.999)  # landing is not a violation
    # landing, including t_final - t equal to the proposal
    assert get(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.995, 1) == ("ok", 1.0 - 0.995)
    assert get(0.3, 0, 0.25, 0, 0, 0, 0, 0, 0.0, 0.25, 0.75, 1) == ("ok", 0.25)
    assert get(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 0.5, 1) == ("ok", dt)
    assert get(0.3, 0, dt, 0, 0, 0, 0, 0, 1.0, dt, 1.0, 1) == ("ok", 0.0)


def test_replay_lands_on_t_final():
    """The loop of the steppers with the twin: a rate that doubles half way; the steps sum to t_final"""
    rates = [10.0] * 40 + [25.0] * 400
    dts, props = ref.replay(rates, 0.02, 1.0, cfl=0.3, dt_max=0.05)
    assert abs(dts.sum() - 1.0) <= 1e-12 and len(dts) == len(props)
    assert dts[0] == 0.025 and dts.max() == 0.3 / 10.0 and np.all(dts[45:-1] == 0.3 / 25.0)
    assert np.all(dts[1:] <= 1.25 * dts[:-1] * (1 + 1e-15))


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_dt": "int hdg_set_dt(hdg_handle* h, double dt);",
    "hdg_get_dt": "int hdg_get_dt(const hdg_handle* h, double* dt);",
    "hdg_get_step_rates": "int hdg_get_step_rates(hdg_handle* h, double rates[4]);",
    "hdg_step_proposal": "int hdg_step_proposal(const hdg_step_control* control, double A, double dt, double t, double t_final, double* dt_new);",
    "hdg_propose_dt": "int hdg_propose_dt(hdg_handle* h, const hdg_step_control* control, double t, double t_final, double* dt_new);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.ADAPTIVE_DT_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_adaptive_dt.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include")))
                     if f != "hdg_adaptive_dt.h")
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    h, dp = C.c_void_p, C.POINTER(C.c_double)
    assert _lib.ADAPTIVE_DT_SIGNATURES["hdg_set_dt"] == [h, C.c_double]
    assert _lib.ADAPTIVE_DT_SIGNATURES["hdg_get_step_rates"] == [h, dp]
    assert _lib.ADAPTIVE_DT_SIGNATURES["hdg_propose_dt"] == [h, C.POINTER(_lib.hdg_step_control), C.c_double, C.c_double, dp]
    assert [f[0] for f in _lib.hdg_step_control._fields_] == ["cfl", "dt_min", "dt_max", "grow", "band", "caps"]
    assert C.sizeof(_lib.hdg_step_control) == 8 * 8
    fields = re.search(r"typedef struct hdg_step_control \{(.*?)\} hdg_step_control;", header, re.S).group(1)
    assert re.findall(r"double (\w+)", fields) == ["cfl", "dt_min", "dt_max", "grow", "band", "caps"]
    assert _lib.ADAPTIVE_DT_HEADER.endswith(os.path.join("include", "hdg_adaptive_dt.h")) and os.path.isfile(_lib.ADAPTIVE_DT_HEADER)
    for name in ("set_dt", "get_dt", "step_rates", "propose_dt"):
        assert callable(getattr(_lib.Engine, name))
    c = _lib.step_control(0.3, dt_max=0.5, caps=[None, 0.25, None])
    assert (c.cfl, c.dt_min, c.dt_max, c.grow, c.band, list(c.caps)) == (0.3, 0.0, 0.5, 0.0, 0.0, [0.0, 0.25, 0.0])
    assert _lib.hdg_config._fields_[-1][0] == "n_tracers" and len(_lib.Engine.LAUNCH_CLASSES) == 13


def test_the_rule_header_is_plain_cxx(tmp_path):
    """csrc/hdg_step_control.hpp compiles on its own with g++ -Wall -Wextra -Werror: no HIP header behind it"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    csrc = os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc")
    src = open(os.path.join(csrc, "hdg_step_control.hpp")).read()
    assert "hip" not in src.split("#pragma once")[1].split("namespace hdg")[0]
    tu = tmp_path / "tu.cpp"
    tu.write_text('#include "hdg_step_control.hpp"\n')
    subprocess.run([shutil.which("g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc, "-c", str(tu), "-o", str(tmp_path / "tu.o")], check=True)


def test_the_diagnostics_and_the_rate_kernels_share_the_per_cell_piece():
    """cell_max_speed is defined once and called by the diagnostics cell pass and by both rate kernels (source check; the
    diagnostics tests on the GPU check that the rows are what they were)"""
    csrc = os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc")
    rate, diag = open(os.path.join(csrc, "hdg_step_rate.hpp")).read(), open(os.path.join(csrc, "hdg_diagnostics.hpp")).read()
    assert rate.count("double cell_max_speed(") == 1 and "cell_max_speed(" not in diag.replace("cell_max_speed<K, false>(", "")
    assert diag.count("cell_max_speed<K, false>(") == 1 and rate.count("cell_max_speed<K, true>(") == 2
    assert "__dmul_rn" not in diag and '#include "hdg_step_rate.hpp"' in diag


# ---- solve and the driver refuse before anything runs
class _Stub:
    """A stepper without an engine: _step_controller reads _dt only"""
    from incompressibleeulerhdg_amd.timesteppers.common import IncompressibleEuler as _Base

    _dt = 0.01
    check = _Base._step_controller


def test_solve_checks_its_adaptive_keywords():
    chk = lambda **kw: _Stub().check(kw.pop("T", 1.0), kw.pop("warmup", False), kw.pop("checkpoint", None), kw.pop("restart", None),
                                     kw.pop("cfl", None), kw.pop("dt_min", None), kw.pop("dt_max", None), kw.pop("adapt_every", 1),
                                     kw.pop("max_steps", None))
    assert chk() is None
    assert chk(cfl=0.3) == (1, 1000, 0.0, 0.01)  # dt_max: the constructor's dt; max_steps: 10 ceil(T / dt)
    assert chk(cfl=0.3, dt_max=0.05, dt_min=1e-4, adapt_every=4, max_steps=77) == (4, 77, 1e-4, 0.05)
    assert chk(cfl=0.3, warmup=True) is None  # the one step of a warm-up run is the constructor's
    for bad in (0, -0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cfl must be a finite number > 0"):
            chk(cfl=bad)
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="adapt_every must be an integer >= 1"):
            chk(cfl=0.3, adapt_every=bad)
    with pytest.raises(ValueError, match="max_steps must be an integer >= 1"):
        chk(cfl=0.3, max_steps=0)
    for kw in ({"checkpoint": "c.bin"}, {"restart": "c.bin"}):
        with pytest.raises(ValueError, match="cfl= does not go with checkpoint= or restart="):
            chk(cfl=0.3, **kw)
    for kw in ({"dt_min": 0.02}, {"dt_min": -1.0}, {"dt_max": 0.0}, {"dt_max": float("nan")}):
        with pytest.raises(ValueError, match="0 <= dt_min <= dt_max"):
            chk(cfl=0.3, **kw)
    for kw in ({"dt_min": 1e-3}, {"dt_max": 0.1}, {"max_steps": 5}, {"adapt_every": 2}):
        with pytest.raises(ValueError, match="needs cfl="):
            chk(**kw)


def test_solve_takes_the_adaptive_keywords_on_every_family():
    import inspect

    from incompressibleeulerhdg_amd import timesteppers as ts

    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        p = inspect.signature(cls.solve).parameters
        assert [p[n].default for n in ("cfl", "dt_min", "dt_max", "adapt_every", "max_steps")] == [None, None, None, 1, None], cls
        assert list(p)[-3:] == ["checkpoint", "checkpoint_every", "restart"], cls


def test_driver_parses_the_adaptive_options_and_refuses_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.cfl is None and driver.adaptive_keywords(args) == {}
    args = driver.build_parser().parse_args(["--cfl", "0.5", "--dt_min", "1e-4", "--dt_max", "0.1", "--adapt_every", "3", "--max_steps", "50"])
    assert driver.adaptive_keywords(args) == {"cfl": 0.5, "dt_min": 1e-4, "dt_max": 0.1, "adapt_every": 3, "max_steps": 50}
    assert driver.adaptive_keywords(driver.build_parser().parse_args(["--cfl", "0.5"])) == {"cfl": 0.5}

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(RuntimeError, match="--cfl must be a finite number > 0"):
            driver.main(["--cfl", bad])
    with pytest.raises(RuntimeError, match="--adapt_every must be at least 1"):
        driver.main(["--cfl", "0.5", "--adapt_every", "0"])
    with pytest.raises(RuntimeError, match="--max_steps must be at least 1"):
        driver.main(["--cfl", "0.5", "--max_steps", "0"])
    with pytest.raises(RuntimeError, match="0 <= dt_min <= dt_max"):
        driver.main(["--cfl", "0.5", "--dt_min", "1"])
    with pytest.raises(RuntimeError, match="--cfl does not go with --checkpoint: a checkpoint carries the step size"):
        driver.main(["--cfl", "0.5", "--checkpoint", "c.bin"])
    with pytest.raises(RuntimeError, match="--cfl does not go with --test_pressure_solver"):
        driver.main(["--cfl", "0.5", "--test_pressure_solver"])
    for name in ("dt_min", "dt_max", "adapt_every", "max_steps"):
        with pytest.raises(RuntimeError, match=f"--{name} needs --cfl"):
            driver.main([f"--{name}", "1"])
    for argv in (["--cfl", "0.5"], ["--cfl", "0.5", "--gpus", "2"]):  # a request that is fine does go on
        with pytest.raises(AssertionError, match="too late"):
            driver.main(argv)
