"""driver.py --gpus N: the strip partition from the command line.  The refusals are checked on the CPU (no process may be
started); the runs themselves (two ranks sharing the test GPU over the shared-memory transport) against --gpus 1."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.mark.parametrize("extra", [
    ["--tracer_advection"],
    ["--animation"],
    ["--test_pressure_solver"],
    ["--discretisation", "dg", "--timestepper", "implicit"],
    ["--problem", "kelvinhelmholtz"],
    ["--nx", "9"],
    ["--problem", "shear", "--nx", "10", "--gpus", "4"],
])
def test_driver_refuses_before_starting_ranks(monkeypatch, extra):
    from incompressibleeulerhdg_amd import driver

    def no_child(*a, **k):
        raise AssertionError("a child process was started")

    monkeypatch.setattr(subprocess, "call", no_child)
    monkeypatch.setattr(subprocess, "run", no_child)
    monkeypatch.setattr(subprocess, "Popen", no_child)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    argv = ["--gpus", "2"] + extra
    with pytest.raises(RuntimeError, match="does not support"):
        driver.main(argv)


def test_driver_gpus_option_defaults_to_one():
    from incompressibleeulerhdg_amd import driver

    assert driver.build_parser().parse_args([]).gpus == 1
    with pytest.raises(RuntimeError, match="at least 1"):
        driver.check_multi_gpu(driver.build_parser().parse_args(["--gpus", "0"]))


def _driver(args, cwd):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


def _csv(path):
    lines = path.read_text().strip().splitlines()
    return lines[0], np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])


@pytest.mark.gpu
def test_driver_gpus_shear_layer(hip_lib, tmp_path):
    nx = 32
    dt = 0.25 * 2 * np.pi / nx
    base = ["--problem", "shear", "--nx", str(nx), "--degree", "2", "--dt", repr(dt), "--tfinal", repr(2 * dt),
            "--diagnostics", "f.csv", "--output", "o.pvd"]
    d1, d2 = tmp_path / "one", tmp_path / "two"
    d1.mkdir()
    d2.mkdir()
    out1 = _driver(base + ["--gpus", "1"], d1)
    out2 = _driver(base + ["--gpus", "2"], d2)
    # rank 0 alone prints: the same lines once
    assert out2.count("model problem = shear") == 1 and out2.count("solver events") == 1, out2[-2000:]
    h1, r1 = _csv(d1 / "f.csv")
    h2, r2 = _csv(d2 / "f.csv")
    assert h1 == h2 and r1.shape == r2.shape == (3, 11)
    names = h1.split(",")[2:]
    unorm = np.sqrt(2 * r1[0, 2])
    for i, c in enumerate(names):
        a, b = r2[:, 2 + i], r1[:, 2 + i]
        if c.startswith("tracer"):
            assert np.all(np.isnan(a)) and np.all(np.isnan(b))
            continue
        atol = 1e-10 * unorm if c in ("div_l2", "jump_l2", "p_integral") else 0.0
        assert np.allclose(a, b, rtol=1e-11, atol=atol), (c, a, b)
    # one collection, one piece with the global cell count
    assert sorted(os.listdir(d2)) == ["f.csv", "o.pvd", "o_0.vtu"]
    vtu = (d2 / "o_0.vtu").read_text()
    assert f'NumberOfCells="{2 * nx * nx}"' in vtu
    assert (d1 / "o_0.vtu").read_text().count("DataArray") == vtu.count("DataArray")


@pytest.mark.gpu
def test_driver_gpus_taylor_green(hip_lib, tmp_path):
    base = ["--nx", "16", "--degree", "2", "--dt", "0.0125", "--tfinal", "0.025", "--use_projection_method", "--output", ""]
    out1 = _driver(base + ["--gpus", "1"], tmp_path)
    out2 = _driver(base + ["--gpus", "2"], tmp_path)

    def errors(out):
        return [float(re.search(rf"{w} error = ([0-9.eE+-]+)", out).group(1)) for w in ("velocity", "pressure")]

    e1, e2 = errors(out1), errors(out2)
    assert np.allclose(e2, e1, rtol=1e-9, atol=0), (e1, e2)
    assert out2.count("velocity error") == 1
