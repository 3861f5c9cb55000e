"""Lagrangian particles on the CPU: the numpy checker tests/particle_reference.py on closed forms, the host / device ownership
rule against its host-only form (tests/host/particle_locate_check.cpp, g++), the C-ABI table and the driver's options."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import particle_reference as par

HERE = os.path.dirname(os.path.abspath(__file__))


def _rotation(c):
    return lambda step, xy: np.stack([-(xy[:, 1] - c), xy[:, 0] - c], axis=1)


def test_reference_integrator_is_second_order_on_a_rigid_rotation():
    c, T = 0.5, 1.0
    xy0 = np.array([[0.7, 0.5], [0.5, 0.85], [0.3, 0.4], [0.55, 0.45]])
    R = np.array([[np.cos(T), -np.sin(T)], [np.sin(T), np.cos(T)]])
    exact = (xy0 - c) @ R.T + c
    errs = []
    for nt in (20, 40, 80, 160):
        rows, nclamp, _ = par.heun(_rotation(c), xy0, T / nt, nt)
        assert rows.shape == (nt + 1, len(xy0), 2) and nclamp == 0 and np.array_equal(rows[0], xy0)
        errs.append(np.max(np.abs(rows[-1] - exact)))
    rates = np.log2(np.array(errs[:-1]) / np.array(errs[1:]))
    assert np.all(np.abs(rates - 2.0) < 0.1), (errs, rates)
    # one step is the linear map I + dt J + dt^2 J^2 / 2 of the rotation's generator J
    dt = 0.1
    J = np.array([[0.0, -1.0], [1.0, 0.0]])
    M = np.eye(2) + dt * J + 0.5 * dt * dt * J @ J
    rows, _, _ = par.heun(_rotation(c), xy0, dt, 3)
    assert np.max(np.abs(rows[3] - ((xy0 - c) @ np.linalg.matrix_power(M, 3).T + c))) < 1e-15


def test_reference_integrator_clamps_and_measures_edge_margins():
    uniform = lambda step, xy: np.tile([1.0, 0.5], (len(xy), 1))  # noqa: E731
    rows, nclamp, margins = par.heun(uniform, [[0.9, 0.2], [0.1, 0.1]], 0.25, 2, L=1.0, square=(4, 1.0, False))
    assert np.array_equal(rows[-1], [[1.0, 0.45], [0.6, 0.35]]) and nclamp == 4  # the first particle: X* and X, twice
    assert margins.shape == (4, 2)
    assert margins[0, 0] == pytest.approx(min(0.4, 0.2, abs(0.6 + 0.8 - 1) / np.sqrt(2)))  # (0.9, 0.2) in cell (3, 0)
    assert margins[1, 0] == 0.0  # X* of the first particle sits on the boundary
    m = par.edge_margin([[0.25, 0.3], [0.3, 0.2], [7.0 + 0.125, -3.0 + 0.0625]], 4, 1.0, True)
    assert m[0] == 0.0 and m[1] == pytest.approx(0.0, abs=1e-15) and m[2] == pytest.approx(0.25 / np.sqrt(2))  # fx = 0.5, fy = 0.25: the diagonal
    rows, nclamp, _ = par.heun(uniform, [[0.9, 0.2]], 0.25, 8)  # no clamping: unwrapped positions
    assert nclamp == 0 and np.allclose(rows[-1], [[2.9, 1.2]], rtol=0, atol=1e-15)


@pytest.mark.parametrize("periodic", [False, True])
def test_host_device_ownership_rule_locates_as_before(tmp_path, periodic):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "particle_locate_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-o", str(exe), os.path.join(HERE, "host", "particle_locate_check.cpp")],
                   check=True)
    for nx, L in ((6, 1.0), (24, 2 * np.pi)):
        out = subprocess.run([str(exe), str(nx), repr(L), str(int(periodic))], check=True, capture_output=True, text=True).stdout
        v = dict(ln.split() for ln in out.strip().splitlines())
        assert "error" not in v
        assert int(v["locate_points"]) >= 100000 and int(v["locate_special"]) > 1000
        assert int(v["locate_located"]) > (90000 if periodic else 5000)
        assert int(v["locate_mismatch"]) == 0


def test_c_abi_declares_the_particle_entry_points():
    from incompressibleeulerhdg_amd import _lib

    for name in ("hdg_set_particles", "hdg_get_particles", "hdg_advance_particles"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES) + 1 == 65  # hdg_last_error has a signature of its own
    header = open(os.path.join(os.path.dirname(HERE), "include", "hdg_mi355x.h")).read()
    assert "int hdg_set_particles(hdg_handle* h, int n, const double* xy, int capacity, int record_every);" in header


def test_driver_parses_particle_options_and_refuses_the_disk(tmp_path):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.particles is None and args.particle_output == "particles.npz" and args.particle_every == 1
    args = driver.build_parser().parse_args(["--particles", "p.txt", "--particle_output", "o.npz", "--particle_every", "3"])
    assert (args.particles, args.particle_output, args.particle_every) == ("p.txt", "o.npz", 3)
    driver.check_particles(args)
    # refused before any engine is built (no GPU and no library are needed to get here)
    with pytest.raises(RuntimeError, match="--particles does not support --problem kelvinhelmholtz"):
        driver.main(["--problem", "kelvinhelmholtz", "--particles", str(tmp_path / "none.txt")])
    with pytest.raises(RuntimeError, match="--particle_every"):
        driver.main(["--problem", "shear", "--particles", "p.txt", "--particle_every", "0"])
    driver.check_particles(driver.build_parser().parse_args(["--problem", "kelvinhelmholtz"]))  # without particles: fine
