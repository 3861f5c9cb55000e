"""Point values on the CPU: the host / device basis and the bucket locator (tests/host/point_basis_check.cpp, g++), the numpy
checker tests/probe_reference.py on closed forms, the ownership rule against csrc/hdg_points.hpp, and the driver's --probes
parsing."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import fem
import probe_reference as pr

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("pbc") / "point_basis_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-pthread", "-o", str(exe), os.path.join(HERE, "host", "point_basis_check.cpp")],
                   check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([str(exe), *map(str, args)], check=True, capture_output=True, text=True).stdout
    assert "error" not in out, out
    return out


def test_point_basis_matches_dubiner_eval(check_exe):
    v = dict(ln.split() for ln in _run(check_exe, "basis").strip().splitlines())
    assert int(v["basis_points"]) > 400
    assert float(v["basis_max_err"]) < 1e-13


def test_bucket_locator_matches_brute_force_on_the_level4_disk(check_exe, tmp_path):
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh

    m = UnitDiskMesh(4)
    path = tmp_path / "disk4.txt"
    with open(path, "w") as f:
        f.write(f"{len(m.vertices)} {len(m.cells)}\n")
        np.savetxt(f, m.vertices, fmt="%.17g")
        np.savetxt(f, m.cells, fmt="%d")
    v = dict(ln.split() for ln in _run(check_exe, "locate", path).strip().splitlines())
    assert int(v["locate_mismatch"]) == 0
    assert int(v["locate_outside"]) > 1000 and int(v["locate_inside"]) > 10000


def _special_points(nx, L):
    h = L / nx
    g = np.arange(nx + 1) * h
    pts = [(x, y) for x in g for y in g]                                           # vertices
    pts += [(x + 0.5 * h, y) for x in g[:-1] for y in g] + [(x, y + 0.5 * h) for x in g for y in g[:-1]]  # edges
    pts += [(x + t * h, y + (1 - t) * h) for x in g[:-1] for y in g[:-1] for t in (0.25, 0.5)]  # diagonals
    return pts


@pytest.mark.parametrize("periodic", [False, True])
def test_ownership_rule_matches_the_engine_rule(check_exe, tmp_path, periodic):
    nx, L = 4, (2 * np.pi if periodic else 1.0)
    pts = _special_points(nx, L)
    e = 1e-13 * L
    pts += [(-e, 0.3), (L + e, 0.3), (0.3, -e), (0.3, L + e), (-e, -e), (L + e, L + e)]  # clamped on the unit square
    d = 1e-9 * L
    pts += [(-d, 0.3), (L + d, 0.3), (0.3, -d), (0.3, L + d)]                             # outside the unit square
    pts += [(L, 0.5), (0.5, L), (L, L), (-L, 0.25), (3 * L + 0.1, -2 * L + 0.2), (np.nextafter(L, 0), 0.1)]  # seam
    path = tmp_path / "pts.txt"
    np.savetxt(path, np.array(pts), fmt="%.17g")
    got = {}
    for ln in _run(check_exe, "square", nx, nx, repr(L), int(periodic), path).strip().splitlines():
        f = ln.split()
        got[int(f[1])] = None if f[2] == "out" else (int(f[2]), int(f[3]), int(f[4]))
    assert len(got) == len(pts)
    for t, (x, y) in enumerate(pts):
        o = pr.owner_square(x, y, nx, nx, L, periodic)
        assert (None if o is None else o[:3]) == got[t], (t, x, y)
    # the documented cases
    h = L / nx
    assert pr.owner_square(h, h, nx, nx, L, periodic)[:3] == (1, 1, 0)             # a vertex: the cell above-right, lower
    assert pr.owner_square(0.5 * h, 0.5 * h, nx, nx, L, periodic)[:3] == (0, 0, 0)  # the diagonal: the lower triangle
    assert pr.owner_square(0.5 * h, h, nx, nx, L, periodic)[:3] == (0, 1, 0)        # a horizontal edge: the row above
    if periodic:
        assert pr.owner_square(L, L, nx, nx, L, True)[:3] == (0, 0, 0)             # the seam wraps to 0
        assert pr.owner_square(-0.5 * h, 0.25 * h, nx, nx, L, True)[:3] == (nx - 1, 0, 0)
    else:
        assert pr.owner_square(L, L, nx, nx, L, False)[:3] == (nx - 1, nx - 1, 1)  # the corner: the last cell
        assert pr.owner_square(-1e-13, 0.5, nx, nx, L, False) is not None
        assert pr.owner_square(-1e-9, 0.5, nx, nx, L, False) is None


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("mesh_kind", ["square", "periodic", "disk"])
def test_reference_evaluator_reproduces_polynomials(k, mesh_kind):
    if mesh_kind == "disk":
        m = fem.unit_disk_mesh(2)
        ev_kw = dict(general=(m.vertices, m.cells))
    else:
        periodic = mesh_kind == "periodic"
        m = fem.Mesh(3, periodic=periodic, L=2.0 if periodic else 1.0)
        ev_kw = dict(square=(3, 3, m.L, periodic))
    xq, xp = pr.node_coordinates(m, k + 1), pr.node_coordinates(m, k)
    ev = pr.PointEvaluator(k, xq, **ev_kw)
    a = np.arange(1.0, 20.0)
    ux = lambda x, y: a[0] + a[1] * x ** (k + 1) + a[2] * x * y ** k + a[3] * y  # noqa: E731  degree k + 1
    uy = lambda x, y: a[4] * x - a[5] * y ** (k + 1) + a[6] * x ** k * y  # noqa: E731
    curl = lambda x, y: a[4] + k * a[6] * x ** (k - 1) * y - k * a[2] * x * y ** (k - 1) - a[3]  # noqa: E731
    pf = lambda x, y: 0.5 + x ** k - 2 * y ** k + x * y ** (k - 1)  # noqa: E731  degree k
    Q = np.stack([ux(*xq.T), uy(*xq.T)], axis=1)
    rng = np.random.default_rng(k)
    if mesh_kind == "disk":
        r, th = 0.9 * np.sqrt(rng.random(60)), 2 * np.pi * rng.random(60)
        xy = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
    else:
        xy = rng.random((60, 2)) * m.L
    vals, located = ev.evaluate(xy, Q, pf(*xp.T), 2 * pf(*xp.T))
    assert located.all()
    x, y = xy.T
    scale = 1.0 + np.abs(vals)
    for col, ref in ((0, ux(x, y)), (1, uy(x, y)), (2, pf(x, y)), (3, 2 * pf(x, y)), (4, curl(x, y))):
        assert np.max(np.abs(vals[:, col] - ref) / scale[:, col]) < 1e-12, col
    # a linear velocity with known curl, and NaN columns for fields not given
    vals, _ = ev.evaluate(xy, np.stack([2 * xq[:, 0] - 3 * xq[:, 1], 5 * xq[:, 0] + xq[:, 1]], axis=1))
    assert np.allclose(vals[:, 4], 8.0, rtol=0, atol=1e-12)
    assert np.isnan(vals[:, 2:4]).all()


def test_reference_evaluator_outside_points_are_nan():
    m = fem.unit_disk_mesh(2)
    ev = pr.PointEvaluator(1, pr.node_coordinates(m, 2), general=(m.vertices, m.cells))
    vals, located = ev.evaluate([[0.0, 0.0], [0.99, 0.99], [0.999 * np.cos(0.3), 0.999 * np.sin(0.3)]],
                                np.zeros((len(m.cells) * 6, 2)))
    assert located.tolist() == [True, False, False]  # the last one: inside the circle, outside the polygon
    assert np.isnan(vals[1:]).all() and not np.isnan(vals[0, :2]).any()


def test_driver_parses_probe_options_and_reads_points(tmp_path):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.probes is None and args.probe_output == "probes.csv"
    args = driver.build_parser().parse_args(["--probes", "pts.txt", "--probe_output", "out.csv"])
    assert args.probes == "pts.txt" and args.probe_output == "out.csv"
    path = tmp_path / "pts.txt"
    path.write_text("# probe points\n\n0.25 0.5\n  0.75   0.125  # second\n#0.1 0.1\n1e-1 2E-1\n")
    xy, lines = driver.read_probe_points(str(path))
    assert xy.tolist() == [[0.25, 0.5], [0.75, 0.125], [0.1, 0.2]]
    assert lines == [3, 4, 6]
    path.write_text("0.1 0.2\n0.3\n")
    with pytest.raises(RuntimeError, match=":2:"):
        driver.read_probe_points(str(path))
