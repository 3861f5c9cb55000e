"""The CPU reference of the flow diagnostics (tests/diagnostics_reference.py) on closed forms."""
import numpy as np
import pytest

from diagnostics_reference import diagnostics, pressure_nodes, square_mesh, velocity_nodes
from oracle.fem import unit_disk_mesh


def _field(mesh, k, fu, fp=None):
    X = velocity_nodes(mesh, k)
    Q = np.stack(fu(X[:, 0], X[:, 1]), axis=1)
    Xp = pressure_nodes(mesh, k)
    p = fp(Xp[:, 0], Xp[:, 1]) if fp else np.zeros(len(Xp))
    return Q, p


@pytest.mark.parametrize("k", [1, 2, 3])
def test_rotation_on_unit_square(k):
    """u = (-y, x): energy 1/3, enstrophy 2, no divergence; continuous, so only the four sides (u.n)^2 = 1/3 each count."""
    mesh = square_mesh(4)
    Q, p = _field(mesh, k, lambda x, y: (-y, x), lambda x, y: x + y)
    d = diagnostics(mesh, k, Q, p, q=p, dt=0.1)
    assert d["energy"] == pytest.approx(1 / 3, rel=1e-13)
    assert d["enstrophy"] == pytest.approx(2.0, rel=1e-13)
    assert d["div_l2"] < 1e-13
    assert d["jump_l2"] == pytest.approx(np.sqrt(4 / 3), rel=1e-13)
    assert d["p_integral"] == pytest.approx(1.0, rel=1e-13)
    assert d["tracer_integral"] == pytest.approx(1.0, rel=1e-13)
    assert d["tracer_half_sq"] == pytest.approx(7 / 12, rel=1e-13)
    assert d["max_speed"] == pytest.approx(np.sqrt(2), rel=1e-15)
    # the corner cell at (1, 1) carries |u| = sqrt 2 at its node; every cell's shortest edge is h = 1/4
    assert d["cfl"] == pytest.approx(0.1 * np.sqrt(2) * 4, rel=1e-15)


def test_no_tracer_gives_nan():
    mesh = square_mesh(2)
    Q, p = _field(mesh, 1, lambda x, y: (x, y))
    d = diagnostics(mesh, 1, Q, p)
    assert np.isnan(d["tracer_integral"]) and np.isnan(d["tracer_half_sq"])
    assert d["div_l2"] == pytest.approx(np.sqrt(4.0), rel=1e-13)  # div (x, y) = 2 on the unit square


@pytest.mark.parametrize("k", [1, 3])
def test_constant_field_on_periodic_square(k):
    L = 2 * np.pi
    mesh = square_mesh(6, periodic=True, L=L)
    Q, p = _field(mesh, k, lambda x, y: (0.3 + 0 * x, -1.1 + 0 * y))
    d = diagnostics(mesh, k, Q, p)
    assert d["energy"] == pytest.approx(0.5 * (0.09 + 1.21) * L * L, rel=1e-13)
    assert d["enstrophy"] < 1e-25 and d["div_l2"] < 1e-13 and d["jump_l2"] < 1e-13


@pytest.mark.parametrize("k", [1, 2])
def test_known_jumps(k):
    # (1, 0) in one cell of the periodic square and zero elsewhere: the jumps are u.n on that cell's three edges,
    # h (0)^2 + h (1)^2 + sqrt 2 h (1 / sqrt 2)^2 for the lower triangle with legs h
    mesh = square_mesh(4, periodic=True)
    nu = (k + 2) * (k + 3) // 2
    Q = np.zeros((mesh.ncells * nu, 2))
    Q[5 * 2 * nu: 5 * 2 * nu + nu, 0] = 1.0  # cell 10 = lower triangle of square (1, 1)
    p = np.zeros(mesh.ncells * (k + 1) * (k + 2) // 2)
    d = diagnostics(mesh, k, Q, p)
    h = 0.25
    assert d["jump_l2"] == pytest.approx(np.sqrt(h * (1.0 + 0.5 * np.sqrt(2))), rel=1e-13)
    # u = (1, 0) left of x = 1/2, 0 right of it: two lines of vertical edges (x = 1/2 and the wrapped x = 0) with [u.n] = 1
    X = velocity_nodes(mesh, k).reshape(mesh.ncells, nu, 2)
    left = X[:, :, 0].mean(axis=1) < 0.5  # whole cells left of x = 1/2
    Q = np.zeros((mesh.ncells, nu, 2))
    Q[left, :, 0] = 1.0
    d = diagnostics(mesh, k, Q.reshape(-1, 2), p)
    assert d["jump_l2"] == pytest.approx(np.sqrt(2.0), rel=1e-13)
    assert d["enstrophy"] < 1e-25 and d["div_l2"] < 1e-13


@pytest.mark.parametrize("level", [1, 3])
def test_disk_against_volume(level):
    mesh = unit_disk_mesh(level)
    k = 2
    Q, p = _field(mesh, k, lambda x, y: (1.0 + 0 * x, 2.0 + 0 * y), lambda x, y: 1.0 + 0 * x)
    d = diagnostics(mesh, k, Q, p, q=p)
    vol = mesh.volume
    assert d["energy"] == pytest.approx(0.5 * 5.0 * vol, rel=1e-13)
    assert d["p_integral"] == pytest.approx(vol, rel=1e-13)
    assert d["tracer_integral"] == pytest.approx(vol, rel=1e-13)
    assert d["tracer_half_sq"] == pytest.approx(0.5 * vol, rel=1e-13)
    assert d["enstrophy"] < 1e-24 and d["div_l2"] < 1e-12
    bnd = mesh.edge_minus < 0
    un = mesh.edge_normal_plus[bnd] @ np.array([1.0, 2.0])
    assert d["jump_l2"] == pytest.approx(np.sqrt(np.sum(mesh.edge_len[bnd] * un * un)), rel=1e-13)
    # rigid rotation (-y, x) on the disk: enstrophy = 2 |Omega_h|
    Q, p = _field(mesh, k, lambda x, y: (-y, x))
    assert diagnostics(mesh, k, Q, p)["enstrophy"] == pytest.approx(2.0 * vol, rel=1e-13)
