"""The tile kernels of the trace preconditioner (hdg_trace_tile.hpp), the post kernel holding its stage values once (d0 in Ds,
z0 in Zs, re-read at the thread's own slot instead of crossing the barrier in registers: four workgroups per CU at k = 2),
against the five row-stencil launches they replace (HDG_TRACE_NO_TILE=1: the same arithmetic per corner).  Two steps of
Taylor-Green with SSP2(3,3,2), projection, R = 2, both engines in one process; meshes with one tile column, partial right and
top tiles and an odd vertex grid, every degree the corner form serves, and the periodic square (wrapped halo columns).

The two paths differ in the order of the five CG inner products (per tile / per row), so they agree to rounding amplified by
the solves, not bit for bit.  PARENT below holds what the commit before this change gave for the same cases on an MI355X: the
iteration sums of the four solve classes (tentative, pressure, final pressure, pressure reconstruction) of either path, which
both paths must reproduce exactly, and the relative maximum difference of Q, p and lambda between the paths, of which twice
is allowed.  Largest differences of the parent over the cases: Q 1.10e-10 (k = 3, nx = 24), p 5.71e-11 (k = 2, nx = 24),
lambda 4.68e-11 (k = 3, nx = 24).  (With the changed post kernel the tile path gives the parent's bits, so the differences
measured after the change are the parent's.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (k, nx, periodic): (iteration sums with tiles, with row stencils, relative difference of Q, p, lambda between the paths)
PARENT = {
    (2, 16, False): ([210.0, 97.0, 24.0, 24.0], [210.0, 97.0, 24.0, 24.0], 9.028834370871391e-11, 4.611868000644583e-11, 3.732934970361676e-11),
    (2, 17, False): ([207.0, 160.0, 37.0, 39.0], [207.0, 160.0, 37.0, 39.0], 2.1220208464160975e-11, 8.042322102141525e-12, 7.947289223803044e-12),
    (2, 24, False): ([209.0, 96.0, 24.0, 24.0], [209.0, 96.0, 24.0, 24.0], 7.878716218703961e-11, 5.7128816936822164e-11, 4.539169587461272e-11),
    (2, 33, False): ([202.0, 283.0, 58.0, 63.0], [202.0, 283.0, 58.0, 63.0], 1.0680474491146846e-11, 4.093991161488919e-12, 2.9415756861737706e-12),
    (1, 24, False): ([254.0, 88.0, 22.0, 22.0], [254.0, 88.0, 22.0, 22.0], 1.1018807887305297e-11, 3.2512852072987574e-12, 3.125342210033233e-12),
    (3, 24, False): ([241.0, 104.0, 26.0, 26.0], [241.0, 104.0, 26.0, 26.0], 1.1006929429712951e-10, 5.280494643876874e-11, 4.675591286470062e-11),
    (2, 16, True): ([219.0, 95.0, 22.0, 22.0], [219.0, 95.0, 22.0, 22.0], 4.540308859101118e-11, 1.2124893468828792e-11, 9.146347399452137e-12),
    (2, 18, True): ([218.0, 115.0, 24.0, 27.0], [218.0, 115.0, 24.0, 27.0], 8.988581616441901e-12, 2.9147494289145724e-12, 2.0746328441434284e-12),
}


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _two_steps(k, nx, periodic):
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    # periodic: the square of side 2, one period of the Taylor-Green field
    L = 2.0 if periodic else 1.0
    dt = 0.25 * L / nx
    mesh = PeriodicSquareMesh(nx, nx, L=L) if periodic else UnitSquareMesh(nx, nx)
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=True, n_richardson=2)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), 2 * dt, fused=True)
    lam = ts._engine.get_field(_lib.HDG_STATE_CURRENT, Q=False, p=False)[2]
    sums, cnt = ts._engine.iteration_stats()
    return Q.dat.data.copy(), p.dat.data.copy(), lam.copy(), [float(s) for s in sums], ts._engine.kernel_forms()["trace_precond"]


def both_paths(k, nx, periodic, setenv, delenv):
    """(result with the tile kernels, result with the row-stencil kernels); the switch is read when an engine is built"""
    delenv("HDG_TRACE_NO_TILE")
    delenv("HDG_TRACE_TILE3")
    tile = _two_steps(k, nx, periodic)
    setenv("HDG_TRACE_NO_TILE", "1")
    rows = _two_steps(k, nx, periodic)
    delenv("HDG_TRACE_NO_TILE")
    return tile, rows


CASES = [(2, 16, False), (2, 17, False), (2, 24, False), (2, 33, False), (1, 24, False), (3, 24, False), (2, 16, True), (2, 18, True)]


@pytest.mark.parametrize("k,nx,periodic", CASES)
def test_tile_kernels_equal_the_row_stencils(hip_lib, k, nx, periodic, monkeypatch):
    tile, rows = both_paths(k, nx, periodic, monkeypatch.setenv, lambda name: monkeypatch.delenv(name, raising=False))
    assert tile[4] == 1 and rows[4] == 0  # hdg_get_kernel_forms: tiles with one thread per corner / row stencils
    its_tile, its_rows, dQ, dp, dl = PARENT[(k, nx, periodic)]
    diffs = [_rel(tile[q], rows[q]) for q in range(3)]
    print(f"k={k} nx={nx} periodic={periodic}: its tile {tile[3]} rows {rows[3]}  rel. diff Q {diffs[0]:.3e} p {diffs[1]:.3e} lam {diffs[2]:.3e}")
    assert tile[3] == its_tile and rows[3] == its_rows, (tile[3], rows[3])
    for q, (d, parent) in enumerate(zip(diffs, (dQ, dp, dl))):
        assert d <= 2.0 * parent, (q, d, parent)
