"""The numpy / scipy twin of the stream function (tests/streamfunction_reference.py) tested on its own: no GPU, no library.

What the GPU tests (tests/test_gpu_streamfunction.py) take from the twin is only as good as the twin, so it has to recover
polynomial stream functions, satisfy the energy identity of the minimisation, and show the two-level behaviour the device
solver is held to.
"""
import functools

import numpy as np
import pytest

from streamfunction_reference import PSI_K1, PSI_K2, StreamfunctionReference


@functools.lru_cache(maxsize=None)
def _ref(nx, k, periodic=False):
    return StreamfunctionReference(nx, k, periodic=periodic, L=2.0 if periodic else 1.0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("nx", [4, 8])
def test_polynomial_stream_functions_are_recovered(k, nx):
    """psi* in P_{k+1}, u its nodal curl: psi = psi* up to the gauge, to 1e-12, and the defect vanishes"""
    ref = _ref(nx, k)
    fn = PSI_K1 if k == 1 else PSI_K2
    Q = ref.d.interpolate_velocity(lambda x, y: fn(x, y)[1])
    exact = ref.shift(fn(ref.tr.cg_coords[:, 0], ref.tr.cg_coords[:, 1])[0])
    psi = ref.solve(Q)
    assert np.abs(psi - exact).max() < 1e-12 * max(np.abs(exact).max(), 1.0)
    defect, unorm = ref.defect(Q, psi)
    assert defect < 1e-12 * unorm
    assert abs(ref.gauge @ psi) < 1e-14


@pytest.mark.parametrize("k,nx", [(1, 6), (2, 4), (3, 3), (4, 4)])
def test_energy_identity_on_the_unit_square(k, nx):
    """psi minimises |u - curl psi|: defect^2 = |u|^2 - b^T psi (Pythagoras; b^T psi = |curl psi|^2)"""
    ref = _ref(nx, k)
    Q = np.random.default_rng(5).standard_normal((ref.d.mesh.ncells * ref.d.nu, 2))
    psi = ref.solve(Q)
    defect, unorm = ref.defect(Q, psi)
    b = ref.rhs(Q)
    assert abs(b.sum()) < 1e-12 * np.abs(b).sum()  # the right-hand side sums to zero
    assert abs(defect ** 2 - (unorm ** 2 - b @ psi)) < 1e-11 * unorm ** 2
    assert abs(psi @ (ref.K @ psi) - b @ psi) < 1e-11 * unorm ** 2


@pytest.mark.parametrize("k,periodic", [(2, False), (2, True)])
def test_operators_of_the_twin(k, periodic):
    from oracle.hdg_oracle import HDGDiscretisation
    from oracle.tracer_oracle import TracerOracle

    ref = _ref(4, k, periodic)
    d = HDGDiscretisation(4, k, periodic=periodic, L=ref.L)  # the twin's tables and numbering are the oracle's
    tr = TracerOracle(d)
    assert np.array_equal(d.cUg, ref.d.cUg) and np.array_equal(d.cU, ref.d.cU) and np.array_equal(d.cwdet, ref.d.cwdet)
    assert np.array_equal(tr.cg_of_dg, ref.tr.cg_of_dg) and np.array_equal(tr.cg_coords, ref.tr.cg_coords) and (tr.R != ref.tr.R).nnz == 0
    assert np.abs(ref.K @ np.ones(ref.ncg)).max() < 1e-12  # constants are the kernel
    assert np.abs(ref.P @ np.ones(ref.nv) - 1.0).max() < 1e-14  # P reproduces constants
    Ac = (ref.P.T @ ref.K @ ref.P).toarray()
    assert np.abs(Ac.diagonal().max() - 4.0) < 1e-12  # the Galerkin coarse operator is the 5-point Laplacian
    if not periodic:  # ... and linear functions at the dof coordinates
        V, X = ref.vertex_coordinates(), ref.tr.cg_coords
        assert np.abs(ref.P @ (2.0 * V[:, 0] - 3.0 * V[:, 1]) - (2.0 * X[:, 0] - 3.0 * X[:, 1])).max() < 1e-13
    else:  # a constant velocity has the stream function zero and is its own mean flow
        Q = np.tile([0.75, -1.25], (ref.d.mesh.ncells * ref.d.nu, 1))
        assert np.abs(ref.solve(Q)).max() < 1e-13 and np.abs(ref.mean_flow(Q) - [0.75, -1.25]).max() < 1e-14


@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("periodic", [False, True])
def test_the_coarse_level_works_in_the_twin(k, periodic):
    """the two conditions the device solver is held to, for the twin with an exact coarse solve: random right-hand side, rtol
    1e-10; the two-level iterations at nx = 16 are at most 1.25 times those at nx = 8 and at most half of Jacobi's at nx = 16"""
    its = {}
    for nx in (8, 16):
        ref = _ref(nx, k, periodic)
        b = np.random.default_rng(7).standard_normal(ref.ncg)
        b -= b.mean()
        x, its[nx] = ref.pcg(b, 1e-10)
        assert np.abs(ref.K @ x - b).max() < 1e-7 * np.abs(b).max()
    _, jacobi = _ref(16, k, periodic).pcg(b, 1e-10, two_level=False)
    print(f"k = {k}, periodic = {periodic}: two-level {its[8]} -> {its[16]}, Jacobi at 16: {jacobi}")
    assert its[16] <= 1.25 * its[8]
    assert its[16] <= 0.5 * jacobi
