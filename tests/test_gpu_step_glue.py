"""The stage bookkeeping of a fused IMEX step folded into the kernels next to it (`HDG_NO_GLUE_FUSION`):
the stage right-hand side formed inside k_pgrad_terms, and pointer exchanges for the copies of begin_step and of the Chebyshev
iterate.  Every one of them repeats the arithmetic of the launch it replaces operation for operation, so an engine built
with the switch set and one built without it must agree BITWISE in every field a caller can read, after every step, and
must take the same Krylov iterations.  The launch census says that the passes are really gone."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STAGES, RICHARDSON = 3, 2  # SSP2(3,3,2): two implicit stages, two Richardson passes each
SOLVES_PER_STEP = (STAGES - 1) * RICHARDSON

# k = 2, nx = 96: paired lift (above nx = 64); nx = 32: gather lift, no V-cycle leg carries the p / x update; nx = 65: odd,
# partial tiles; k = 1, nx = 64: fat ellipse, the Chebyshev iterate ends in either buffer; k = 3: matrix-core kernels, whose
# pressure gradient and back-substitution keep the old launches
SHAPES = [(2, 96), (2, 32), (2, 65), (1, 64), (3, 64)]


def _pair(monkeypatch, make):
    """(fused, unfused): two engines on the same inputs, the second built with HDG_NO_GLUE_FUSION in the environment"""
    monkeypatch.delenv("HDG_NO_GLUE_FUSION", raising=False)
    new = make()
    monkeypatch.setenv("HDG_NO_GLUE_FUSION", "1")
    old = make()
    monkeypatch.delenv("HDG_NO_GLUE_FUSION", raising=False)
    return new, old


def _imex(k, nx):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(nx, nx), k, 0.25 / nx, flux="upwind", use_projection_method=True,
                                            n_richardson=RICHARDSON)
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    e = ts._engine
    e.set_state(ts._V_Q.interpolate(mp.Q_stationary), ts._V_p.interpolate(mp.p_stationary))
    e.reconstruct_trace()
    e.set_forcing_profile(mp.f_rhs().profile)
    return ts


def _scales(nsteps, dt, t0=0.0, kappa=0.5):
    g = lambda t: -kappa * np.exp(-kappa * t)
    return np.array([[g(t0 + (n + c) * dt) for c in (0.0, 1.0, 0.5, 1.0)] for n in range(nsteps)])


def _fields(e):
    """every field hdg_get_field hands out: current state, update, stage states, tentative velocities"""
    from incompressibleeulerhdg_amd import _lib

    out = {}
    for name, which in [("current", _lib.HDG_STATE_CURRENT), ("update", _lib.HDG_STATE_UPDATE)] + [(f"stage{i}", i) for i in range(1, STAGES)]:
        for part, a in zip("Qpl", e.get_field(which)):
            out[f"{name}.{part}"] = a
    for i in range(1, STAGES):
        out[f"Qtent{i}"] = e.get_field(100 + i, p=False, lam=False)[0]
    return out


def _assert_same(fa, fb, what):
    assert fa.keys() == fb.keys()
    for name in fa:
        a, b = fa[name], fb[name]
        assert np.all(np.isfinite(b)), f"{what}: {name} is not finite"
        assert np.array_equal(a, b), f"{what}: {name} differs on {np.count_nonzero(a != b)} entries, max {np.max(np.abs(a - b)):.3e}"


def _census(e):
    st = e.launch_stats(reset=True)
    return st["vector_update"][0], st["copy_fill"][0]


@pytest.mark.parametrize("k,nx", SHAPES)
def test_two_steps_bitwise_and_same_iterations(hip_lib, monkeypatch, k, nx):
    new, old = _pair(monkeypatch, lambda: _imex(k, nx))
    dt = 0.25 / nx
    for ts in (new, old):
        ts._engine.iteration_stats(reset=True)
        ts._engine.run_separable(_scales(2, dt))
    _assert_same(_fields(new._engine), _fields(old._engine), f"k={k} nx={nx} after 2 steps")
    (sa, ca), (sb, cb) = new._engine.iteration_stats(), old._engine.iteration_stats()
    print(f"k={k} nx={nx}: iteration sums {sa} / {sb}, counts {ca} / {cb}")
    assert np.array_equal(sa, sb) and np.array_equal(ca, cb)
    assert ca[0] == 2 * SOLVES_PER_STEP and sa[0] > 0


# The launches the fusion removes from three fused steps (12 tentative solves), per shape.  The solver path is deterministic
# (tests/test_gpu_determinism.py), so the counts are exact:
#   vector_update: k <= 2: the k_lincomb of every stage right-hand side, one per tentative solve, 4 a step = 12; k = 3 keeps
#                  it (matrix-core pressure gradient): 0;
#   copy_fill:     the three copies of begin_step, 3 a step = 9, and one copy for every tentative solve whose newest Chebyshev
#                  iterate ends in the second buffer ("exchanges").
# (k, nx, exchanges): at k = 2, nx = 96 solves end in each of the two buffers (7 of 12 in the second), at k = 1, nx = 64 every
# one ends in the second
CENSUS = [(2, 96, 7), (1, 64, 12), (3, 64, 6)]


@pytest.mark.parametrize("k,nx,exchanges", CENSUS)
def test_three_steps_fields_after_each_and_launch_census(hip_lib, monkeypatch, k, nx, exchanges):
    """Fields through hdg_get_field after EVERY step (a pointer exchanged but still read at its old address would show), and
    the launches the fusion removes from the steps, counted from hdg_get_launch_stats: exactly the numbers of CENSUS, so a
    fused form that quietly fell back to the old launches on some of the solves fails here."""
    new, old = _pair(monkeypatch, lambda: _imex(k, nx))
    dt = 0.25 / nx
    nsteps = 3
    vec = np.zeros(2, dtype=int)
    cpy = np.zeros(2, dtype=int)
    for n in range(nsteps):
        for q, ts in enumerate((new, old)):
            ts._engine.launch_stats(reset=True)
            ts._engine.run_separable(_scales(1, dt, t0=n * dt))
            v, c = _census(ts._engine)
            vec[q] += v
            cpy[q] += c
        _assert_same(_fields(new._engine), _fields(old._engine), f"k={k} nx={nx} after step {n + 1}")
    nsolves = nsteps * SOLVES_PER_STEP
    lincombs = nsolves if k <= 2 else 0
    print(f"k={k} nx={nx}: vector_update {vec[0]} / {vec[1]}, copy_fill {cpy[0]} / {cpy[1]} (fused / old launches)")
    assert vec[1] - vec[0] == lincombs
    assert cpy[1] - cpy[0] == 3 * nsteps + exchanges
    assert 0 < exchanges <= nsolves
    if (k, nx) == (2, 96):
        # both endings of a solve occur in this run: in the engine's own buffer (no copy before, none now) and in the second
        # one (a copy before, a pointer exchange now)
        assert exchanges < nsolves


def test_implicit_step_bitwise(hip_lib, monkeypatch):
    """The first-order implicit stepper shares cheb_gmres and passes Qtent[0]: the exchange must work there too."""
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGImplicit

    k, nx = 1, 32

    def make():
        ts = IncompressibleEulerHDGImplicit(UnitSquareMesh(nx, nx), k, 0.25 / nx, use_projection_method=True)
        mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
        e = ts._engine
        e.set_state(ts._V_Q.interpolate(mp.Q_stationary), ts._V_p.interpolate(mp.p_stationary))
        e.reconstruct_trace()
        e.set_forcing_profile(mp.f_rhs().profile)
        e.set_forcing_scale(0, -0.5)
        return ts

    new, old = _pair(monkeypatch, make)
    for n in range(2):  # the second step starts from known bounds
        its = [ts._engine.implicit_step() for ts in (new, old)]
        print(f"implicit step {n + 1}: iterations {its[0]} / {its[1]}")
        assert its[0] == its[1] and its[0][0] > 0
        for which in (_lib.HDG_STATE_CURRENT, _lib.HDG_STATE_UPDATE):
            for part, a, b in zip("Qpl", new._engine.get_field(which), old._engine.get_field(which)):
                assert np.array_equal(a, b), f"implicit step {n + 1}, state {which}, {part}"
        a, b = (ts._engine.get_field(100, p=False, lam=False)[0] for ts in (new, old))
        assert np.array_equal(a, b), f"implicit step {n + 1}: tentative velocity"
