"""The machinery the per-step outputs share: the row log of the engine (csrc/hdg_row_log.hpp) through the C boundary, for the
diagnostics, the probes and the particles alike, and the time loop of timesteppers/common.py under each stepper class."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PROBES = np.array([[0.25, 0.25], [0.75, 0.5], [0.4, 0.9]])
SEEDS = np.array([[0.3, 0.3], [0.6, 0.7]])


def _engine():
    """unit square, k = 1, 8 x 8, IMEX SSP2(3,3,2) with the Taylor-Green state set: (engine, re-set the state)"""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(8, 8), 1, 0.25 / 8, use_projection_method=True, n_richardson=2)
    eng = ts._engine
    Q0, p0 = TaylorGreen(ts._V_Q, ts._V_p).initial_condition()
    Q0, p0 = ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0)

    def set_state():
        eng.set_state(Q0, p0)
        eng.reconstruct_trace()

    set_state()
    return eng, set_state


# per recorder: switch on with a capacity (0: off), the C entry with what it takes after n_rows, fetch the rows, NaN allowed
RECORDERS = {
    "diagnostics": (lambda e, cap: e.set_diagnostics(cap), lambda e: (e.lib.hdg_get_diagnostics, ()),
                    lambda e, reset=True: e.diagnostics(reset=reset), True),
    "probes": (lambda e, cap: e.set_probes(PROBES if cap else None, cap), lambda e: (e.lib.hdg_get_probes, ()),
               lambda e, reset=True: e.probes(reset=reset), True),
    "particles": (lambda e, cap: e.set_particles(SEEDS if cap else None, cap), lambda e: (e.lib.hdg_get_particles, (None,)),
                  lambda e, reset=True: e.particles(reset=reset)[0], False),
}


@pytest.mark.parametrize("which", sorted(RECORDERS))
def test_row_log_through_the_c_boundary(hip_lib, which):
    """(a) capacity 2, three steps: the fetch raises with the dropped rows and the capacity in its text, a max_rows = 0 call
    reports 2 rows.  Row 0 is the state at the time the recorder is set, so the log is full after the first step: the text
    holds "1 row(s) dropped beyond the capacity of 2" after the second step and "2 row(s) ..." after the third (both are
    asserted; three steps drop two rows, not one).  (b) the same engine at capacity 5 (the buffer grows) over three steps
    from the re-set state gives the four rows, bit for bit, of a fresh engine that started at capacity 5 (same device, same
    launch order).  hdg_set_state re-sets Q and p only: the Krylov solves of a step start from the update, stage and
    reconstruction vectors the step before left, and stop relative to that start, so three steps after three others are not
    the three steps of an untouched engine (the rows differ from the fourth digit on).  The fresh engine therefore takes
    the three steps of (a) too, at capacity 5, and re-sets its state the same way: the two engines issue the same launches
    on the same data and differ only in the log (capacity 2, overflowed, then grown against capacity 5 throughout).
    (c) switched off, a step issues the launches of an engine that never recorded."""
    from incompressibleeulerhdg_amd import _lib

    set_cap, entry, fetch, nan_ok = RECORDERS[which]
    eng, set_state = _engine()
    # (a)
    set_cap(eng, 2)
    fn, extra = entry(eng)
    for dropped in (0, 1, 2):
        eng.step()
        n = C.c_int(-7)
        rc = fn(eng.h, None, 0, C.byref(n), *extra, 0)
        assert rc == (-1 if dropped else 0) and n.value == 2
        if dropped:
            with pytest.raises(_lib.HDGError) as ei:
                fetch(eng, reset=dropped == 2)
            assert f"{which}: {dropped} row(s) dropped beyond the capacity of 2 rows" in str(ei.value)
    # (b)
    set_state()
    set_cap(eng, 5)
    for _ in range(3):
        eng.step()
    grown = fetch(eng)
    fresh_eng, fresh_set_state = _engine()
    set_cap(fresh_eng, 5)
    for _ in range(3):
        fresh_eng.step()
    assert fetch(fresh_eng).shape[0] == 4  # nothing dropped: this log never overflows and never grows
    fresh_set_state()
    set_cap(fresh_eng, 5)
    for _ in range(3):
        fresh_eng.step()
    fresh = fetch(fresh_eng)
    assert grown.shape[0] == 4 and grown.shape == fresh.shape
    assert np.isfinite(fresh).any() and (nan_ok or np.isfinite(fresh).all())
    assert np.array_equal(grown, fresh, equal_nan=nan_ok)
    assert not np.array_equal(fresh[0], fresh[3], equal_nan=nan_ok)  # the rows do record the steps
    # (c) the same six steps without a recorder, then one step of each
    set_cap(eng, 0)
    never, never_set_state = _engine()
    for n in range(6):
        if n == 3:
            never_set_state()
        never.step()
    eng.launch_stats(reset=True)
    never.launch_stats(reset=True)
    eng.step()
    never.step()
    assert eng.launch_stats() == never.launch_stats()


NT, DT = 6, 0.04  # tests/test_gpu_timestep.py runs k = 1, 8 x 8 with dt = 0.04 (and 0.25 / 8, a power of two: no rounding at all)


@pytest.mark.parametrize("which", ["imex", "implicit", "dg"])
def test_time_loop_hands_every_class_its_own_times_and_names(hip_lib, which):
    """The shared loop keeps what differed between the three solve() bodies: the time handed to callbacks (IMEX k dt + dt,
    the implicit classes (k + 1) dt: not the same double for every k), the names of the Functions the callbacks receive
    and of those solve() returns, and the order "recorders started, then the t = 0 callbacks"."""
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import (IncompressibleEulerDGImplicit, IncompressibleEulerHDGImplicit,
                                                         IncompressibleEulerHDGIMEXSSP2_332)

    imex_times = [0] + [k * DT + DT for k in range(NT)]
    implicit_times = [0] + [(k + 1) * DT for k in range(NT)]
    assert imex_times != implicit_times  # the two formulas differ in the last bit for some k < NT

    class Collect:
        def __init__(self):
            self.times, self.names, self.diagnostics_at_0 = [], [], "not called"

        def reset(self):
            self.times, self.names = [], []

        def __call__(self, Q, p, t, q_tracer=None):
            if not self.times:
                self.diagnostics_at_0 = ts.diagnostics
            self.times.append(t)
            self.names.append((Q.name(), p.name()))

    cb = Collect()
    mesh = UnitSquareMesh(8, 8)
    if which == "imex":
        ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, 1, DT, use_projection_method=True, n_richardson=2, callbacks=[cb])
        kw, times, cb_names, names = {"fused": True}, imex_times, ("Q", "p"), ("Q", "p")
    else:
        cls = IncompressibleEulerHDGImplicit if which == "implicit" else IncompressibleEulerDGImplicit
        ts = cls(mesh, 1, DT, callbacks=[cb])
        kw, times, cb_names, names = {}, implicit_times, (None, None), ("velocity", "pressure")
    mp = TaylorGreen(ts._V_Q, ts._V_p, "exponential", 0.5)
    ts.diagnostics = {"stale": True}  # of an earlier run: cleared when the recorders start, before the t = 0 callbacks
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), NT * DT, diagnostics=True, **kw)
    assert cb.times == times  # exactly: list equality of doubles
    assert cb.names == [cb_names] * (NT + 1)
    assert cb.diagnostics_at_0 is None
    assert (Q.name(), p.name()) == names
    assert ts.diagnostics["energy"].shape == (NT + 1,) and np.array_equal(ts.diagnostics["t"], np.arange(NT + 1) * DT)
