"""Checkpoint and restart (include/hdg_checkpoint.h) on the GPU.  The rule of tests/test_gpu_determinism.py
-- two engines with the same history agree bit for bit -- gives the feature its definition of done: a run that is saved,
destroyed, loaded into a fresh engine and continued equals the uninterrupted run in every bit of every field a getter returns,
in every iteration count and in the state digest.  Every comparison below is np.array_equal or == on integers."""
import os
import re
import struct
import subprocess
import sys
import uuid

import numpy as np
import pytest

import checkpoint_reference as ref

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
N = 3  # steps before the save and after it


# ---------------------------------------------------------------------------------------------------------------- helpers
class Killed(Exception):
    pass


class KillAfter:
    """Callback of solve: ends the run (like a kill would) once `nsteps` steps are complete -- after their checkpoint."""

    def __init__(self, nsteps):
        self.nsteps, self.calls = nsteps, 0

    def reset(self):
        self.calls = 0

    def __call__(self, Q, p, t, q_tracer=None):
        self.calls += 1
        if self.calls == self.nsteps + 1:  # call 1 is the initial state
            raise Killed()


def snapshot(ts, tracer=False):
    """Everything the C-ABI shows of an engine between steps.  The digest first: on the periodic square a trace getter
    refreshes ghost rows, which are part of the state."""
    e = ts._engine
    s = e.nstages
    out = {"digest": e.state_digest()}
    sums, cnt = e.iteration_stats()
    out["it_sums"], out["it_counts"] = sums, cnt
    out["events"] = e.solver_events()
    out["current"] = e.get_field(0)
    out["update"] = e.get_field(-1)
    out["recon"] = e.get_field(-2, Q=False)[1:]
    for i in range(1, s):
        out[f"stage{i}"] = e.get_field(i)
    for i in range(s):
        out[f"tentative{i}"] = e.get_field(100 + i, p=False, lam=False)[:1]
    for i in range(max(s - 1, 1)):
        out[f"qstar{i}"] = e.get_field(200 + i, p=False, lam=False)[:1]
    if tracer:
        out["tracer"] = (e.get_tracer(),)
    return out


def assert_same(a, b, what):
    assert sorted(a) == sorted(b)
    for key in a:
        if key == "events" or key == "digest":
            assert a[key] == b[key], (what, key, a[key], b[key])
        elif key.startswith("it_"):
            assert np.array_equal(a[key], b[key]), (what, key, a[key], b[key])
        else:
            for n, (x, y) in enumerate(zip(a[key], b[key])):
                assert x.shape == y.shape
                assert np.array_equal(x, y), (what, key, n, int(np.count_nonzero(x != y)), float(np.max(np.abs(x - y))))


def record_solves(ts, log):
    """per-solve iteration counts of the per-solve path: every tentative / pressure / unsplit solve, in order"""
    e = ts._engine
    for name in ("tentative_solve", "pressure_solve", "unsplit_solve"):
        def wrapped(*a, _f=getattr(e, name), _n=name):
            its = _f(*a)
            log.append((_n, a, its))
            return its
        setattr(e, name, wrapped)


def twin_runs(make, problem, tmp_path, solve_kw=None, tracer=None, per_solve=False):
    """The uninterrupted run of 2 N steps and its twin: N steps, save, (killed, engine destroyed), fresh engine, load, N steps.
    make(callbacks) builds a stepper; problem(ts) gives (Q0, p0, f_rhs).  Returns the two steppers' results for further checks:
    (uninterrupted stepper, restarted stepper, the blob)."""
    solve_kw = dict(solve_kw or {})
    path = str(tmp_path / "run.ckpt")
    full = make(None)
    Q0, p0, f = problem(full)
    T = 2 * N * full._dt
    log_full, log_twin = [], []
    if per_solve:
        record_solves(full, log_full)
    full.solve(Q0, p0, tracer, f, T, **solve_kw)
    want = snapshot(full, tracer is not None)

    first = make([KillAfter(N)])
    Q0, p0, f = problem(first)
    if per_solve:
        record_solves(first, log_twin)
    with pytest.raises(Killed):
        first.solve(Q0, p0, tracer, f, T, checkpoint=path, checkpoint_every=N, **solve_kw)
    assert not os.path.exists(path + ".tmp")
    first._engine.close()
    del first
    blob = open(path, "rb").read()

    again = make(None)
    _, _, f = problem(again)
    # save -> load into a fresh engine -> save: the same bytes
    step, t = again._engine.load_checkpoint(blob)
    assert step == N and t == N * again._dt
    assert again._engine.save_checkpoint(step, t) == blob
    if per_solve:
        record_solves(again, log_twin)
    again.solve(None, None, None, f, T, restart=path, **solve_kw)
    got = snapshot(again, tracer is not None)
    assert_same(want, got, "restarted against uninterrupted")
    if per_solve:
        assert len(log_full) > 0 and log_full == log_twin
    return full, again, blob


def imex(name, k, nx, **kw):
    from incompressibleeulerhdg_amd import timesteppers as T
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh

    cls = getattr(T, name)
    return lambda callbacks: cls(UnitSquareMesh(nx, nx), k, 0.25 / nx, callbacks=callbacks, **kw)


def taylor_green(ts):
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen

    mp = TaylorGreen(ts._V_Q, ts._V_p)
    return (*mp.initial_condition(), mp.f_rhs())


# ---------------------------------------------------------------------------------------------------------------- 1. digest
@pytest.fixture(scope="module")
def small_engine(hip_lib):
    ts = imex("IncompressibleEulerHDGIMEXSSP2_332", 1, 8)(None)
    yield ts._engine
    ts._engine.close()


@pytest.mark.parametrize("n", ref.LENGTHS)
def test_digest_kernel_equals_the_formula(small_engine, n):
    """hdg_digest_vector (k_digest + k_digest_final) against the numpy restatement, as integers: random bit patterns, NaNs with
    payloads, +-0, denormals and all-ones words (every partial sum wraps); the long length on random patterns and all-ones."""
    kinds = ref.KINDS if n <= 2 ** 16 + 3 else ("random", "ones")
    for kind in kinds:
        v = ref.patterns(kind, n, seed=n)
        assert small_engine.digest_vector(v) == ref.digest(v), (kind, n)


def test_digest_kernel_equals_the_host_formula_through_a_checkpoint(small_engine):
    """The C++ host formula on the same bytes: every digest in a blob's table was taken by the kernel on the device and then
    confirmed by digest_words on the downloaded bytes (a save that disagrees fails); here the table is read back and every
    section's bytes are digested once more in numpy, and the state digest is the digest of those digests."""
    blob = small_engine.save_checkpoint(0, 0.0)
    secs = sections(blob)
    assert [s[0] for s in secs][:3] == ["curQ", "curP", "curL"] and [s[0] for s in secs][-2:] == ["solver", "outputs"]
    for name, kind, length, offset, d in secs:
        data = blob[offset:offset + (8 * length if kind == 0 else length)]
        assert (ref.digest(np.frombuffer(data, dtype=np.uint64)) if kind == 0 else ref.digest_bytes(data)) == d, name
    assert small_engine.state_digest() == ref.digest_of_digests([s[4] for s in secs])


def sections(blob):
    """(id, kind, length, offset, digest) of every table entry of a blob (csrc/hdg_checkpoint.hpp)"""
    nsec, fp_len = struct.unpack_from("<I", blob, 12)[0], struct.unpack_from("<Q", blob, 40)[0]
    t0 = 64 + (fp_len + 7) // 8 * 8
    out = []
    for i in range(nsec):
        ident, kind, _, length, offset, d0, d1 = struct.unpack_from("<24sIIQQQQ", blob, t0 + 64 * i)
        out.append((ident.split(b"\0")[0].decode(), kind, length, offset, (d0, d1)))
    return out


# ---------------------------------------------------------------------------------------------------------------- 2. continuation
@pytest.mark.parametrize("k,nx", [(2, 96), (2, 32), (1, 64), (3, 64), (4, 64)])
def test_continuation_is_bitwise_ssp2_fused(hip_lib, tmp_path, k, nx):
    """Unit square, SSP2(3,3,2) fused, the smallest shapes that take the solver paths of the real sizes
    (tests/test_gpu_step_glue.py): paired and gather lift, V-cycle legs with and without the riding update, edge-form tiles."""
    twin_runs(imex("IncompressibleEulerHDGIMEXSSP2_332", k, nx), taylor_green, tmp_path, dict(fused=True))


FAMILIES = {
    "ssp2_per_solve": (imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 32), dict(fused=False), True),
    "ars3_443": (imex("IncompressibleEulerHDGIMEXARS3_443", 2, 32), dict(fused=True), False),
    "imex_implicit": (imex("IncompressibleEulerHDGIMEXImplicit", 2, 32), dict(fused=True), False),
    "ssp2_unsplit": (imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 16, use_projection_method=False), dict(fused=True), False),
    "hdg_implicit_projection": (imex("IncompressibleEulerHDGImplicit", 2, 16, use_projection_method=True), {}, False),
    "hdg_implicit_monolithic": (imex("IncompressibleEulerHDGImplicit", 2, 16, use_projection_method=False), {}, False),
    "dg_implicit": (imex("IncompressibleEulerDGImplicit", 1, 16), {}, False),
}


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_continuation_is_bitwise_in_every_family(hip_lib, tmp_path, family):
    make, kw, per_solve = FAMILIES[family]
    twin_runs(make, taylor_green, tmp_path, kw, per_solve=per_solve)


def test_continuation_across_a_bounds_re_estimate(hip_lib, tmp_path, monkeypatch):
    """HDG_CHEB_EVERY=4 (read when an engine is built): a stage's solve counter stands at 6 when the state is saved after three
    steps (two Richardson passes per step) and the bounds are re-estimated at 8, in the second step after the restart -- a blob
    that forgets ch_count re-estimates at the wrong solve and the iteration counts differ."""
    monkeypatch.setenv("HDG_CHEB_EVERY", "4")
    twin_runs(imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 32), taylor_green, tmp_path, dict(fused=True))


# ---------------------------------------------------------------------------------------------------------------- 3. everything on
def assert_series_equal(a, b):
    for name in ("diagnostics", "probes", "particles"):
        x, y = getattr(a, name), getattr(b, name)
        assert (x is None) == (y is None), name
        if x is None:
            continue
        assert sorted(x) == sorted(y)
        for key in x:
            assert np.array_equal(np.asarray(x[key]), np.asarray(y[key]), equal_nan=True), (name, key)


def test_everything_on_at_once_periodic_square(hip_lib, tmp_path):
    """Shear layer, k = 2, nx = 32, three tracers, diagnostics, 8 probes, 64 particles recorded every second step, saved after
    the third step (between two particle rows): the full series -- rows from before the save included --, the clamp and lost
    counts and the tracers of the restarted run are those of the uninterrupted one."""
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    nx, L = 32, 2 * np.pi
    rng = np.random.default_rng(5)
    probes, seeds = rng.random((8, 2)) * L, rng.random((64, 2)) * L
    make = lambda cb: IncompressibleEulerHDGIMEXSSP2_332(PeriodicSquareMesh(nx, nx, L=L), 2, 0.25 * L / nx, callbacks=cb, n_tracers=3)  # noqa: E731

    def problem(ts):
        return (*DoubleLayerShearFlow(ts._V_Q, ts._V_p).initial_condition(), None)

    q0 = [lambda x, y, m=m: np.sin((m + 1) * x) * np.cos((m + 1) * y) for m in range(3)]
    kw = dict(fused=True, diagnostics=True, probes=probes, particles=seeds, particle_every=2)
    full, again, blob = twin_runs(make, problem, tmp_path, kw, tracer=q0)
    from incompressibleeulerhdg_amd._lib import Engine

    info = Engine.checkpoint_info(blob)
    assert info["step"] == 3 and info["tracer"] and info["diagnostics"] and info["n_probes"] == 8 and info["n_particles"] == 64
    assert_series_equal(full, again)
    assert full.diagnostics["t"].shape == (2 * N + 1,) and full.probes["u"].shape == (2 * N + 1, 8, 2)
    assert full.particles["xy"].shape == (N + 1, 64, 2)
    for a, b in zip(full.q_tracers, again.q_tracers):
        assert np.array_equal(a.dat.data, b.dat.data)
    # a request that disagrees with the blob: ValueError, before the engine is touched
    other = make(None)
    before = other._engine.state_digest()
    with pytest.raises(ValueError, match="without|with"):
        other.solve(None, None, None, None, 2 * N * other._dt, fused=True, restart=str(tmp_path / "run.ckpt"), diagnostics=True)
    with pytest.raises(ValueError, match="8 probes"):
        other.solve(None, None, None, None, 2 * N * other._dt, fused=True, restart=str(tmp_path / "run.ckpt"), diagnostics=True,
                    probes=probes[:5], particles=seeds, particle_every=2)
    assert other._engine.state_digest() == before


def test_everything_on_at_once_disk(hip_lib, tmp_path):
    """The same on the level-3 disk (general mesh), k = 2: Kelvin-Helmholtz with one tracer, diagnostics and probes."""
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh
    from incompressibleeulerhdg_amd.model_problems import KelvinHelmholtz
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    mesh = UnitDiskMesh(refinement_level=3)
    rng = np.random.default_rng(6)
    probes = (rng.random((8, 2)) - 0.5) * 1.2
    make = lambda cb: IncompressibleEulerHDGIMEXSSP2_332(mesh, 2, 0.01, callbacks=cb)  # noqa: E731

    def problem(ts):
        return (*KelvinHelmholtz(ts._V_Q, ts._V_p).initial_condition(), None)

    kw = dict(fused=True, diagnostics=True, probes=probes)
    full, again, _ = twin_runs(make, problem, tmp_path, kw, tracer=lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y))
    assert_series_equal(full, again)
    assert np.array_equal(full.q_tracer.dat.data, again.q_tracer.dat.data)


# ---------------------------------------------------------------------------------------------------------------- 4. strips
def _strips(mode, kind, path, tmp_path):
    """Start the two ranks of tests/checkpoint_strip_worker.py under a time limit; a rank that fails ends the test, the other is
    killed and nothing further is started."""
    token = "/hdg_ckpt_" + uuid.uuid4().hex[:12]
    procs, outs = [], []
    for r in range(2):
        out = str(tmp_path / f"{kind}_{mode}_{r}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "checkpoint_strip_worker.py"), str(r), "2", token, kind,
                                       mode, path, out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    try:
        for proc in procs:
            o, _ = proc.communicate(timeout=300)
            logs.append(o.decode(errors="replace"))
    finally:
        for proc in procs:
            if proc.poll() is None:
                proc.kill()
                proc.wait()
    bad = [r for r, proc in enumerate(procs) if proc.returncode != 0]
    assert not bad, logs[bad[0]][-3000:]
    return [dict(np.load(o, allow_pickle=False)) for o in outs]


@pytest.mark.parametrize("kind", ["square", "periodic"])
def test_strips_continue_bitwise_and_refuse_the_other_ranks_blob(hip_lib, tmp_path, kind):
    """P = 2 over the shared-memory transport (periodic: with particles): each rank saves and loads its own PATH.<rank>; the
    restarted pair equals the uninterrupted pair bit for bit; a rank offered the other rank's blob refuses it, naming the rank,
    and stays what it was (the continuation that follows in the same engines is still the uninterrupted run)."""
    path = str(tmp_path / f"{kind}.ckpt")
    full = _strips("full", kind, path, tmp_path)
    _strips("first", kind, path, tmp_path)
    assert os.path.exists(path + ".0") and os.path.exists(path + ".1") and not os.path.exists(path)
    again = _strips("restart", kind, path, tmp_path)
    for r in range(2):
        assert "fingerprint field 'rank'" in str(again[r]["refusal"]), again[r]["refusal"]
        assert sorted(full[r]) == sorted(k for k in again[r] if k != "refusal")
        differ = [key for key in full[r] if not np.array_equal(full[r][key], again[r][key], equal_nan=True)]
        assert not differ, (r, differ)
    assert ("particle_rows" in full[0]) == (kind == "periodic")


# ---------------------------------------------------------------------------------------------------------------- 5. refusals
def _one_step_after(ts, attempt):
    """set the state, let `attempt` try its loads on the engine, take one step: what the engine then shows"""
    Q0, p0, f = taylor_green(ts) if not getattr(ts._mesh, "general", False) and not getattr(ts._mesh, "periodic", False) else (
        lambda x, y: (np.sin(x) * np.cos(y), -np.cos(x) * np.sin(y)), lambda x, y: 0.0 * x, None)
    e = ts._engine
    e.set_state(ts._as_nodal_velocity(Q0), ts._as_nodal_pressure(p0))
    e.reconstruct_trace()
    for i in range(e.nstages + 1):
        e.set_forcing_scale(i, 0.0)
    attempt(e)
    e.step()
    return snapshot(ts)


@pytest.fixture(scope="module")
def base_blob(hip_lib):
    """an SSP2 engine, k = 2, 16 x 16, after one step: its blob"""
    ts = imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 16)(None)
    _one_step_after(ts, lambda e: None)
    blob = ts._engine.save_checkpoint(1, ts._dt)
    ts._engine.close()
    return blob


def _other_engines():
    from incompressibleeulerhdg_amd import timesteppers as T
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh

    ssp2 = T.IncompressibleEulerHDGIMEXSSP2_332
    return {
        "nx": (lambda: ssp2(UnitSquareMesh(8, 8), 2, 0.25 / 16), "'nx'"),
        "degree": (lambda: ssp2(UnitSquareMesh(16, 16), 1, 0.25 / 16), "'degree'"),
        "dt": (lambda: ssp2(UnitSquareMesh(16, 16), 2, 0.25 / 16 * (1 + 2.0 ** -52)), "'dt'"),
        "tableau": (lambda: T.IncompressibleEulerHDGIMEXARS2_232(UnitSquareMesh(16, 16), 2, 0.25 / 16), r"'a_expl\[3\]'"),
        "n_tracers": (lambda: ssp2(UnitSquareMesh(16, 16), 2, 0.25 / 16, n_tracers=3), "'n_tracers'"),
        "mesh_kind": (lambda: ssp2(PeriodicSquareMesh(16, 16, L=1.0), 2, 0.25 / 16), "'mesh_kind'"),
        "engine_kind": (lambda: ssp2(UnitDiskMesh(refinement_level=1), 2, 0.25 / 16), "'engine_kind'"),
    }


@pytest.mark.parametrize("what", ["nx", "degree", "dt", "tableau", "n_tracers", "mesh_kind", "engine_kind"])
def test_a_blob_of_another_engine_is_refused_by_field_name(hip_lib, base_blob, what):
    from incompressibleeulerhdg_amd._lib import HDGError

    make, field = _other_engines()[what]

    def attempt(e):
        with pytest.raises(HDGError, match=f"HDG_ERR_ARG: checkpoint: fingerprint field {field} differs"):
            e.load_checkpoint(base_blob)

    tried, clean = make(), make()
    assert_same(_one_step_after(clean, lambda e: None), _one_step_after(tried, attempt), what)


def test_damaged_blobs_and_a_save_inside_a_step_are_refused(hip_lib, base_blob):
    from incompressibleeulerhdg_amd._lib import HDGError

    secs = {s[0]: s for s in sections(base_blob)}

    def flipped(offset):
        b = bytearray(base_blob)
        b[offset] ^= 0x10
        return bytes(b)

    def attempt(e):
        for cut in (0, 63, 64, len(base_blob) // 2, len(base_blob) - 1):
            with pytest.raises(HDGError, match="checkpoint: (truncated|byte count)"):
                e.load_checkpoint(base_blob[:cut])
        with pytest.raises(HDGError, match="byte count"):
            e.load_checkpoint(base_blob + b"\0" * 8)
        for name in ("curQ", "recL", "Qtent1", "solver", "outputs"):
            with pytest.raises(HDGError, match=f"checkpoint: section '{name}': the bytes do not match the digest"):
                e.load_checkpoint(flipped(secs[name][3] + 5))
        with pytest.raises(HDGError, match="format version 2 is not the version 1"):
            e.load_checkpoint(base_blob[:8] + b"\2" + base_blob[9:])
        with pytest.raises(HDGError, match="bad magic"):
            e.load_checkpoint(b"X" + base_blob[1:])
        # a save is valid between steps only
        e.begin_step()
        for call in (lambda: e.save_checkpoint(0, 0.0), e.state_digest):
            with pytest.raises(HDGError, match="HDG_ERR_ARG: checkpoint: a step is open"):
                call()
        for i in range(1, e.nstages):
            e.project_bdm(i - 1, i - 1)
            for _ in range(2):
                e.tentative_solve(i)
                e.pressure_solve(i)
                e.shift_pressure(-1)
                e.stage_update(i)
            e.shift_pressure(i)
        e.pressure_solve(0)
        e.pressure_solve(-1)
        e.finish_step()
        assert len(e.save_checkpoint(1, 0.0)) > 0  # the step is complete

    def per_solve_step(e):
        e.begin_step()
        for i in range(1, e.nstages):
            e.project_bdm(i - 1, i - 1)
            for _ in range(2):
                e.tentative_solve(i)
                e.pressure_solve(i)
                e.shift_pressure(-1)
                e.stage_update(i)
            e.shift_pressure(i)
        e.pressure_solve(0)
        e.pressure_solve(-1)
        e.finish_step()

    make = imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 16)
    tried, clean = make(None), make(None)
    assert_same(_one_step_after(clean, per_solve_step), _one_step_after(tried, attempt), "damaged blobs")
    # the undamaged blob does load into the engine that refused the damaged ones
    assert tried._engine.load_checkpoint(base_blob) == (1, tried._dt)


# ---------------------------------------------------------------------------------------------------------------- 6. read-only, free when off
def test_saving_changes_nothing_and_costs_nothing_when_off(hip_lib, tmp_path):
    """A run that saves after every step equals the run that never saves, bit for bit.  The launch census of a step
    (hdg_get_launch_stats) after a save is the census of the same step in an engine that never saved; the save itself adds
    launches to the class `other` alone: two per device section (k_digest and its second stage)."""
    make = imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 32)
    a, b = make(None), make(None)
    T = 4 * a._dt
    Q0, p0, f = taylor_green(a)
    a.solve(Q0, p0, None, f, T, fused=True)
    Q0, p0, f = taylor_green(b)
    b.solve(Q0, p0, None, f, T, fused=True, checkpoint=str(tmp_path / "every.ckpt"), checkpoint_every=1)
    assert_same(snapshot(a), snapshot(b), "saving every step")

    def tg3(ts):
        Q0, p0, f = taylor_green(ts)
        return Q0, p0, None, f

    c, d = make(None), make(None)
    census = []
    for ts, save in ((c, False), (d, True)):
        ts.solve(*tg3(ts), ts._dt, fused=True)
        e = ts._engine
        if save:
            e.launch_stats(reset=True)
            blob = e.save_checkpoint(1, ts._dt)
            during = e.launch_stats(reset=True)
            ndev = sum(1 for s in sections(blob) if s[1] == 0)
            assert during["other"][0] == 2 * ndev and all(v[0] == 0 for kname, v in during.items() if kname != "other")
        e.launch_stats(reset=True)
        for i in range(e.nstages + 1):
            e.set_forcing_scale(i, -0.4)
        e.step()
        census.append(e.launch_stats())
    assert census[0] == census[1]


def test_outputs_that_were_switched_off_again_are_not_state(hip_lib):
    """Recording is read-only: a run with diagnostics, probes, particles and a tracer that is switched off afterwards ends in
    the state, and with the state digest, of the run that had none of them."""
    make = imex("IncompressibleEulerHDGIMEXSSP2_332", 2, 16)
    a, b = make(None), make(None)
    T = 2 * a._dt
    Q0, p0, f = taylor_green(a)
    a.solve(Q0, p0, None, f, T, fused=True)
    Q0, p0, f = taylor_green(b)
    xy = np.random.default_rng(3).random((5, 2))
    b.solve(Q0, p0, None, f, T, fused=True, diagnostics=True, probes=xy, particles=xy)
    b._engine.apply_tracer_advection(np.zeros(b._engine.shape_p), np.zeros(b._engine.shape_Q))  # allocates the tracer vectors
    assert_same(snapshot(a), snapshot(b), "recorded against plain")
    assert a._engine.save_checkpoint(2, T) == b._engine.save_checkpoint(2, T)


# ---------------------------------------------------------------------------------------------------------------- 7. driver
def _driver(args, cwd, ok=True):
    r = subprocess.run([sys.executable, "-m", "incompressibleeulerhdg_amd.driver", *args], cwd=cwd, capture_output=True,
                       text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert (r.returncode == 0) == ok, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout, r.stderr


def test_driver_restart_prints_the_same_lines(hip_lib, tmp_path):
    """--tfinal of 6 steps against 3 steps with --checkpoint and a --restart to the same --tfinal: the printed error norms and
    the `state digest` line are the same strings; a restart with another --degree exits non-zero with the engine's message."""
    dt = 0.25 / 16
    base = ["--nx", "16", "--degree", "2", "--dt", repr(dt), "--use_projection_method", "--fused", "--output", ""]
    lines = lambda out: re.findall(r"^(?:velocity error|pressure error|state digest) = .*$", out, re.M)  # noqa: E731
    whole, _ = _driver(base + ["--tfinal", repr(6 * dt)], tmp_path)
    _driver(base + ["--tfinal", repr(3 * dt), "--checkpoint", "c.bin"], tmp_path)
    rest, _ = _driver(base + ["--tfinal", repr(6 * dt), "--restart", "c.bin"], tmp_path)
    assert len(lines(whole)) == 3 and lines(whole) == lines(rest), (lines(whole), lines(rest))
    assert sorted(ln.split(" = ")[0] for ln in lines(whole)) == ["pressure error", "state digest", "velocity error"]
    assert any(re.fullmatch(r"state digest = [0-9a-f]{32}", ln) for ln in lines(whole))
    bad = list(base)
    bad[3] = "1"
    out, err = _driver(bad + ["--tfinal", repr(6 * dt), "--restart", "c.bin"], tmp_path, ok=False)
    assert "fingerprint field 'degree' differs" in err
