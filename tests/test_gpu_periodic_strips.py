"""Periodic strips: the doubly periodic square (the shear layer's mesh) partitioned into P strips, P processes sharing the one
GPU of the test box over the shared-memory transport.  The ranks form a ring (rank r's neighbours are r -/+ 1 mod P; with
P = 2 both are the same peer), own their rows without a duplicated top row, and must reproduce the single-rank periodic run
to Krylov tolerance."""
import os
import re
import subprocess
import sys
import uuid

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
L = 2 * np.pi
TOL = 2e-8


def _run(nranks, k, nx, nsteps, tmp_path, extra=(), env=None, want_logs=False, tag="s"):
    """Start the P ranks (or the single-rank run, nranks = 1) of tests/periodic_strip_worker.py; kill them all on a failure."""
    token = "/hdg_ptest_" + uuid.uuid4().hex[:12]
    procs, outs = [], []
    for r in range(nranks):
        out = str(tmp_path / f"{tag}{nranks}_{r}.npz")
        outs.append(out)
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "periodic_strip_worker.py"), str(r), str(nranks), token,
                                       str(k), str(nx), str(nsteps), out, *extra],
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=dict(os.environ, **(env or {}))))
    logs = []
    try:
        for pr in procs:
            o, _ = pr.communicate(timeout=300)
            logs.append(o.decode(errors="replace"))
    finally:
        for q in procs:
            if q.poll() is None:
                q.kill()
                q.wait()
    bad = [r for r, pr in enumerate(procs) if pr.returncode != 0]
    if bad:
        for q in procs:
            if q.poll() is None:
                q.kill()
        raise AssertionError(f"rank {bad[0]} failed:\n{logs[bad[0]][-3000:]}")
    parts = [dict(np.load(o)) for o in outs]
    return (parts, logs) if want_logs else parts


def _assemble(parts, k, nx):
    """Concatenate the strips per cell array and per edge family (H, V, D): no duplicated row on the periodic square."""
    P = len(parts)
    nyl, nl = nx // P, k + 1
    Q = np.concatenate([d["Q"] for d in parts])
    p = np.concatenate([d["p"] for d in parts])
    fam = [[d["lam"].reshape(3, nx * nyl, nl)[f] for d in parts] for f in range(3)]
    lam = np.concatenate([np.concatenate(f) for f in fam]).ravel()
    return Q, p, lam


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _compare(parts, single, k, nx, its=True):
    Q, p, lam = _assemble(parts, k, nx)
    assert Q.shape == single["Q"].shape and lam.shape == single["lam"].shape
    assert _rel(Q, single["Q"]) < TOL and _rel(p, single["p"]) < TOL and _rel(lam, single["lam"]) < TOL, \
        (_rel(Q, single["Q"]), _rel(p, single["p"]), _rel(lam, single["lam"]))
    for d in parts[1:]:  # global values are the same on every rank
        assert np.array_equal(d["l2"], parts[0]["l2"]) and d["pint"] == parts[0]["pint"]
        assert np.array_equal(d["its"], parts[0]["its"])
    assert np.allclose(parts[0]["l2"], single["l2"], rtol=1e-7) and abs(parts[0]["pint"] - single["pint"]) < 1e-9
    if its:  # condensed CG: the same counts up to reduction order
        assert np.all(np.abs(parts[0]["its"][1:] - single["its"][1:]) <= 1.0), (parts[0]["its"], single["its"])


# (2, *): the ring of two (one peer on both sides); (4, 1, 8): strips of 2 rows, the minimum; (2, 3, 16) / (2, 4, 16): strips of
# 8 rows, the tiled preconditioner (corner / edge form); (2, 2, 18): a partial tile column; (4, 2, 256): the shear layer's size
@pytest.mark.parametrize("nranks,k,nx", [(2, 1, 8), (4, 1, 8), (3, 2, 12), (2, 2, 18), (2, 3, 16), (2, 4, 16), (4, 2, 256)])
def test_periodic_strips_match_single_rank(hip_lib, tmp_path, nranks, k, nx):
    parts = _run(nranks, k, nx, 2, tmp_path)
    single = _run(1, k, nx, 2, tmp_path)[0]
    _compare(parts, single, k, nx)
    # node coordinates: physical y in [0, L) on every strip, the strips' own rows
    xq = np.concatenate([d["xq"] for d in parts])
    assert np.allclose(xq, single["xq"], rtol=0, atol=1e-13)
    assert all(d["xq"][:, 1].min() > -1e-13 and d["xq"][:, 1].max() < L + 1e-13 for d in parts)
    tiled = nx >= 16 and nx // nranks >= 8
    assert all(int(d["trace_form"]) == (0 if not tiled else (2 if k == 4 else 1)) for d in parts)


@pytest.mark.parametrize("nranks,k,nx,extra", [
    (2, 2, 16, ("opt:trace_precond=0",)),
    (3, 2, 12, ("opt:tent_solver=0",)),
    (2, 1, 16, ("opt:tent_precond=0",)),
    (2, 2, 16, ("opt:tent_precond=1",)),
    (2, 1, 8, ("unsplit",)),
    (2, 2, 8, ("implicit",)),
    (3, 1, 12, ("implicit_mono",)),
    (2, 2, 16, ("perstep",)),
    (4, 2, 16, ("tab:imex_ars3_443",)),
])
def test_periodic_strips_other_solver_paths(hip_lib, tmp_path, nranks, k, nx, extra):
    parts = _run(nranks, k, nx, 2, tmp_path, extra)
    single = _run(1, k, nx, 2, tmp_path, extra)[0]
    _compare(parts, single, k, nx, its=False)


@pytest.mark.parametrize("nranks,k,nx", [(2, 2, 16), (3, 1, 12), (2, 3, 32)])
def test_periodic_strips_self_check_and_overlap(hip_lib, tmp_path, nranks, k, nx):
    """HDG_FLOW_CHECK: every exchange the ghost-row bookkeeping skips is carried out anyway and compared; HDG_OVERLAP: the
    interior / boundary split around the exchanges gives the same result as the plain order."""
    parts, logs = _run(nranks, k, nx, 2, tmp_path, env={"HDG_FLOW_CHECK": "1", "HDG_DEBUG": "1", "HDG_OVERLAP": "1"},
                       want_logs=True, tag="o")
    m = re.search(r"\[flow check\] (\d+) skipped exchanges verified, worst relative deviation ([0-9.eE+-]+)", logs[0])
    assert m, logs[0][-2000:]
    assert int(m.group(1)) > 20 and float(m.group(2)) < 1e-12, m.group(0)
    m2 = re.search(r"\((\d+) of them beside an interior launch\)", logs[0])
    assert m2 and int(m2.group(1)) > 10, logs[0][-2000:]
    plain = _run(nranks, k, nx, 2, tmp_path, env={"HDG_NO_OVERLAP": "1"}, tag="p")
    for a, b in zip(parts, plain):
        for f in ("Q", "p", "lam"):
            assert _rel(a[f], b[f]) < 1e-12, f


def test_periodic_strips_against_the_oracle(hip_lib, tmp_path):
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow
    from oracle import hdg_oracle as orc

    k, nx, nsteps = 1, 8, 2
    parts = _run(2, k, nx, nsteps, tmp_path)
    Q, p, lam = _assemble(parts, k, nx)
    d = orc.HDGDiscretisation(nx, k, periodic=True, L=L)
    dt = 0.25 * L / nx
    shear = DoubleLayerShearFlow(None, None)
    Q0, p0 = shear.initial_condition()
    prof = d.interpolate_velocity(lambda x, y: (np.sin(y) * np.cos(2 * x), 0.5 * np.cos(y) * np.sin(x)))
    o = orc.OracleHDGIMEX(d, dt, "imex_ssp2_332")
    oQ, op = o.solve(d.interpolate_velocity(Q0), d.interpolate_pressure(p0), lambda t: (1.0 + 0.5 * np.sin(t)) * prof, nsteps * dt)
    assert _rel(Q, oQ) < TOL and _rel(p, op) < TOL and _rel(lam, o.lam) < TOL
    assert _rel(oQ, d.interpolate_velocity(Q0)) > 1e-3


@pytest.mark.parametrize("nranks", [2, 4])
def test_periodic_strips_diagnostics(hip_lib, tmp_path, nranks):
    """The recorded series on periodic strips against one rank, with the tolerances of the unit-square strip test
    (tests/test_gpu_diagnostics.py); every rank holds the same global series."""
    from incompressibleeulerhdg_amd._lib import DIAGNOSTICS

    k, nx, nsteps = 2, 16, 3
    parts = _run(nranks, k, nx, nsteps, tmp_path, ("diag",))
    r = _run(1, k, nx, nsteps, tmp_path, ("diag",))[0]["series"]
    names = list(DIAGNOSTICS)
    for d in parts:
        s = d["series"]
        assert s.shape == r.shape == (nsteps + 1, 9)
        unorm = np.sqrt(2 * r[0, 0])
        for i, c in enumerate(names):
            if c.startswith("tracer"):
                assert np.all(np.isnan(s[:, i]))
                continue
            atol0 = 1e-13 * unorm if c in ("div_l2", "jump_l2", "p_integral") else 0.0
            assert np.allclose(s[0, i], r[0, i], rtol=1e-13, atol=atol0), (c, s[0, i], r[0, i])
            atol = 1e-10 * unorm if c in ("div_l2", "jump_l2", "p_integral") else 0.0
            assert np.allclose(s[1:, i], r[1:, i], rtol=1e-11, atol=atol), (c, s[:, i], r[:, i])
        assert s[0, 7] == r[0, 7] and s[0, 8] == r[0, 8]
        assert np.array_equal(s, parts[0]["series"], equal_nan=True)


def test_periodic_strips_refuse_the_single_rank_spaces(hip_lib, tmp_path):
    """Tracer, vorticity and the DG step stay single-rank: their existing error on a periodic strip handle."""
    parts = _run(2, 1, 8, 1, tmp_path, ("refusals",))
    for d in parts:
        assert np.all(d["codes"] < 0), d["codes"]


@pytest.mark.parametrize("nranks,nx", [(4, 4), (3, 8)])
def test_periodic_strips_refuse_bad_partitions(hip_lib, tmp_path, nranks, nx):
    """Strips thinner than the minimum (4 ranks on 4 rows: 1 row each) and ny % P != 0 are refused with HDG_ERR_ARG (-1)."""
    parts = _run(nranks, 1, nx, 1, tmp_path)
    for d in parts:
        assert int(d["create_code"]) == -1, d
    if nx % nranks == 0:
        assert "at least 2 cell rows" in str(parts[0]["create_msg"])
