"""Worker of tests/test_gpu_probes.py: one rank of a strip-partitioned run (or the single-rank run, NRANKS 1) that evaluates
global fields at points on the cuts and records probe rows over a few steps.

usage: probe_strip_worker.py RANK NRANKS TOKEN K NX NSTEPS MESH OUTFILE       MESH: square | periodic
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def probe_points(nx, L):
    """Points on every cut of P = 2, 3, 4 (rows nx/P multiples), on vertices of the cuts, and a few interior points."""
    h = L / nx
    rng = np.random.default_rng(5)
    pts = [(x, j * h) for j in range(nx + 1) for x in (0.0, 0.37 * L, 3 * h, 0.5 * h)]
    pts += list(map(tuple, rng.random((40, 2)) * L))
    return np.array(pts)


def main():
    rank, nranks, token, k, nx, nsteps, kind, out = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                                                     int(sys.argv[5]), int(sys.argv[6]), sys.argv[7], sys.argv[8])
    from incompressibleeulerhdg_amd.mesh import Function, PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow, TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    periodic = kind == "periodic"
    L = 2 * np.pi if periodic else 1.0
    mesh = PeriodicSquareMesh(nx, nx, L=L) if periodic else UnitSquareMesh(nx, nx)
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    dt = 0.25 * L / nx
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=True, n_richardson=2, **kw)
    eng = ts._engine
    xy = probe_points(nx, L)
    # global smooth fields, interpolated on this rank's strip
    ux = lambda x, y: np.sin(2 * np.pi * x / L) * np.cos(2 * np.pi * y / L) + 0.3 * y  # noqa: E731
    uy = lambda x, y: -np.cos(2 * np.pi * x / L) * np.sin(2 * np.pi * y / L) + 0.2 * x * y  # noqa: E731
    Q0 = ts._V_Q.interpolate(lambda x, y: (ux(x, y), uy(x, y)))
    p0 = ts._V_p.interpolate(lambda x, y: np.cos(x + 2 * y) + x)
    vals, located = eng.evaluate_points(xy, Q0, p0, 2 * p0)
    at_u = Function(ts._V_Q, Q0).at(xy[:5])
    # recorded rows over a few steps of the model problem of the mesh (as the other strip tests run it)
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p) if periodic else TaylorGreen(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt, fused=True, probes=xy)
    np.savez(out, vals=vals, located=located, at_u=at_u, u=ts.probes["u"], p=ts.probes["p"], q=ts.probes["q"],
             omega=ts.probes["omega"], xy=xy)


if __name__ == "__main__":
    main()
