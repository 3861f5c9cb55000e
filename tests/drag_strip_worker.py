"""Worker of tests/test_gpu_drag.py: one rank of a strip-partitioned run with the linear drag, or the single-rank run of the same
configuration (NRANKS 1): three fused SSP2(3,3,2) steps at k = 2, nx = 8 with S dt = 0.3.  The mask, the target and the tags
are functions of position that are not symmetric in y, evaluated on the rank's own cells.

usage: drag_strip_worker.py RANK NRANKS TOKEN KIND OUTFILE       KIND: square | periodic
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, nranks, token, kind, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5]
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow, TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    k, nx, nsteps = 2, 8, 3
    L = 2 * np.pi if kind == "periodic" else 1.0
    dt = 0.25 * L / nx
    S = 0.3 / dt
    # a blob below the middle (its peak S on a vertex) that reaches across the cut between two strips, and a weaker band near the top
    sigma = lambda x, y: S * np.maximum(0.0, 1.0 - ((x - 0.375 * L) ** 2 + (y - 0.375 * L) ** 2) / (0.3 * L) ** 2) + 0.25 * S * (y > 0.8 * L) * x / L
    target = lambda x, y: (0.5 + 0.3 * np.sin(2 * np.pi * x / L) + 0.2 * y / L, -0.2 + 0.4 * np.cos(2 * np.pi * (x + 2 * y) / L))
    region = lambda x, y: (y > 0.3 * L).astype(int) + (y > 0.6 * L) + (x > 0.7 * L)
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    mesh = PeriodicSquareMesh(nx, nx, L=L) if kind == "periodic" else UnitSquareMesh(nx, nx)
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=True, n_richardson=2, drag=sigma, drag_target=target,
                                            drag_region=region, **kw)
    eng = ts._engine
    mp = (DoubleLayerShearFlow if kind == "periodic" else TaylorGreen)(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt, fused=True)
    np.savez(out, Q=Q.dat.data, p=p.dat.data, sigma=eng.drag(), number=eng.drag_number()[1], force=eng.drag_force())


if __name__ == "__main__":
    main()
