"""Worker of tests/test_gpu_diagnostics.py: one rank of a strip-partitioned HDG-IMEX run that records the flow diagnostics.

usage: diag_strip_worker.py RANK NRANKS TOKEN K NX NSTEPS OUTFILE
Saves the recorded series (every rank receives the global values) and compute_diagnostics of its final strip fields.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, nranks, token, k, nx, nsteps, out = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                                               int(sys.argv[5]), int(sys.argv[6]), sys.argv[7])
    from incompressibleeulerhdg_amd._lib import DIAGNOSTICS
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    dt = 0.25 / nx
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(nx, nx), k, dt, use_projection_method=True, n_richardson=2, **kw)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt, fused=True, diagnostics=True)
    series = np.stack([ts.diagnostics[c] for c in DIAGNOSTICS], axis=1)
    final = ts._engine.compute_diagnostics(Q.dat.data, p.dat.data)
    np.savez(out, series=series, t=ts.diagnostics["t"], final=final)


if __name__ == "__main__":
    main()
