"""Worker of tests/test_gpu_streamfunction.py, a process of its own because a switch is read when an engine is built and a
strip partition needs one process per rank.

usage: streamfunction_worker.py iterations                 prints "KIND K NX ITERATIONS" for the cases of the iteration test,
                                                           with whatever HDG_PSI_JACOBI of the environment selects
       streamfunction_worker.py strip RANK NRANKS TOKEN    one rank of a strip partition: the call has to be refused
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERATION_CASES = [(kind, k, nx) for kind in ("square", "periodic") for k in (2, 4) for nx in (8, 16)]
ITERATION_RTOL = 1e-10


def engine(kind, k, nx, **kw):
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    L = 2.0 if kind == "periodic" else 1.0
    mesh = PeriodicSquareMesh(nx, nx, L=L) if kind == "periodic" else UnitSquareMesh(nx, nx)
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, 0.125 * L / nx, use_projection_method=True, n_richardson=2, **kw)
    return ts, ts._engine


def iterations(kind, k, nx):
    """iterations of the solve for a random velocity (a random right-hand side), whatever preconditioner the environment selects"""
    _, eng = engine(kind, k, nx)
    Q = np.random.default_rng(100 * k + nx).standard_normal(eng.shape_Q)
    return eng.streamfunction(Q, rtol=ITERATION_RTOL)[1]["iterations"]


def main():
    if sys.argv[1] == "iterations":
        for kind, k, nx in ITERATION_CASES:
            print(kind, k, nx, iterations(kind, k, nx), flush=True)
        return 0
    from incompressibleeulerhdg_amd._lib import HDGError

    rank, nranks, token = int(sys.argv[2]), int(sys.argv[3]), sys.argv[4]
    _, eng = engine("square", 2, 8, rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    calls = (lambda: eng.streamfunction(), lambda: eng.psi_vertex_count())
    for call in calls:
        try:
            call()
        except HDGError as e:
            print("refused", e.code, flush=True)
            if e.code != -5:
                return 1
        else:
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
