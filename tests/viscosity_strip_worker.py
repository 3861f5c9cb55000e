"""Worker of tests/test_gpu_viscosity.py: one rank of a strip-partitioned viscous run, or the single-rank run of the same
configuration (NRANKS 1): three fused SSP2(3,3,2) steps at k = 2, nx = 8 with the viscous diffusion number at 0.35.

usage: viscosity_strip_worker.py RANK NRANKS TOKEN KIND WALL OUTFILE       KIND: square | periodic
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, nranks, token, kind, wall, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5], sys.argv[6]
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow, TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    k, nx, nsteps = 2, 8, 3
    L = 2 * np.pi if kind == "periodic" else 1.0
    dt = 0.25 * L / nx
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    mesh = PeriodicSquareMesh(nx, nx, L=L) if kind == "periodic" else UnitSquareMesh(nx, nx)
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=True, n_richardson=2, **kw)
    eng = ts._engine
    eng.set_viscosity(1.0, wall)
    eng.set_viscosity(0.35 / (dt * eng.viscosity_number()[0]), wall)
    mp = (DoubleLayerShearFlow if kind == "periodic" else TaylorGreen)(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt, fused=True)
    np.savez(out, Q=Q.dat.data, p=p.dat.data, nu=eng.viscosity()[0], number=eng.viscosity_number()[1],
             other=eng.launch_stats()["other"][0])


if __name__ == "__main__":
    main()
