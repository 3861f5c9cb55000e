"""Worker of tests/test_gpu_moving_walls.py: one rank of a strip-partitioned run between moving no-slip walls, or the single-rank
run of the same configuration (NRANKS 1): three fused SSP2(3,3,2) steps at k = 2, nx = 8 from the Taylor-Green field, the
viscous diffusion number at 0.35, all four wall speeds non-zero; then the wall force (a collective call).

usage: moving_walls_strip_worker.py RANK NRANKS TOKEN OUTFILE
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPEEDS = (0.3, -0.7, 1.0, 0.45)


def main():
    rank, nranks, token, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    k, nx, nsteps = 2, 8, 3
    dt = 0.25 / nx
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(nx, nx), k, dt, use_projection_method=True, n_richardson=2, **kw)
    eng = ts._engine
    eng.set_viscosity(1.0, "no_slip")
    eng.set_viscosity(0.35 / (dt * eng.viscosity_number()[0]), "no_slip")
    eng.set_wall_velocity(SPEEDS)
    mp = TaylorGreen(ts._V_Q, ts._V_p)
    Q, p = ts.solve(*mp.initial_condition(), None, mp.f_rhs(), nsteps * dt, fused=True)
    np.savez(out, Q=Q.dat.data, p=p.dat.data, nu=eng.viscosity()[0], U=eng.wall_velocity(), F=eng.wall_force())


if __name__ == "__main__":
    main()
