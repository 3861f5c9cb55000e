"""Worker of tests/test_gpu_tracer_implicit.py: one rank of a two-strip engine that asks for the implicit tracer diffusion; the
error code and message go back to the test.

usage: tracer_implicit_strip_worker.py RANK NRANKS TOKEN OUTFILE
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, nranks, token, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    ts = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(8, 8), 1, 0.01, use_projection_method=True, n_richardson=2, rank=rank,
                                            nranks=nranks, comm_backend="shm", comm_token=token)
    code, msg = 0, ""
    try:
        ts._engine.set_tracer_diffusion_mode("implicit")
    except _lib.HDGError as e:
        code, msg = e.code, str(e)
    np.savez(out, code=code, msg=msg)


if __name__ == "__main__":
    main()
