"""Worker of tests/test_gpu_tracer_walls.py: one rank of a two-strip engine that tries to set tracer walls; the error code and
message, and the message hdg_set_tracer gives on the same handle, go back to the test.

usage: tracer_walls_strip_worker.py RANK NRANKS TOKEN OUTFILE
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
                                            nranks=nranks, comm_backend="shm", comm_token=token, n_tracers=2)
    eng = ts._engine
    code, msg, tracer_msg = 0, "", ""
    try:
        eng.set_tracer_walls([{"bottom": 1.0}, {}])
    except _lib.HDGError as e:
        code, msg = e.code, str(e)
    try:
        eng.set_tracer(np.zeros(eng.shape_q))
    except _lib.HDGError as e:
        tracer_msg = str(e)
    np.savez(out, code=code, msg=msg, tracer_msg=tracer_msg)


if __name__ == "__main__":
    main()
