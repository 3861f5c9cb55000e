"""Worker of tests/test_gpu_transfer.py: one rank of a strip-partitioned engine offers its strip to a one-rank engine, and the
other way round; every call must come back HDG_ERR_UNSUPPORTED naming the ranks, with the fields of both untouched.

usage: transfer_strip_worker.py RANK NRANKS TOKEN
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def main():
    rank, nranks, token = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    kw = dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    strip = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(8, 8), 1, 0.01, use_projection_method=True, n_richardson=2, **kw)
    one = IncompressibleEulerHDGIMEXSSP2_332(UnitSquareMesh(4, 4), 1, 0.01, use_projection_method=True, n_richardson=2)
    rng = np.random.default_rng(rank)
    for ts in (strip, one):
        ts._engine.set_state(rng.standard_normal(ts._engine.shape_Q), rng.standard_normal(ts._engine.shape_p))
    before = [ts._engine.get_field(0, lam=False)[:2] for ts in (strip, one)]
    for call in (lambda: one._engine.transfer_from(strip._engine), lambda: strip._engine.transfer_from(one._engine),
                 lambda: one._engine.difference_norms(strip._engine)):
        try:
            call()
        except _lib.HDGError as e:
            assert e.code == -5 and "more than one rank" in str(e), str(e)
        else:
            raise AssertionError("a strip engine was accepted")
    after = [ts._engine.get_field(0, lam=False)[:2] for ts in (strip, one)]
    for b, a in zip(before, after):
        assert np.array_equal(b[0], a[0]) and np.array_equal(b[1], a[1])
    print("refused ok")


if __name__ == "__main__":
    main()
