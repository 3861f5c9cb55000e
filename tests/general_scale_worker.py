"""Worker of tests/test_gpu_general_mesh_scale.py: Kelvin-Helmholtz runs on the unit disk in a process of its own (the engine
reads HDG_AMG_MAX_COARSE / HDG_AMG_UNFUSED when an engine is built; a process of its own keeps the cases apart).  usage: general_scale_worker.py LEVEL RUNS OUTFILE, RUNS a
comma-separated list of run names of tests/general_mesh_checks.py kh_runs: ssp2_k<K>_<fused|solve>, implicit_k<K>_<proj|mono>"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_run(name):
    kind, k, option = name.split("_")
    return name, int(k[1:]), kind, option in ("fused", "proj")


def main():
    level, names, out = int(sys.argv[1]), sys.argv[2].split(","), sys.argv[3]
    from general_mesh_checks import kh_runs
    from incompressibleeulerhdg_amd.mesh import UnitDiskMesh

    res = kh_runs(UnitDiskMesh(level), [parse_run(n) for n in names])
    np.savez(out, **{f"{n}.{f}": v for n, r in res.items() for f, v in r.items()})


if __name__ == "__main__":
    main()
