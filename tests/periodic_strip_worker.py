"""Worker of tests/test_gpu_periodic_strips.py: one rank of a strip-partitioned run on the doubly periodic square (the
double-layer shear flow's initial state plus a smooth forcing), or the single-rank run of the same configuration (NRANKS 1).

usage: periodic_strip_worker.py RANK NRANKS TOKEN K NX NSTEPS OUTFILE [flags] [tab:NAME] [opt:NAME=INT ...]
flags: unsplit (monolithic IMEX), implicit / implicit_mono (IncompressibleEulerHDGImplicit, projection / monolithic),
       perstep (per-solve loop instead of hdg_step), diag (record the flow diagnostics), refusals (try the single-rank
       entry points on the strip handle)
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    rank, nranks, token, k, nx, nsteps, out = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], int(sys.argv[4]),
                                               int(sys.argv[5]), int(sys.argv[6]), sys.argv[7])
    flags = sys.argv[8:]
    opts = {a[4:].split("=")[0]: int(a.split("=")[1]) for a in flags if a.startswith("opt:")}
    tab = next((a[4:] for a in flags if a.startswith("tab:")), "imex_ssp2_332")
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd._lib import DIAGNOSTICS
    from incompressibleeulerhdg_amd.driver import TIMESTEPPERS
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow, SeparableForcing
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGImplicit

    L = 2 * np.pi
    dt = 0.25 * L / nx
    kw = {} if nranks == 1 else dict(rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    mesh = PeriodicSquareMesh(nx, nx, L=L)
    try:
        if "implicit" in flags or "implicit_mono" in flags:
            ts = IncompressibleEulerHDGImplicit(mesh, k, dt, use_projection_method="implicit" in flags, n_richardson=2, **kw,
                                                **opts)
        else:
            ts = TIMESTEPPERS[tab](mesh, k, dt, use_projection_method="unsplit" not in flags, n_richardson=2, **kw, **opts)
    except _lib.HDGError as e:  # a refused partition: the code and message go back to the test
        np.savez(out, create_code=e.code, create_msg=str(e))
        return
    eng = ts._engine
    if "refusals" in flags:
        # the continuous space (tracer, vorticity) and the DG discretisation stay single-rank: their existing error
        codes = []
        for call in (lambda: eng.set_tracer(np.zeros(eng.shape_p)), lambda: eng.vorticity(np.zeros(eng.shape_Q)),
                     lambda: eng.dg_implicit_step()):
            try:
                call()
                codes.append(0)
            except _lib.HDGError as e:
                codes.append(e.code)
            except TypeError:
                codes.append(1)  # wrong Python signature: not what is being tested
        np.savez(out, codes=np.array(codes))
        return
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p)
    profile = ts._V_Q.interpolate(lambda x, y: (np.sin(y) * np.cos(2 * x), 0.5 * np.cos(y) * np.sin(x)))
    forcing = SeparableForcing(profile, lambda t: 1.0 + 0.5 * np.sin(t))
    fkw = {} if ("implicit" in flags or "implicit_mono" in flags) else {"fused": "perstep" not in flags}
    Q, p = ts.solve(*mp.initial_condition(), None, forcing, nsteps * dt, diagnostics="diag" in flags, **fkw)
    lam = eng.get_field(_lib.HDG_STATE_CURRENT, Q=False, p=False)[2]
    xq, xp = eng.node_coordinates()
    sums, cnt = eng.iteration_stats()
    res = dict(Q=Q.dat.data, p=p.dat.data, lam=lam, xq=xq, xp=xp, its=sums / np.maximum(cnt, 1),
               l2=np.array(eng.l2_norms(Q.dat.data, p.dat.data)), pint=eng.integrate_pressure(p.dat.data),
               trace_form=eng.kernel_forms()["trace_precond"])
    if "diag" in flags:
        res["series"] = np.stack([ts.diagnostics[c] for c in DIAGNOSTICS], axis=1)
    np.savez(out, **res)


if __name__ == "__main__":
    main()
