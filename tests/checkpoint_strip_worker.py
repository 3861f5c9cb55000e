"""Worker of tests/test_gpu_checkpoint.py: one rank of a strip-partitioned run of 6 steps that is either uninterrupted, killed
after the checkpoint of step 3, or restarted from that checkpoint (after first being offered the other rank's file).

usage: checkpoint_strip_worker.py RANK NRANKS TOKEN MESH MODE PATH OUTFILE    MESH: square | periodic   MODE: full | first | restart
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

NSTEPS, NSAVE = 6, 3


class Killed(Exception):
    pass


class KillAfter:
    def __init__(self, nsteps):
        self.nsteps, self.calls = nsteps, 0

    def reset(self):
        self.calls = 0

    def __call__(self, Q, p, t, q_tracer=None):
        self.calls += 1
        if self.calls == self.nsteps + 1:
            raise Killed()


def main():
    rank, nranks, token, kind, mode, path, out = (int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4], sys.argv[5],
                                                  sys.argv[6], sys.argv[7])
    from incompressibleeulerhdg_amd._lib import HDGError
    from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh
    from incompressibleeulerhdg_amd.model_problems import DoubleLayerShearFlow, TaylorGreen
    from incompressibleeulerhdg_amd.timesteppers import IncompressibleEulerHDGIMEXSSP2_332

    periodic = kind == "periodic"
    k, nx = 2, 24
    L = 2 * np.pi if periodic else 1.0
    mesh = PeriodicSquareMesh(nx, nx, L=L) if periodic else UnitSquareMesh(nx, nx)
    dt = 0.25 * L / nx
    callbacks = [KillAfter(NSAVE)] if mode == "first" else None
    ts = IncompressibleEulerHDGIMEXSSP2_332(mesh, k, dt, use_projection_method=True, n_richardson=2, callbacks=callbacks,
                                            rank=rank, nranks=nranks, comm_backend="shm", comm_token=token)
    mp = DoubleLayerShearFlow(ts._V_Q, ts._V_p) if periodic else TaylorGreen(ts._V_Q, ts._V_p)
    kw = dict(fused=True)
    if periodic:  # particles on both sides of the cut and anywhere
        rng = np.random.default_rng(11)
        kw.update(particles=(0.05 + 0.9 * rng.random((24, 2))) * L, particle_every=2)
    extra = {}
    if mode == "full":
        ts.solve(*mp.initial_condition(), None, mp.f_rhs(), NSTEPS * dt, **kw)
    elif mode == "first":
        try:
            ts.solve(*mp.initial_condition(), None, mp.f_rhs(), NSTEPS * dt, checkpoint=path, checkpoint_every=NSAVE, **kw)
        except Killed:
            np.savez(out, killed=1)
            return
        raise SystemExit("the run was not killed")
    else:
        e = ts._engine
        before = e.state_digest()
        try:  # the other rank's blob: refused before anything collective happens, the engine stays what it was
            e.load_checkpoint(open(f"{path}.{1 - rank}", "rb").read())
            raise SystemExit("the other rank's blob was accepted")
        except HDGError as err:
            extra["refusal"] = str(err)
        if e.state_digest() != before:
            raise SystemExit("a refused load changed the engine")
        ts.solve(None, None, None, mp.f_rhs(), NSTEPS * dt, restart=path, **kw)
    e = ts._engine
    digest = np.array(e.state_digest(), dtype=np.uint64)
    sums, counts = e.iteration_stats()
    Q, p, lam = e.get_field(0)
    uQ, up, ul = e.get_field(-1)
    res = dict(digest=digest, it_sums=sums, it_counts=counts, events=np.array(list(e.solver_events().values())), Q=Q, p=p, lam=lam,
               upd_Q=uQ, upd_p=up, upd_lam=ul, stage1_Q=e.get_field(1)[0], tent1=e.get_field(101, p=False, lam=False)[0])
    # the digest of every section a checkpoint of the final state holds: says WHICH vector differs when one does
    import struct

    blob = e.save_checkpoint(NSTEPS, NSTEPS * dt)
    nsec, fp_len = struct.unpack_from("<I", blob, 12)[0], struct.unpack_from("<Q", blob, 40)[0]
    for i in range(nsec):
        ident, _, _, _, _, d0, d1 = struct.unpack_from("<24sIIQQQQ", blob, 64 + (fp_len + 7) // 8 * 8 + 64 * i)
        res["section_" + ident.split(b"\0")[0].decode()] = np.array([d0, d1], dtype=np.uint64)
    if periodic:
        P = ts.particles
        res.update(particle_rows=P["xy"], particle_t=P["t"], clamped=P["clamped"], lost=P["lost"])
    np.savez(out, **res, **extra)


if __name__ == "__main__":
    main()
