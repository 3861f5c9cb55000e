"""TEST INFRASTRUCTURE ONLY -- numpy / scipy twin of the stream-function diagnostic (include/hdg_streamfunction.h, DESIGN.md
section 27), assembled from the oracle's tables (HDGDiscretisation.cUg, cU, cwdet; R, cg_of_dg, cg_coords as TracerOracle has them).

psi in CG_{k+1} with (grad psi, grad tau) = int (u_x d_y tau - u_y d_x tau) dx for all tau, no essential boundary condition.
Gauge: the arithmetic mean over the 4 nx boundary mesh vertices of the unit square, over all mesh vertices of the periodic
square, is zero.  Nothing here touches the GPU library; the engine's dofs are matched to the oracle's by coordinates
(StreamfunctionReference.to_engine), as the vorticity tests do.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

from oracle.hdg_oracle import HDGDiscretisation

__all__ = ["StreamfunctionReference", "ContinuousSpace", "PSI_K1", "PSI_K2"]


class _Tables(HDGDiscretisation):
    """The oracle's mesh, spaces and quadrature tables without its assembled HDG operators, which the stream function does not
    use and which take minutes at nx = 130."""

    def _build_constant_operators(self):
        pass


class ContinuousSpace:
    """CG_{k+1} as the coincident nodes of the broken space: R, cg_of_dg, cg_coords, ncg exactly as oracle.tracer_oracle.TracerOracle
    builds them (tests/test_streamfunction_cpu.py holds the two against each other), without its mass-matrix factorisations."""

    def __init__(self, d):
        m = d.mesh
        nc, nu = m.ncells, d.nu
        X = d.node_coords(d.PU).reshape(-1, 2)
        key = np.round(X * (m.nx * 1e6 / m.L)).astype(np.int64)
        if m.periodic:
            key = key % int(round(m.nx * 1e6))
        _, first, inv = np.unique(key, axis=0, return_index=True, return_inverse=True)
        self.cg_of_dg = inv.reshape(-1)
        self.ncg = int(self.cg_of_dg.max()) + 1
        self.cg_coords = X[first]
        self.R = sp.csr_matrix((np.ones(nc * nu), (np.arange(nc * nu), self.cg_of_dg)), shape=(nc * nu, self.ncg))


def PSI_K1(x, y):
    """psi* = x^2 - x y and its curl (d_y psi, -d_x psi)"""
    return x * x - x * y, (-x, y - 2.0 * x)


def PSI_K2(x, y):
    """psi* = x^2 y - y^2 + x^3 / 2 and its curl"""
    return x * x * y - y * y + 0.5 * x ** 3, (x * x - 2.0 * y, -2.0 * x * y - 1.5 * x * x)


class StreamfunctionReference:
    def __init__(self, nx, k, periodic=False, L=1.0):
        self.nx, self.k, self.periodic, self.L = nx, k, periodic, float(L)
        self.d = d = _Tables(nx, k, periodic=periodic, L=L)
        self.tr = tr = ContinuousSpace(d)
        m = d.mesh
        nc, nu = m.ncells, d.nu
        self.ncg = tr.ncg
        self.h = self.L / nx
        self.vs = nx if periodic else nx + 1  # vertices per row: vertex (i, j) is column j * vs + i, the engine's numbering
        self.nv = self.vs * self.vs
        # ---- stiffness matrix K = R^T blockdiag(int grad phi_i . grad phi_j) R
        Kc = np.einsum("cq,cqid,cqjd->cij", d.cwdet, d.cUg, d.cUg)
        rows = (np.arange(nc * nu).reshape(nc, nu)[:, :, None] + np.zeros((1, 1, nu), dtype=np.int64)).reshape(-1)
        cols = (np.arange(nc * nu).reshape(nc, nu)[:, None, :] + np.zeros((1, nu, 1), dtype=np.int64)).reshape(-1)
        Kb = sp.csr_matrix((Kc.reshape(-1), (rows, cols)), shape=(nc * nu, nc * nu))
        self.K = (tr.R.T @ Kb @ tr.R).tocsr()
        # ---- nested P1 interpolation P (ncg x nv): barycentric coordinates of every node in its cell
        xi, eta = d.PU.nodes[:, 0], d.PU.nodes[:, 1]
        lam = np.stack([1.0 - xi - eta, xi, eta], axis=1)  # [nu, 3]: weights of the cell's vertices 0, 1, 2
        vcol = self._vertex_column(m.cell_vertices.reshape(-1, 2)).reshape(nc, 3)
        _, first = np.unique(tr.cg_of_dg, return_index=True)  # one broken node per continuous dof
        cell, node = first // nu, first % nu
        prow = np.repeat(np.arange(self.ncg), 3)
        self.P = sp.csr_matrix((lam[node].reshape(-1), (prow, vcol[cell].reshape(-1))), shape=(self.ncg, self.nv))
        self.P.sum_duplicates()
        # ---- gauge functional: mean over the boundary vertices | all vertices, as a vector on the continuous dofs
        V = self.vertex_coordinates()
        on = np.ones(self.nv, dtype=bool)
        if not periodic:
            t = 1e-9 * self.L
            on = (V[:, 0] < t) | (V[:, 0] > self.L - t) | (V[:, 1] < t) | (V[:, 1] > self.L - t)
        assert on.sum() == (self.nv if periodic else 4 * nx)
        vdof = self._cg_dof_at(V)  # continuous dof of every vertex
        self.vertex_dof = vdof
        self.gauge = np.zeros(self.ncg)
        self.gauge[vdof[on]] = 1.0 / on.sum()
        A = sp.bmat([[self.K, sp.csr_matrix(self.gauge[:, None])], [sp.csr_matrix(self.gauge[None, :]), None]]).tocsc()
        self._lu = spla.splu(A)
        self._coarse = None

    # ------------------------------------------------------------------ numbering
    def _key(self, X):
        key = np.round(np.asarray(X) * (self.nx * 1e6 / self.L)).astype(np.int64)
        return key % int(round(self.nx * 1e6)) if self.periodic else key

    def _vertex_column(self, X):
        ij = np.round(np.asarray(X) / self.h).astype(np.int64)
        if self.periodic:
            ij = ij % self.nx
        return ij[:, 1] * self.vs + ij[:, 0]

    def vertex_coordinates(self):
        j, i = np.divmod(np.arange(self.nv), self.vs)
        return np.stack([i * self.h, j * self.h], axis=1)

    def _cg_dof_at(self, X):
        table = {tuple(k): n for n, k in enumerate(self._key(self.tr.cg_coords))}
        return np.array([table[tuple(k)] for k in self._key(X)], dtype=np.int64)

    def to_engine(self, engine_xy):
        """index array ix with  v_oracle[ix] = the vector in the engine's dof order (engine_xy = Engine.cg_coordinates())"""
        ix = self._cg_dof_at(engine_xy)
        assert len(ix) == self.ncg and len(np.unique(ix)) == self.ncg
        return ix

    # ------------------------------------------------------------------ forms
    def rhs(self, Q):
        """b_n = int (u_x d_y phi_n - u_y d_x phi_n) dx of the broken nodal velocity Q [nc*nu, 2]"""
        d = self.d
        Qc = np.asarray(Q).reshape(d.mesh.ncells, d.nu, 2)
        Qq = np.einsum("qa,cad->cqd", d.cU, Qc)
        b = np.einsum("cq,cqi,cq->ci", d.cwdet, d.cUg[..., 1], Qq[..., 0]) - np.einsum("cq,cqi,cq->ci", d.cwdet, d.cUg[..., 0], Qq[..., 1])
        return self.tr.R.T @ b.reshape(-1)

    def solve(self, Q):
        """the gauged psi (oracle dof order) by a direct solve"""
        return self._lu.solve(np.concatenate([self.rhs(Q), [0.0]]))[:-1]

    def mean_flow(self, Q):
        d = self.d
        if not self.periodic:
            return np.zeros(2)
        Qq = np.einsum("qa,cad->cqd", d.cU, np.asarray(Q).reshape(d.mesh.ncells, d.nu, 2))
        return np.einsum("cq,cqd->d", d.cwdet, Qq) / self.L ** 2

    def curl(self, psi):
        """curl psi = (d_y psi, -d_x psi) at the quadrature points [c, q, 2]"""
        d = self.d
        pc = (self.tr.R @ psi).reshape(d.mesh.ncells, d.nu)
        g = np.einsum("cqid,ci->cqd", d.cUg, pc)
        return np.stack([g[..., 1], -g[..., 0]], axis=-1)

    def defect(self, Q, psi):
        """(|u - ubar - curl psi|_{L2}, |u|_{L2});  ubar = 0 on the unit square"""
        d = self.d
        Qq = np.einsum("qa,cad->cqd", d.cU, np.asarray(Q).reshape(d.mesh.ncells, d.nu, 2))
        e = Qq - self.mean_flow(Q)[None, None, :] - self.curl(psi)
        return (float(np.sqrt(np.einsum("cq,cqd,cqd->", d.cwdet, e, e))), float(np.sqrt(np.einsum("cq,cqd,cqd->", d.cwdet, Qq, Qq))))

    def defect_floor(self, Q, psi):
        """What double precision leaves of the defect: u - curl psi is formed from sums of n_u products, d_y psi = sum_i d_y phi_i
        psi_i with |d phi_i| ~ p^2 / h, so each value carries a rounding error of up to n_u eps (sum_i |grad phi_i| |psi_i| + |u|);
        the L2 norm of that bound, once for the twin and once for the device."""
        d = self.d
        pc = np.abs(self.tr.R @ psi).reshape(d.mesh.ncells, d.nu)
        g = np.einsum("cqid,ci->cqd", np.abs(d.cUg), pc)
        Qq = np.einsum("qa,cad->cqd", np.abs(d.cU), np.abs(np.asarray(Q)).reshape(d.mesh.ncells, d.nu, 2))
        b = g[..., ::-1] + Qq
        return 2.0 * d.nu * np.finfo(float).eps * float(np.sqrt(np.einsum("cq,cqd,cqd->", d.cwdet, b, b)))

    def shift(self, psi):
        """psi moved into the gauge"""
        return psi - float(self.gauge @ psi)

    # ------------------------------------------------------------------ preconditioned CG with an exact coarse solve
    def _coarse_solve(self, rc):
        if self._coarse is None:
            Ac = (self.P.T @ self.K @ self.P).tocsr()
            one = sp.csr_matrix(np.full((self.nv, 1), 1.0 / self.nv))
            self._coarse = spla.splu(sp.bmat([[Ac, one], [one.T, None]]).tocsc())
        return self._coarse.solve(np.concatenate([rc - rc.mean(), [0.0]]))[:-1]

    def pcg(self, b, rtol, two_level=True, maxit=5000):
        """iterations of CG on K x = b with z = r / diag(K) [+ P Ac^-1 P^T r], stopped at (r, z) <= rtol^2 (r0, z0); returns
        (x, iterations)"""
        dg = self.K.diagonal()

        def B(r):
            z = r / dg
            return z + self.P @ self._coarse_solve(self.P.T @ r) if two_level else z

        x = np.zeros_like(b)
        r = b - b.mean()
        z = B(r)
        p = z.copy()
        rz = rz0 = float(r @ z)
        for it in range(1, maxit + 1):
            Kp = self.K @ p
            alpha = rz / float(p @ Kp)
            x += alpha * p
            r -= alpha * Kp
            z = B(r)
            rzn = float(r @ z)
            if rzn <= rtol * rtol * rz0:
                return x, it
            p = z + (rzn / rz) * p
            rz = rzn
        raise RuntimeError("reference PCG did not converge")
