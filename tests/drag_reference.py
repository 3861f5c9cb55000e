"""TEST INFRASTRUCTURE ONLY -- numpy reference of the linear drag term, on top of oracle/hdg_oracle.py,
tests/viscosity_reference.py and tests/moving_walls_reference.py, which it imports and does not change.

    du/dt + ... = ... - sigma(x) (u - u_s(x)),    sigma >= 0 linear on every cell, given by its three vertex values sig[c, v]

The Galerkin term D(w, u) = sum_K int_K sigma w.u on [DG_{k+1}]^2 in the nodal basis of the oracle's velocity space with the
oracle's cell rule (degree 3k + 4 >= 2k + 3: exact).  M and D are block diagonal per cell and both carry the factor det J, so a
cell's block of M^-1 D needs the reference element and the three vertex values only: the blockwise functions serve meshes of
any size without an assembled discretisation.  The term is explicit and rides in the forcing slots exactly as the viscous term
does, so the whole-step loops are those of viscosity_reference, called with moving_walls_reference.Affine(A, b),
A = nu M^-1 V + M^-1 C - M^-1 D and b = M^-1 D u_s, and nu = 1."""
import numpy as np

from moving_walls_reference import Affine, integral  # noqa: F401
from viscosity_reference import (dg_with_viscosity, imex_with_viscosity, implicit_with_viscosity, l2_error_velocity,  # noqa: F401
                                 taylor_green_Qs)

__all__ = ["reference_element", "sigma_at_points", "blocks", "apply_blocks", "drag_matrix", "minv_d", "load", "affine", "bound",
           "closed_form", "force_blockwise", "cell_areas", "mass_dot", "integral_blockwise", "Affine", "integral", "DraggedTaylorGreen", "imex_with_viscosity",
           "implicit_with_viscosity", "dg_with_viscosity", "l2_error_velocity", "taylor_green_Qs"]

_REF = {}


def reference_element(k, variant="gll"):
    """(qp [q, 2], qw [q], U [q, nu]): the oracle's cell rule and its nodal velocity basis at the rule's points"""
    from oracle.fem import PolySpace2D, triangle_quadrature

    if (k, variant) not in _REF:
        qp, qw = triangle_quadrature(3 * k + 4)
        _REF[(k, variant)] = (qp, qw, PolySpace2D(k + 1, variant).tabulate(qp))
    return _REF[(k, variant)]


def sigma_at_points(sig, qp):
    """sigma of every cell at the reference points: [nc, q] from the vertex values [nc, 3]"""
    lam = np.stack([1.0 - qp[:, 0] - qp[:, 1], qp[:, 0], qp[:, 1]], axis=0)  # [3, q]
    return np.asarray(sig, dtype=float) @ lam


def cell_areas(verts):
    """|K| from cell vertices [nc, 3, 2]"""
    a, b = verts[:, 1] - verts[:, 0], verts[:, 2] - verts[:, 0]
    return 0.5 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])


def _weighted(sig, k):
    """sum_q w_q sigma_c(q) phi_i phi_j / sum_q w_q: [nc, nu, nu], the sigma-weighted mass block per unit area"""
    qp, qw, U = reference_element(k)
    return np.einsum("q,cq,qi,qj->cij", qw / qw.sum(), sigma_at_points(sig, qp), U, U)


def blocks(sig, k):
    """The per-cell blocks of M^-1 D acting on one component: [nc, nu, nu]"""
    qp, qw, U = reference_element(k)
    Mref = np.einsum("q,qi,qj->ij", qw / qw.sum(), U, U)
    return np.linalg.solve(Mref[None], _weighted(sig, k))


def apply_blocks(B, Q, target=None):
    """- M^-1 D (Q - u_s) blockwise: what hdg_apply_drag returns; Q and target nodal [N, 2]"""
    W = np.asarray(Q, dtype=float) - (0.0 if target is None else np.asarray(target, dtype=float))
    nc, nu = B.shape[0], B.shape[1]
    return -np.einsum("cij,cjd->cid", B, W.reshape(nc, nu, 2)).reshape(-1, 2)


def force_blockwise(sig, k, areas, Q, target=None, region=None):
    """(4, 3): per region (F_x, F_y, P) = (- int sigma (u - u_s), - int sigma (u - u_s) . u) over the cells tagged r"""
    Dc = _weighted(sig, k) * np.asarray(areas)[:, None, None]  # int_K sigma phi_i phi_j
    nc, nu = Dc.shape[0], Dc.shape[1]
    u = np.asarray(Q, dtype=float).reshape(nc, nu, 2)
    w = u - (0.0 if target is None else np.asarray(target, dtype=float).reshape(nc, nu, 2))
    Dw = np.einsum("cij,cjd->cid", Dc, w)
    per_cell = np.concatenate([-Dw.sum(axis=1), -np.einsum("cid,cid->c", u, Dw)[:, None]], axis=1)  # the nodal basis sums to 1
    region = np.zeros(nc, dtype=int) if region is None else np.asarray(region)
    return np.stack([per_cell[region == r].sum(axis=0) for r in range(4)])


def _mass_ref(k):
    qp, qw, U = reference_element(k)
    return np.einsum("q,qi,qj->ij", qw / qw.sum(), U, U)


def mass_dot(k, areas, a, b):
    """a^T M b of two nodal velocity-space fields, blockwise: M's block is |K| times the reference mass matrix per unit area"""
    nc = len(areas)
    A, B = np.asarray(a, dtype=float).reshape(nc, -1, 2), np.asarray(b, dtype=float).reshape(nc, -1, 2)
    return float(np.einsum("c,cid,ij,cjd->", np.asarray(areas), A, _mass_ref(k), B))


def integral_blockwise(k, areas, f):
    """(int f_x, int f_y) of a nodal velocity-space field, blockwise"""
    nc = len(areas)
    return np.einsum("c,i,cid->d", np.asarray(areas), _mass_ref(k).sum(axis=0), np.asarray(f, dtype=float).reshape(nc, -1, 2))


def drag_matrix(d, sig):
    """D as a dense [NQ, NQ] matrix in the nodal basis (rows and columns d.dofQ)"""
    blk = np.einsum("cq,cq,qi,qj->cij", d.cwdet, sigma_at_points(sig, reference_element(d.k)[0]), d.cU, d.cU)
    D = np.zeros((d.NQ, d.NQ))
    for c in range(d.mesh.ncells):
        for comp in range(2):
            D[np.ix_(d.dofQ[c, :, comp], d.dofQ[c, :, comp])] += blk[c]
    return D


def minv_d(d, sig, D=None):
    """M^-1 D, dense"""
    D = drag_matrix(d, sig) if D is None else D
    return np.linalg.solve(d.MQ.toarray(), D)


def load(d, sig, target, A=None):
    """M^-1 D u_s as a flat vector"""
    A = minv_d(d, sig) if A is None else A
    return A @ np.asarray(target, dtype=float).ravel()


def affine(d, sig, target=None, A=None, base=None):
    """Q -> (base - M^-1 D) Q + M^-1 D u_s: the velocity-linear part of a slot with the drag on; base: nu M^-1 V + M^-1 C or None"""
    A = minv_d(d, sig) if A is None else A
    b = np.zeros(d.NQ) if target is None else load(d, sig, target, A)
    return Affine((0.0 if base is None else base) - A, b)


def bound(sig):
    """S = the largest vertex value, the derived bound of rho(M^-1 D)"""
    return float(np.max(sig))


def closed_form(sigma_xy, u, target=None):
    """- sigma (u - u_s) at the nodes, sigma_xy the values of sigma there"""
    return -np.asarray(sigma_xy)[:, None] * (np.asarray(u) - (0.0 if target is None else np.asarray(target)))


class DraggedTaylorGreen:
    """oracle.hdg_oracle.TaylorGreen with a drag towards rest: the same solution a(t) Q_s, the forcing's profile gains
    + sigma Q_s (nodal, as the package's model problem interpolates it)."""

    def __init__(self, disc, sigma, kappa=0.5):
        from oracle.hdg_oracle import TaylorGreen

        self.tg = TaylorGreen(disc, "exponential", kappa)

        def profile(x, y):
            qx, qy = taylor_green_Qs(x, y)
            s = sigma(x, y)
            return (-kappa + s) * qx, (-kappa + s) * qy

        self.profile = disc.interpolate_velocity(profile)

    def initial_condition(self):
        return self.tg.initial_condition()

    def f_rhs(self, t):
        return np.exp(-self.tg.kappa * t) * self.profile

    def solution(self, t):
        return self.tg.solution(t)
