"""CPU checker of the transfer between nested structured meshes (helper of the transfer tests, not a test module).

An independent numpy L2 projection built on ``probe_reference.PointEvaluator``: the nodal bases of the oracle
(``fem.PolySpace2D`` of the engine's node family), the cells' affine maps read off the node coordinates, and the evaluator's
floating-point ownership rule to find the coarse cell of a fine cell (through its centroid).  Nothing here uses the engine's
modal basis, its transfer tables or its integer child enumeration.

Every integral is a quadrature of degree 12 >= (4 + 1) + (4 + 1) over the cells of the FINER of the two meshes, on which both
fields are polynomials: a prolongation projects cell by cell, a restriction sums each coarse cell's right-hand side and mass
matrix over its children, and the norm of a difference is summed over the fine cells.
"""
import numpy as np

from oracle import fem

from probe_reference import PointEvaluator, node_coordinates

QUAD_DEGREE = 12


def evaluator(nx, k, L=1.0, periodic=False, xq=None):
    """PointEvaluator of the (nx, k) engine; xq: its velocity node coordinates (default: the oracle mesh's)."""
    if xq is None:
        xq = node_coordinates(fem.Mesh(nx, periodic=periodic, L=L), k + 1)
    ev = PointEvaluator(k, xq, square=(nx, nx, L, periodic))
    ev.nx = nx
    return ev


def nodes(ev, which):
    """Node coordinates (ncells * ndof, 2) of the velocity ("u") or scalar ("p") space, in the host layout."""
    V = ev.Vu if which == "u" else ev.Vp
    v0, J = _affine(ev)
    return (v0[:, None, :] + np.einsum("cdr,qr->cqd", J, V.nodes)).reshape(-1, 2)


def _affine(ev):
    X = ev.xq
    v0, v1, v2 = X[:, 0], X[:, ev.k + 1], X[:, -1]
    return v0, np.stack([v1 - v0, v2 - v0], axis=-1)  # x = v0 + J xi


class _Pair:
    """Quadrature points of every cell of the finer mesh, with their reference coordinates in the owning coarse cell."""

    def __init__(self, fine, coarse):
        self.fine, self.coarse = fine, coarse
        self.ref, w = fem.triangle_quadrature(QUAD_DEGREE)
        v0, J = _affine(fine)
        self.w = w[None, :] * np.abs(np.linalg.det(J))[:, None]  # (cells, q)
        x = v0[:, None, :] + np.einsum("cdr,qr->cqd", J, self.ref)
        centroid = v0 + J @ np.array([1.0 / 3.0, 1.0 / 3.0])
        self.owner = np.array([coarse.locate(cx, cy)[0] for cx, cy in centroid])
        cv0, cJ = _affine(coarse)
        self.cref = np.einsum("crd,cqd->cqr", np.linalg.inv(cJ)[self.owner], x - cv0[self.owner][:, None, :])
        assert self.cref.min() > -1e-12 and (1.0 - self.cref.sum(axis=-1)).min() > -1e-12  # the meshes are nested

    def basis(self, which):
        """(fine basis at the points (q, nf), coarse basis at the points (cells, q, nc))"""
        Vf = self.fine.Vu if which == "u" else self.fine.Vp
        Vc = self.coarse.Vu if which == "u" else self.coarse.Vp
        return Vf.tabulate(self.ref), Vc.tabulate(self.cref)


def _columns(field, ndof):
    f = np.asarray(field, dtype=float)
    return f.reshape(-1, ndof, 1) if f.ndim == 1 else f.reshape(-1, ndof, f.shape[-1])


def project(src, dst, field, which):
    """L2 projection of the nodal `field` of evaluator `src` (velocity "u": (N, 2), scalar "p": (N,)) onto `dst`'s space."""
    shape_tail = np.asarray(field).shape[1:]
    if dst.nx >= src.nx:  # prolongation (or a change of degree): cell by cell of the destination
        pair = _Pair(dst, src)
        phi_f, phi_c = pair.basis(which)
        u = np.einsum("cqn,cnd->cqd", phi_c, _columns(field, phi_c.shape[-1])[pair.owner])
        M = np.einsum("cq,qi,qj->cij", pair.w, phi_f, phi_f)
        b = np.einsum("cq,qi,cqd->cid", pair.w, phi_f, u)
        out = np.linalg.solve(M, b)
    else:  # restriction: every coarse cell sums over its children
        pair = _Pair(src, dst)
        phi_f, phi_c = pair.basis(which)
        u = np.einsum("qn,cnd->cqd", phi_f, _columns(field, phi_f.shape[-1]))
        nc = len(dst.xq)
        M = np.zeros((nc, phi_c.shape[-1], phi_c.shape[-1]))
        b = np.zeros((nc, phi_c.shape[-1], u.shape[-1]))
        np.add.at(M, pair.owner, np.einsum("cq,cqi,cqj->cij", pair.w, phi_c, phi_c))
        np.add.at(b, pair.owner, np.einsum("cq,cqi,cqd->cid", pair.w, phi_c, u))
        out = np.linalg.solve(M, b)
    return out.reshape((-1,) + shape_tail)


def difference_norm(a, b, fa, fb, which):
    """L2 norm of fa (on evaluator a) - fb (on evaluator b) by quadrature on the finer mesh."""
    (fine, ff), (coarse, fc) = ((a, fa), (b, fb)) if a.nx >= b.nx else ((b, fb), (a, fa))
    pair = _Pair(fine, coarse)
    phi_f, phi_c = pair.basis(which)
    uf = np.einsum("qn,cnd->cqd", phi_f, _columns(ff, phi_f.shape[-1]))
    uc = np.einsum("cqn,cnd->cqd", phi_c, _columns(fc, phi_c.shape[-1])[pair.owner])
    return float(np.sqrt(np.einsum("cq,cqd->", pair.w, (uf - uc) ** 2)))
