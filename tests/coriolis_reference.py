"""TEST INFRASTRUCTURE ONLY -- numpy reference of the Coriolis term, on top of oracle/hdg_oracle.py and
tests/viscosity_reference.py, which it imports and does not change.

    du/dt + ... = ... - f_c(y) k x u,    f_c = f0 + beta y,    - f_c k x u = (f_c u_y, - f_c u_x)

The Galerkin term C(w, u) = sum_K int_K f_c (w_x u_y - w_y u_x) on [DG_{k+1}]^2, assembled in the nodal basis of the oracle's
velocity space with the oracle's cell rule (degree 3k + 4 >= 2k + 3: exact).  The term is explicit and rides in the forcing
slots exactly as the viscous term does, so the whole-step loops are those of viscosity_reference, called with
A = nu M^-1 V + M^-1 C and nu = 1: they are generic in A."""
import numpy as np

from viscosity_reference import (dg_with_viscosity, imex_with_viscosity, implicit_with_viscosity, kinetic_energy,  # noqa: F401
                                 l2_error_velocity, taylor_green_Qs)

__all__ = ["coriolis_matrix", "minv_c", "vertex_bound", "closed_form", "RotatingTaylorGreen", "imex_with_viscosity",
           "implicit_with_viscosity", "dg_with_viscosity", "kinetic_energy", "l2_error_velocity", "taylor_green_Qs"]


def _cell_points(d):
    """physical coordinates of the cell rule's points, [nc, nq, 2]"""
    from oracle.fem import triangle_quadrature

    m = d.mesh
    qp, _ = triangle_quadrature(3 * d.k + 4)
    return m.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,qr->cqd", m.J, qp)


def coriolis_matrix(d, f0, beta):
    """C as a dense [NQ, NQ] matrix in the nodal basis (rows and columns d.dofQ): C[i, j] = C(phi_i, phi_j)."""
    fc = f0 + beta * _cell_points(d)[..., 1]
    blk = np.einsum("cq,cq,qi,qj->cij", d.cwdet, fc, d.cU, d.cU)  # int_K f_c phi_i phi_j
    C = np.zeros((d.NQ, d.NQ))
    for c in range(d.mesh.ncells):
        C[np.ix_(d.dofQ[c, :, 0], d.dofQ[c, :, 1])] += blk[c]   # w_x u_y
        C[np.ix_(d.dofQ[c, :, 1], d.dofQ[c, :, 0])] -= blk[c]   # - w_y u_x
    return C


def minv_c(d, f0, beta, C=None):
    """M^-1 C, dense: what hdg_apply_coriolis applies to Q.ravel()."""
    C = coriolis_matrix(d, f0, beta) if C is None else C
    return np.linalg.solve(d.MQ.toarray(), C)


def vertex_bound(d, f0, beta):
    """F = max over the mesh vertices of |f_c|, the derived bound of rho(M^-1 C)"""
    return float(np.max(np.abs(f0 + beta * d.mesh.cell_vertices[..., 1])))


def closed_form(f0, beta, x, y, u):
    """(f_c u_y, - f_c u_x) at the points"""
    fc = f0 + beta * y
    return np.stack([fc * u[:, 1], -fc * u[:, 0]], axis=-1)


class RotatingTaylorGreen:
    """oracle.hdg_oracle.TaylorGreen in a rotating frame: the same solution a(t) Q_s, the forcing gains a(t) f_c k x Q_s
    (nodal, as the package's model problem interpolates it) and 2 pi^2 nu a(t) Q_s."""

    def __init__(self, disc, kappa=0.5, viscosity=0.0, coriolis=(0.0, 0.0)):
        from oracle.hdg_oracle import TaylorGreen

        self.tg = TaylorGreen(disc, "exponential", kappa)
        self.viscosity = viscosity
        f0, beta = coriolis
        c = -kappa + 2.0 * np.pi ** 2 * viscosity

        def profile(x, y):
            qx, qy = taylor_green_Qs(x, y)
            fc = f0 + beta * y
            return c * qx - fc * qy, c * qy + fc * qx

        self.profile = disc.interpolate_velocity(profile)

    def initial_condition(self):
        return self.tg.initial_condition()

    def f_rhs(self, t):
        return np.exp(-self.tg.kappa * t) * self.profile

    def solution(self, t):
        return self.tg.solution(t)
