"""TEST INFRASTRUCTURE ONLY -- numpy reference of the moving no-slip walls and the viscous wall force, on
top of tests/viscosity_reference.py, which it imports and does not change.

Sides of the unit square in the order bottom (y = 0), right (x = 1), top (y = 1), left (x = 0); U_w is the Cartesian tangential
speed of side w: the wall's u_x on bottom and top, its u_y on left and right.  With wall = "no_slip" the tangential Nitsche term
of the viscous form V acts on u.t - U_w, so the momentum equation gains nu M^-1 l(U),

    l(w; U) = sum_{wall e on side s} U_s int_e ( eta_b (w.t) - t.dn w ) ds,       t = e_x on bottom / top, e_y on left / right

and the viscous force on the fluid through side w is the form tested against the constants e_c, restricted to w:

    F_w . e_c = nu int_w (e_c.n)( n.dn u - eta_b u.n ) ds                          always
              + nu int_w (e_c.t)( t.dn u - eta_b (u.t - U_w) ) ds                  no slip only

so that sum_w F_w = int nu M^-1 (V u + l(U)) dx for every broken u.  Assembled in the nodal basis of the oracle's velocity space
with its exact edge rule, as viscosity_reference.viscous_matrix.  The loops are those of viscosity_reference with M^-1 l(U)
placed wherever M^-1 V Q is: they take the affine map Q -> A Q + b in the place of the matrix A."""
import numpy as np

import viscosity_reference as vr

__all__ = ["SIDES", "speeds", "side_of_edges", "unit_loads", "load_vector", "force_functionals", "wall_force", "Affine", "affine",
           "imex_with_moving_walls", "implicit_with_moving_walls", "dg_with_moving_walls", "integral"]

SIDES = ("bottom", "right", "top", "left")
TANGENTIAL = (0, 1, 0, 1)  # the Cartesian component along side w


def speeds(U):
    """{side: speed} or four values -> (4,)"""
    if isinstance(U, dict):
        out = np.zeros(4)
        for s, u in U.items():
            out[SIDES.index(s)] = float(u)
        return out
    out = np.asarray(U, dtype=float).reshape(-1)
    assert out.shape == (4,)
    return out


def side_of_edges(d):
    """The side index of every boundary edge of the unit square, in the order of d.ebnd."""
    m, eb = d.mesh, d.ebnd
    mid = 0.5 * (m.edge_a[eb] + m.edge_b[eb])
    L = float(np.max(m.edge_b[:, 0]))
    tol = 1e-9 * L
    side = np.full(len(eb), -1)
    side[np.abs(mid[:, 1]) < tol] = 0
    side[np.abs(mid[:, 0] - L) < tol] = 1
    side[np.abs(mid[:, 1] - L) < tol] = 2
    side[np.abs(mid[:, 0]) < tol] = 3
    assert np.all(side >= 0)
    return side


def _wall_edges(d):
    """(cells, side, lv [m, nu], |e| eta_b [m]) of the boundary edges: lv[i] = int_e ( eta_b phi_i - dn phi_i ) of one component"""
    m, eb = d.mesh, d.ebnd
    _, eta_b = vr.penalties(d)
    cells, nb = m.edge_plus[eb], m.edge_normal_plus[eb]
    val, dn, wl = vr._edge_tab_u(d, eb, cells, nb)
    lv = eta_b[:, None] * np.einsum("mq,mqi->mi", wl, val) - np.einsum("mq,mqi->mi", wl, dn)
    return cells, side_of_edges(d), lv, eta_b * wl.sum(axis=1)


def unit_loads(d):
    """[4, NQ]: l(.; U) of the unit speed on one side at a time, before M^-1"""
    cells, side, lv, _ = _wall_edges(d)
    out = np.zeros((4, d.NQ))
    for i in range(len(cells)):
        out[side[i], d.dofQ[cells[i], :, TANGENTIAL[side[i]]]] += lv[i]
    return out


def load_vector(d, U, loads=None):
    """l(.; U) [NQ], before M^-1"""
    loads = unit_loads(d) if loads is None else loads
    return speeds(U) @ loads


def force_functionals(d, wall="no_slip"):
    """(G [4, 2, NQ], g0 [4, 2]): F_w . e_c = nu (G[w, c] . u + U_w g0[w, c]).  G[w, c] = - int_w ( eta_b phi - dn phi ) on
    component c: the normal component always, the tangential one with no slip only, where g0 = int_w eta_b as well."""
    assert wall in vr.WALLS
    cells, side, lv, etalen = _wall_edges(d)
    G, g0 = np.zeros((4, 2, d.NQ)), np.zeros((4, 2))
    for i in range(len(cells)):
        w = side[i]
        t = TANGENTIAL[w]
        G[w, 1 - t, d.dofQ[cells[i], :, 1 - t]] -= lv[i]
        if wall == "no_slip":
            G[w, t, d.dofQ[cells[i], :, t]] -= lv[i]
            g0[w, t] += etalen[i]
    return G, g0


def wall_force(d, nu, U, Q, wall="no_slip", functionals=None):
    """F [4, 2] of the nodal field Q"""
    G, g0 = force_functionals(d, wall) if functionals is None else functionals
    return nu * (G @ np.asarray(Q).ravel() + speeds(U)[:, None] * g0)


def integral(d, f):
    """(int f_x, int f_y) of a nodal velocity-space field"""
    r = d.MQ @ np.asarray(f).ravel()
    return np.array([r[0::2].sum(), r[1::2].sum()])


class Affine:
    """Q -> A Q + b with the `@` of a matrix: what the loops of viscosity_reference apply to Q.ravel()"""

    def __init__(self, A, b):
        self.A, self.b = A, b

    def __matmul__(self, x):
        return self.A @ x + self.b


def affine(d, U, A=None, loads=None, Minv_loads=None):
    """M^-1 (V . + l(U)), A = M^-1 V in the no-slip mode: what hdg_apply_moving_walls applies"""
    A = vr.minv_v(d, "no_slip") if A is None else A
    if Minv_loads is None:
        loads = unit_loads(d) if loads is None else loads
        Minv_loads = np.linalg.solve(d.MQ.toarray(), loads.T).T
    return Affine(A, speeds(U) @ Minv_loads)


def imex_with_moving_walls(o, Ab, nu, Q0, p0, f_rhs, T_final, **kw):
    """viscosity_reference.imex_with_viscosity with nu (A Q^(j) + M^-1 l(U)) in every forcing slot; Ab: affine(...)"""
    return vr.imex_with_viscosity(o, Ab, nu, Q0, p0, f_rhs, T_final, **kw)


def implicit_with_moving_walls(d, Ab, nu, dt, Q0, p0, f_rhs, T_final, **kw):
    return vr.implicit_with_viscosity(d, Ab, nu, dt, Q0, p0, f_rhs, T_final, **kw)


def dg_with_moving_walls(d, Ab, nu, dt, Q0, p0, f_rhs, nsteps, **kw):
    return vr.dg_with_viscosity(d, Ab, nu, dt, Q0, p0, f_rhs, nsteps, **kw)
