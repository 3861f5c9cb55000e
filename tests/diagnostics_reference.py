"""Independent CPU reference of the flow diagnostics (hdg_compute_diagnostics).

Built from the oracle's public pieces only: the meshes of oracle/fem.py (``Mesh`` for the unit and the periodic square,
``TriMesh`` for general triangulations), its nodal Lagrange bases and quadrature rules.  Works on the nodal arrays of the
library boundary (velocity (nc * nu, 2), pressure / tracer (nc * np,)) and evaluates every integral by quadrature of the
nodal interpolants -- no modal basis, no orthonormality, none of the engine's tables.
"""
import numpy as np

from oracle.fem import Mesh, PolySpace2D, gauss_legendre_01, triangle_quadrature

NAMES = ("energy", "enstrophy", "div_l2", "jump_l2", "p_integral", "tracer_integral", "tracer_half_sq", "max_speed", "cfl")


def square_mesh(nx, periodic=False, L=1.0):
    return Mesh(nx, periodic=periodic, L=L)


def shortest_edges(mesh):
    v = mesh.cell_vertices
    return np.min(np.stack([np.linalg.norm(v[:, (l + 1) % 3] - v[:, l], axis=1) for l in range(3)], axis=1), axis=1)


def diagnostics(mesh, k, Q, p, q=None, dt=1.0, variant="gll"):
    """The nine diagnostics of nodal fields on `mesh` (fem.Mesh / fem.TriMesh) as a dict keyed by NAMES."""
    PU, PP = PolySpace2D(k + 1, variant), PolySpace2D(k, variant)
    nc = mesh.ncells
    Qc = np.asarray(Q, dtype=float).reshape(nc, PU.ndof, 2)
    pc = np.asarray(p, dtype=float).reshape(nc, PP.ndof)
    # cells: the rule is exact for degree 2k + 2 (|u|^2); gradients are physical, J^{-T} times the reference ones
    xq, wq = triangle_quadrature(2 * k + 2)
    U, Ug = PU.tabulate(xq, deriv=1)
    P = PP.tabulate(xq)
    wdet = mesh.detJ[:, None] * wq[None, :]
    uq = np.einsum("qn,cnd->cqd", U, Qc)
    G = np.einsum("crd,qnr,cna->cqad", mesh.Jinv, Ug, Qc)  # G[..., a, d] = d_d u_a
    curl = G[..., 1, 0] - G[..., 0, 1]
    div = G[..., 0, 0] + G[..., 1, 1]
    out = {
        "energy": 0.5 * float(np.sum(wdet * np.sum(uq * uq, axis=-1))),
        "enstrophy": 0.5 * float(np.sum(wdet * curl * curl)),
        "div_l2": float(np.sqrt(np.sum(wdet * div * div))),
        "p_integral": float(np.sum(wdet * (pc @ P.T))),
    }
    if q is None:
        out["tracer_integral"] = out["tracer_half_sq"] = float("nan")
    else:
        qq = np.asarray(q, dtype=float).reshape(nc, PP.ndof) @ P.T
        out["tracer_integral"] = float(np.sum(wdet * qq))
        out["tracer_half_sq"] = 0.5 * float(np.sum(wdet * qq * qq))
    # edges: [u.n] of the two sides (the '+' side alone on a boundary edge), Gauss rule exact for degree 2k + 3
    t, w = gauss_legendre_01(k + 2)
    x = mesh.edge_a[:, None, :] + t[None, :, None] * (mesh.edge_b - mesh.edge_a)[:, None, :]
    n = mesh.edge_normal_plus

    def side(cells, xe):
        return np.einsum("eqn,end->eqd", PU.tabulate(mesh.ref_coords(cells, xe)), Qc[cells])

    jump = np.einsum("eqd,ed->eq", side(mesh.edge_plus, x), n)
    inner = mesh.edge_minus >= 0
    jump[inner] -= np.einsum("eqd,ed->eq", side(mesh.edge_minus[inner], x[inner]), n[inner])
    out["jump_l2"] = float(np.sqrt(np.sum(mesh.edge_len[:, None] * w[None, :] * jump * jump)))
    # nodes of V_Q
    speed = np.linalg.norm(Qc, axis=-1)  # [c, node]
    out["max_speed"] = float(speed.max())
    out["cfl"] = float(dt * np.max(speed.max(axis=1) / shortest_edges(mesh)))
    return {name: out[name] for name in NAMES}


def velocity_nodes(mesh, k, variant="gll"):
    """Physical coordinates of the velocity nodes, (nc * nu, 2) in the boundary numbering."""
    PU = PolySpace2D(k + 1, variant)
    X = mesh.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,nr->cnd", mesh.J, PU.nodes)
    return X.reshape(-1, 2)


def pressure_nodes(mesh, k, variant="gll"):
    PP = PolySpace2D(k, variant)
    X = mesh.cell_vertices[:, 0][:, None, :] + np.einsum("cdr,nr->cnd", mesh.J, PP.nodes)
    return X.reshape(-1, 2)
