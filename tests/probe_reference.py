"""CPU checker of point values (helper of the probe tests, not a test module).

Restates the ownership rule of include/hdg_mi355x.h (hdg_evaluate_points) and evaluates nodal fields in
the host layouts of hdg_set_state from the public pieces of the oracle only: the nodal basis ``oracle.fem.PolySpace2D`` of
the engine's node family, and the cell's affine map read off the node coordinates (hdg_node_coordinates: nodes 0, n and the
last one of a cell are its vertices 0, 1, 2).  Nothing here uses the engine's modal basis.

Columns of a row: ux, uy, p, q, omega = d_x uy - d_y ux inside the owning cell; NaN for a field not given or a point outside.
"""
import math

import numpy as np

from oracle import fem

TOL = 1e-12
NCOL = 5


def owner_square(x, y, nx, ny, L, periodic):
    """(i, j, s, x, y) of the owning cell and the (wrapped / clamped) point, or None outside the unit square.  The same
    operations, one per statement, as square_locate in csrc/hdg_points.hpp."""
    x, y = float(x), float(y)
    h = L / nx
    Lx = L
    Ly = L if ny == nx else ny * h
    if not (math.isfinite(x) and math.isfinite(y)):
        return None
    if periodic:
        wx = math.floor(x / Lx) * Lx
        wy = math.floor(y / Ly) * Ly
        x = x - wx
        y = y - wy
        if x >= Lx or x < 0.0:
            x = 0.0
        if y >= Ly or y < 0.0:
            y = 0.0
    else:
        tx, ty = TOL * Lx, TOL * Ly
        if x < -tx or x > Lx + tx or y < -ty or y > Ly + ty:
            return None
        x = min(max(x, 0.0), Lx)
        y = min(max(y, 0.0), Ly)
    i = min(math.floor(x / h), nx - 1)
    j = min(math.floor(y / h), ny - 1)
    fx = x / h - i
    fy = y / h - j
    s = 0 if fx + fy <= 1.0 else 1
    return i, j, s, x, y


def owner_general(vertices, cells, x, y):
    """Lowest-numbered cell whose barycentric coordinates are all >= -TOL (brute force), or None."""
    v = np.asarray(vertices, dtype=float)[np.asarray(cells)]
    d = np.array([x, y]) - v[:, 0]
    J = np.stack([v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], axis=-1)
    ref = np.einsum("crd,cd->cr", np.linalg.inv(J), d)
    ok = (ref[:, 0] >= -TOL) & (ref[:, 1] >= -TOL) & (1.0 - ref[:, 0] - ref[:, 1] >= -TOL)
    hit = np.flatnonzero(ok)
    return int(hit[0]) if len(hit) else None


def node_coordinates(mesh, n, variant="gll"):
    """Physical positions of the nodes of the broken P_n space of an oracle mesh (fem.Mesh / fem.TriMesh), cell-major: the
    layout of hdg_node_coordinates (structured cell (i, j, s) at 2 (j nx + i) + s, as fem.Mesh numbers its cells)."""
    nodes = fem.triangle_nodes(n, variant)
    v0 = mesh.cell_vertices[:, 0]
    return (v0[:, None, :] + np.einsum("cdr,qr->cqd", mesh.J, nodes)).reshape(-1, 2)


class PointEvaluator:
    """Point values of nodal fields given the node coordinates xq (velocity, P_{k+1}) of the engine or node_coordinates."""

    def __init__(self, k, xq, variant="gll", square=None, general=None):
        """square = (nx, ny, L, periodic) or general = (vertices, cells)."""
        self.k = k
        self.Vu, self.Vp = fem.PolySpace2D(k + 1, variant), fem.PolySpace2D(k, variant)
        self.nu, self.np_ = self.Vu.ndof, self.Vp.ndof
        self.xq = np.asarray(xq, dtype=float).reshape(-1, self.nu, 2)
        self.square, self.general = square, general

    def locate(self, x, y):
        """(cell, physical point used) or None."""
        if self.square is not None:
            nx, ny, L, periodic = self.square
            o = owner_square(x, y, nx, ny, L, periodic)
            if o is None:
                return None
            i, j, s, xw, yw = o
            return 2 * (j * nx + i) + s, (xw, yw)
        c = owner_general(*self.general, x, y)
        return None if c is None else (c, (float(x), float(y)))

    def evaluate(self, xy, Q=None, p=None, q=None):
        """(values (n, 5), located (n,) bool)."""
        xy = np.asarray(xy, dtype=float).reshape(-1, 2)
        out = np.full((len(xy), NCOL), np.nan)
        located = np.zeros(len(xy), dtype=bool)
        Qc = None if Q is None else np.asarray(Q, dtype=float).reshape(-1, self.nu, 2)
        pc = None if p is None else np.asarray(p, dtype=float).reshape(-1, self.np_)
        qc = None if q is None else np.asarray(q, dtype=float).reshape(-1, self.np_)
        for t, (x, y) in enumerate(xy):
            loc = self.locate(x, y)
            if loc is None:
                continue
            located[t] = True
            c, pt = loc
            X = self.xq[c]
            v0, v1, v2 = X[0], X[self.k + 1], X[-1]
            J = np.stack([v1 - v0, v2 - v0], axis=1)
            Ji = np.linalg.inv(J)
            ref = Ji @ (np.array(pt) - v0)
            phi, dphi = self.Vu.tabulate(ref[None, :], deriv=1)
            grad = dphi[0] @ Ji  # physical gradients (nu, 2)
            if Qc is not None:
                u = phi[0] @ Qc[c]
                out[t, 0:2] = u
                out[t, 4] = grad[:, 0] @ Qc[c][:, 1] - grad[:, 1] @ Qc[c][:, 0]
            psi = self.Vp.tabulate(ref[None, :])[0]
            if pc is not None:
                out[t, 2] = psi @ pc[c]
            if qc is not None:
                out[t, 3] = psi @ qc[c]
        return out, located
