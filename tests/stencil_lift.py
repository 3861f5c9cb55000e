"""TEST INFRASTRUCTURE ONLY -- carry a dense reference operator of a small structured mesh to a large one by translation.

On the uniform structured meshes (the unit square, the doubly periodic square) the stencil operators of DESIGN.md sections 19-24
(M^-1 V, M^-1 D, their wall terms and loads, the force and flux functionals, the buoyancy, the Coriolis term with beta = 0) are
translation invariant: the block row of a cell depends on its shape, on which of its edges lie on which wall, and on a power of
h.  So the dense numpy reference of a mesh with nx0 = 3 cells a side (periodic: 4), where every class of cell occurs, gives the
reference of any nx: copy the blocks of the class representative, find the neighbours by (shape, i, j), scale by
(h / h0)^exponent.  tests/test_stencil_lift_cpu.py checks that against the dense reference built directly on the larger mesh.

    class of a cell   (shape, on a vertical wall, on a horizontal wall).  Shape 0 (the lower left triangle of its square) touches
                      the left and the bottom wall, shape 1 the right and the top one: the class tells the four sides apart.  A
                      periodic mesh has one class per shape.
    cell map          (shape, i, j) of every cell is derived from its vertices; no numbering is assumed.
    layout check      the nodes of every cell, relative to its square and divided by h, must equal those of its class
                      representative on the small mesh: another vertex or node order raises instead of comparing wrong blocks.
    dof sets          whole cells: 'Q' is both velocity components interleaved (d.dofQ), 'P' the DG_k nodes (d.dofP); an
                      operator may map one to the other (the buoyancy).

Exponents of h: M^-1 V, M^-1 D, their wall terms and their affine parts (M^-1 l, the moving-wall loads) -2; the flux loads l_w and
the wall-force functionals 0 (eta_b |e| and int_e dn phi are both free of h); buoyancy and Coriolis 0; int phi (the row sums of M) 2."""
import numpy as np
import scipy.sparse as sp

__all__ = ["Grid", "Lift", "LiftedOperator", "LiftedFunctional", "nested_dissection", "DirectSolve", "references", "SPEEDS", "WALLS3", "GRAVITY", "F0"]

SPEEDS = (0.3, -0.7, 1.0, 0.45)                      # bottom, right, top, left: four distinct wall speeds
WALLS3 = {"left": 0.5, "right": -0.25, "top": 1.5}  # three fixed sides at distinct values, the bottom no flux
GRAVITY = (0.3, -1.0)
F0 = 1.3

LAYOUT_TOL = 1e-9   # node positions in units of h
STENCIL_TOL = 1e-12  # what a block outside the stencil, or the difference of two cells of one class, may hold: relative to max|A0|


class Grid:
    """A structured mesh as its owner reports it: vertices (N_c, 3, 2), node coordinates xq (N_c n_u, 2) and xp (N_c n_p, 2)."""

    def __init__(self, vertices, xq, xp, nx, L=1.0, periodic=False):
        v = np.asarray(vertices, dtype=float)
        self.nx, self.L, self.periodic = int(nx), float(L), bool(periodic)
        self.h = self.L / self.nx
        self.ncells = nc = len(v)
        if nc != 2 * self.nx * self.nx:
            raise ValueError(f"{nc} cells are not the 2 nx^2 cells of a structured mesh with nx = {nx}")
        c = v.mean(axis=1) / self.h
        i, j = np.floor(c[:, 0]).astype(int), np.floor(c[:, 1]).astype(int)
        frac = c[:, 0] - i + c[:, 1] - j  # 2/3 in the lower left triangle, 4/3 in the upper right one
        if np.max(np.abs(np.where(frac > 1.0, frac - 4.0 / 3.0, frac - 2.0 / 3.0))) > 1e-6:
            raise ValueError("a cell is neither the lower left nor the upper right triangle of a square of side h")
        self.s, self.i, self.j = (frac > 1.0).astype(int), i, j
        if i.min() < 0 or j.min() < 0 or i.max() >= self.nx or j.max() >= self.nx:
            raise ValueError("a cell lies outside the square")
        self.cell_of = np.full((2, self.nx, self.nx), -1)
        self.cell_of[self.s, i, j] = np.arange(nc)
        if np.any(self.cell_of < 0):
            raise ValueError("the cells do not cover every (shape, i, j) once")
        last = self.nx - 1
        if self.periodic:
            vw = hw = np.zeros(nc, dtype=int)
        else:
            vw = np.where(self.s == 0, i == 0, i == last).astype(int)
            hw = np.where(self.s == 0, j == 0, j == last).astype(int)
        self.cls = 4 * self.s + 2 * vw + hw
        corner = np.stack([i, j], axis=-1)[:, None, :] * self.h
        self.rel = {"Q": (np.asarray(xq, dtype=float).reshape(nc, -1, 2) - corner) / self.h,
                    "P": (np.asarray(xp, dtype=float).reshape(nc, -1, 2) - corner) / self.h}
        self.n = {"Q": 2 * self.rel["Q"].shape[1], "P": self.rel["P"].shape[1]}

    @classmethod
    def of_oracle(cls, d):
        m = d.mesh
        return cls(m.cell_vertices, d.node_coords(d.PU), d.node_coords(d.PP), m.nx, getattr(m, "L", 1.0), getattr(m, "periodic", False))

    @classmethod
    def of_engine(cls, eng):
        xq, xp = eng.node_coordinates()
        per = bool(eng.cfg.periodic)
        return cls(eng.cell_vertices(), xq, xp, eng.cfg.nx, eng.cfg.length if per else 1.0, per)

    def neighbour(self, cells, s, di, dj):
        """the cell (s, i + di, j + dj) of every cell in `cells`; i and j wrap on a periodic mesh"""
        i, j = self.i[cells] + di, self.j[cells] + dj
        if self.periodic:
            i, j = i % self.nx, j % self.nx
        elif i.min() < 0 or j.min() < 0 or i.max() >= self.nx or j.max() >= self.nx:
            raise ValueError("a neighbour lies outside the mesh: the class of a cell does not say where its walls are")
        return self.cell_of[s, i, j]


class Lift:
    """The classes of a small discretisation d0 (oracle) matched with the cells of a target Grid."""

    def __init__(self, d0, target):
        self.d0, self.g0, self.t = d0, Grid.of_oracle(d0), target
        g0, t = self.g0, target
        if g0.periodic != t.periodic:
            raise ValueError("the small and the target mesh differ in periodicity")
        self.classes = [int(c) for c in np.unique(t.cls)]
        self.rep = {}
        for c in self.classes:
            hit = np.nonzero(g0.cls == c)[0]
            if hit.size == 0:
                raise ValueError(f"the small mesh has no cell of class {c}")
            self.rep[c] = int(hit[0])
        for space in ("Q", "P"):  # the layout check
            if g0.n[space] != t.n[space]:
                raise ValueError(f"space {space}: {t.n[space]} dofs a cell on the target, {g0.n[space]} on the small mesh")
            for c in self.classes:
                err = np.max(np.abs(t.rel[space][t.cls == c] - g0.rel[space][self.rep[c]][None]))
                if err > LAYOUT_TOL:
                    raise ValueError(f"space {space}, class {c}: the local node layout of a target cell differs from its "
                                     f"representative's by {err:.3e} h")
        # the neighbours of every representative over its interior edges: (shape, di, dj)
        m = d0.mesh
        plus, minus = np.asarray(m.edge_plus), np.asarray(m.edge_minus)
        self.slots, self.slot_cells = {}, {}
        half = g0.nx // 2
        for c, c0 in self.rep.items():
            nb = [int(minus[e]) for e in np.nonzero((plus == c0) & (minus >= 0))[0]] + [int(plus[e]) for e in np.nonzero(minus == c0)[0]]
            slots = [(int(g0.s[c0]), 0, 0)]
            for n in nb:
                di, dj = int(g0.i[n] - g0.i[c0]), int(g0.j[n] - g0.j[c0])
                if g0.periodic:
                    di, dj = (di + half) % g0.nx - half, (dj + half) % g0.nx - half
                slots.append((int(g0.s[n]), di, dj))
            if len(set(slots)) != len(slots) or any(abs(di) > 1 or abs(dj) > 1 for _, di, dj in slots):
                raise ValueError("the small mesh is too small to tell the neighbours of a cell apart")
            self.slots[c], self.slot_cells[c] = slots, [c0] + nb

    def scale(self, exponent):
        return (self.t.h / self.g0.h) ** exponent

    def _blocks(self, A0, rows, cols):
        """Per class the blocks of the representative's row, one per slot; checks that the row holds nothing else and that every
        cell of the small mesh carries the blocks of its class."""
        g0 = self.g0
        nr, ncl = g0.n[rows], g0.n[cols]
        A4 = np.asarray(A0).reshape(g0.ncells, nr, g0.ncells, ncl)
        top = max(np.max(np.abs(A4)), 1e-300)
        out = {}
        for c, c0 in self.rep.items():
            row = A4[c0].copy()
            out[c] = [row[:, n, :].copy() for n in self.slot_cells[c]]
            row[:, self.slot_cells[c], :] = 0.0
            if np.max(np.abs(row)) > STENCIL_TOL * top:
                raise ValueError(f"class {c}: the operator couples a cell with more than its edge neighbours")
            for other in np.nonzero(g0.cls == c)[0]:
                for (s, di, dj), blk in zip(self.slots[c], out[c]):
                    n = g0.neighbour(np.array([other]), s, di, dj)[0]
                    if np.max(np.abs(A4[other, :, n, :] - blk)) > STENCIL_TOL * top:
                        raise ValueError(f"class {c}: two cells of one class carry different blocks: the operator is not translation invariant")
        return out

    def operator(self, A0, b0=None, exponent=0, rows="Q", cols=None, displace_x=None):
        """The lifted operator x -> A x + b.  A0: dense over the dofs of d0 (rows x cols, 'Q' or 'P' each); b0: the affine part
        over the row dofs.  displace_x: a mask over the target cells whose x-neighbours are taken one column too far to the right
        (a deliberately wrong reference, for the tests that show a comparison can fail)."""
        cols = rows if cols is None else cols
        g0, t = self.g0, self.t
        blocks = self._blocks(A0, rows, cols)
        sc = self.scale(exponent)
        nr = g0.n[rows]
        parts = []
        for c in self.classes:
            cells = np.nonzero(t.cls == c)[0]
            for (s, di, dj), blk in zip(self.slots[c], blocks[c]):
                nb = t.neighbour(cells, s, di, dj)
                if displace_x is not None and di != 0:
                    bad = np.asarray(displace_x)[cells]
                    nb = np.where(bad, t.cell_of[s, (t.i[cells] + di + 1) % t.nx, t.j[nb]], nb)
                parts.append((cells, nb, sc * blk))
        b = None
        if b0 is not None:
            b = np.zeros((t.ncells, nr))
            b0 = np.asarray(b0).reshape(g0.ncells, nr)
            for c in self.classes:
                b[t.cls == c] = sc * b0[self.rep[c]]
                for other in np.nonzero(g0.cls == c)[0]:
                    if np.max(np.abs(b0[other] - b0[self.rep[c]])) > STENCIL_TOL * max(np.max(np.abs(b0)), 1e-300):
                        raise ValueError(f"class {c}: two cells of one class carry different affine parts")
            b = b.reshape(-1)
        return LiftedOperator(t.ncells, nr, g0.n[cols], parts, b)

    def functional(self, F0, c0=None, exponent=0, space="Q"):
        """Lifted linear functionals x -> F x + c.  F0: (m, dofs of d0); the entries on a cell depend on its class alone.  c0 (m,):
        constants that are sums of equal parts over the cells on which functional r does not vanish (int_w eta_b over side w)."""
        g0, t = self.g0, self.t
        n = g0.n[space]
        F3 = np.asarray(F0).reshape(len(F0), g0.ncells, n)
        top = max(np.max(np.abs(F3)), 1e-300)
        sc = self.scale(exponent)
        parts = []
        c = None if c0 is None else np.zeros(len(F3))
        for k in self.classes:
            blk = F3[:, self.rep[k], :]
            for other in np.nonzero(g0.cls == k)[0]:
                if np.max(np.abs(F3[:, other, :] - blk)) > STENCIL_TOL * top:
                    raise ValueError(f"class {k}: two cells of one class carry different functional entries")
            live = np.max(np.abs(blk), axis=1) > 0.0
            if live.any():
                parts.append((np.nonzero(t.cls == k)[0], sc * blk))
        if c0 is not None:
            for r in range(len(F3)):
                on0 = np.max(np.abs(F3[r]), axis=1) > 0.0          # the cells of the small mesh that functional r reads
                if on0.any():
                    on = np.isin(t.cls, np.unique(g0.cls[on0]))
                    c[r] = sc * float(c0[r]) / np.count_nonzero(on0) * np.count_nonzero(on)
        return LiftedFunctional(t.ncells, n, parts, c)


class LiftedOperator:
    """x -> A x + b, applied class by class and block by block (a gather and an einsum each)."""

    def __init__(self, ncells, nr, ncl, parts, b):
        self.ncells, self.nr, self.ncl, self.parts, self.b = ncells, nr, ncl, parts, b

    def linear(self, x, dtype=np.float64):
        """A x alone; dtype=np.longdouble evaluates the products and sums in extended precision"""
        x = np.asarray(x).reshape(self.ncells, self.ncl).astype(dtype)
        y = np.zeros((self.ncells, self.nr), dtype=dtype)
        for cells, nb, blk in self.parts:
            y[cells] += np.einsum("ab,nb->na", blk.astype(dtype), x[nb])
        return y.reshape(-1)

    def apply(self, x, dtype=np.float64):
        y = self.linear(x, dtype)
        return y if self.b is None else y + self.b.astype(dtype)

    __matmul__ = apply

    def matrix(self):
        """A as scipy.sparse CSR"""
        rows, cols, vals = [], [], []
        a, b = np.arange(self.nr), np.arange(self.ncl)
        for cells, nb, blk in self.parts:
            rows.append(np.broadcast_to((cells[:, None] * self.nr + a)[:, :, None], (len(cells), self.nr, self.ncl)).ravel())
            cols.append(np.broadcast_to((nb[:, None] * self.ncl + b)[:, None, :], (len(cells), self.nr, self.ncl)).ravel())
            vals.append(np.broadcast_to(blk[None], (len(cells), self.nr, self.ncl)).ravel())
        N, M = self.ncells * self.nr, self.ncells * self.ncl
        return sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(N, M)).tocsr()

    def system(self, tau):
        """(I - tau A as CSC, tau b): the backward-Euler system (I - tau A) x = q + tau b"""
        assert self.nr == self.ncl
        S = (sp.identity(self.ncells * self.nr, format="csr") - tau * self.matrix()).tocsc()
        return S, (np.zeros(self.ncells * self.nr) if self.b is None else tau * self.b)


class LiftedFunctional:
    """x -> F x + c for a few functionals with entries on some classes of cells only"""

    def __init__(self, ncells, n, parts, c):
        self.ncells, self.n, self.parts, self.c = ncells, n, parts, c

    def linear(self, x, dtype=np.float64):
        x = np.asarray(x).reshape(self.ncells, self.n).astype(dtype)
        out = 0
        for cells, blk in self.parts:
            out = out + np.einsum("mb,nb->m", blk.astype(dtype), x[cells])
        return out

    def dense(self):
        """F as a dense (m, N) array"""
        m = len(self.parts[0][1])
        F = np.zeros((m, self.ncells, self.n))
        for cells, blk in self.parts:
            F[:, cells, :] = blk[:, None, :]
        return F.reshape(m, -1)


def references(d):
    """The dense references of one discretisation, built by the existing reference modules, with what a Lift needs to carry them:
    ({name: (A, b, exponent, rows, cols)}, {name: (F, c, exponent, space)}, the tracers' WallOperator or None).  The GPU tests
    lift these from the small mesh; tests/test_stencil_lift_cpu.py builds them on both meshes and compares."""
    import buoyancy_reference as bref
    import coriolis_reference as cref
    import moving_walls_reference as mref
    import tracer_diffusion_reference as tdref
    import tracer_walls_reference as twref
    import viscosity_reference as vref

    periodic = bool(getattr(d.mesh, "periodic", False))
    MQ = d.MQ.toarray()
    ops, funs, wallop = {}, {}, None
    ops["viscosity free_slip"] = (vref.minv_v(d, "free_slip"), None, -2, "Q", "Q")
    eye = np.eye(d.NP)
    ops["buoyancy"] = (np.stack([bref.B(d, eye[n], 1.0, GRAVITY).ravel() for n in range(d.NP)], axis=1), None, 0, "Q", "P")
    ops["coriolis beta=0"] = (cref.minv_c(d, F0, 0.0), None, 0, "Q", "Q")
    ones = np.zeros((2, d.NQ))
    ones[0, 0::2] = ones[1, 1::2] = 1.0
    funs["integral"] = (ones @ MQ, None, 2, "Q")
    if periodic:
        ops["tracer diffusion"] = (tdref.minv_d(d), None, -2, "P", "P")
        return ops, funs, wallop
    A = vref.minv_v(d, "no_slip")
    ops["viscosity no_slip"] = (A, None, -2, "Q", "Q")
    Mi = np.linalg.solve(MQ, mref.unit_loads(d).T).T
    ops["moving walls"] = (A, mref.affine(d, SPEEDS, A, Minv_loads=Mi).b, -2, "Q", "Q")
    for wall in vref.WALLS:
        G, g0 = mref.force_functionals(d, wall)
        funs["wall force " + wall] = (G.reshape(8, -1), g0.reshape(8), 0, "Q")
    wallop = twref.WallOperator(d)
    ops["tracer diffusion"] = (wallop.A0, None, -2, "P", "P")
    ops["tracer walls"] = wallop.minv(WALLS3) + (-2, "P", "P")
    funs["flux loads"] = (np.stack([t[1] for t in wallop.terms]), None, 0, "P")
    return ops, funs, wallop


def nested_dissection(grid, n):
    """A fill-reducing elimination order of the dofs (n a cell) of a structured mesh: the squares are split recursively by a
    line of squares (both triangles of it: every edge neighbour of a cell lies in its own square or in an adjacent one), the
    halves come first and the line last.  SuperLU's own orderings know nothing of the mesh: at nx = 72, k = 4 COLAMD fills
    2.9e8 entries (66 s), this order 1.1e8 (16 s)."""
    out = []

    def split(i0, i1, j0, j1):
        ni, nj = i1 - i0, j1 - j0
        if ni <= 0 or nj <= 0:
            return
        if ni * nj <= 4:
            out.extend((i, j) for j in range(j0, j1) for i in range(i0, i1))
        elif ni >= nj:
            m = (i0 + i1) // 2
            split(i0, m, j0, j1)
            split(m + 1, i1, j0, j1)
            out.extend((m, j) for j in range(j0, j1))
        else:
            m = (j0 + j1) // 2
            split(i0, i1, j0, m)
            split(i0, i1, m + 1, j1)
            out.extend((i, m) for i in range(i0, i1))

    split(0, grid.nx, 0, grid.nx)
    sq = np.array(out)
    cells = np.stack([grid.cell_of[0, sq[:, 0], sq[:, 1]], grid.cell_of[1, sq[:, 0], sq[:, 1]]], axis=1).ravel()
    return (cells[:, None] * n + np.arange(n)).ravel()


class DirectSolve:
    """splu of a sparse system in a given elimination order (nested_dissection): x = solve(r)"""

    def __init__(self, S, perm):
        import scipy.sparse.linalg as spla

        self.perm = perm
        self.lu = spla.splu(S.tocsr()[perm][:, perm].tocsc(), permc_spec="NATURAL", diag_pivot_thresh=0.0, options=dict(SymmetricMode=True))

    def solve(self, r):
        x = np.empty(len(r))
        x[self.perm] = self.lu.solve(np.asarray(r, dtype=float)[self.perm])
        return x
