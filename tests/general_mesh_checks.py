"""Shared checks of the general-mesh path (helper of tests/test_gpu_general_mesh.py, tests/test_gpu_general_mesh_scale.py,
tests/general_scale_worker.py and tests/test_host.py; not a test module): the operator checks against the oracle, meshes at
the benchmarked sizes, index maps between two engines derived from geometry alone, and the Kelvin-Helmholtz runs with a
tracer."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

RTOL = 1e-10  # operators
TRACE_RTOL = 1e-9  # the condensed trace operator (an LU solve on the oracle side)
TOL = 2e-8  # whole steps: two converged solvers


def rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def engine(pm, k, dt=0.01, **kw):
    from incompressibleeulerhdg_amd._lib import Engine
    from oracle.hdg_oracle import TABLEAUX

    tb = TABLEAUX["imex_ssp2_332"]
    return Engine(vertices=pm.vertices, cells=pm.cells, degree=k, dt=dt, nstages=3, a_expl=tb["a_expl"], a_impl=tb["a_impl"],
                  b_expl=tb["b_expl"], b_impl=tb["b_impl"], c_expl=tb["c_expl"], **kw)


def condensed_trace_operator(d):
    """lam -> S lam = K_ll lam - K_l1 K_11^-1 K_1l lam, the Schur complement of the oracle's hybridised mixed-Poisson matrix
    with one sparse LU of K_11 (the dense complement does not scale: 9.4k^2 on the level-4 disk at k = 2)"""
    n1 = d.NQ + d.NP
    K = d.K_mp.tocsc()
    K11, K1l, Kl1, Kll = K[:n1, :n1].tocsc(), K[:n1, n1:].tocsr(), K[n1:, :n1].tocsr(), K[n1:, n1:].tocsr()
    lu = spla.splu(K11)
    return lambda lam: Kll @ lam - Kl1 @ lu.solve(K1l @ lam)


def check_operators_against_oracle(pm, om, d, k, seed):
    """Every operator of the general path against the oracle on the same triangulation: sizes and topology, node
    coordinates, conversions, norms and integral, BDM projection, advection with both fluxes, weak and broken divergence,
    condensed trace operator, trace reconstruction and the pressure shift."""
    from incompressibleeulerhdg_amd import _lib

    e = engine(pm, k)
    assert (e.n_cells, e.n_edges, e.n_u, e.n_p, e.n_l) == (om.ncells, om.nedges, d.nu, d.np_, d.nl)
    ev, ec = e.general_topology()
    assert np.array_equal(ev, om.edge_vertices) and np.array_equal(ec[:, 0], om.edge_plus) and np.array_equal(ec[:, 1], om.edge_minus)
    xq, xp = e.node_coordinates()
    assert np.allclose(xq, d.node_coords(d.PU).reshape(-1, 2), atol=1e-13) and np.allclose(xp, d.node_coords(d.PP).reshape(-1, 2), atol=1e-13)
    rng = np.random.default_rng(seed)
    Q, x = rng.standard_normal(e.shape_Q), rng.standard_normal(e.shape_Q)
    p, lam = rng.standard_normal(e.shape_p), rng.standard_normal(e.shape_l)
    # conversions, norms, integrals
    e.set_field(1, Q, p, lam)
    Q2, p2, l2 = e.get_field(1)
    assert rel(Q2, Q) < 1e-12 and rel(p2, p) < 1e-12 and rel(l2, lam) < 1e-12
    nq, npr = e.l2_norms(Q, p)
    assert abs(nq - d.l2_norm_velocity(Q)) < 1e-11 * nq and abs(npr - d.l2_norm_pressure(p)) < 1e-11 * npr
    assert abs(e.integrate_pressure(p) - d.int_p @ p) < 1e-12 * max(1.0, abs(d.int_p @ p))
    # BDM projection (common.py:91-108)
    assert rel(e.project_bdm_nodal(Q), d.project_bdm(Q)) < RTOL
    # advection operator (hdg_imex.py:313-331), both fluxes
    Qstar = d.project_bdm(Q)
    gamma = 0.05
    for flux in ("upwind", "centered"):
        ef = engine(pm, k, flux=flux)
        F = d.assemble_f_impl(Qstar, flux)
        ref = x.ravel() - gamma * spla.spsolve(d.MQ.tocsc(), F @ x.ravel())
        assert rel(ef.apply_advection(Qstar, x, gamma).ravel(), ref) < RTOL, flux
        del ef
    # weak / broken divergence
    Mi = spla.splu(d.MP.tocsc())
    assert rel(e.apply_weak_divergence(Q), Mi.solve(d.Wdiv @ Q.ravel())) < RTOL
    assert rel(e.apply_weak_divergence(Q, broken=True), Mi.solve(d.Bdiv @ Q.ravel())) < RTOL
    # condensed trace operator vs the oracle's Schur complement
    S = condensed_trace_operator(d)
    mult = np.where(np.repeat(om.interior, d.nl), 2.0, 1.0)
    Mtr = (sp.diags(1.0 / mult) @ (d.Lm.tocsc() / d.tau)).tocsc()
    assert rel(e.apply_trace_operator(lam), spla.spsolve(Mtr, -S(lam))) < TRACE_RTOL
    assert np.max(np.abs(e.apply_trace_operator(np.ones(e.shape_l)))) < TRACE_RTOL
    # trace reconstruction and the pressure shift
    e.set_state(Q, p)
    e.reconstruct_trace()
    _, p_dev, l_dev = e.get_field(_lib.HDG_STATE_CURRENT)
    p0 = p - (d.int_p @ p) / om.volume
    assert rel(p_dev, p0) < RTOL and rel(l_dev, d.reconstruct_trace(Q, p0)) < RTOL
    e.set_field(1, Q, p, lam)
    e.shift_pressure(1)
    _, p1, l1 = e.get_field(1)
    ps, ls = d.shift_pressure(p, lam)
    assert rel(p1, ps) < RTOL and rel(l1, ls) < RTOL


def check_continuous_space_against_oracle(pm, d, tr, k, seed):
    """CG_{k+1} on a general triangulation (common.py:110-129, callbacks.py:43-69): dof set, L2 projection of a broken
    velocity, vorticity and the tracer transport operator against the oracle's restatement (oracle/tracer_oracle.py)."""
    e = engine(pm, k)
    assert e.cg_size() == tr.ncg
    key = lambda X: {tuple(np.round(x * 1e6).astype(np.int64)) for x in X}
    assert key(e.cg_coordinates()) == key(tr.cg_coords) and len(key(e.cg_coordinates())) == tr.ncg
    rng = np.random.default_rng(seed)
    u = rng.standard_normal(e.shape_Q)
    P = e.cg_project_nodal(u)
    assert rel(P, tr.cg_project(u)) < 1e-10
    assert rel(e.cg_project_nodal(P), P) < 1e-10
    cont = d.interpolate_velocity(lambda x, y: (x ** (k + 1) - y, x * y ** k + 1.0))
    assert rel(e.cg_project_nodal(cont), cont) < 1e-10
    Q = rng.standard_normal(e.shape_Q)
    w, xy = tr.vorticity(Q)
    wd = e.vorticity(Q)
    order = lambda X: np.lexsort((np.round(X[:, 1] * 1e6), np.round(X[:, 0] * 1e6)))
    assert rel(wd[order(e.cg_coordinates())], w[order(xy)]) < 1e-10
    assert rel(e.cg_to_broken(wd), tr.R @ w) < 1e-10
    # rigid rotation (-y, x): vorticity 2 everywhere, also on the polygonal boundary
    rot = d.interpolate_velocity(lambda x, y: (-y, x))
    assert np.max(np.abs(e.vorticity(rot) - 2.0)) < 1e-9
    q = rng.standard_normal(e.shape_p)
    assert rel(e.apply_tracer_advection(q, u, project=True), tr.tracer_tendency(q, u)) < 1e-10
    uc = tr.cg_project(u)
    assert rel(e.apply_tracer_advection(q, uc, project=False), tr._lu_mp.solve(tr.tracer_form(q, uc))) < 1e-10


# --- meshes


def square_as_general_mesh(nx):
    """the structured triangulation of the unit square (oracle/fem.py Mesh(nx).cell_vertices, the cells of the structured
    engine) as (vertices, cells) for the general path, vertices numbered by their coordinates"""
    from oracle import fem

    cv = fem.Mesh(nx).cell_vertices
    X, inv = np.unique(np.round(cv.reshape(-1, 2) * nx).astype(np.int64), axis=0, return_inverse=True)
    return X / float(nx), inv.reshape(-1, 3)


def relabelled(vertices, cells, seed):
    """the same triangulation under a random numbering: vertices and cells permuted, every cell's vertex list rotated by a
    random amount, and half of the cells reversed (clockwise)"""
    rng = np.random.default_rng(seed)
    nv, nc = len(vertices), len(cells)
    pv = rng.permutation(nv)  # new vertex i is old vertex pv[i]
    new_of_old = np.empty(nv, dtype=np.int64)
    new_of_old[pv] = np.arange(nv)
    C = new_of_old[np.asarray(cells)][rng.permutation(nc)]
    rot = rng.integers(0, 3, nc)
    C = np.stack([C[np.arange(nc), (rot + j) % 3] for j in range(3)], axis=1)
    rev = rng.permutation(nc)[: nc // 2]
    C[rev] = C[rev][:, ::-1]
    return np.asarray(vertices)[pv], C


# --- index maps from geometry


def _nearest(xa, xb, tol):
    """m with xb[m] == xa to within tol, asserting that m is a bijection"""
    from scipy.spatial import cKDTree

    dist, m = cKDTree(xb).query(xa)
    assert len(xa) == len(xb) and np.max(dist) < tol, np.max(dist)
    assert len(np.unique(m)) == len(m)
    return m


def _within(xa, xb, tol):
    """[n, m] xa, xb of n cells: j with xb[c, j[c]] == xa[c] per cell, asserting a bijection in every cell"""
    dist = np.linalg.norm(xa[:, :, None, :] - xb[:, None, :, :], axis=-1)
    j = np.argmin(dist, axis=2)
    assert np.max(np.min(dist, axis=2)) < tol
    assert np.array_equal(np.sort(j, axis=1), np.broadcast_to(np.arange(xa.shape[1]), j.shape))
    return j


class GeometricMap:
    """Index maps from engine A's layout to engine B's on the same triangulation, from coordinates alone: cells by centroid,
    velocity and pressure nodes by their coordinates within a cell, edges by their end points, the direction of the trace
    nodes on an edge by which end point comes first.  edges_a / edges_b: [n_edges, 2 (end), 2 (x, y)] in each engine's edge
    order.  q / p / l: the index in B of every entry of A (every map asserted to be a bijection)."""

    def __init__(self, ea, eb, edges_a, edges_b):
        nu, np_, nl = ea.n_u, ea.n_p, ea.n_l
        assert (ea.n_cells, ea.n_edges, nu, np_, nl) == (eb.n_cells, eb.n_edges, eb.n_u, eb.n_p, eb.n_l)
        h = np.min(np.linalg.norm(edges_a[:, 1] - edges_a[:, 0], axis=1))
        tol = 1e-9 * h
        xqa, xpa = ea.node_coordinates()
        xqb, xpb = eb.node_coordinates()
        cell = _nearest(xqa.reshape(-1, nu, 2).mean(axis=1), xqb.reshape(-1, nu, 2).mean(axis=1), tol)
        jq = _within(xqa.reshape(-1, nu, 2), xqb.reshape(-1, nu, 2)[cell], tol)
        jp = _within(xpa.reshape(-1, np_, 2), xpb.reshape(-1, np_, 2)[cell], tol)
        self.cell = cell
        self.q = (cell[:, None] * nu + jq).ravel()
        self.p = (cell[:, None] * np_ + jp).ravel()
        assert np.allclose(xqb[self.q], xqa, atol=1e-13) and np.allclose(xpb[self.p], xpa, atol=1e-13)
        edge = _nearest(edges_a.mean(axis=1), edges_b.mean(axis=1), tol)
        same = np.linalg.norm(edges_a[:, 0] - edges_b[edge, 0], axis=1) < tol
        assert np.all(same | (np.linalg.norm(edges_a[:, 0] - edges_b[edge, 1], axis=1) < tol))
        jl = np.where(same[:, None], np.arange(nl), nl - 1 - np.arange(nl))  # the edge nodes are symmetric (GLL)
        self.l = (edge[:, None] * nl + jl).ravel()

    @staticmethod
    def _to_b(v, idx):
        out = np.empty_like(v)
        out[idx] = v
        return out

    def Qb(self, Q):
        return self._to_b(Q, self.q)

    def pb(self, p):
        return self._to_b(p, self.p)

    def lb(self, lam):
        return self._to_b(lam, self.l)


def general_edges(e, vertices):
    ev, _ = e.general_topology()
    return np.asarray(vertices)[ev]


def structured_edges(nx):
    from oracle import fem

    m = fem.Mesh(nx)
    return np.stack([m.edge_a, m.edge_b], axis=1)


def compare_engines(A, B, M, seed, tracer_and_dg=True):
    """Every operator of the check against the oracle, plus the continuous space (through cg_to_broken), the tracer operator
    and the DG operators, on engine pair A (the reference layout) and B (mapped through GeometricMap M).  A / B: dicts
    {"upwind": engine, "centered": engine} on the same triangulation and degree."""
    from incompressibleeulerhdg_amd import _lib

    ea, eb = A["upwind"], B["upwind"]
    rng = np.random.default_rng(seed)
    Q, x = rng.standard_normal(ea.shape_Q), rng.standard_normal(ea.shape_Q)
    p, lam = rng.standard_normal(ea.shape_p), rng.standard_normal(ea.shape_l)
    Qb, pb, lb = M.Qb(Q), M.pb(p), M.lb(lam)
    # conversions, norms, integral
    eb.set_field(1, Qb, pb, lb)
    Q2, p2, l2 = eb.get_field(1)
    assert rel(Q2[M.q], Q) < 1e-12 and rel(p2[M.p], p) < 1e-12 and rel(l2[M.l], lam) < 1e-12
    na, nb = ea.l2_norms(Q, p), eb.l2_norms(Qb, pb)
    assert abs(na[0] - nb[0]) < 1e-11 * na[0] and abs(na[1] - nb[1]) < 1e-11 * na[1]
    ia = ea.integrate_pressure(p)
    assert abs(eb.integrate_pressure(pb) - ia) < 1e-12 * max(1.0, abs(ia))
    # BDM projection, advection with both fluxes
    Qs = ea.project_bdm_nodal(Q)
    assert rel(eb.project_bdm_nodal(Qb)[M.q], Qs) < RTOL
    for flux in ("upwind", "centered"):
        assert rel(B[flux].apply_advection(M.Qb(Qs), M.Qb(x), 0.05)[M.q], A[flux].apply_advection(Qs, x, 0.05)) < RTOL, flux
    # weak / broken divergence, condensed trace operator
    for broken in (False, True):
        assert rel(eb.apply_weak_divergence(Qb, broken=broken)[M.p], ea.apply_weak_divergence(Q, broken=broken)) < RTOL, broken
    assert rel(eb.apply_trace_operator(lb)[M.l], ea.apply_trace_operator(lam)) < TRACE_RTOL
    assert np.max(np.abs(eb.apply_trace_operator(np.ones(eb.shape_l)))) < TRACE_RTOL
    # trace reconstruction and the pressure shift
    for e, args in ((ea, (Q, p)), (eb, (Qb, pb))):
        e.set_state(*args)
        e.reconstruct_trace()
    _, pa_, la_ = ea.get_field(_lib.HDG_STATE_CURRENT)
    _, pb_, lb_ = eb.get_field(_lib.HDG_STATE_CURRENT)
    assert rel(pb_[M.p], pa_) < RTOL and rel(lb_[M.l], la_) < RTOL
    ea.set_field(1, Q, p, lam)
    eb.set_field(1, Qb, pb, lb)
    ea.shift_pressure(1)
    eb.shift_pressure(1)
    _, pa_, la_ = ea.get_field(1)
    _, pb_, lb_ = eb.get_field(1)
    assert rel(pb_[M.p], pa_) < RTOL and rel(lb_[M.l], la_) < RTOL
    if not tracer_and_dg:
        return
    # continuous space: L2 projection, vorticity (compared as broken fields), tracer operator
    u = rng.standard_normal(ea.shape_Q)
    Pa = ea.cg_project_nodal(u)
    assert rel(eb.cg_project_nodal(M.Qb(u))[M.q], Pa) < RTOL
    assert rel(eb.cg_to_broken(eb.vorticity(Qb))[M.q], ea.cg_to_broken(ea.vorticity(Q))) < RTOL
    q = rng.standard_normal(ea.shape_p)
    assert rel(eb.apply_tracer_advection(M.pb(q), M.Qb(u), project=True)[M.p], ea.apply_tracer_advection(q, u, project=True)) < RTOL
    assert rel(eb.apply_tracer_advection(M.pb(q), M.Qb(Pa), project=False)[M.p], ea.apply_tracer_advection(q, Pa, project=False)) < RTOL
    # DG: averaged trace and the coupled operator
    assert rel(eb.dg_avg_trace(pb)[M.l], ea.dg_avg_trace(p)) < RTOL
    oua, opa = ea.apply_dg_operator(Qs, x, p, 0.05)
    oub, opb = eb.apply_dg_operator(M.Qb(Qs), M.Qb(x), pb, 0.05)
    assert rel(oub[M.q], oua) < RTOL and rel(opb[M.p], opa) < RTOL


def smooth_data(seed):
    """smooth random data for which nothing cancels: (Q0(x, y), p0(x, y), f(t)(x, y))"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.0, 1.0, size=(3, 6))
    Q0 = lambda x, y: (a[0, 0] * np.sin(2 * x + a[0, 1]) * np.cos(1.5 * y) + a[0, 2] * y, a[0, 3] * np.cos(1.7 * x) * np.sin(2 * y + a[0, 4]) + a[0, 5] * x)
    p0 = lambda x, y: a[1, 0] * np.cos(2 * x + a[1, 1]) * np.sin(1.3 * y + a[1, 2])
    f = lambda t: (lambda x, y: (a[2, 0] * np.sin(3 * t + x + a[2, 1] * y), a[2, 2] * np.cos(2 * t - y + a[2, 3] * x)))
    return Q0, p0, f


# --- Kelvin-Helmholtz with a tracer (the benchmarked set-up, tools/kh_bench.py)

KH_DT = 0.005


def kh_tracer(x, y):
    return np.sin(1.5 * x + 0.3) * np.cos(1.2 * y) + 0.2 * x


def kh_runs(pm, runs, dt=KH_DT):
    """Product runs of the Kelvin-Helmholtz data (with the tracer for SSP2): runs = [(name, k, kind, option)], kind "ssp2"
    (option: fused, two steps) or "implicit" (option: use_projection_method, one step).  {name: dict(Q, p, q, its)}"""
    from incompressibleeulerhdg_amd import timesteppers as tsm
    from incompressibleeulerhdg_amd.model_problems import KelvinHelmholtz

    out = {}
    for name, k, kind, option in runs:
        if kind == "ssp2":
            ts = tsm.IncompressibleEulerHDGIMEXSSP2_332(pm, k, dt, use_projection_method=True, n_richardson=2)
            kh = KelvinHelmholtz(ts._V_Q, ts._V_p)
            Q, p = ts.solve(*kh.initial_condition(), kh_tracer, kh.f_rhs(), 2 * dt, fused=option)
            q = ts.q_tracer.dat.data.copy()
        else:
            ts = tsm.IncompressibleEulerHDGImplicit(pm, k, dt, use_projection_method=option)
            kh = KelvinHelmholtz(ts._V_Q, ts._V_p)
            Q, p = ts.solve(*kh.initial_condition(), None, kh.f_rhs(), dt)
            q = np.zeros(0)
        sums, cnt = ts._engine.iteration_stats()
        ev = ts._engine.solver_events()
        out[name] = dict(Q=Q.dat.data.copy(), p=p.dat.data.copy(), q=q, its=sums / np.maximum(cnt, 1), cnt=cnt,
                         events=np.array([ev["cg_residual_replacements"], ev["cg_floor_exits"], ev["sstep_gmres_fallbacks"]]))
        ts._engine.close()
    return out
