"""The lifted references of tests/stencil_lift.py against the dense references built directly on the larger mesh (no GPU).

Every operator and functional that tests/test_gpu_stencil_sizes.py compares a kernel with is lifted from nx0 = 3 to nx = 5 and 7
on the unit square (k = 1 .. 4) and from 4 to 6 on the periodic square (k = 1, 2): two target sizes pin the exponent of h.

Bound: 1e-12 relative max-norm on broken random data.  The dense reference reproduces itself under translation to about 4e-15
(measured on the CPU: M^-1 V 2.1e-15 .. 3.6e-15, the tracers' wall operator 1.4e-15 .. 2.3e-15), so the bound leaves room for the
conditioning of the k = 4 mass matrix and none for a wrong block: one class of cells with its x-neighbour displaced by a column
misses it by more than 1e-3 (the negative check)."""
import numpy as np
import pytest

import stencil_lift as sl

BOUND = 1e-12
L_PER = 2 * np.pi
_D = {}


def _disc(kind, nx, k):
    """(discretisation, its references): once per mesh and degree; read-only"""
    from oracle import hdg_oracle as orc

    if (kind, nx, k) not in _D:
        d = orc.HDGDiscretisation(nx, k, periodic=True, L=L_PER) if kind == "periodic" else orc.HDGDiscretisation(nx, k)
        ops, funs, wallop = sl.references(d)
        for A, b, *_ in list(ops.values()) + list(funs.values()):
            A.setflags(write=False)
            if b is not None:
                b.setflags(write=False)
        _D[kind, nx, k] = (d, ops, funs)
    return _D[kind, nx, k]


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


CASES = [("square", 3, nx, k) for k in (1, 2, 3, 4) for nx in (5, 7)] + [("periodic", 4, 6, k) for k in (1, 2)]


@pytest.mark.parametrize("kind,nx0,nx,k", CASES)
def test_lifted_references_equal_the_dense_ones(kind, nx0, nx, k):
    d0, ops0, funs0 = _disc(kind, nx0, k)
    d1, ops1, funs1 = _disc(kind, nx, k)
    assert set(ops0) == set(ops1) and set(funs0) == set(funs1)
    if kind == "square":  # every operator the GPU tests use
        assert set(ops0) == {"viscosity free_slip", "viscosity no_slip", "moving walls", "tracer diffusion", "tracer walls", "buoyancy", "coriolis beta=0"}
        assert set(funs0) == {"wall force no_slip", "wall force free_slip", "flux loads", "integral"}
    lift = sl.Lift(d0, sl.Grid.of_oracle(d1))
    rng = np.random.default_rng(100 * nx + k)
    for name, (A0, b0, exponent, rows, cols) in ops0.items():
        A1, b1 = ops1[name][:2]
        op = lift.operator(A0, b0, exponent, rows, cols)
        x = rng.standard_normal(A1.shape[1])
        want = A1 @ x + (0.0 if b1 is None else b1)
        err = _rel(op @ x, want)
        aff = 0.0 if b1 is None else _rel(op.b, b1)
        mat = _rel(op.matrix() @ x, A1 @ x)  # the sparse form of the same operator
        print(f"{kind} {nx0} -> {nx} k={k} {name}: {err:.3e}, affine part {aff:.3e}, sparse {mat:.3e}")
        assert max(err, aff, mat) <= BOUND, name
        if b1 is not None:
            assert np.max(np.abs(b1)) > 1e-3 * np.max(np.abs(want))  # the affine part is no rounding matter
    for name, (F0, c0, exponent, space) in funs0.items():
        F1, c1 = funs1[name][:2]
        fun = lift.functional(F0, c0, exponent, space)
        x = rng.standard_normal(F1.shape[1])
        live = np.max(np.abs(F1), axis=1) > 0.0  # free slip: the tangential functionals vanish, on both sides of the comparison
        got = fun.linear(x)
        assert np.all(got[~live] == 0.0)
        err = _rel(got[live], (F1 @ x)[live])
        dense = _rel(fun.dense(), F1)
        const = 0.0 if c1 is None else _rel(fun.c, c1)
        print(f"{kind} {nx0} -> {nx} k={k} {name}: {err:.3e}, entries {dense:.3e}, constants {const:.3e}")
        assert max(err, dense, const) <= BOUND, name


def test_the_backward_euler_system_is_the_dense_one():
    d0, ops0, _ = _disc("square", 3, 2)
    d1, ops1, _ = _disc("square", 5, 2)
    lift = sl.Lift(d0, sl.Grid.of_oracle(d1))
    A1, b1 = ops1["tracer walls"][:2]
    S, load = lift.operator(*ops0["tracer walls"]).system(0.37)
    assert _rel(S.toarray(), np.eye(len(b1)) - 0.37 * A1) <= BOUND and _rel(load, 0.37 * b1) <= BOUND


@pytest.mark.parametrize("kind,nx0,nx,name", [("square", 3, 7, "viscosity no_slip"), ("square", 3, 7, "tracer walls"), ("periodic", 4, 6, "tracer diffusion")])
def test_a_displaced_neighbour_is_seen(kind, nx0, nx, name):
    """one class of cells (the interior lower-left triangles) takes its x-neighbour from one column too far"""
    d0, ops0, _ = _disc(kind, nx0, 1)
    d1, ops1, _ = _disc(kind, nx, 1)
    t = sl.Grid.of_oracle(d1)
    lift = sl.Lift(d0, t)
    A1, b1 = ops1[name][:2]
    x = np.random.default_rng(7).standard_normal(A1.shape[1])
    want = A1 @ x + (0.0 if b1 is None else b1)
    good = lift.operator(*ops0[name])
    bad = lift.operator(*ops0[name], displace_x=t.cls == 0)
    print(f"{kind} {name}: right {_rel(good @ x, want):.3e}, displaced {_rel(bad @ x, want):.3e}")
    assert _rel(good @ x, want) <= BOUND
    assert _rel(bad @ x, want) > 1e-3


def test_the_layout_check_is_loud():
    """another node order, another vertex numbering or a mesh of another kind raise; none of them compares wrong blocks quietly"""
    d0, ops0, _ = _disc("square", 3, 1)
    d1, _, _ = _disc("square", 5, 1)
    m = d1.mesh
    xq, xp = d1.node_coords(d1.PU), d1.node_coords(d1.PP)
    sl.Lift(d0, sl.Grid(m.cell_vertices, xq, xp, m.nx))  # as it is: fine
    with pytest.raises(ValueError, match="local node layout"):
        sl.Lift(d0, sl.Grid(m.cell_vertices, xq, xp[:, ::-1], m.nx))  # the nodes of a cell in another order
    with pytest.raises(ValueError, match="local node layout"):
        sl.Lift(d0, sl.Grid(m.cell_vertices, np.roll(xq, 1, axis=1), xp, m.nx))
    perm = np.random.default_rng(3).permutation(m.ncells)  # another cell numbering is no error: the map is derived
    lift = sl.Lift(d0, sl.Grid(m.cell_vertices[perm], xq[perm], xp[perm], m.nx))
    A1 = _disc("square", 5, 1)[1]["tracer diffusion"][0]
    x = np.random.default_rng(4).standard_normal(A1.shape[1])
    n = d1.np_
    got = (lift.operator(*ops0["tracer diffusion"]) @ x.reshape(-1, n)[perm].ravel()).reshape(-1, n)
    assert _rel(got, (A1 @ x).reshape(-1, n)[perm]) <= BOUND
    with pytest.raises(ValueError, match="periodicity"):
        sl.Lift(_disc("periodic", 4, 1)[0], sl.Grid(m.cell_vertices, xq, xp, m.nx))
    with pytest.raises(ValueError, match="cells"):
        sl.Grid(m.cell_vertices[:-2], xq[:-2], xp[:-2], m.nx)
