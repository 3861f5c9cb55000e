"""The wall and diffusion stencil kernels on meshes of many waves, against the references of
tests/*_reference.py carried to the size by tests/stencil_lift.py (checked without a GPU in tests/test_stencil_lift_cpu.py).

The hook tests of sections 19-24 and 28 compare on meshes below one workgroup (nx = 3; periodic 4 or 8), where every wave
touches every wall.  Here the same hooks run where the launch geometry (Engine::bs(), the Geo set-up, HDG_CELL_PROLOGUE) differs:

    nx = 20    one workgroup of 64 with a partial wave; rows_xcd = 3: band 6 holds two rows, band 7 none
    nx = 72    bs = 128: wave 0 is full with lane 0 alone on the left wall, wave 1 has 8 live lanes and the right wall, the
               interior rows give waves with no wall cell; rows_xcd = 9; R = 84 rows, no padding row
    nx = 130   two workgroups a row, the second with 2 live lanes and a dead wave; rows_xcd = 17, the last band 11 rows; the
               channel rule pads R = 142 by 4 rows (32 nx R mod 2^19 = 2.03 2^15, the first admissible pad gives 2.54 2^15)
    periodic 72 and 132 (R = 144, no padding row): the x-wrap joins lane 0 and lane nx - 1 of different waves and
               workgroups, the ghost rows wrap in y

Degrees: k = 1 .. 4 at nx = 20 and 72 (both kinds), k = 1, 2 at nx = 130 and 132, and k = 4 at nx = 130 as well: the lifted
reference of that case is a gather and an einsum over 33 800 cells of 42 dofs (0.1 s, 50 MB).

Bounds, the project's own: relative max-norm 1e-10 for the operator hooks (HOOK of test_gpu_viscosity.py,
test_gpu_tracer_diffusion.py, test_gpu_moving_walls.py), 1e-12 for the buoyancy (HOOK of test_gpu_buoyancy.py), 1e-9 for the
solve (HOOK of test_gpu_tracer_implicit.py).  The operators are local and the bounds relative: the mesh size does not move them.
The forward-Euler step of a batch is compared through its increment (q_new - q) / (dt kappa_t): the subtraction costs
eps / (dt kappa_t Lambda) >= eps / 0.35 of max|A q|, far below the hook's 1e-10, which is the bound used.

The smooth field on the periodic meshes is the one exception.  It is made of the wavenumbers 0 .. 2 on a square of side 2 pi, so
M^-1 V Q is of size 10 where the entries of the operator times the field are of size Lambda = 5e5 .. 7e5: both sides of the
comparison lose five to six digits by cancellation, and relative to max|out| the lifted reference itself, evaluated in
np.longdouble, moves by 1.06e-10 (nx = 72, k = 3), 1.31e-10 (72, 4) and 9.9e-11 (132, 2) for M^-1 V and by 4.7e-11 (72, 4) for
M^-1 D, which is the hook bound already; the device is 3.5e-10 .. 5.6e-10 (M^-1 V) and 2.7e-10 (M^-1 D) from the extended
reference.  The same cases on the tiny meshes pass 1e-10, and the broken random field and the jump across the seam pass it here
(at most 4.5e-14).  So where the smooth periodic field misses 1e-10 the test measures the reference's rounding in that case and
allows ten times it, never more than ten times the largest measured: 1.3e-9 for M^-1 V, 4.7e-10 for M^-1 D.

The direct solves: SuperLU on the lifted sparse system in a nested-dissection order.  The slowest cases of the module are these
solves at nx = 72: 2 s a case at k = 3 and 6 s at k = 4 (155 520 unknowns) next to an MI355X; everything else is below a second."""
import numpy as np
import pytest

import stencil_lift as sl

pytestmark = pytest.mark.gpu
HOOK, BUOYANCY, SOLVE = 1e-10, 1e-12, 1e-9
SMOOTH_V, SMOOTH_D = 1.3e-9, 4.7e-10  # the smooth field on the periodic meshes: ten times the reference's own rounding (docstring)
L_PER = 2 * np.pi
DT = 0.01
TB = {1: 4, 2: 4, 3: 2, 4: 1}  # tracers per thread (TracerBlock<K>, csrc/hdg_cg.hpp)
NUMBERS = (0.5, 50.0, 5000.0)
SQUARE = [(nx, k) for nx in (20, 72) for k in (1, 2, 3, 4)] + [(130, 1), (130, 2), (130, 4)]
PERIODIC = [(72, k) for k in (1, 2, 3, 4)] + [(132, 1), (132, 2)]
SOLVES = [(nx, k) for nx in (20, 72) for k in (1, 2, 3, 4)] + [(130, 1)]
COLS = 64  # cells of a row in the first wave
_SMALL = {}


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300)


def _small(kind, k):
    """The dense references of the small mesh (nx0 = 3, periodic 4): once per kind and degree; read-only"""
    from oracle import hdg_oracle as orc

    if (kind, k) not in _SMALL:
        d0 = orc.HDGDiscretisation(4, k, periodic=True, L=L_PER) if kind == "periodic" else orc.HDGDiscretisation(3, k)
        ops, funs, wallop = sl.references(d0)
        for A, b, *_ in list(ops.values()) + list(funs.values()):
            A.setflags(write=False)
            if b is not None:
                b.setflags(write=False)
        _SMALL[kind, k] = (d0, ops, funs, wallop)
    return _SMALL[kind, k]


def _stepper(which, mesh, k, dt, **kw):
    from incompressibleeulerhdg_amd import timesteppers as tsm

    cls = {"ssp2": tsm.IncompressibleEulerHDGIMEXSSP2_332, "implicit": tsm.IncompressibleEulerHDGImplicit}[which]
    kw.update(use_projection_method=True, n_richardson=2)
    return cls(mesh, k, dt, **kw)


class _Case:
    """One engine on the large mesh with the lift of the small references onto it and the fields of the hook tests."""

    def __init__(self, kind, nx, k, n_tracers):
        from incompressibleeulerhdg_amd.mesh import PeriodicSquareMesh, UnitSquareMesh

        self.kind, self.nx, self.k = kind, nx, k
        mesh = PeriodicSquareMesh(nx, nx, L=L_PER) if kind == "periodic" else UnitSquareMesh(nx, nx)
        self.eng = _stepper("implicit", mesh, k, DT, n_tracers=n_tracers)._engine
        self.d0, self.ops, self.funs, self.wallop = _small(kind, k)
        self.grid = sl.Grid.of_engine(self.eng)
        self.lift = sl.Lift(self.d0, self.grid)
        xq, xp = self.eng.node_coordinates()
        rng = np.random.default_rng(31 + k)
        w = 2 * np.pi / (L_PER if kind == "periodic" else 1.0)

        def smooth(x, y):
            return sum(rng.uniform(-1, 1) * np.sin(w * (m * x + n * y) + rng.uniform(0, 6)) for m in range(3) for n in range(3))

        x, y = xq[:, 0], xq[:, 1]
        self.xq, self.xp = xq, xp
        self.Q = {"broken": rng.standard_normal(xq.shape), "smooth": np.stack([smooth(x, y), smooth(x, y)], axis=-1)}
        x, y = xp[:, 0], xp[:, 1]
        self.q = {"broken": rng.standard_normal(len(x)), "smooth": smooth(x, y)}
        if kind == "periodic":  # a jump across the seam
            self.Q["seam"] = np.stack([xq[:, 0] + 2.0 * xq[:, 1] - 0.5 * xq[:, 0] * xq[:, 1], xq[:, 1] ** 2 - xq[:, 0]], axis=-1)
            self.q["seam"] = x + 2.0 * y - 0.5 * x * y
        self.label = f"{kind} nx={nx} k={k}"

    def op(self, name, **kw):
        return self.lift.operator(*self.ops[name], **kw)

    def fun(self, name):
        return self.lift.functional(*self.funs[name])

    def close(self):
        self.eng.close()


def _compare(c, what, fields, device, op, bound, smooth_cap=None):
    """device(field) against the lifted operator on every field; prints every figure, then asserts.  Where a field misses the
    bound the reference is evaluated in extended precision as well, which tells its own rounding from the device's error.
    smooth_cap: the smooth field alone may then take ten times that measured rounding of the reference as its bound, up to the
    cap (the module's docstring); nothing of this is read off the device's output"""
    errs, allowed = {}, {}
    for name, f in fields.items():
        got, want = np.ravel(device(f)), op @ np.ravel(f)
        errs[name], allowed[name] = _rel(got, want), bound
        if errs[name] > bound:
            ext = op.apply(np.ravel(f), np.longdouble)
            own = _rel(want, ext)
            print(f"{c.label} {what} {name}: in extended precision the reference moves by {own:.3e}, the device is {_rel(got, ext):.3e} from it")
            if name == "smooth" and smooth_cap is not None:
                allowed[name] = min(max(bound, 10.0 * own), smooth_cap)
    print(f"{c.label} {what}: " + ", ".join(f"{n} {e:.3e}" for n, e in errs.items()))
    assert all(errs[n] <= allowed[n] for n in errs), (what, errs, allowed)
    return max(errs.values())


def _walls_of(t):
    """fixed values on left, right and top, distinct per side and per tracer; the bottom is no flux"""
    return {s: v * (1.0 + 0.5 * t) + 0.1 * t for s, v in sl.WALLS3.items()}


def _betas(n):
    """distinct, beta_1 = 0 when there is a tracer 1 (test_gpu_buoyancy.py)"""
    return np.array([0.0 if t == 1 else (-1.0) ** t * (0.5 + 0.25 * t) for t in range(n)]) if n > 1 else np.array([1.7])


# ---- what both kinds of mesh share
def _viscosity(c, wall):
    A = c.op("viscosity " + wall)
    _compare(c, f"apply_viscosity {wall}", c.Q, lambda Q: c.eng.apply_viscosity(Q, wall), A, HOOK, SMOOTH_V if c.kind == "periodic" else None)
    assert c.eng.viscosity() == (0.0, "free_slip")  # the hook sets nothing


def _tracer_diffusion(c):
    A = c.op("tracer diffusion")
    _compare(c, "apply_tracer_diffusion", c.q, c.eng.apply_tracer_diffusion, A, HOOK, SMOOTH_D if c.kind == "periodic" else None)
    lam = c.eng.tracer_diffusion_number()[0]
    const = np.max(np.abs(c.eng.apply_tracer_diffusion(np.ones(c.eng.shape_p))))
    print(f"{c.label} apply_tracer_diffusion: constants map to {const / lam:.3e} Lambda (Lambda {lam:.6g})")
    assert const <= 1e-9 * lam


def _buoyancy(c):
    eng, n = c.eng, c.eng.n_tracers
    beta = _betas(n)
    B = c.op("buoyancy")  # with beta = 1
    names = list(c.q)
    q = np.stack([(1.0 + 0.1 * t) * c.q[names[t % len(names)]] for t in range(n)])
    eng.set_tracer(np.zeros(eng.shape_q))
    eng.set_buoyancy(beta, sl.GRAVITY)
    want = (B @ (beta @ q)).reshape(-1, 2)
    got = eng.apply_buoyancy(q if n > 1 else q[0])
    err = _rel(got, want)
    print(f"{c.label} apply_buoyancy, {n} tracers: {err:.3e}")
    if n > 1:  # a passive tracer is not read
        q[1] = np.nan
        assert np.array_equal(eng.apply_buoyancy(q), got)
    eng.set_buoyancy(None)
    eng.set_tracer(None)
    assert err <= BUOYANCY


def _coriolis(c):
    A = c.op("coriolis beta=0")
    _compare(c, f"apply_coriolis f0={sl.F0} beta=0", c.Q, lambda Q: c.eng.apply_coriolis(Q, sl.F0, 0.0), A, HOOK)
    if c.kind == "square" and c.nx in (72, 130):  # beta != 0: exact on a field of degree <= k, f_c being linear
        import coriolis_reference as cref

        x, y, k = c.xq[:, 0], c.xq[:, 1], c.k
        poly = np.stack([1.0 + x - 2.0 * y + (x * y if k > 1 else 0.0) + (y ** k), 0.5 - y + 0.3 * x - (x ** k)], axis=-1)
        for f0, beta in ((0.0, 2.1), (-1.3, 2.6)):  # the second: an equator inside the mesh
            err = _rel(c.eng.apply_coriolis(poly, f0, beta), cref.closed_form(f0, beta, x, y, poly))
            print(f"{c.label} apply_coriolis f0={f0} beta={beta} against the closed form: {err:.3e}")
            assert err <= HOOK
    assert c.eng.coriolis() == (0.0, 0.0)


# ---- 1. the unit square
@pytest.fixture(scope="class", params=SQUARE, ids=lambda p: f"nx{p[0]}-k{p[1]}")
def square(request, hip_lib):
    nx, k = request.param
    c = _Case("square", nx, k, TB[k] + 1)
    yield c
    c.close()


class TestSquare:
    @pytest.mark.parametrize("wall", ["free_slip", "no_slip"])
    def test_apply_viscosity(self, square, wall):
        _viscosity(square, wall)

    def test_apply_moving_walls(self, square):
        c = square
        Ab = c.op("moving walls")
        _compare(c, "apply_moving_walls", c.Q, lambda Q: c.eng.apply_moving_walls(Q, sl.SPEEDS), Ab, HOOK)
        Q = c.Q["broken"]
        load = np.max(np.abs(c.eng.apply_moving_walls(Q, sl.SPEEDS) - c.eng.apply_viscosity(Q, "no_slip"))) / np.max(np.abs(Ab @ Q.ravel()))
        print(f"{c.label} apply_moving_walls: the load is {load:.3e} of the output")
        assert load > 1e-3  # the load is no rounding matter
        assert not c.eng.wall_velocity().any()

    def test_wall_force_of(self, square):
        c = square
        total = c.fun("integral")
        for wall, U in (("no_slip", np.array(sl.SPEEDS)), ("free_slip", np.zeros(4))):
            G = c.fun("wall force " + wall)
            worst = worst_budget = 0.0
            for name, Q in c.Q.items():
                want = (G.linear(Q) + np.repeat(U, 2) * G.c).reshape(4, 2)
                got = c.eng.wall_force_of(Q, U, wall)
                err = _rel(got, want)
                # the budget on the device: the sum over the sides against the integral of the hook's output
                out = c.eng.apply_moving_walls(Q, U, wall)
                integral = total.linear(out)
                budget = np.max(np.abs(got.sum(axis=0) - integral)) / np.max(np.abs(got))
                print(f"{c.label} wall_force_of {wall} {name}: force {err:.3e}, budget {budget:.3e} (sum {got.sum(axis=0)}, integral {integral})")
                worst, worst_budget = max(worst, err), max(worst_budget, budget)
                assert np.array_equal(c.eng.wall_force_of(Q, U, wall), got)  # two calls: the same bits
                if wall == "free_slip":  # the normal part only
                    assert np.all(got[[0, 2], 0] == 0.0) and np.all(got[[1, 3], 1] == 0.0)
            assert worst <= HOOK and worst_budget <= HOOK, (wall, worst, worst_budget)

    def test_apply_tracer_diffusion(self, square):
        _tracer_diffusion(square)

    def test_apply_tracer_wall_diffusion(self, square):
        c = square
        for t in range(c.eng.n_tracers):  # the walls of every tracer of the batch below, one at a time through the hook
            walls = _walls_of(t)
            Ab = c.lift.operator(*c.wallop.minv(walls), exponent=-2, rows="P")
            _compare(c, f"apply_tracer_wall_diffusion, walls of tracer {t}", c.q, lambda q: c.eng.apply_tracer_wall_diffusion(q, walls), Ab, HOOK)
        assert c.eng.tracer_walls() is None  # the hook sets nothing

    def test_a_batch_with_distinct_kappa_and_walls(self, square):
        """TB + 1 tracers, each with its own kappa and wall values: the wall flux against kappa_t l_w . (g - q_t) with the
        lifted loads, and one forward-Euler step at rest (the tracer-block tail of k_tracer_diff<K, TB, true>) against
        q_t + dt kappa_t (A q_t + b_t)"""
        c, eng = square, square.eng
        n = eng.n_tracers
        walls = [_walls_of(t) for t in range(n)]
        eng.set_tracer_walls(walls)
        lam = eng.tracer_diffusion_number()[0]
        kappa = np.array([0.35 / (DT * lam) * (t + 2.0) / (n + 1.0) for t in range(n)])  # distinct; the largest number 0.35
        eng.set_tracer_diffusivity(kappa)
        names = list(c.q)
        q = np.stack([(1.0 + 0.1 * t) * c.q[names[t % len(names)]] for t in range(n)])
        eng.set_state(np.zeros(eng.shape_Q), np.zeros(eng.shape_p))
        eng.set_forcing_scale(0, 0.0)
        eng.set_tracer(q if n > 1 else q[0])
        q_in = eng.get_tracer().reshape(n, -1)  # as the engine holds it (nodal -> modal -> nodal)
        loads = c.fun("flux loads")
        one = loads.linear(np.ones(eng.shape_p))
        sides = ("bottom", "right", "top", "left")
        want = np.array([[kappa[t] * (walls[t][s] * one[w] - loads.linear(q_in[t])[w]) if s in walls[t] else 0.0 for w, s in enumerate(sides)] for t in range(n)])
        flux = eng.tracer_wall_flux()
        err = _rel(flux, want)
        print(f"{c.label} tracer_wall_flux, {n} tracers: {err:.3e}")
        assert np.array_equal(eng.tracer_wall_flux(), flux) and np.all(flux[:, 0] == 0.0)  # the same bits; the no-flux side
        eng.implicit_step()
        q_out = eng.get_tracer().reshape(n, -1)
        worst = 0.0
        for t in range(n):
            Ab = c.lift.operator(*c.wallop.minv(walls[t]), exponent=-2, rows="P")
            e = _rel((q_out[t] - q_in[t]) / (DT * kappa[t]), Ab @ q_in[t])
            worst = max(worst, e)
        print(f"{c.label} one forward-Euler step at rest, {n} tracers: largest |increment - reference| = {worst:.3e} max|A q + b|")
        eng.set_tracer_diffusivity(None)
        eng.set_tracer_walls(None)
        eng.set_tracer(None)
        assert err <= HOOK and worst <= HOOK

    def test_apply_buoyancy(self, square):
        _buoyancy(square)

    def test_apply_coriolis(self, square):
        _coriolis(square)


# ---- 2. the doubly periodic square
@pytest.fixture(scope="class", params=PERIODIC, ids=lambda p: f"nx{p[0]}-k{p[1]}")
def periodic(request, hip_lib):
    nx, k = request.param
    c = _Case("periodic", nx, k, TB[k] + 1)
    yield c
    c.close()


class TestPeriodic:
    def test_apply_viscosity(self, periodic):
        _viscosity(periodic, "free_slip")

    def test_apply_tracer_diffusion(self, periodic):
        _tracer_diffusion(periodic)

    def test_apply_buoyancy(self, periodic):
        _buoyancy(periodic)

    def test_apply_coriolis(self, periodic):
        _coriolis(periodic)


# ---- 3. the backward-Euler solve against the direct solve of the lifted system
def _solve_case(c, walls, number, displace_x=None):
    """(the device's solutions of three fields, its iteration counts, the direct solutions) at tau = number / Lambda"""
    eng = c.eng
    eng.set_tracer_walls(walls)
    eng.set_tracer_diffusion_mode("explicit", rtol=1e-12)  # the hook solves in either mode, to the rtol that is set
    tau = number / eng.tracer_diffusion_number()[0]  # Lambda with the walls that are set
    q = np.stack(list(c.q.values()) + [c.q["broken"][::-1]])[:3]
    got, its = eng.solve_tracer_diffusion([tau] * 3, q)
    assert np.array_equal(eng.tracer_diffusion_solve()[0], its) and np.all(its > 0)  # positive, and reported
    assert np.all(eng.tracer_diffusion_solve()[1] <= 1e-12)
    eng.set_tracer_walls(None)
    perm = sl.nested_dissection(c.grid, c.grid.n["P"])
    wants = []
    for dx in (None, displace_x) if displace_x is not None else (None,):
        op = c.lift.operator(*(c.wallop.minv(walls) if walls else c.ops["tracer diffusion"][:2]), exponent=-2, rows="P", displace_x=dx)
        S, load = op.system(tau)
        lu = sl.DirectSolve(S, perm)
        wants.append(np.stack([lu.solve(q[t] + load) for t in range(3)]))
    return got, its, wants


@pytest.fixture(scope="class", params=SOLVES, ids=lambda p: f"nx{p[0]}-k{p[1]}")
def solver(request, hip_lib):
    nx, k = request.param
    c = _Case("square", nx, k, 3)
    yield c
    c.close()


class TestSolve:
    @pytest.mark.parametrize("number", NUMBERS)
    @pytest.mark.parametrize("walls", [None, sl.WALLS3], ids=["noflux", "walls"])
    def test_solve_tracer_diffusion(self, solver, walls, number):
        c = solver
        got, its, (want,) = _solve_case(c, walls, number)
        errs = [_rel(got[t], want[t]) for t in range(3)]
        print(f"{c.label} solve_tracer_diffusion walls={bool(walls)} number {number:g}: iterations {its.tolist()}, " + ", ".join(f"{e:.3e}" for e in errs) + " max|x|")
        assert max(errs) <= SOLVE


# ---- 4. the comparisons can fail: a reference whose x-neighbour is displaced by one column for the cells with i >= 64 at nx = 72
@pytest.fixture(scope="module")
def beyond_the_first_wave(hip_lib):
    c = _Case("square", 72, 1, 3)
    yield c, c.grid.i >= COLS
    c.close()


def _seen(c, what, got, good, bad, bound, far, n):
    """the right reference within the bound; the displaced one misses it by orders of magnitude, in the displaced cells alone
    when the operator is local"""
    right, wrong = _rel(got, good), _rel(got, bad)
    print(f"{c.label} {what}: right reference {right:.3e}, displaced beyond column {COLS} {wrong:.3e}")
    assert right <= bound
    assert wrong >= 1e-3  # seven orders above the hooks' bound, six above the solve's
    if n:  # a local operator: the rows of the other cells are untouched
        keep = ~np.repeat(far, n)
        assert _rel(np.ravel(got)[keep], np.ravel(bad)[keep]) <= bound


def test_a_displaced_neighbour_beyond_the_first_wave_is_seen_by_the_viscosity(beyond_the_first_wave):
    c, far = beyond_the_first_wave
    Q = c.Q["broken"]
    got = c.eng.apply_viscosity(Q, "no_slip")
    good, bad = (c.op("viscosity no_slip", displace_x=dx) @ Q.ravel() for dx in (None, far))
    _seen(c, "apply_viscosity no_slip", got.ravel(), good, bad, HOOK, far, c.grid.n["Q"])


def test_a_displaced_neighbour_beyond_the_first_wave_is_seen_by_the_tracer_diffusion(beyond_the_first_wave):
    c, far = beyond_the_first_wave
    q = c.q["broken"]
    got = c.eng.apply_tracer_wall_diffusion(q, sl.WALLS3)
    good, bad = (c.op("tracer walls", displace_x=dx) @ q for dx in (None, far))
    _seen(c, "apply_tracer_wall_diffusion", got, good, bad, HOOK, far, c.grid.n["P"])


def test_a_displaced_neighbour_beyond_the_first_wave_is_seen_by_the_solve(beyond_the_first_wave):
    c, far = beyond_the_first_wave
    got, its, (good, bad) = _solve_case(c, sl.WALLS3, 50.0, displace_x=far)
    _seen(c, "solve_tracer_diffusion number 50", got, good, bad, SOLVE, far, 0)
