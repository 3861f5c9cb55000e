"""The linear drag term without a GPU: the numpy reference's own properties, the stability report, the
host packing (a stand-alone g++ program under the address and undefined-behaviour sanitizers), the C-ABI table, the Python
surface on a stand-in engine, the two model problems and the driver's refusals."""
import os
import re
import shutil
import subprocess
import warnings

import numpy as np
import pytest

import drag_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_REFS = {}


def reference(k):
    """3 x 3 unit square: discretisation, random non-negative vertex values (broken across cells), M^-1 D; read-only"""
    from oracle import hdg_oracle as orc

    if k not in _REFS:
        d = orc.HDGDiscretisation(3, k)
        sig = np.random.default_rng(11 + k).uniform(0.0, 2.5, (d.mesh.ncells, 3))
        sig[4] = 0.0  # a cell outside the mask
        A = ref.minv_d(d, sig)
        for a in (sig, A):
            a.setflags(write=False)
        _REFS[k] = (d, sig, A)
    return _REFS[k]


# ---- the reference
@pytest.mark.parametrize("k", [1, 2])
def test_reference_is_symmetric_and_its_spectrum_lies_in_0_S(k):
    d, sig, A = reference(k)
    M = d.MQ.toarray()
    MA = M @ A
    assert np.max(np.abs(MA - MA.T)) <= 1e-13 * np.max(np.abs(MA))
    ev = np.linalg.eigvals(A)
    S = ref.bound(sig)
    assert np.max(np.abs(ev.imag)) <= 1e-12 * S and ev.real.min() >= -1e-12 * S and ev.real.max() <= S * (1 + 1e-12)
    B = ref.blocks(sig, k)  # the blockwise form is the same operator
    Q = np.random.default_rng(1).standard_normal((d.NQ // 2, 2))
    assert np.max(np.abs(ref.apply_blocks(B, Q) + (A @ Q.ravel()).reshape(-1, 2))) <= 1e-13 * S * np.max(np.abs(Q))
    print(f"k={k}: spectrum in [{ev.real.min():.4g}, {ev.real.max():.4g}], S {S:.4g}")


@pytest.mark.parametrize("k", [1, 2])
def test_reference_is_pointwise_for_polynomials_and_its_force_is_its_integral(k):
    d, sig, A = reference(k)
    X = d.node_coords(d.PU).reshape(-1, 2)
    x, y = X[:, 0], X[:, 1]
    V = d.mesh.cell_vertices
    Xc = X.reshape(len(V), -1, 2)
    J = np.stack([V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]], axis=-1)
    lam = np.einsum("cij,cnj->cni", np.linalg.inv(J), Xc - V[:, None, 0])
    s_nodes = (sig[:, None, 0] + (sig[:, 1] - sig[:, 0])[:, None] * lam[..., 0] + (sig[:, 2] - sig[:, 0])[:, None] * lam[..., 1]).reshape(-1)
    Q = np.stack([1.0 + x - 2.0 * y + (x * y if k > 1 else 0.0) + y ** k, 0.5 - y + 0.3 * x - x ** k], axis=-1)  # degree <= k
    us = np.stack([0.3 - x + 0.5 * y, 0.1 + 0.2 * x + y], axis=-1)
    Ab = ref.affine(d, sig, us, A=A)
    out = (Ab @ Q.ravel()).reshape(-1, 2)
    exact = ref.closed_form(s_nodes, Q, us)
    assert np.max(np.abs(out - exact)) <= 1e-12 * np.max(np.abs(exact))
    # sum_r F_r is the M-weighted integral of - M^-1 D (Q - u_s); P <= 0 for u_s = 0
    areas = ref.cell_areas(V)
    rng = np.random.default_rng(2)
    W = rng.standard_normal(Q.shape)
    region = rng.integers(0, 4, len(V))
    F = ref.force_blockwise(sig, k, areas, W, us, region)
    out = (Ab @ W.ravel()).reshape(-1, 2)
    assert np.max(np.abs(F[:, :2].sum(axis=0) - ref.integral(d, out))) <= 1e-12 * np.max(np.abs(F))
    assert abs(F[:, 2].sum() - W.ravel() @ (d.MQ @ out.ravel())) <= 1e-12 * np.max(np.abs(F))
    P0 = ref.force_blockwise(sig, k, areas, W, None, region)[:, 2]
    assert np.all(P0 <= 0.0) and P0.sum() < 0.0
    assert np.max(np.abs(ref.mass_dot(k, areas, W, out) - W.ravel() @ (d.MQ @ out.ravel()))) <= 1e-12 * np.max(np.abs(F))


# ---- the stability report
def test_warning_thresholds_of_the_combined_number():
    """the warning sits at explicit_stability_limit of the tableau for (nu Lambda_u + S) dt, whatever the split between the two
    (the tableaux written out here are checked against the steppers' own in the next test)"""
    from incompressibleeulerhdg_amd.timesteppers import common

    fe = ([[0.0]], [1.0])
    ssp2 = ([[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0]], [1 / 3, 1 / 3, 1 / 3])  # SSP2(3,3,2), explicit part
    g = 1.0 - 1.0 / np.sqrt(2.0)
    dl = -2.0 * np.sqrt(2.0) / 3.0
    ars2 = ([[0, 0, 0], [g, 0, 0], [dl, 1 - dl, 0]], [0.0, 1 - g, g])  # ARS2(2,3,2), explicit part

    def speaks(ab, number):
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            common.warn_if_diffusion_unstable(number, common.explicit_stability_limit(*ab), what="drag")
        said = [str(w.message) for w in rec if issubclass(w.category, RuntimeWarning)]
        assert all(s.startswith("drag:") and "upper bound" in s for s in said)
        return bool(said)

    assert common.explicit_stability_limit(*fe) == pytest.approx(2.0, rel=1e-12)
    for ab in (fe, ssp2, ars2):
        limit = common.explicit_stability_limit(*ab)
        assert np.isfinite(limit) and limit >= 2.0 * (1 - 1e-9)
        assert not speaks(ab, limit * (1 - 1e-6)) and speaks(ab, limit * (1 + 1e-6))
        for viscous in (0.0, 0.4 * limit):  # the two parts add
            assert not speaks(ab, viscous + (limit * (1 - 1e-6) - viscous)) and speaks(ab, viscous + (limit * (1 + 1e-6) - viscous))


def test_the_tableaux_of_the_threshold_test_are_the_steppers():
    from incompressibleeulerhdg_amd import timesteppers as ts
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import common

    seen = {}

    class Probe(_FakeEngine):
        def __init__(self, **kw):
            super().__init__(**kw)
            seen["ab"] = (np.asarray(kw["a_expl"], dtype=float).reshape(-1), np.asarray(kw["b_expl"], dtype=float).reshape(-1))

    import unittest.mock as um

    g = 1.0 - 1.0 / np.sqrt(2.0)
    dl = -2.0 * np.sqrt(2.0) / 3.0
    want = {ts.IncompressibleEulerHDGIMEXSSP2_332: ([0, 0, 0, 0.5, 0, 0, 0.5, 0.5, 0], [1 / 3, 1 / 3, 1 / 3]),
            ts.IncompressibleEulerHDGIMEXARS2_232: ([0, 0, 0, g, 0, 0, dl, 1 - dl, 0], [0.0, 1 - g, g])}
    for cls, (a, b) in want.items():
        with um.patch.object(common, "Engine", Probe):
            cls(UnitSquareMesh(4, 4), 1, 0.01)
        assert np.allclose(seen["ab"][0][:9], a, atol=1e-14) and np.allclose(seen["ab"][1][:3], b, atol=1e-14), cls


def test_step_caps_with_the_drag_rate():
    """rates[2] is nu Lambda_u + S while the drag is on: _step_caps bounds dt by the real-axis limit over it, unchanged"""
    from incompressibleeulerhdg_amd.timesteppers import common

    class Cfg:
        a_expl = [0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 0.5, 0.0] + [0.0] * 16
        b_expl = [1 / 3, 1 / 3, 1 / 3, 0.0, 0.0]

    class Eng:
        cfg, nstages = Cfg, 3

    class St:
        _engine = Eng

    limit = common.explicit_stability_limit(Cfg.a_expl[:9], Cfg.b_expl[:3])
    nuL, S = 7.0, 30.0
    assert common.IncompressibleEuler._step_caps(St, [1.0, 0.0, nuL + S, 0.0]) == [None, limit / (nuL + S), None]
    assert common.IncompressibleEuler._step_caps(St, [1.0, 0.0, S, 0.0]) == [None, limit / S, None]  # drag alone
    assert common.IncompressibleEuler._step_caps(St, [1.0, 0.0, 0.0, 0.0]) == [None, None, None]


# ---- host packing and tables
_EXE = {}


def _host_program(where):
    if "exe" not in _EXE:
        exe = where / "drag_check"
        subprocess.run([shutil.which("g++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-g", "-o", str(exe), os.path.join(HERE, "host", "drag_check.cpp")], check=True)
        _EXE["exe"] = exe
    return _EXE["exe"]


def test_host_packing_permutation_bound_and_validation(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = _host_program(tmp_path.parent)
    r = subprocess.run([str(exe), "pack"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    for nx in (3, 12, 130):
        assert f"nx {nx} ny {nx} " in r.stdout
    assert r.stdout.count("nx 8 ny 4 ") == 2  # the two strips of a two-rank run


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_host_tables_form_the_reference_block(tmp_path, k):
    """sigma_0 I + (sigma_1 - sigma_0) L_1 + (sigma_2 - sigma_0) L_2 as the kernels form it, mapped to the nodal basis, against
    the reference block entry by entry at 1e-11 max|entry| (section 21's bound)"""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = _host_program(tmp_path.parent)
    out = tmp_path / "block.bin"
    worst = 0.0
    for s in ((0.3, 1.7, 0.9), (2.0, 0.0, 0.0), (0.0, 0.0, 3.5), (1.25, 1.25, 1.25), (0.0, 4.0, 1.0)):
        r = subprocess.run([str(exe), "block", str(k)] + [repr(x) for x in s] + [str(out)], capture_output=True, text=True)
        assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
        raw = np.fromfile(out)
        n = int(raw[0])
        got = raw[1:].reshape(n, n)
        want = ref.blocks(np.array([s]), k)[0]
        assert got.shape == want.shape
        dev = np.max(np.abs(got - want)) / np.max(np.abs(want))
        worst = max(worst, dev)
        assert dev <= 1e-11, (s, dev)
    print(f"k={k}: largest deviation {worst:.3e} max|entry|")


# ---- C-ABI and Python surface
SIGNATURES_IN_C = {
    "hdg_set_drag": "int hdg_set_drag(hdg_handle* h, const double* sigma, const double* target, const int* region);",
    "hdg_get_drag": "int hdg_get_drag(hdg_handle* h, double* sigma, double out2[2]);",
    "hdg_apply_drag": "int hdg_apply_drag(hdg_handle* h, const double* sigma, const double* target, const double* Q, double* out);",
    "hdg_get_drag_force": "int hdg_get_drag_force(hdg_handle* h, double F[12]);",
    "hdg_apply_drag_force": "int hdg_apply_drag_force(hdg_handle* h, const double* sigma, const double* target, const int* region, const double* Q, double F[12]);",
}


def test_c_abi_declares_the_entry_points_in_their_own_header():
    import ctypes as C
    import inspect

    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd import timesteppers as ts

    assert set(_lib.DRAG_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_drag.h")).read()
    others = "".join(open(os.path.join(ROOT, "include", f)).read() for f in sorted(os.listdir(os.path.join(ROOT, "include")))
                     if f != "hdg_drag.h")
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header and name not in others and name not in _lib.SIGNATURES, name
        assert re.search(rf"^int {name}\(", engine, re.M), name
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    assert "#define HDG_DRAG_REGIONS 4" in header and _lib.HDG_DRAG_REGIONS == 4
    h, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
    assert _lib.DRAG_SIGNATURES["hdg_set_drag"] == [h, dp, dp, ip]
    assert _lib.DRAG_SIGNATURES["hdg_get_drag"] == [h, dp, dp]
    assert _lib.DRAG_SIGNATURES["hdg_apply_drag"] == [h, dp, dp, dp, dp]
    assert _lib.DRAG_SIGNATURES["hdg_get_drag_force"] == [h, dp]
    assert _lib.DRAG_SIGNATURES["hdg_apply_drag_force"] == [h, dp, dp, ip, dp, dp]
    assert _lib.DRAG_HEADER.endswith(os.path.join("include", "hdg_drag.h")) and os.path.isfile(_lib.DRAG_HEADER)
    for name in ("set_drag", "drag", "drag_number", "apply_drag", "drag_force", "drag_force_of", "cell_vertices"):
        assert callable(getattr(_lib.Engine, name))
    for name, last in (("set_drag", "region"), ("apply_drag", "target"), ("drag_force_of", "region")):
        pars = inspect.signature(getattr(_lib.Engine, name)).parameters
        assert list(pars)[-1] == last and pars[last].default is None and pars["target"].default is None
    assert len(_lib.Engine.LAUNCH_CLASSES) == 13 and len(_lib.STEP_RATES) == 4
    assert "drag" not in {f[0] for f in _lib.hdg_config._fields_} and _lib.hdg_config._fields_[-1][0] == "n_tracers"
    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        assert any(p.kind is inspect.Parameter.VAR_KEYWORD for p in inspect.signature(cls.__init__).parameters.values()), cls
    # the kernels live in a file of their own, the host packing in a plain header without HIP, and the engine includes both
    assert '#include "hdg_drag.hpp"' in engine and '#include "hdg_drag_host.hpp"' in engine
    kernels = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_drag.hpp")).read()
    for name in ("k_drag", "k_g_drag", "k_drag_force", "k_g_drag_force", "k_drag_force_finish", "drag_cell"):
        assert name in kernels
    assert "atomicAdd" not in kernels and "atomic_" not in kernels  # fixed-order sums only
    host = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_drag_host.hpp")).read()
    assert "#include <hip" not in host and "__global__" not in host and "__device__" not in host


class _FakeEngine:
    """stands in for _lib.Engine: records what a stepper's constructor asks of it"""
    calls = []

    def __init__(self, **kw):
        self.kw = kw
        self.n_edges, self.n_l = 1, 1
        self.nstages = int(kw["nstages"])

        class Cfg:
            a_expl = list(np.asarray(kw["a_expl"], dtype=float).reshape(-1))
            b_expl = list(np.asarray(kw["b_expl"], dtype=float).reshape(-1))

        self.cfg = Cfg
        self.nu = 0.0
        type(self).calls.append(("create", None))

    def node_coordinates(self):
        return np.zeros((1, 2)), np.zeros((1, 2))

    def set_viscosity(self, nu, wall):
        self.nu = nu

    def viscosity(self):
        return self.nu, "free_slip"

    def viscosity_number(self):
        return 100.0, self.nu * 100.0 * self.kw["dt"]

    def set_drag(self, sigma, target=None, region=None):
        type(self).calls.append(("set_drag", (sigma, target, region)))
        self.S = float(sigma)

    def drag_number(self):
        return self.S, self.S * self.kw["dt"]


@pytest.mark.parametrize("family", ["ssp2", "implicit", "dg"])
def test_drag_keywords_on_the_three_stepper_families(monkeypatch, family):
    from incompressibleeulerhdg_amd import timesteppers as ts
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers import common

    cls = {"ssp2": ts.IncompressibleEulerHDGIMEXSSP2_332, "implicit": ts.IncompressibleEulerHDGImplicit, "dg": ts.IncompressibleEulerDGImplicit}[family]
    monkeypatch.setattr(common, "Engine", _FakeEngine)
    dt = 0.01
    _FakeEngine.calls = []
    cls(UnitSquareMesh(4, 4), 1, dt)  # None: no call at all
    assert [c for c, _ in _FakeEngine.calls] == ["create"]
    _FakeEngine.calls = []
    tgt, reg = (lambda x, y: (1.0 + 0 * x, 0 * y)), (lambda x, y: 0 * x)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # S dt = 0.3: below every tableau's limit
        st = cls(UnitSquareMesh(4, 4), 1, dt, drag=30.0, drag_target=tgt, drag_region=reg)
    assert ("set_drag", (30.0, tgt, reg)) in _FakeEngine.calls
    limit = st.drag_limit
    assert limit == common.explicit_stability_limit(st._engine.cfg.a_expl[:st._engine.nstages ** 2], st._engine.cfg.b_expl[:st._engine.nstages])
    with pytest.warns(RuntimeWarning, match="drag: the diffusion number"):
        cls(UnitSquareMesh(4, 4), 1, dt, drag=1.001 * limit / dt)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cls(UnitSquareMesh(4, 4), 1, dt, drag=0.999 * limit / dt)
        cls(UnitSquareMesh(4, 4), 1, dt, viscosity=0.4 * limit, drag=0.599 * limit / dt)  # nu Lambda_u dt = 0.4 limit: the two add
    with pytest.warns(RuntimeWarning, match="drag: the diffusion number"):
        cls(UnitSquareMesh(4, 4), 1, dt, viscosity=0.4 * limit, drag=0.601 * limit / dt)
    with pytest.raises(ValueError, match="need drag="):
        cls(UnitSquareMesh(4, 4), 1, dt, drag_target=tgt)


def test_engine_evaluates_callables_at_vertices_nodes_and_centroids():
    """the conversions of Engine.set_drag on an object that has the geometry but no device"""
    from incompressibleeulerhdg_amd import _lib
    from incompressibleeulerhdg_amd.output import _cell_vertices
    from oracle import hdg_oracle as orc

    d = orc.HDGDiscretisation(3, 1)

    class Stub:
        n_cells, n_u, shape_Q, general, rank = d.mesh.ncells, d.nu, (d.NQ // 2, 2), False, 0

        class cfg:
            nx, ny, periodic, length = 3, 3, 0, 1.0

        def node_coordinates(self):
            return d.node_coords(d.PU).reshape(-1, 2), None

        cell_vertices = _lib.Engine.cell_vertices
        _drag_sigma, _drag_target, _drag_region = _lib.Engine._drag_sigma, _lib.Engine._drag_target, _lib.Engine._drag_region

    e = Stub()
    V = e.cell_vertices()
    assert np.max(np.abs(V - _cell_vertices(3, 3))) < 1e-14 and np.max(np.abs(V - d.mesh.cell_vertices)) < 1e-14
    assert np.array_equal(e._drag_sigma(2.5), np.full((18, 3), 2.5))
    assert np.allclose(e._drag_sigma(lambda x, y: 1.0 + x + 2.0 * y), 1.0 + V[..., 0] + 2.0 * V[..., 1], atol=1e-14)
    assert np.array_equal(e._drag_sigma(lambda x, y: 3.0), np.full((18, 3), 3.0))
    X = e.node_coordinates()[0]
    assert np.array_equal(e._drag_target(lambda x, y: (1.0, y)), np.stack([np.ones(len(X)), X[:, 1]], axis=-1))
    assert e._drag_target(None) is None and e._drag_region(None) is None
    reg = e._drag_region(lambda x, y: (x > 0.5).astype(int) + 2 * (y > 0.5))
    ctr = V.mean(axis=1)
    assert reg.dtype == np.int32 and np.array_equal(reg, (ctr[:, 0] > 0.5) + 2 * (ctr[:, 1] > 0.5))
    with pytest.raises(ValueError):
        e._drag_sigma(np.zeros((17, 3)))
    with pytest.raises(ValueError):
        e._drag_region(np.zeros(17))


# ---- model problems
def test_dragged_taylor_green():
    import inspect

    from incompressibleeulerhdg_amd import model_problems as mp
    from incompressibleeulerhdg_amd.mesh import FunctionSpace, UnitSquareMesh
    from oracle import hdg_oracle as orc

    assert "DraggedTaylorGreen" in mp.__all__ and issubclass(mp.DraggedTaylorGreen, mp.TaylorGreen)
    assert list(inspect.signature(mp.TaylorGreen.__init__).parameters)[-1] == "viscosity"
    assert list(inspect.signature(mp.DraggedTaylorGreen.__init__).parameters)[-1] == "drag"
    d = orc.HDGDiscretisation(3, 1)
    mesh = UnitSquareMesh(3, 3)
    V_Q = FunctionSpace(mesh, "DG", 2, d.node_coords(d.PU).reshape(-1, 2), value_size=2)
    V_p = FunctionSpace(mesh, "DG", 1, d.node_coords(d.PP).reshape(-1, 2))
    for forcing in ("exponential", "constant"):  # None is TaylorGreen itself, with either forcing
        for nu in (0.0, 0.01):
            old = mp.TaylorGreen(V_Q, V_p, forcing=forcing, kappa=0.5, viscosity=nu)
            new = mp.DraggedTaylorGreen(V_Q, V_p, forcing=forcing, kappa=0.5, viscosity=nu)
            for t in (0.0, 0.3):
                assert np.array_equal(old.f_rhs()(t), new.f_rhs()(t))
    with pytest.raises(ValueError, match="not separable"):
        mp.DraggedTaylorGreen(V_Q, V_p, forcing="constant", drag=1.0)
    sigma = lambda x, y: 2.0 * (0.2 + 0.5 * x + 0.3 * y)
    drg = mp.DraggedTaylorGreen(V_Q, V_p, kappa=0.5, drag=sigma)
    want = ref.DraggedTaylorGreen(d, sigma, 0.5)
    f = drg.f_rhs()
    for t in (0.0, 0.3):
        assert f.scale(t) == np.exp(-0.5 * t)
        assert np.allclose(f(t), want.f_rhs(t), rtol=0, atol=1e-14)
        for a, b in zip(drg.solution(t), mp.TaylorGreen(V_Q, V_p, kappa=0.5).solution(t)):
            assert np.array_equal(a.dat.data, b.dat.data)  # the solution is unchanged
    X = d.node_coords(d.PU).reshape(-1, 2)
    qx, qy = ref.taylor_green_Qs(X[:, 0], X[:, 1])
    c = -0.5 + sigma(X[:, 0], X[:, 1])
    assert np.allclose(f.profile, np.stack([c * qx, c * qy], axis=-1), rtol=0, atol=1e-14)
    uni = mp.DraggedTaylorGreen(V_Q, V_p, kappa=0.5, viscosity=0.01, drag=2.0)  # a scalar is uniform friction
    assert np.allclose(uni.f_rhs().profile, (-0.5 + 2 * np.pi ** 2 * 0.01 + 2.0) * np.stack([qx, qy], axis=-1), rtol=0, atol=1e-14)


def test_cylinder_wake():
    from incompressibleeulerhdg_amd import model_problems as mp

    L, nx, S, U = 2 * np.pi, 16, 40.0, 1.5
    w = mp.CylinderWake(None, None, L, L / nx, S, stream=U)
    assert "CylinderWake" in mp.__all__ and w.radius == L / 16 and w.centre == (L / 4, L / 2)
    x, y = np.meshgrid(np.linspace(0, L, 129), np.linspace(0, L, 129))
    s = w.sigma(x, y)
    assert s.min() == 0.0 and s.max() <= S * (1 + 1e-12) and s.max() >= 0.99 * S
    # the centre of the disc: the tanh edge is one cell wide and at nx = 16 the radius is one cell
    assert w.sigma(np.array([L / 4]), np.array([L / 2]))[0] == pytest.approx(0.5 * S * (1 + np.tanh(2.0)), rel=1e-12)
    assert w.sigma(np.array([L / 4 + L / 16]), np.array([L / 2]))[0] == pytest.approx(0.5 * S, rel=1e-12)  # its rim: the tanh edge
    far = (np.hypot(x - L / 4, y - L / 2) > L / 16 + 6 * L / nx) & (x < 0.875 * L)
    assert np.all(s[far] == 0.0)  # exactly zero away from the body and the fringe
    assert w.sigma(np.array([0.9375 * L]), np.array([0.1]))[0] == pytest.approx(S, rel=1e-12)  # the crest of the sin^2 fringe
    assert w.sigma(np.array([L]), np.array([0.1]))[0] == pytest.approx(0.0, abs=1e-25 * S)
    ux, uy = w.target(x, y)
    assert np.all(ux[x >= 0.875 * L] == U) and np.all(ux[x < 0.87 * L] == 0.0) and not np.any(uy)
    r = w.region(x, y)
    assert set(np.unique(r)) == {0, 1, 2} and np.all(r[x > 0.88 * L] == 2) and r[64, 32] == 1
    assert np.all(r[(s == 0.0)] == 0) or np.all(r[(s == 0.0) & (x < 0.875 * L)] == 0)
    qx, qy = w.initial_condition()[0](x, y)
    assert np.all(qx == U) and not np.any(qy) and w.f_rhs() is None and w.solution(1.0) is None
    cd, cl = w.coefficients(np.array([-3.0, 0.5, -1.0]))
    q = 0.5 * U ** 2 * 2 * (L / 16)
    assert cd == pytest.approx(3.0 / q) and cl == pytest.approx(-0.5 / q)  # the body feels the negative of the force on the fluid


# ---- driver
def test_driver_refuses_bad_drag_before_any_engine(monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.drag is None and args.obstacle_drag is None and args.stream is None
    driver.check_drag(args)
    driver.check_drag(driver.build_parser().parse_args(["--drag", "2"]))
    driver.check_drag(driver.build_parser().parse_args(["--drag", "2", "--problem", "shear", "--gpus", "2"]))
    driver.check_drag(driver.build_parser().parse_args(["--problem", "cylinder", "--viscosity", "1e-2", "--obstacle_drag", "50", "--stream", "2"]))

    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    for bad in (["--drag", "nan"], ["--drag", "inf"], ["--drag=-1"]):
        with pytest.raises(RuntimeError, match="--drag .* is not a finite number >= 0"):
            driver.main(bad)
    with pytest.raises(RuntimeError, match="needs --forcing exponential"):
        driver.main(["--drag", "1", "--problem", "taylorgreen", "--forcing", "constant"])
    with pytest.raises(RuntimeError, match="covers one of the two"):
        driver.main(["--drag", "1", "--coriolis", "2"])
    with pytest.raises(RuntimeError, match="--problem cylinder needs --viscosity"):
        driver.main(["--problem", "cylinder"])
    for name in ("--obstacle_drag", "--stream"):
        with pytest.raises(RuntimeError, match=f"{name} needs --problem cylinder"):
            driver.main([name, "3"])
    with pytest.raises(RuntimeError, match="--obstacle_drag .* is not a finite number > 0"):
        driver.main(["--problem", "cylinder", "--viscosity", "1e-2", "--obstacle_drag", "0"])
    with pytest.raises(RuntimeError, match="--stream .* is not a finite number != 0"):
        driver.main(["--problem", "cylinder", "--viscosity", "1e-2", "--stream", "nan"])
    with pytest.raises(RuntimeError, match="has no walls"):
        driver.main(["--problem", "cylinder", "--viscosity", "1e-2", "--wall", "no_slip"])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(["--drag", "2", "--gpus", "2"])
    with pytest.raises(AssertionError, match="too late"):
        driver.main(["--problem", "cylinder", "--viscosity", "1e-2", "--nx", "16"])


def test_cylinder_default_puts_the_combined_number_at_half_the_limit():
    """the engine-side part of the wake's set-up: S from Lambda_u, and the refusal when viscosity alone is above half the limit"""
    from incompressibleeulerhdg_amd import driver
    from incompressibleeulerhdg_amd.timesteppers import common

    class Cfg:
        a_expl = [0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.5, 0.5, 0.0] + [0.0] * 16
        b_expl = [1 / 3, 1 / 3, 1 / 3, 0.0, 0.0]

    limit = common.explicit_stability_limit(Cfg.a_expl[:9], Cfg.b_expl[:3])

    class Eng:
        cfg, nstages = Cfg, 3
        number = 0.2 * limit

        def viscosity_number(self):
            return self.number / (0.02 * 1e-2), self.number

    class St:
        _engine, _V_Q, _V_p = Eng(), None, None

    args = driver.build_parser().parse_args(["--problem", "cylinder", "--viscosity", "1e-2", "--nx", "16", "--dt", "0.02"])
    w = driver.cylinder_drag(args, St)
    assert w.S == pytest.approx(0.3 * limit / 0.02, rel=1e-12) and w.U == 1.0 and w.h == pytest.approx(2 * np.pi / 16)
    args.obstacle_drag, args.stream = 7.0, 2.0
    w = driver.cylinder_drag(args, St)
    assert w.S == 7.0 and w.U == 2.0
    St._engine.number = 0.51 * limit
    with pytest.raises(RuntimeError, match="alone is above half the stability limit"):
        driver.cylinder_drag(args, St)
