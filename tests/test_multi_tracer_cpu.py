"""Several passive tracers (hdg_config::n_tracers, --tracers, solve(q_initial=[...])): what can be checked without a GPU --
the config field in the header and in the ctypes struct, the driver's flag and its refusals, the stepper's stacking of a
list of initial fields."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_n_tracers_is_the_last_config_field():
    from incompressibleeulerhdg_amd import _lib

    header = open(os.path.join(ROOT, "include", "hdg_mi355x.h")).read()
    body = re.search(r"typedef struct hdg_config \{(.*?)\} hdg_config;", header, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    members = [m.strip() for m in body.split(";") if m.strip()]
    assert members[-1] == "int n_tracers"
    assert _lib.hdg_config._fields_[-1][0] == "n_tracers"
    assert _lib.hdg_config._fields_[-1][1] is _lib.C.c_int
    assert re.search(r"#define HDG_MAX_TRACERS 16\b", header) and _lib.HDG_MAX_TRACERS == 16
    assert _lib.hdg_config().n_tracers == 0  # a zeroed struct: one tracer


def test_tracers_flag_defaults_to_one():
    from incompressibleeulerhdg_amd.driver import build_parser

    assert build_parser().parse_args([]).tracers == 1
    assert build_parser().parse_args(["--tracers", "5"]).tracers == 5


@pytest.mark.parametrize("argv,what", [(["--tracers", "0", "--tracer_advection"], "1 .. 16"), (["--tracers", "17", "--tracer_advection"], "1 .. 16"),
                                       (["--tracers", "-3"], "1 .. 16"), (["--tracers", "2"], "--tracer_advection")])
def test_main_refuses_before_any_engine_is_built(monkeypatch, argv, what):
    from incompressibleeulerhdg_amd import _lib, driver

    def never(*a, **kw):
        raise AssertionError("an engine (or the ranks of one) was started")

    monkeypatch.setattr(_lib, "load_library", never)
    monkeypatch.setattr(_lib.Engine, "__init__", never)
    monkeypatch.setattr(driver, "_Ranks", never)
    monkeypatch.setattr(driver, "launch_ranks", never)
    with pytest.raises(RuntimeError, match=re.escape(what)):
        driver.main(argv)


def test_initial_fields_of_the_driver():
    from incompressibleeulerhdg_amd.driver import tracer_initial

    x, y = np.random.default_rng(0).random((2, 50))
    assert np.array_equal(tracer_initial(0)(x, y), np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y))  # driver.py:342
    assert np.allclose(tracer_initial(2)(x, y), np.sin(6 * np.pi * x) * np.sin(6 * np.pi * y), rtol=0, atol=1e-14)


class _FakeEngine:
    def __init__(self, n_tracers, n):
        self.n_tracers, self.n, self.block = n_tracers, n, None

    def set_tracer(self, q):
        self.block = None if q is None else np.array(q, dtype=float)

    def get_tracer(self):
        return self.block.copy()


def _stepper(n_tracers, n=12):
    from incompressibleeulerhdg_amd.mesh import UnitSquareMesh
    from incompressibleeulerhdg_amd.timesteppers.common import IncompressibleEuler

    class Bare(IncompressibleEuler):
        def solve(self, *a, **kw):
            raise NotImplementedError

    ts = Bare(UnitSquareMesh(2, 2), 1, 0.1)
    ts._engine = _FakeEngine(n_tracers, n)
    ts._V_q = ts._V_p = None  # arrays only: nothing is interpolated
    return ts


def test_a_list_of_initial_fields_is_stacked_tracer_major():
    from incompressibleeulerhdg_amd.mesh import Function

    ts = _stepper(3)
    a, b, c = (np.arange(12.0) + 100 * m for m in range(3))
    assert ts._init_tracer([a, Function(None, b, "b"), tuple(c)]) is True
    assert ts._engine.block.shape == (3, 12) and np.array_equal(ts._engine.block, np.stack([a, b, c]))
    assert [f.name() for f in ts.q_tracers] == ["tracer_0", "tracer_1", "tracer_2"]
    assert ts.q_tracer is ts.q_tracers[0] and np.array_equal(ts.q_tracers[2].dat.data, c)
    assert ts._tracer_function() is ts.q_tracers and len(ts.q_tracers) == 3  # what the callbacks are given
    # one tracer: the single field, the single Function, the old name
    one = _stepper(1)
    assert one._init_tracer(a) is True
    assert one._engine.block.shape == (12,) and [f.name() for f in one.q_tracers] == ["tracer"]
    assert one._tracer_function() is one.q_tracer
    assert one._init_tracer(None) is False and one.q_tracer is None and one.q_tracers == [] and one._engine.block is None


@pytest.mark.parametrize("bad", [[np.zeros(12)] * 2, [np.zeros(12)] * 4, np.zeros(12), np.zeros((3, 12))])
def test_a_list_of_the_wrong_length_is_refused_before_the_engine_sees_it(bad):
    ts = _stepper(3)
    ts._engine.block = "untouched"
    with pytest.raises(ValueError, match="3 tracer fields"):
        ts._init_tracer(bad)
    assert ts._engine.block == "untouched"


def test_the_animation_callback_writes_every_member():
    from incompressibleeulerhdg_amd.auxilliary.callbacks import AnimationCallback

    written = []
    cb = AnimationCallback.__new__(AnimationCallback)
    cb.vorticity = lambda Q: "vorticity"
    cb.outfile = type("F", (), {"write": lambda self, *fields, time: written.append(fields)})()
    cb("Q", "p", 0.0, q_tracer=["tracer_0", "tracer_1"])
    cb("Q", "p", 0.1, q_tracer="tracer")
    cb("Q", "p", 0.2)
    assert written == [("Q", "p", "vorticity", "tracer_0", "tracer_1"), ("Q", "p", "vorticity", "tracer"), ("Q", "p", "vorticity")]
