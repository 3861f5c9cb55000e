"""ctypes binding of libhdg_mi355x.so (C-ABI declared in include/hdg_mi355x.h).

The product has no CPU fallback: if the HIP library is missing or a call fails, an exception is
raised.  Nothing here imports ``oracle``.
"""

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# HDG_LIB_PATH: load an alternative build of the SAME library (kernel experiments with -D switches, tools/)
LIB_PATH = os.environ.get("HDG_LIB_PATH") or os.path.join(_HERE, "libhdg_mi355x.so")
SRC = os.path.join(_HERE, "csrc", "hdg_engine.hip")
HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_mi355x.h"))
CHECKPOINT_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_checkpoint.h"))
TRANSFER_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_transfer.h"))
TRACER_DIFFUSION_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_tracer_diffusion.h"))
BUOYANCY_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_buoyancy.h"))
VISCOSITY_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_viscosity.h"))
CORIOLIS_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_coriolis.h"))
TRACER_WALL_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_tracer_walls.h"))
MOVING_WALL_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_moving_walls.h"))
ADAPTIVE_DT_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_adaptive_dt.h"))
DRAG_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_drag.h"))
STREAMFUNCTION_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_streamfunction.h"))
TRACER_IMPLICIT_HEADER = os.path.normpath(os.path.join(_HERE, "..", "include", "hdg_tracer_implicit.h"))

HDG_MAX_STAGES = 5
HDG_MAX_TRACERS = 16
HDG_KEY_FINAL_STAGE = 0
HDG_KEY_PRESSURE_RECONSTRUCTION = -1
HDG_STATE_CURRENT = 0
HDG_STATE_UPDATE = -1
HDG_STATE_RECON = -2

ERRORS = {-1: "HDG_ERR_ARG", -2: "HDG_ERR_HIP", -3: "HDG_ERR_NOT_CONVERGED", -4: "HDG_ERR_SINGULAR", -5: "HDG_ERR_UNSUPPORTED",
          -6: "HDG_ERR_COMM"}
HDG_COMM_RCCL = 1
HDG_COMM_SHM = 2


# columns of hdg_compute_diagnostics / hdg_get_diagnostics
DIAGNOSTICS = ("energy", "enstrophy", "div_l2", "jump_l2", "p_integral", "tracer_integral", "tracer_half_sq", "max_speed", "cfl")


# columns of hdg_evaluate_points / hdg_get_probes
POINT_COLUMNS = ("ux", "uy", "p", "q", "omega")


class HDGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"{ERRORS.get(code, code)}: {msg}")
        self.code = code


class hdg_config(C.Structure):
    _fields_ = [
        ("nx", C.c_int),
        ("ny", C.c_int),
        ("degree", C.c_int),
        ("dt", C.c_double),
        ("flux_upwind", C.c_int),
        ("use_projection", C.c_int),
        ("n_richardson", C.c_int),
        ("tau", C.c_double),
        ("alpha_penalty", C.c_double),
        ("nstages", C.c_int),
        ("a_expl", C.c_double * (HDG_MAX_STAGES * HDG_MAX_STAGES)),
        ("a_impl", C.c_double * (HDG_MAX_STAGES * HDG_MAX_STAGES)),
        ("b_expl", C.c_double * HDG_MAX_STAGES),
        ("b_impl", C.c_double * (HDG_MAX_STAGES + 1)),
        ("c_expl", C.c_double * HDG_MAX_STAGES),
        ("equispaced_nodes", C.c_int),
        ("tent_rtol", C.c_double),
        ("tent_maxit", C.c_int),
        ("gmres_restart", C.c_int),
        ("tent_precond", C.c_int),
        ("tent_solver", C.c_int),
        ("trace_rtol", C.c_double),
        ("trace_maxit", C.c_int),
        ("trace_precond", C.c_int),
        ("unsplit_rtol", C.c_double),
        ("unsplit_inner_rtol", C.c_double),
        ("unsplit_restart", C.c_int),
        ("unsplit_maxit", C.c_int),
        ("device", C.c_int),
        ("periodic", C.c_int),
        ("length", C.c_double),
        ("dg_rtol", C.c_double),
        ("dg_restart", C.c_int),
        ("dg_maxit", C.c_int),
        ("n_tracers", C.c_int),  # always the last field (include/hdg_mi355x.h)
    ]


def build_library(force=False, verbose=False):
    """Compile the HIP engine for gfx950 into the package directory (in-tree, travels with gpurun)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [HEADER, CHECKPOINT_HEADER, TRANSFER_HEADER, TRACER_DIFFUSION_HEADER, BUOYANCY_HEADER, VISCOSITY_HEADER, CORIOLIS_HEADER, TRACER_WALL_HEADER, MOVING_WALL_HEADER, ADAPTIVE_DT_HEADER, DRAG_HEADER, STREAMFUNCTION_HEADER, TRACER_IMPLICIT_HEADER] + [os.path.join(csrc, f) for f in sorted(os.listdir(csrc)) if f.endswith((".hpp", ".hip"))]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(s) for s in srcs):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-o", LIB_PATH, SRC,
           "-L/opt/rocm/lib", "-lrccl", "-lrt", "-lpthread"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


_lib = None

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_lp = C.POINTER(C.c_long)
_h = C.c_void_p

# every symbol include/hdg_mi355x.h declares, with its argument types
SIGNATURES = {
    "hdg_create": [C.POINTER(hdg_config), C.POINTER(_h)],
    "hdg_create_distributed": [C.POINTER(hdg_config), C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(_h)],
    "hdg_rccl_unique_id": [C.c_char_p],
    "hdg_create_general": [C.POINTER(hdg_config), C.c_int, _dp, C.c_int, _ip, C.POINTER(_h)],
    "hdg_general_topology": [_h, _ip, _ip],
    "hdg_destroy": [_h],
    "hdg_get_sizes": [_h, _lp, _lp, _ip, _ip, _ip],
    "hdg_set_state": [_h, _dp, _dp],
    "hdg_get_field": [_h, C.c_int, _dp, _dp, _dp],
    "hdg_set_field": [_h, C.c_int, _dp, _dp, _dp],
    "hdg_set_forcing_nodal": [_h, C.c_int, _dp],
    "hdg_set_forcing_profile": [_h, _dp],
    "hdg_set_forcing_scale": [_h, C.c_int, C.c_double],
    "hdg_reconstruct_trace": [_h],
    "hdg_project_bdm": [_h, C.c_int, C.c_int],
    "hdg_project_bdm_nodal": [_h, _dp, _dp],
    "hdg_begin_step": [_h],
    "hdg_tentative_solve": [_h, C.c_int, _ip],
    "hdg_pressure_solve": [_h, C.c_int, _ip],
    "hdg_unsplit_solve": [_h, C.c_int, _ip],
    "hdg_shift_pressure": [_h, C.c_int],
    "hdg_stage_update": [_h, C.c_int],
    "hdg_finish_step": [_h],
    "hdg_step": [_h],
    "hdg_run_separable": [_h, C.c_int, _dp],
    "hdg_implicit_step": [_h, _ip, _ip],
    "hdg_dg_implicit_step": [_h, _ip],
    "hdg_apply_dg_operator": [_h, _dp, _dp, _dp, C.c_double, _dp, _dp],
    "hdg_dg_avg_trace": [_h, _dp, _dp],
    "hdg_get_iteration_stats": [_h, _dp, _lp, C.c_int],
    "hdg_get_solver_events": [_h, _lp, C.c_int],
    "hdg_get_kernel_forms": [_h, _ip],
    "hdg_rccl_selftest": [C.c_int, C.c_int, _dp],
    "hdg_get_timers": [_h, _dp, _dp, _lp, C.c_int],
    "hdg_set_kernel_timing": [_h, C.c_int],
    "hdg_get_launch_stats": [_h, _lp, _dp, C.c_int],
    "hdg_get_comm_info": [_h, _ip, _ip, _ip, C.c_char_p],
    "hdg_set_tracer": [_h, _dp],
    "hdg_get_tracer": [_h, _dp],
    "hdg_tracer_begin_step": [_h],
    "hdg_tracer_stage": [_h, C.c_int],
    "hdg_tracer_finish_step": [_h],
    "hdg_apply_tracer_advection": [_h, _dp, _dp, C.c_int, _dp],
    "hdg_cg_size": [_h, _lp],
    "hdg_cg_coordinates": [_h, _dp],
    "hdg_cg_project_nodal": [_h, _dp, _dp],
    "hdg_vorticity": [_h, _dp, _dp],
    "hdg_cg_to_broken": [_h, _dp, _dp],
    "hdg_node_coordinates": [_h, _dp, _dp],
    "hdg_l2_norms": [_h, _dp, _dp, _dp, _dp],
    "hdg_integrate_pressure": [_h, _dp, _dp],
    "hdg_apply_advection": [_h, _dp, _dp, C.c_double, _dp],
    "hdg_apply_trace_operator": [_h, _dp, _dp],
    "hdg_apply_weak_divergence": [_h, _dp, C.c_int, _dp],
    "hdg_time_kernel": [_h, C.c_int, C.c_int, _dp],
    "hdg_compute_diagnostics": [_h, _dp, _dp, _dp, _dp],
    "hdg_set_diagnostics": [_h, C.c_int],
    "hdg_get_diagnostics": [_h, _dp, C.c_int, _ip, C.c_int],
    "hdg_evaluate_points": [_h, _dp, _dp, _dp, C.c_int, _dp, _dp, _ip],
    "hdg_set_probes": [_h, C.c_int, _dp, C.c_int],
    "hdg_get_probes": [_h, _dp, C.c_int, _ip, C.c_int],
    "hdg_set_particles": [_h, C.c_int, _dp, C.c_int, C.c_int],
    "hdg_get_particles": [_h, _dp, C.c_int, _ip, _lp, C.c_int],
    "hdg_advance_particles": [_h, C.c_double, C.c_int],
}

_ullp = C.POINTER(C.c_ulonglong)
# checkpoint and restart: the symbols include/hdg_checkpoint.h declares, in a table of their own (the table above is exactly
# include/hdg_mi355x.h); load_library walks both
CHECKPOINT_SIGNATURES = {
    "hdg_checkpoint_size": [_h, _lp],
    "hdg_checkpoint_save": [_h, C.c_long, C.c_double, C.c_void_p, C.c_long],
    "hdg_checkpoint_load": [_h, C.c_void_p, C.c_long, _lp, _dp],
    "hdg_state_digest": [_h, _ullp],
    "hdg_digest_vector": [_h, _dp, C.c_long, _ullp],
}

# transfer between engines: the symbols include/hdg_transfer.h declares, in a table of their own like the checkpoint's
TRANSFER_SIGNATURES = {
    "hdg_transfer_state": [_h, _h, C.c_int],
    "hdg_transfer_difference": [_h, _h, _dp, _dp, _dp],
}

# tracer diffusion: the symbols include/hdg_tracer_diffusion.h declares, in a table of their own like the two above
TRACER_DIFFUSION_SIGNATURES = {
    "hdg_set_tracer_diffusivity": [_h, C.c_int, _dp],
    "hdg_get_tracer_diffusion_number": [_h, _dp],
    "hdg_apply_tracer_diffusion": [_h, _dp, _dp],
}

# Boussinesq buoyancy: the symbols include/hdg_buoyancy.h declares, in a table of their own like the three above
BUOYANCY_SIGNATURES = {
    "hdg_set_buoyancy": [_h, C.c_int, _dp, _dp],
    "hdg_get_buoyancy": [_h, C.c_int, _dp, _dp],
    "hdg_apply_buoyancy": [_h, _dp, _dp],
}

# viscous term: the symbols include/hdg_viscosity.h declares, in a table of their own like the four above
VISCOSITY_SIGNATURES = {
    "hdg_set_viscosity": [_h, C.c_double, C.c_int],
    "hdg_get_viscosity": [_h, _dp, C.POINTER(C.c_int), _dp],
    "hdg_apply_viscosity": [_h, C.c_int, _dp, _dp],
}
WALL_MODES = {"free_slip": 0, "no_slip": 1}

# Coriolis term: the symbols include/hdg_coriolis.h declares, in a table of their own like the five above
CORIOLIS_SIGNATURES = {
    "hdg_set_coriolis": [_h, C.c_double, C.c_double],
    "hdg_get_coriolis": [_h, _dp, _dp, _dp],
    "hdg_apply_coriolis": [_h, C.c_double, C.c_double, _dp, _dp],
}

# tracer wall conditions: the symbols include/hdg_tracer_walls.h declares, in a table of their own like the six above
TRACER_WALL_SIGNATURES = {
    "hdg_set_tracer_walls": [_h, C.c_int, _ip, _dp],
    "hdg_get_tracer_wall_flux": [_h, C.c_int, _dp],
    "hdg_apply_tracer_wall_diffusion": [_h, _ip, _dp, _dp, _dp],
}
WALL_SIDES = ("bottom", "right", "top", "left")  # the sides of the structured unit square, in the order of the C-ABI

# moving no-slip walls and the wall force: the symbols include/hdg_moving_walls.h declares, in a table of their own like the seven above
MOVING_WALL_SIGNATURES = {
    "hdg_set_wall_velocity": [_h, _dp],
    "hdg_get_wall_velocity": [_h, _dp],
    "hdg_get_wall_force": [_h, _dp],
    "hdg_apply_moving_walls": [_h, C.c_int, _dp, _dp, _dp],
    "hdg_apply_wall_force": [_h, C.c_int, _dp, _dp, _dp],
}

# adaptive time step: the symbols include/hdg_adaptive_dt.h declares, in a table of their own like the eight above
class hdg_step_control(C.Structure):
    """The controller's settings; a zeroed field means its default (include/hdg_adaptive_dt.h)"""
    _fields_ = [("cfl", C.c_double), ("dt_min", C.c_double), ("dt_max", C.c_double), ("grow", C.c_double), ("band", C.c_double),
                ("caps", C.c_double * 3)]


ADAPTIVE_DT_SIGNATURES = {
    "hdg_set_dt": [_h, C.c_double],
    "hdg_get_dt": [_h, _dp],
    "hdg_get_step_rates": [_h, _dp],
    "hdg_propose_dt": [_h, C.POINTER(hdg_step_control), C.c_double, C.c_double, _dp],
    "hdg_step_proposal": [C.POINTER(hdg_step_control), C.c_double, C.c_double, C.c_double, C.c_double, _dp],
}
STEP_RATES = ("advection", "tracer_diffusion", "viscosity", "rotation")  # the entries of hdg_get_step_rates

# linear drag and volume penalisation: the symbols include/hdg_drag.h declares, in a table of their own like the nine above
DRAG_SIGNATURES = {
    "hdg_set_drag": [_h, _dp, _dp, _ip],
    "hdg_get_drag": [_h, _dp, _dp],
    "hdg_apply_drag": [_h, _dp, _dp, _dp, _dp],
    "hdg_get_drag_force": [_h, _dp],
    "hdg_apply_drag_force": [_h, _dp, _dp, _ip, _dp, _dp],
}
HDG_DRAG_REGIONS = 4

# stream function of the velocity: the symbols include/hdg_streamfunction.h declares, in a table of their own like the ten above
STREAMFUNCTION_SIGNATURES = {
    "hdg_streamfunction": [_h, _dp, C.c_double, _dp, _dp],
    "hdg_apply_cg_stiffness": [_h, _dp, _dp],
    "hdg_psi_transfer": [_h, C.c_int, _dp, _dp],
    "hdg_apply_psi_preconditioner": [_h, C.c_int, _dp, _dp],
    "hdg_psi_vertex_count": [_h, _lp],
}
# implicit tracer diffusion: the symbols include/hdg_tracer_implicit.h declares, in a table of their own like the eleven above
TRACER_IMPLICIT_SIGNATURES = {
    "hdg_set_tracer_diffusion_mode": [_h, C.c_int, C.c_double, C.c_int],
    "hdg_get_tracer_diffusion_solve": [_h, C.c_int, _ip, _dp],
    "hdg_solve_tracer_diffusion": [_h, C.c_int, _dp, _dp, _dp, _ip],
}
TRACER_DIFFUSION_MODES = {"explicit": 0, "implicit": 1}
STREAMFUNCTION_INFO = ("iterations", "residual", "defect", "u_l2", "mean_flow_x", "mean_flow_y", "psi_min", "psi_max")


def step_control(cfl, dt_min=None, dt_max=None, grow=None, band=None, caps=None):
    """The hdg_step_control of the given settings; None: the default of the rule (a zeroed field)"""
    c = hdg_step_control()
    c.cfl = float(cfl)
    for name, v in (("dt_min", dt_min), ("dt_max", dt_max), ("grow", grow), ("band", band)):
        setattr(c, name, 0.0 if v is None else float(v))
    for i, v in enumerate(caps if caps is not None else ()):
        c.caps[i] = 0.0 if v is None else float(v)
    return c


def step_proposal(control, A, dt, t, t_final):
    """The rule of csrc/hdg_step_control.hpp for the rate A and the held step size dt (no engine, no launch).  Raises HDGError
    HDG_ERR_NOT_CONVERGED when A is not finite, HDG_ERR_ARG when the proposal falls below dt_min or the control is bad."""
    out = C.c_double()
    rc = load_library().hdg_step_proposal(C.byref(control), float(A), float(dt), float(t), float(t_final), C.byref(out))
    if rc == -3:
        raise HDGError(rc, f"step proposal at t = {t!r}: velocity is not finite (rate {A!r})")
    if rc != 0:
        raise HDGError(rc, f"step proposal at t = {t!r}: the proposal dt = {out.value!r} is below dt_min = {control.dt_min!r}"
                       if out.value == out.value else "step proposal: cfl must be > 0 and no field of the control negative or NaN")
    return out.value


def wall_velocity_array(v):
    """{side: speed} (a missing side stands still) or four values in the order bottom, right, top, left -> (4,) float64"""
    if isinstance(v, dict):
        out = np.zeros(4)
        for side, u in v.items():
            if side not in WALL_SIDES:
                raise ValueError(f"unknown wall side {side!r}; one of {', '.join(WALL_SIDES)}")
            out[WALL_SIDES.index(side)] = float(u)
        return out
    out = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
    if out.shape != (4,):
        raise ValueError(f"wall_velocity must be a dict {{side: speed}} or four values (got {out.size})")
    return out


def wall_code(wall):
    """'free_slip' / 'no_slip' -> the integer of include/hdg_viscosity.h"""
    if wall not in WALL_MODES:
        raise ValueError(f"wall must be one of {sorted(WALL_MODES)} (got {wall!r})")
    return WALL_MODES[wall]


def load_library():
    """Load libhdg_mi355x.so; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: the HIP engine has not been built "
            "(run `python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback."
        )
    lib = C.CDLL(LIB_PATH)
    for name, args in list(SIGNATURES.items()) + list(CHECKPOINT_SIGNATURES.items()) + list(TRANSFER_SIGNATURES.items()) + \
            list(TRACER_DIFFUSION_SIGNATURES.items()) + list(BUOYANCY_SIGNATURES.items()) + list(VISCOSITY_SIGNATURES.items()) + \
            list(CORIOLIS_SIGNATURES.items()) + list(TRACER_WALL_SIGNATURES.items()) + list(MOVING_WALL_SIGNATURES.items()) + \
            list(ADAPTIVE_DT_SIGNATURES.items()) + list(DRAG_SIGNATURES.items()) + list(STREAMFUNCTION_SIGNATURES.items()) + \
            list(TRACER_IMPLICIT_SIGNATURES.items()):
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.hdg_last_error.argtypes = [_h]
    lib.hdg_last_error.restype = C.c_char_p
    _lib = lib
    return lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _arr(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != tuple(shape):
        raise ValueError(f"expected array of shape {shape}, got {a.shape}")
    return a


class Engine:
    """Thin object wrapper around one hdg_handle."""

    def __init__(self, **kw):
        self.lib = load_library()
        cfg = hdg_config()
        s = int(kw["nstages"])
        cfg.nx = int(kw.get("nx", 1))
        cfg.ny = int(kw.get("ny", kw.get("nx", 1)))
        cfg.degree = int(kw["degree"])
        cfg.dt = float(kw["dt"])
        cfg.flux_upwind = 1 if kw.get("flux", "upwind") == "upwind" else 0
        cfg.use_projection = 1 if kw.get("use_projection_method", True) else 0
        cfg.n_richardson = int(kw.get("n_richardson", 2))
        cfg.tau = float(kw.get("tau", 1.0))
        cfg.alpha_penalty = float(kw.get("alpha_penalty", 1.0))
        cfg.nstages = s
        for name in ("a_expl", "a_impl"):
            m = np.zeros(s * s)
            if name in kw:
                m[:] = np.asarray(kw[name], dtype=float).reshape(-1)[: s * s]
            for i in range(s * s):
                getattr(cfg, name)[i] = m[i]
        for name, n in (("b_expl", s), ("b_impl", s), ("c_expl", s)):
            if name in kw:
                v = np.asarray(kw[name], dtype=float).reshape(-1)
                for i in range(min(len(v), n if name != "b_impl" else HDG_MAX_STAGES + 1)):
                    getattr(cfg, name)[i] = v[i]
        cfg.equispaced_nodes = 1 if kw.get("node_variant", "gll") == "equispaced" else 0
        cfg.tent_rtol = float(kw.get("tent_rtol", 1e-10))
        cfg.tent_maxit = int(kw.get("tent_maxit", 2000))
        cfg.gmres_restart = int(kw.get("gmres_restart", 8))
        # hybrid two-level preconditioner Pi + Dinv (I - Pi): one lift kernel per application
        cfg.tent_precond = int(kw.get("tent_precond", 2))
        # hybrid preconditioner: Chebyshev on a thin ellipse for the bulk of the spectrum, hand-over of the tail to GMRES
        # (k >= 2) beats pure GMRES(8) at every degree (512^2, MDOF-updates/s: k=3 252 -> 288,
        # k=4 184 -> 218) and the fat-ellipse iteration at k = 2 (C3 136.5 -> 118.8 ms/step); the other preconditioners
        # keep their round-1 choice
        _cheb_default = 1 if (cfg.tent_precond == 2 or int(kw["degree"]) <= 3) else 0
        cfg.tent_solver = int(kw.get("tent_solver", _cheb_default))
        cfg.trace_rtol = float(kw.get("trace_rtol", 1e-12))
        cfg.trace_maxit = int(kw.get("trace_maxit", 10000))
        cfg.trace_precond = int(kw.get("trace_precond", 1))
        cfg.unsplit_rtol = float(kw.get("unsplit_rtol", 1e-10))
        cfg.unsplit_inner_rtol = float(kw.get("unsplit_inner_rtol", 1e-3))
        cfg.unsplit_restart = int(kw.get("unsplit_restart", 30))
        cfg.unsplit_maxit = int(kw.get("unsplit_maxit", 600))
        cfg.device = int(kw.get("device", 0))
        cfg.periodic = 1 if kw.get("periodic", False) else 0
        cfg.length = float(kw.get("length", 1.0))
        # outer FGMRES of the implicit DG step (same tolerance as the unsplit HDG solves).  The outer iteration count grows
        # like 1 / h: with restarts of 30 the solve stagnates on 64^2 at k = 1, hence the long cycles
        cfg.dg_rtol = float(kw.get("dg_rtol", 1e-10))
        cfg.dg_restart = int(kw.get("dg_restart", 100))
        cfg.dg_maxit = int(kw.get("dg_maxit", 3000))
        # passive tracers carried through the one flow (0 means 1; the library refuses anything outside 0 .. HDG_MAX_TRACERS)
        cfg.n_tracers = int(kw.get("n_tracers", 0))
        self.cfg = cfg
        self.h = _h()
        self.rank, self.nranks = int(kw.get("rank", 0)), int(kw.get("nranks", 1))
        self.general = kw.get("vertices") is not None
        if self.general:
            # general affine triangulation (hdg_create_general): vertices (nv, 2), cells (nc, 3)
            self._vertices = np.ascontiguousarray(kw["vertices"], dtype=np.float64)
            self._cells = np.ascontiguousarray(kw["cells"], dtype=np.int32)
            if self._vertices.ndim != 2 or self._vertices.shape[1] != 2 or self._cells.ndim != 2 or self._cells.shape[1] != 3:
                raise ValueError("general mesh: vertices (nv, 2) and cells (nc, 3) expected")
            rc = self.lib.hdg_create_general(C.byref(cfg), len(self._vertices), _ptr(self._vertices), len(self._cells),
                                             self._cells.ctypes.data_as(_ip), C.byref(self.h))
        elif self.nranks > 1:
            backend = {"rccl": HDG_COMM_RCCL, "shm": HDG_COMM_SHM}[kw.get("comm_backend", "rccl")]
            token = kw["comm_token"]
            token = token if isinstance(token, bytes) else str(token).encode()
            rc = self.lib.hdg_create_distributed(C.byref(cfg), self.rank, self.nranks, backend, token, C.byref(self.h))
        else:
            rc = self.lib.hdg_create(C.byref(cfg), C.byref(self.h))
        if rc != 0:
            raise HDGError(rc, self.lib.hdg_last_error(None).decode())
        nc, ne = C.c_long(), C.c_long()
        nu, np_, nl = C.c_int(), C.c_int(), C.c_int()
        self._ck(self.lib.hdg_get_sizes(self.h, C.byref(nc), C.byref(ne), C.byref(nu), C.byref(np_), C.byref(nl)))
        self.n_cells, self.n_edges = nc.value, ne.value
        self.n_u, self.n_p, self.n_l = nu.value, np_.value, nl.value
        self.nstages = s
        self.shape_Q = (self.n_cells * self.n_u, 2)
        self.shape_p = (self.n_cells * self.n_p,)
        self.shape_l = (self.n_edges * self.n_l,)
        # the tracer block of set_tracer / get_tracer: one field, or (n_tracers, N_p) tracer-major
        self.n_tracers = max(1, cfg.n_tracers)
        self.shape_q = self.shape_p if self.n_tracers == 1 else (self.n_tracers,) + self.shape_p
        # dimension of the GLOBAL mixed state (Q, p, lambda) advanced per step
        nxg, nyg = cfg.nx, cfg.ny
        self.n_total = 2 * nxg * nyg * (2 * self.n_u + self.n_p) + (3 * nxg * nyg + (0 if cfg.periodic else nxg + nyg)) * self.n_l
        if self.general:
            self.n_total = self.n_cells * (2 * self.n_u + self.n_p) + self.n_edges * self.n_l

    def _ck(self, rc):
        if rc != 0:
            raise HDGError(rc, self.lib.hdg_last_error(self.h).decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.hdg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- state
    def set_state(self, Q, p):
        Q, p = _arr(Q, self.shape_Q), _arr(p, self.shape_p)
        self._ck(self.lib.hdg_set_state(self.h, _ptr(Q), _ptr(p)))

    def get_field(self, which, Q=True, p=True, lam=True):
        oQ = np.empty(self.shape_Q) if Q else None
        op = np.empty(self.shape_p) if p else None
        ol = np.empty(self.shape_l) if lam else None
        self._ck(self.lib.hdg_get_field(self.h, which, _ptr(oQ), _ptr(op), _ptr(ol)))
        return oQ, op, ol

    def set_field(self, which, Q=None, p=None, lam=None):
        Q = None if Q is None else _arr(Q, self.shape_Q)
        p = None if p is None else _arr(p, self.shape_p)
        lam = None if lam is None else _arr(lam, self.shape_l)
        self._ck(self.lib.hdg_set_field(self.h, which, _ptr(Q), _ptr(p), _ptr(lam)))

    def set_forcing_nodal(self, slot, f):
        f = _arr(f, self.shape_Q)
        self._ck(self.lib.hdg_set_forcing_nodal(self.h, slot, _ptr(f)))

    def set_forcing_profile(self, profile):
        f = _arr(profile, self.shape_Q)
        self._ck(self.lib.hdg_set_forcing_profile(self.h, _ptr(f)))

    def set_forcing_scale(self, slot, scale):
        self._ck(self.lib.hdg_set_forcing_scale(self.h, slot, float(scale)))

    # --- pieces of the solve loop
    def reconstruct_trace(self):
        self._ck(self.lib.hdg_reconstruct_trace(self.h))

    def project_bdm(self, src_stage, dst):
        self._ck(self.lib.hdg_project_bdm(self.h, src_stage, dst))

    def project_bdm_nodal(self, Q):
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_project_bdm_nodal(self.h, _ptr(Q), _ptr(out)))
        return out

    def begin_step(self):
        self._ck(self.lib.hdg_begin_step(self.h))

    def tentative_solve(self, stage):
        its = C.c_int()
        self._ck(self.lib.hdg_tentative_solve(self.h, stage, C.byref(its)))
        return its.value

    def unsplit_solve(self, stage):
        its = C.c_int()
        self._ck(self.lib.hdg_unsplit_solve(self.h, stage, C.byref(its)))
        return its.value

    def pressure_solve(self, key):
        its = C.c_int()
        self._ck(self.lib.hdg_pressure_solve(self.h, key, C.byref(its)))
        return its.value

    def shift_pressure(self, which):
        self._ck(self.lib.hdg_shift_pressure(self.h, which))

    def stage_update(self, stage):
        self._ck(self.lib.hdg_stage_update(self.h, stage))

    def finish_step(self):
        self._ck(self.lib.hdg_finish_step(self.h))

    def step(self):
        self._ck(self.lib.hdg_step(self.h))

    def run_separable(self, scales):
        scales = _arr(scales)
        assert scales.ndim == 2 and scales.shape[1] == self.nstages + 1
        self._ck(self.lib.hdg_run_separable(self.h, scales.shape[0], _ptr(scales)))

    def implicit_step(self):
        a, b = C.c_int(), C.c_int()
        self._ck(self.lib.hdg_implicit_step(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def dg_implicit_step(self):
        """One step of the implicit DG discretisation (hdg_dg_implicit_step); returns the outer iterations."""
        its = C.c_int()
        self._ck(self.lib.hdg_dg_implicit_step(self.h, C.byref(its)))
        return its.value

    def apply_dg_operator(self, Qstar, u, p, dt):
        """(out_u, out_p) = the DG operator of dg_implicit.py:48-71 applied to (u, p), mapped back through the mass matrices."""
        Qstar, u, p = _arr(Qstar, self.shape_Q), _arr(u, self.shape_Q), _arr(p, self.shape_p)
        ou, op = np.empty(self.shape_Q), np.empty(self.shape_p)
        self._ck(self.lib.hdg_apply_dg_operator(self.h, _ptr(Qstar), _ptr(u), _ptr(p), float(dt), _ptr(ou), _ptr(op)))
        return ou, op

    def dg_avg_trace(self, p):
        """avg(p) in DGT_k (nodal trace layout)."""
        p = _arr(p, self.shape_p)
        lam = np.empty(self.shape_l)
        self._ck(self.lib.hdg_dg_avg_trace(self.h, _ptr(p), _ptr(lam)))
        return lam

    def iteration_stats(self, reset=False):
        sums = np.zeros(4)
        cnt = np.zeros(4, dtype=np.int64)
        self._ck(self.lib.hdg_get_iteration_stats(self.h, _ptr(sums), cnt.ctypes.data_as(_lp), 1 if reset else 0))
        return sums, cnt

    def solver_events(self, reset=False):
        """Residual replacements / rounding-floor exits of the condensed solves since the last reset (dict)."""
        ev = np.zeros(4, dtype=np.int64)
        self._ck(self.lib.hdg_get_solver_events(self.h, ev.ctypes.data_as(_lp), 1 if reset else 0))
        return {"cg_residual_replacements": int(ev[0]), "cg_floor_exits": int(ev[1]), "sstep_cycles": int(ev[2]),
                "sstep_gmres_fallbacks": int(ev[3])}

    def kernel_forms(self):
        """Which form of its kernels the engine launches (hdg_get_kernel_forms): dict of small integers."""
        f = (C.c_int * 4)()
        self._ck(self.lib.hdg_get_kernel_forms(self.h, f))
        return {"lift": f[0], "advection": f[1], "trace_precond": f[2], "schur": f[3]}

    # --- passive tracer, continuous-space diagnostics
    def set_tracer(self, q):
        """q: (N_p,) with one tracer, (n_tracers, N_p) with several (Engine(n_tracers=...)); None switches all of them off."""
        q = None if q is None else _arr(q, self.shape_q)
        self._ck(self.lib.hdg_set_tracer(self.h, _ptr(q)))
        self._tracer_on = q is not None

    def get_tracer(self):
        q = np.empty(self.shape_q)
        self._ck(self.lib.hdg_get_tracer(self.h, _ptr(q)))
        return q

    def tracer_begin_step(self):
        self._ck(self.lib.hdg_tracer_begin_step(self.h))

    def tracer_stage(self, i):
        self._ck(self.lib.hdg_tracer_stage(self.h, int(i)))

    def tracer_finish_step(self):
        self._ck(self.lib.hdg_tracer_finish_step(self.h))

    def apply_tracer_advection(self, q, u, project=True):
        q, u = _arr(q, self.shape_p), _arr(u, self.shape_Q)
        out = np.empty(self.shape_p)
        self._ck(self.lib.hdg_apply_tracer_advection(self.h, _ptr(q), _ptr(u), 1 if project else 0, _ptr(out)))
        return out

    # --- tracer diffusion (include/hdg_tracer_diffusion.h)
    def set_tracer_diffusivity(self, kappa):
        """kappa: one value for every tracer or a sequence of n_tracers values, finite and >= 0; None or zeros: off."""
        if kappa is not None:
            kappa = np.asarray(kappa, dtype=np.float64)
            kappa = np.full(self.n_tracers, float(kappa)) if kappa.ndim == 0 else np.ascontiguousarray(kappa.reshape(-1))
        self._ck(self.lib.hdg_set_tracer_diffusivity(self.h, 0 if kappa is None else len(kappa), _ptr(kappa)))

    def tracer_diffusion_number(self):
        """(Lambda, kappa_max dt Lambda): Lambda is an upper bound of the spectral radius of M^-1 D."""
        out = np.zeros(2)
        self._ck(self.lib.hdg_get_tracer_diffusion_number(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    def apply_tracer_diffusion(self, q):
        """M^-1 D q of one nodal DG_k field, without kappa (test hook)."""
        q = _arr(q, self.shape_p)
        out = np.empty(self.shape_p)
        self._ck(self.lib.hdg_apply_tracer_diffusion(self.h, _ptr(q), _ptr(out)))
        return out

    # --- tracer wall conditions (include/hdg_tracer_walls.h)
    def _wall_arrays(self, walls, rows):
        """walls: a dict {side: value} for every tracer, or a sequence of `rows` such dicts -> (kind, value), each (rows, 4).
        Sides: 'bottom', 'right', 'top', 'left' on the structured unit square, 'boundary' on a general mesh; a missing side
        is no flux."""
        sides = ("boundary",) if self.general else WALL_SIDES
        if isinstance(walls, dict):
            walls = [walls] * rows
        walls = list(walls)
        if len(walls) != rows or not all(isinstance(w, dict) for w in walls):
            raise ValueError(f"walls must be a dict or a sequence of {rows} dicts, one per tracer")
        kind, value = np.zeros((rows, 4), dtype=np.int32), np.zeros((rows, 4))
        for t, w in enumerate(walls):
            for side, v in w.items():
                if side not in sides:
                    raise ValueError(f"tracer {t}: unknown wall side {side!r}; this mesh has {', '.join(sides)}")
                kind[t, sides.index(side)] = 1
                value[t, sides.index(side)] = float(v)
        return kind, value

    def set_tracer_walls(self, walls):
        """Hold tracers at fixed values on wall sides: walls is a dict {side: value} applied to every tracer, or a sequence
        of n_tracers such dicts; a missing side is no flux; None or no fixed side at all: off.  The values act through the
        diffusivity: with kappa = 0 they do nothing."""
        if walls is None:
            self._ck(self.lib.hdg_set_tracer_walls(self.h, 0, None, None))
            self._tracer_walls = None
            return
        kind, value = self._wall_arrays(walls, self.n_tracers)
        self._ck(self.lib.hdg_set_tracer_walls(self.h, self.n_tracers, kind.ctypes.data_as(_ip), _ptr(value)))
        sides = ("boundary",) if self.general else WALL_SIDES
        self._tracer_walls = [{sides[w]: float(value[t, w]) for w in range(len(sides)) if kind[t, w]} for t in range(self.n_tracers)]
        if not kind.any():
            self._tracer_walls = None

    def tracer_walls(self):
        """The walls as they are set: a list of n_tracers dicts {side: value}, or None while the feature is off."""
        return getattr(self, "_tracer_walls", None)

    def tracer_wall_flux(self):
        """(n_tracers, 4): the flux kappa_t int_w (dn q_t - eta_b (q_t - g)) of the current tracers through every side, positive
        into the domain, 0 on a no-flux side; with zero velocity d/dt int q_t is the sum over the sides."""
        flux = np.zeros((self.n_tracers, 4))
        self._ck(self.lib.hdg_get_tracer_wall_flux(self.h, self.n_tracers, _ptr(flux)))
        return flux

    def apply_tracer_wall_diffusion(self, q, walls):
        """M^-1 (D + sum_w D_w) q + M^-1 sum_w l_w of one nodal DG_k field for one dict of walls, without kappa (test hook;
        it sets nothing)."""
        q = _arr(q, self.shape_p)
        kind, value = self._wall_arrays(walls, 1)
        out = np.empty(self.shape_p)
        self._ck(self.lib.hdg_apply_tracer_wall_diffusion(self.h, kind.ctypes.data_as(_ip), _ptr(value), _ptr(q), _ptr(out)))
        return out

    # --- implicit tracer diffusion (include/hdg_tracer_implicit.h)
    def set_tracer_diffusion_mode(self, mode, rtol=1e-10, max_iterations=2000):
        """mode: 'explicit' (the default of an engine) or 'implicit' (or the integers 0 / 1 of the C-ABI).  Implicit: a step
        transports the tracers without their diffusion and ends with one backward-Euler solve per tracer with kappa_t != 0,
        conjugate gradients on the device to |r| <= rtol |b| (a Lie splitting, first order in dt)."""
        code = TRACER_DIFFUSION_MODES.get(mode, mode) if isinstance(mode, str) else mode
        if isinstance(code, str):
            raise ValueError(f"tracer_diffusion must be one of {sorted(TRACER_DIFFUSION_MODES)} (got {mode!r})")
        self._ck(self.lib.hdg_set_tracer_diffusion_mode(self.h, int(code), float(rtol), int(max_iterations)))
        self._tracer_diffusion_mode = int(code)

    def tracer_diffusion_mode(self):
        """'explicit' or 'implicit', as it is set"""
        return "implicit" if getattr(self, "_tracer_diffusion_mode", 0) == 1 else "explicit"

    def tracer_diffusion_solve(self):
        """(iterations (n_tracers,) int, relative residuals (n_tracers,)) of the last implicit solve; zeros for a tracer with
        kappa_t = 0 and before any solve."""
        its, res = np.zeros(self.n_tracers, dtype=np.int32), np.zeros(self.n_tracers)
        self._ck(self.lib.hdg_get_tracer_diffusion_solve(self.h, self.n_tracers, its.ctypes.data_as(_ip), _ptr(res)))
        return its, res

    def solve_tracer_diffusion(self, tau, q):
        """(x, iterations): x[t] solves (I - tau[t] M^-1 D_w) x = q[t] + tau[t] M^-1 l_w for n <= n_tracers nodal DG_k fields
        q (n, *shape_p), field t with the walls set for tracer t, to the rtol that is set (test hook; it sets nothing)."""
        tau = np.ascontiguousarray(np.asarray(tau, dtype=np.float64).reshape(-1))
        q = _arr(q, (len(tau),) + tuple(self.shape_p))
        out = np.empty_like(q)
        its = np.zeros(len(tau), dtype=np.int32)
        self._ck(self.lib.hdg_solve_tracer_diffusion(self.h, len(tau), _ptr(tau), _ptr(q), _ptr(out), its.ctypes.data_as(_ip)))
        return out, its

    # --- Boussinesq buoyancy (include/hdg_buoyancy.h)
    def set_buoyancy(self, beta, gravity=(0.0, -1.0)):
        """The tracers force the flow: + sum_t beta_t q_t g in the momentum equation.  beta: one value for every tracer or a
        sequence of n_tracers values (0: that tracer stays passive); None or zeros: off.  Needs a tracer (set_tracer)."""
        if beta is not None:
            beta = np.asarray(beta, dtype=np.float64)
            beta = np.full(self.n_tracers, float(beta)) if beta.ndim == 0 else np.ascontiguousarray(beta.reshape(-1))
        g = np.ascontiguousarray(np.asarray(gravity, dtype=np.float64).reshape(-1))
        if g.shape != (2,):
            raise ValueError(f"gravity must have two components (got {g.size})")
        self._ck(self.lib.hdg_set_buoyancy(self.h, 0 if beta is None else len(beta), _ptr(beta), _ptr(g)))

    def buoyancy(self):
        """(beta (n_tracers,), gravity (2,)) as they are set; beta is all zero while the term is off."""
        beta, g = np.zeros(self.n_tracers), np.zeros(2)
        self._ck(self.lib.hdg_get_buoyancy(self.h, self.n_tracers, _ptr(beta), _ptr(g)))
        return beta, g

    def apply_buoyancy(self, q):
        """B(q) = sum_t beta_t q_t g of nodal tracer fields (the layout of set_tracer) as a nodal velocity-space field
        (the layout of get_field's Q), with the beta and gravity currently set (test hook)."""
        q = _arr(q, self.shape_q)
        f = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_apply_buoyancy(self.h, _ptr(q), _ptr(f)))
        return f

    # --- viscous term (include/hdg_viscosity.h)
    def set_viscosity(self, nu, wall="free_slip"):
        """+ nu Laplace u in the momentum equation, explicit in time: the symmetric interior-penalty form on the velocity
        space with free-slip ('free_slip') or no-slip ('no_slip') walls.  nu = 0: off."""
        self._ck(self.lib.hdg_set_viscosity(self.h, float(nu), wall_code(wall)))

    def _get_viscosity(self):
        nu, wall, out = C.c_double(), C.c_int(), np.zeros(2)
        self._ck(self.lib.hdg_get_viscosity(self.h, C.byref(nu), C.byref(wall), _ptr(out)))
        return nu.value, wall.value, out

    def viscosity(self):
        """(nu, wall) as they are set; nu is 0 while the term is off."""
        nu, wall, _ = self._get_viscosity()
        return nu, {v: k for k, v in WALL_MODES.items()}[wall]

    def viscosity_number(self):
        """(Lambda_u, nu dt Lambda_u): Lambda_u is an upper bound of the spectral radius of M^-1 V in the wall mode set."""
        out = self._get_viscosity()[2]
        return float(out[0]), float(out[1])

    def apply_viscosity(self, Q, wall="free_slip"):
        """M^-1 V Q of a nodal velocity-space field (the layout of get_field's Q), without nu (test hook)."""
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_apply_viscosity(self.h, wall_code(wall), _ptr(Q), _ptr(out)))
        return out

    # --- moving no-slip walls and the wall force (include/hdg_moving_walls.h)
    def set_wall_velocity(self, v):
        """Constant tangential speeds of the no-slip walls of the structured unit square: a dict such as {"top": 1.0} (a
        missing side stands still) or four values in the order bottom, right, top, left; the wall's u_x on bottom and top, its
        u_y on left and right.  None or zeros: off.  Needs set_viscosity(nu, "no_slip") before.  On a strip partition every
        rank has to pass the same speeds."""
        self._ck(self.lib.hdg_set_wall_velocity(self.h, None if v is None else _ptr(wall_velocity_array(v))))

    def wall_velocity(self):
        """The four speeds as they are set, in the order bottom, right, top, left."""
        U = np.zeros(4)
        self._ck(self.lib.hdg_get_wall_velocity(self.h, _ptr(U)))
        return U

    def wall_force(self):
        """(4, 2): the viscous force on the fluid through every side (bottom, right, top, left) of the current velocity, with
        the nu, wall mode and speeds that are set; free slip gives the normal part only.  The pressure force is not in it."""
        F = np.zeros((4, 2))
        self._ck(self.lib.hdg_get_wall_force(self.h, _ptr(F)))
        return F

    def apply_moving_walls(self, Q, wall_velocity, wall="no_slip"):
        """M^-1 (V Q + l(U)) of a nodal velocity-space field, without nu (test hook; it sets nothing)."""
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        U = None if wall_velocity is None else wall_velocity_array(wall_velocity)
        self._ck(self.lib.hdg_apply_moving_walls(self.h, wall_code(wall), _ptr(U), _ptr(Q), _ptr(out)))
        return out

    def wall_force_of(self, Q, wall_velocity, wall="no_slip"):
        """(4, 2): the force functionals of a nodal velocity-space field, without nu (test hook; it sets nothing)."""
        Q = _arr(Q, self.shape_Q)
        F = np.zeros((4, 2))
        U = None if wall_velocity is None else wall_velocity_array(wall_velocity)
        self._ck(self.lib.hdg_apply_wall_force(self.h, wall_code(wall), _ptr(U), _ptr(Q), _ptr(F)))
        return F

    # --- adaptive time step (include/hdg_adaptive_dt.h)
    def set_dt(self, dt):
        """Change the step size between completed steps (finite and > 0, else HDGError HDG_ERR_ARG and nothing changes).  The
        value already held is a no-op.  On a strip partition every rank has to pass the same value."""
        self._ck(self.lib.hdg_set_dt(self.h, float(dt)))

    def get_dt(self):
        """The step size the engine holds"""
        dt = C.c_double()
        self._ck(self.lib.hdg_get_dt(self.h, C.byref(dt)))
        return dt.value

    def step_rates(self):
        """(4,) in the order of STEP_RATES: A = max_K (max nodal |u| in K) / h_K of the current velocity (diagnostics column
        'cfl' without its dt; not finite when the velocity is not), kappa_max Lambda, nu Lambda_u (plus S while the drag is
        on: the real-axis rate of the velocity-linear part) and F (0 while the term is off).  Collective on strips: every rank gets the global maximum."""
        rates = np.zeros(4)
        self._ck(self.lib.hdg_get_step_rates(self.h, _ptr(rates)))
        return rates

    def propose_dt(self, control, t, t_final):
        """The rule of csrc/hdg_step_control.hpp applied to step_rates() and the dt held; `control`: step_control(...).  It sets
        nothing.  HDGError HDG_ERR_NOT_CONVERGED when the velocity is not finite, HDG_ERR_ARG below dt_min."""
        out = C.c_double()
        self._ck(self.lib.hdg_propose_dt(self.h, C.byref(control), float(t), float(t_final), C.byref(out)))
        return out.value

    # --- linear drag and volume penalisation (include/hdg_drag.h)
    def cell_vertices(self):
        """(N_c, 3, 2): the vertices of this engine's cells (a rank's own on a strip) in the vertex order of the drag
        coefficients, read off the node coordinates: the velocity nodes contain the cell vertices."""
        from .output import cell_vertex_nodes

        X = self.node_coordinates()[0].reshape(self.n_cells, -1, 2)
        eng = self

        class _Mesh:  # what cell_vertex_nodes asks of a mesh: the first two cells' vertices and the tolerance scale
            general = eng.general
            nx, ny = eng.cfg.nx, eng.cfg.ny
            L = eng.cfg.length if eng.cfg.periodic else 1.0

            def num_cells(self):
                return eng.n_cells

        class _Space:
            value_size = 2

            def mesh(self):
                return mesh

        mesh, space = _Mesh(), _Space()
        if self.general:
            mesh.vertices, mesh.cells = self._vertices, self._cells
            v = self._vertices[self._cells]
            a, b = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
            mesh.volume = float(np.sum(0.5 * np.abs(a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0])))
            space.coordinates = X
        else:  # a strip's rows start at its own offset: the first square of the rank against the first square of the mesh
            space.coordinates = X - np.array([0.0, X[0, :, 1].min()])
        idx = cell_vertex_nodes(space)
        out = np.empty((self.n_cells, 3, 2))
        for s in range(2):
            out[s::2] = X[s::2][:, idx[s]]
        return out

    def _drag_sigma(self, sigma):
        """scalar | (N_c, 3) | callable sigma(x, y) at the cell vertices -> (N_c, 3) float64"""
        if callable(sigma):
            V = self.cell_vertices()
            sigma = np.asarray(sigma(V[..., 0], V[..., 1]), dtype=np.float64) * np.ones((self.n_cells, 3))
        elif np.ndim(sigma) == 0:
            sigma = np.full((self.n_cells, 3), float(sigma))
        return _arr(sigma, (self.n_cells, 3))

    def _drag_target(self, target):
        """None | (N_c n_u, 2) | callable u_s(x, y) -> (u_x, u_y) at the velocity nodes"""
        if target is None:
            return None
        if callable(target):
            X = self.node_coordinates()[0]
            ux, uy = target(X[:, 0], X[:, 1])
            target = np.stack([ux * np.ones(len(X)), uy * np.ones(len(X))], axis=-1)
        return _arr(target, self.shape_Q)

    def _drag_region(self, region):
        """None | N_c tags | callable r(x, y) at the centroids -> (N_c,) int32"""
        if region is None:
            return None
        if callable(region):
            ctr = self.cell_vertices().mean(axis=1)
            region = np.asarray(region(ctr[:, 0], ctr[:, 1])) * np.ones(self.n_cells, dtype=np.int64)
        region = np.ascontiguousarray(region, dtype=np.int32)
        if region.shape != (self.n_cells,):
            raise ValueError(f"expected {self.n_cells} region tags, got shape {region.shape}")
        return region

    def set_drag(self, sigma, target=None, region=None):
        """- sigma (u - u_s) in the momentum equation, explicit in time.  sigma >= 0: a scalar (uniform friction), (N_c, 3)
        vertex values per cell, or a callable sigma(x, y) evaluated at the cell vertices; None or all zeros: off.  target: u_s
        as a nodal velocity field or a callable (x, y) -> (u_x, u_y), None: at rest.  region: tags 0 .. 3 per cell for
        drag_force(), an array or a callable evaluated at the centroids.  Collective on strips."""
        sigma = None if sigma is None else self._drag_sigma(sigma)
        target, region = self._drag_target(target), self._drag_region(region)
        self._ck(self.lib.hdg_set_drag(self.h, _ptr(sigma), _ptr(target), None if region is None else region.ctypes.data_as(_ip)))

    def drag(self):
        """(N_c, 3): the coefficients as they are set; zeros while the term is off."""
        sigma = np.zeros((self.n_cells, 3))
        self._ck(self.lib.hdg_get_drag(self.h, _ptr(sigma), None))
        return sigma

    def drag_number(self):
        """(S, S dt): S = the largest vertex value of sigma (over all ranks), an upper bound of the spectral radius of M^-1 D."""
        out = np.zeros(2)
        self._ck(self.lib.hdg_get_drag(self.h, None, _ptr(out)))
        return float(out[0]), float(out[1])

    def apply_drag(self, Q, sigma, target=None):
        """- M^-1 D (Q - u_s) of a nodal velocity-space field for the given sigma and target (test hook; it sets nothing)."""
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_apply_drag(self.h, _ptr(self._drag_sigma(sigma)), _ptr(self._drag_target(target)), _ptr(Q), _ptr(out)))
        return out

    def drag_force(self):
        """(4, 3): per region (F_x, F_y, P), the force of the term on the fluid, - int sigma (u - u_s), and its rate of work,
        - int sigma (u - u_s) . u, of the current velocity with the setting held.  The force on a body is the negative."""
        F = np.zeros((HDG_DRAG_REGIONS, 3))
        self._ck(self.lib.hdg_get_drag_force(self.h, _ptr(F)))
        return F

    def drag_force_of(self, Q, sigma, target=None, region=None):
        """(4, 3): the same functionals of a nodal velocity-space field (test hook; it sets nothing)."""
        Q = _arr(Q, self.shape_Q)
        F = np.zeros((HDG_DRAG_REGIONS, 3))
        region = self._drag_region(region)
        self._ck(self.lib.hdg_apply_drag_force(self.h, _ptr(self._drag_sigma(sigma)), _ptr(self._drag_target(target)),
                                               None if region is None else region.ctypes.data_as(_ip), _ptr(Q), _ptr(F)))
        return F

    # --- Coriolis term (include/hdg_coriolis.h)
    def set_coriolis(self, f0, beta=0.0):
        """- f_c k x u in the momentum equation, f_c = f0 + beta y (y the mesh's own ordinate), explicit in time.
        f0 = beta = 0: off.  beta != 0 is refused on the doubly periodic square."""
        self._ck(self.lib.hdg_set_coriolis(self.h, float(f0), float(beta)))

    def _get_coriolis(self):
        f0, beta, out = C.c_double(), C.c_double(), np.zeros(2)
        self._ck(self.lib.hdg_get_coriolis(self.h, C.byref(f0), C.byref(beta), _ptr(out)))
        return f0.value, beta.value, out

    def coriolis(self):
        """(f0, beta) as they are set; both 0 while the term is off."""
        return self._get_coriolis()[:2]

    def coriolis_number(self):
        """(F, F dt): F = max over the mesh vertices of |f0 + beta y|, an upper bound of the spectral radius of M^-1 C."""
        out = self._get_coriolis()[2]
        return float(out[0]), float(out[1])

    def apply_coriolis(self, Q, f0, beta=0.0):
        """M^-1 C Q of a nodal velocity-space field (the layout of get_field's Q) for the given f0 and beta (test hook;
        it sets nothing)."""
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_apply_coriolis(self.h, float(f0), float(beta), _ptr(Q), _ptr(out)))
        return out

    def cg_size(self):
        n = C.c_long()
        self._ck(self.lib.hdg_cg_size(self.h, C.byref(n)))
        return n.value

    def cg_coordinates(self):
        xy = np.empty((self.cg_size(), 2))
        self._ck(self.lib.hdg_cg_coordinates(self.h, _ptr(xy)))
        return xy

    def cg_project_nodal(self, Q):
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_cg_project_nodal(self.h, _ptr(Q), _ptr(out)))
        return out

    def vorticity(self, Q=None):
        Q = None if Q is None else _arr(Q, self.shape_Q)
        out = np.empty(self.cg_size())
        self._ck(self.lib.hdg_vorticity(self.h, _ptr(Q), _ptr(out)))
        return out

    # --- stream function (include/hdg_streamfunction.h)
    def streamfunction(self, Q=None, rtol=1e-12):
        """(psi, info): the stream function of the nodal velocity-space field Q (None: the current velocity) at the dofs of
        cg_coordinates(), and a dict with the entries of STREAMFUNCTION_INFO (iterations as an int).  Between steps only."""
        Q = None if Q is None else _arr(Q, self.shape_Q)
        psi = np.empty(self._psi_sizes()[1])
        info = np.zeros(8)
        self._ck(self.lib.hdg_streamfunction(self.h, _ptr(Q), float(rtol), _ptr(psi), _ptr(info)))
        out = dict(zip(STREAMFUNCTION_INFO, (float(v) for v in info)))
        out["iterations"] = int(info[0])
        return psi, out

    def _psi_sizes(self):
        """(vertices, n_cg); the vertex count first, so that a refusal is the stream function's own (a strip: HDG_ERR_UNSUPPORTED)"""
        return self.psi_vertex_count(), self.cg_size()

    def psi_vertex_count(self):
        n = C.c_long()
        self._ck(self.lib.hdg_psi_vertex_count(self.h, C.byref(n)))
        return n.value

    def apply_cg_stiffness(self, x):
        """K x, K the stiffness matrix of the continuous space (test hook; it sets nothing)."""
        ncg = self._psi_sizes()[1]
        x = _arr(x, (ncg,))
        out = np.empty(ncg)
        self._ck(self.lib.hdg_apply_cg_stiffness(self.h, _ptr(x), _ptr(out)))
        return out

    def psi_transfer(self, values, transpose=False):
        """The nested P1 interpolation P from the mesh vertices to the continuous space, or its transpose (test hook)."""
        nv, ncg = self._psi_sizes()
        values = _arr(values, (ncg if transpose else nv,))
        out = np.empty(nv if transpose else ncg)
        self._ck(self.lib.hdg_psi_transfer(self.h, 1 if transpose else 0, _ptr(values), _ptr(out)))
        return out

    def apply_psi_preconditioner(self, r, form=0):
        """B r, B the preconditioner of the stream-function solve (form 0) or the diagonal alone (form 1) (test hook)."""
        ncg = self._psi_sizes()[1]
        r = _arr(r, (ncg,))
        out = np.empty(ncg)
        self._ck(self.lib.hdg_apply_psi_preconditioner(self.h, int(form), _ptr(r), _ptr(out)))
        return out

    def cg_to_broken(self, values):
        values = _arr(values, (self.cg_size(),))
        out = np.empty(self.n_cells * self.n_u)
        self._ck(self.lib.hdg_cg_to_broken(self.h, _ptr(values), _ptr(out)))
        return out

    TIMER_LABELS = ("timestep", "bdm_projection", "tentative_velocity_solve", "pressure_solve", "unsplit_solve")
    # hdg_set_kernel_timing; no reference counterpart: the two kernels of a tentative-velocity iteration by form
    KERNEL_TIMER_LABELS = ("kernel_advection", "kernel_lift", "kernel_advection_plain", "kernel_lift_plain")
    # label 9: the (u, phi) solve of the implicit DG step; reported once it has been called
    DG_TIMER_LABELS = ("dg_implicit_solve",)

    def timers(self, reset=False, kernels=False):
        """Device-side section timers (labels of the reference's PerformanceLog): {label: (ncall, total_s, sumsq_s2)};
        kernels=True adds the per-launch brackets of the two kernels of a tentative-velocity iteration."""
        n = 10  # HDG_N_TIMERS
        tot, sq = np.zeros(n), np.zeros(n)
        cnt = np.zeros(n, dtype=np.int64)
        self._ck(self.lib.hdg_get_timers(self.h, _ptr(tot), _ptr(sq), cnt.ctypes.data_as(_lp), 1 if reset else 0))
        labels = self.TIMER_LABELS + self.KERNEL_TIMER_LABELS + self.DG_TIMER_LABELS
        out = {lab: (int(c), t * 1e-3, q * 1e-6) for lab, c, t, q in zip(labels, cnt, tot, sq)}
        return {lab: v for lab, v in out.items()
                if (lab not in self.KERNEL_TIMER_LABELS or kernels) and (lab not in self.DG_TIMER_LABELS or v[0] > 0)}

    LAUNCH_CLASSES = ("advection_apply", "edge_lift", "stage_rhs", "weak_divergence", "condense", "trace_apply", "trace_smooth",
                      "backsub", "vertex_multigrid", "vector_update", "dot", "copy_fill", "other")

    def launch_stats(self, reset=False):
        """Launch census since the last reset: {class: (launches, algorithmic bytes)} (hdg_get_launch_stats)."""
        n = len(self.LAUNCH_CLASSES)
        calls = np.zeros(n, dtype=np.int64)
        nbytes = np.zeros(n)
        self._ck(self.lib.hdg_get_launch_stats(self.h, calls.ctypes.data_as(_lp), _ptr(nbytes), 1 if reset else 0))
        return {lab: (int(c), float(b)) for lab, c, b in zip(self.LAUNCH_CLASSES, calls, nbytes)}

    def comm_info(self):
        """(rank, ranks of the partition, ranks the transport reports, transport name) -- hdg_get_comm_info"""
        r, n, t = C.c_int(), C.c_int(), C.c_int()
        name = C.create_string_buffer(16)
        self._ck(self.lib.hdg_get_comm_info(self.h, C.byref(r), C.byref(n), C.byref(t), name))
        return r.value, n.value, t.value, name.value.decode()

    def general_topology(self):
        """(edge_vertices (n_edges, 2), edge_cells (n_edges, 2; -1 = boundary)) of a general-mesh engine"""
        ev = np.zeros((self.n_edges, 2), dtype=np.int32)
        ec = np.zeros((self.n_edges, 2), dtype=np.int32)
        self._ck(self.lib.hdg_general_topology(self.h, ev.ctypes.data_as(_ip), ec.ctypes.data_as(_ip)))
        return ev, ec

    def set_kernel_timing(self, on):
        self._ck(self.lib.hdg_set_kernel_timing(self.h, 1 if on else 0))

    # --- helpers
    def node_coordinates(self):
        xq = np.empty(self.shape_Q)
        xp = np.empty((self.n_cells * self.n_p, 2))
        self._ck(self.lib.hdg_node_coordinates(self.h, _ptr(xq), _ptr(xp)))
        return xq, xp

    def l2_norms(self, Q=None, p=None):
        nq, npv = C.c_double(0.0), C.c_double(0.0)
        Q = None if Q is None else _arr(Q, self.shape_Q)
        p = None if p is None else _arr(p, self.shape_p)
        self._ck(self.lib.hdg_l2_norms(self.h, _ptr(Q), _ptr(p), C.byref(nq), C.byref(npv)))
        return nq.value, npv.value

    def integrate_pressure(self, p):
        p = _arr(p, self.shape_p)
        out = C.c_double()
        self._ck(self.lib.hdg_integrate_pressure(self.h, _ptr(p), C.byref(out)))
        return out.value

    def apply_advection(self, Qstar, x, gamma):
        Qstar, x = _arr(Qstar, self.shape_Q), _arr(x, self.shape_Q)
        y = np.empty(self.shape_Q)
        self._ck(self.lib.hdg_apply_advection(self.h, _ptr(Qstar), _ptr(x), float(gamma), _ptr(y)))
        return y

    def apply_trace_operator(self, lam):
        lam = _arr(lam, self.shape_l)
        out = np.empty(self.shape_l)
        self._ck(self.lib.hdg_apply_trace_operator(self.h, _ptr(lam), _ptr(out)))
        return out

    def apply_weak_divergence(self, Q, broken=False):
        Q = _arr(Q, self.shape_Q)
        out = np.empty(self.shape_p)
        self._ck(self.lib.hdg_apply_weak_divergence(self.h, _ptr(Q), 1 if broken else 0, _ptr(out)))
        return out

    # --- flow diagnostics (include/hdg_mi355x.h: hdg_compute_diagnostics / hdg_set_diagnostics / hdg_get_diagnostics)
    def compute_diagnostics(self, Q, p, q=None):
        """The nine diagnostics of nodal fields (DIAGNOSTICS order); q None: no tracer (columns 5, 6 NaN)."""
        Q, p = _arr(Q, self.shape_Q), _arr(p, self.shape_p)
        q = None if q is None else _arr(q, self.shape_p)
        out = np.empty(len(DIAGNOSTICS))
        self._ck(self.lib.hdg_compute_diagnostics(self.h, _ptr(Q), _ptr(p), _ptr(q), _ptr(out)))
        return out

    def set_diagnostics(self, capacity):
        """Record one row per completed step into a device buffer of `capacity` rows (the current state is the first
        row); 0 switches recording off."""
        self._ck(self.lib.hdg_set_diagnostics(self.h, int(capacity)))

    def _fetch_rows(self, fn, shape_tail, reset, *extra):
        """The rows of a per-step output, (n, *shape_tail): `fn` is its hdg_get_* entry, `extra` the pointers that takes
        between the row count and the reset flag.  Two calls: the row count (extras null, no reset), then the rows."""
        n = C.c_int(0)
        rc = fn(self.h, None, 0, C.byref(n), *(None for _ in extra), 0)  # dropped rows (-1): raised by the call below
        if rc not in (0, -1):
            self._ck(rc)
        rows = np.empty((n.value, *shape_tail))
        self._ck(fn(self.h, _ptr(rows) if rows.size else None, n.value if rows.size else 0, C.byref(n), *extra,
                    1 if reset else 0))
        return rows

    def diagnostics(self, reset=False):
        """The recorded rows, (n, 9) in DIAGNOSTICS order.  Raises HDGError when rows were dropped beyond the capacity."""
        return self._fetch_rows(self.lib.hdg_get_diagnostics, (len(DIAGNOSTICS),), reset)

    # --- point values (include/hdg_mi355x.h: hdg_evaluate_points / hdg_set_probes / hdg_get_probes)
    @staticmethod
    def _points(xy):
        xy = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
        return xy

    def evaluate_points(self, xy, Q=None, p=None, q=None):
        """Values at the points xy (n, 2) of nodal fields (any may be None: NaN columns): (values (n, 5) in POINT_COLUMNS
        order, located (n,) bool).  A point outside the domain has a NaN row and located False.  Collective on strips."""
        xy = self._points(xy)
        Q = None if Q is None else _arr(Q, self.shape_Q)
        p = None if p is None else _arr(p, self.shape_p)
        q = None if q is None else _arr(q, self.shape_p)
        n = len(xy)
        out = np.empty((n, len(POINT_COLUMNS)))
        located = np.zeros(n, dtype=np.int32)
        self._ck(self.lib.hdg_evaluate_points(self.h, _ptr(Q), _ptr(p), _ptr(q), n, _ptr(xy), _ptr(out),
                                              located.ctypes.data_as(_ip)))
        return out, located.astype(bool)

    def set_probes(self, xy, capacity):
        """Record the values at the points xy (n, 2) after every completed step into a device buffer of `capacity` rows (the
        current state is the first row); capacity 0 or no points switches recording off.  Raises HDGError (HDG_ERR_ARG) for
        a point outside the domain."""
        xy = self._points(xy) if xy is not None else np.zeros((0, 2))
        self._n_probes = 0
        self._ck(self.lib.hdg_set_probes(self.h, len(xy), _ptr(xy), int(capacity)))
        self._n_probes = len(xy) if capacity > 0 else 0

    def probes(self, reset=True):
        """The recorded rows, (rows, n, 5) in POINT_COLUMNS order.  Raises HDGError when rows were dropped."""
        return self._fetch_rows(self.lib.hdg_get_probes, (getattr(self, "_n_probes", 0), len(POINT_COLUMNS)), reset)

    # --- Lagrangian particles (include/hdg_mi355x.h: hdg_set_particles / hdg_get_particles / hdg_advance_particles)
    def set_particles(self, xy, capacity, record_every=1):
        """Advect the particles seeded at xy (n, 2) through the velocity of every completed step on the device (Heun) and
        record their positions every `record_every`-th step into a device buffer of `capacity` rows (row 0: the seeds);
        capacity 0 or no particles switches the feature off.  Raises HDGError (HDG_ERR_ARG) for a seed outside the domain,
        (HDG_ERR_UNSUPPORTED) on a general mesh."""
        xy = self._points(xy) if xy is not None else np.zeros((0, 2))
        self._n_particles = 0
        self._ck(self.lib.hdg_set_particles(self.h, len(xy), _ptr(xy), int(capacity), int(record_every)))
        self._n_particles = len(xy) if capacity > 0 else 0

    def particles(self, reset=True):
        """(rows (rows, n, 2), counts): the recorded positions and {"clamped", "lost", "dropped"}.  Raises HDGError when
        rows were dropped beyond the capacity."""
        counts = np.zeros(3, dtype=np.int64)
        rows = self._fetch_rows(self.lib.hdg_get_particles, (getattr(self, "_n_particles", 0), 2), reset,
                                counts.ctypes.data_as(_lp))
        return rows, {"clamped": int(counts[0]), "lost": int(counts[1]), "dropped": int(counts[2])}

    def advance_particles(self, dt, nsteps):
        """nsteps Heun steps of size dt through the current velocity held fixed (streamlines of a snapshot); appends one row,
        the positions reached."""
        self._ck(self.lib.hdg_advance_particles(self.h, float(dt), int(nsteps)))

    # --- checkpoint and restart (include/hdg_checkpoint.h)
    # byte offsets of the two counts in the blob header a binding needs to shape recorder rows (csrc/hdg_checkpoint.hpp: Header)
    _CK_HEADER = "<8sIIqdQQiiQ"
    _CK_FLAGS = (("tracer", 1), ("diagnostics", 2), ("probes", 4), ("particles", 8))

    def save_checkpoint(self, step, t):
        """The engine's whole state as bytes (between steps only); `step` and `t` come back from load_checkpoint."""
        n = C.c_long()
        self._ck(self.lib.hdg_checkpoint_size(self.h, C.byref(n)))
        buf = np.empty(n.value, dtype=np.uint8)
        self._ck(self.lib.hdg_checkpoint_save(self.h, int(step), float(t), buf.ctypes.data_as(C.c_void_p), n.value))
        return buf.tobytes()

    @classmethod
    def checkpoint_info(cls, blob):
        """What the header of a checkpoint says, without an engine: step, t, whether a tracer, diagnostics, probes and
        particles were switched on, and the numbers of probe points and particles.  The engine validates the blob when it
        loads it; this only reads the header (ValueError when there is none)."""
        import struct
        if len(blob) < struct.calcsize(cls._CK_HEADER) or bytes(blob[:8]) != b"HDGCKPT\0":
            raise ValueError("not a checkpoint of this engine (bad magic or shorter than a header)")
        hdr = struct.unpack_from(cls._CK_HEADER, blob, 0)
        info = {name: bool(hdr[9] & bit) for name, bit in cls._CK_FLAGS}
        info.update(step=int(hdr[3]), t=float(hdr[4]), n_probes=int(hdr[7]), n_particles=int(hdr[8]))
        return info

    def load_checkpoint(self, blob):
        """Make this engine the one that wrote `blob`; returns (step, t).  Raises HDGError (HDG_ERR_ARG) naming the cause for a
        blob of another engine or a damaged one, and then leaves the engine as it was."""
        buf = np.frombuffer(blob, dtype=np.uint8)
        step, t = C.c_long(), C.c_double()
        self._ck(self.lib.hdg_checkpoint_load(self.h, buf.ctypes.data_as(C.c_void_p), len(buf), C.byref(step), C.byref(t)))
        info = self.checkpoint_info(blob)
        self._n_probes, self._n_particles = info["n_probes"], info["n_particles"]  # the shapes of probes() / particles()
        self._tracer_on = info["tracer"]
        return step.value, t.value

    def state_digest(self):
        """(d0, d1): 16 bytes that say whether two engines are in the same state (hdg_state_digest)."""
        out = (C.c_ulonglong * 2)()
        self._ck(self.lib.hdg_state_digest(self.h, out))
        return int(out[0]), int(out[1])

    def digest_vector(self, v):
        """(d0, d1) of the 64-bit patterns of v, computed by the device kernel (hdg_digest_vector)."""
        v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
        out = (C.c_ulonglong * 2)()
        self._ck(self.lib.hdg_digest_vector(self.h, _ptr(v) if v.size else None, v.size, out))
        return int(out[0]), int(out[1])

    # --- transfer between engines on nested meshes (include/hdg_transfer.h)
    def transfer_from(self, src, tracers=False):
        """Take the state of the engine `src` (another mesh size and degree on a nested mesh): the L2 projection of its velocity,
        pressure and, with tracers=True, its tracers onto this engine's spaces, on the device.  Afterwards this engine is as
        after set_state (and set_tracer) with the transferred fields.  Raises HDGError naming the cause for a pair that does
        not fit (HDG_ERR_ARG; general meshes and strips HDG_ERR_UNSUPPORTED) and then leaves both engines as they were."""
        self._ck(self.lib.hdg_transfer_state(self.h, src.h, 1 if tracers else 0))
        if tracers:
            self._tracer_on = True

    def difference_norms(self, other):
        """{"Q", "p", "q"}: the L2 norms of the differences of the current states of this engine and `other`, exact on the
        common refinement of the two meshes; "q" is an array of n_tracers norms when both carry tracers, else None."""
        nq, npv = C.c_double(0.0), C.c_double(0.0)
        both = getattr(self, "_tracer_on", False) and getattr(other, "_tracer_on", False)
        q = np.zeros(self.n_tracers) if both else None
        self._ck(self.lib.hdg_transfer_difference(self.h, other.h, C.byref(nq), C.byref(npv), _ptr(q)))
        return {"Q": nq.value, "p": npv.value, "q": q}

    def time_kernel(self, kernel, reps):
        ms = C.c_double()
        self._ck(self.lib.hdg_time_kernel(self.h, kernel, reps, C.byref(ms)))
        return ms.value
