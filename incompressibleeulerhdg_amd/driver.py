"""Command-line driver with the flags and printed quantities of the reference's src/driver.py:23-385.

    python -m incompressibleeulerhdg_amd.driver --nx 64 --degree 2 --use_projection_method

``--problem taylorgreen`` (unit square), ``--problem shear`` (doubly periodic square, driver.py:182-183) and
``--problem kelvinhelmholtz`` (UnitDiskMesh(refinement), driver.py:184-185: the general-mesh path, projection and monolithic)
are built with the ``hdg`` discretisation and, with ``--timestepper implicit``, the ``dg`` one (IncompressibleEulerDGImplicit,
driver.py:203-213); the ``conforming`` discretisation raises.  ``--animation`` (evolution.pvd with
the CG vorticity, callbacks.py:30-85) and ``--tracer_advection`` (driver.py:340-344) work on every mesh.  The final fields are written to ``solution.pvd``
(``--output``) like the reference does (driver.py:356-385).

``--problem cavity`` is the unit square at rest with every tracer starting from 0; ``--tracer_wall SIDE VALUE [T]`` holds
tracers at fixed values on wall sides, e.g. a heated cavity:
``--problem cavity --tracer_advection --tracer_diffusivity K --viscosity NU --wall no_slip --buoyancy 1 --tracer_wall left 0.5
--tracer_wall right -0.5``.  The wall flux of every tracer and side is printed at the end.

``--wall_velocity SIDE U`` moves a no-slip wall along itself at the constant speed U; the viscous force
through every side is printed at the end.  The lid-driven cavity at Re = 100:
``--problem cavity --viscosity 1e-2 --wall no_slip --wall_velocity top 1``.

``--particles FILE`` advects Lagrangian particles through the two structured problems on the device
and writes their positions to ``--particle_output`` (``particles.npz``).

``--checkpoint FILE`` writes the engine's whole state after every ``--checkpoint_every``-th step and after the last one;
``--restart FILE`` continues such a file to ``--tfinal``: the same run, bit for bit.  With ``--gpus N``
each rank writes and reads ``FILE.<rank>``.  The final printout carries ``state digest``, 16 bytes that are equal exactly when
two runs ended in the same engine state.

``--start_from FILE`` starts the run at t = 0 from the state a ``--checkpoint`` FILE of another resolution holds: a second
timestepper with ``--start_nx``, ``--start_degree`` and ``--start_dt`` (each defaults to the run's own value) loads FILE, and its
state is L2 projected onto the run's spaces on the device; the meshes must be nested.

``--cfl C`` holds the CFL number at C with a step size that changes during the run: ``--dt`` is the first
step size and, without ``--dt_max``, the largest; the controller decides before the first step and after every
``--adapt_every``-th one, and a proposal below ``--dt_min`` or more than ``--max_steps`` steps stop the run.  One line at the end
gives the number of steps and the range of the step sizes.  Not with ``--checkpoint`` / ``--restart``.

``--gpus N`` (N > 1) runs the two structured problems on N strips (one process per rank, include/hdg_mi355x.h:
hdg_create_distributed): the driver starts ``python -m torch.distributed.run --nproc-per-node=N`` with the same arguments
as a child process and returns its exit status.  Each rank chooses RCCL when every rank has a device of its own and the
shared-memory transport when ranks share one; only rank 0 prints and writes files.
"""
import argparse
import contextlib
import io
import os
import subprocess
import sys
import time

import numpy as np

from ._lib import DIAGNOSTICS, HDG_MAX_TRACERS, POINT_COLUMNS, WALL_SIDES
from .auxilliary.callbacks import AnimationCallback
from .auxilliary.logging import log_summary
from .mesh import Function, FunctionSpace, PeriodicSquareMesh, UnitDiskMesh, UnitSquareMesh
from .model_problems import CylinderWake, DraggedTaylorGreen, Cavity, DoubleLayerShearFlow, KelvinHelmholtz, RotatingTaylorGreen, TaylorGreen
from .output import VTKFile
from .timesteppers import (
    IncompressibleEulerHDGIMEXARS2_232,
    IncompressibleEulerHDGIMEXARS3_443,
    IncompressibleEulerHDGIMEXImplicit,
    IncompressibleEulerHDGIMEXSSP2_332,
    IncompressibleEulerHDGIMEXSSP3_433,
    IncompressibleEulerDGImplicit,
    IncompressibleEulerHDGImplicit,
)

TIMESTEPPERS = {
    "imex_implicit": IncompressibleEulerHDGIMEXImplicit,
    "imex_ars2_232": IncompressibleEulerHDGIMEXARS2_232,
    "imex_ars3_443": IncompressibleEulerHDGIMEXARS3_443,
    "imex_ssp2_332": IncompressibleEulerHDGIMEXSSP2_332,
    "imex_ssp3_433": IncompressibleEulerHDGIMEXSSP3_433,
}


def build_parser():
    """Same flags and defaults as driver.py:26-176."""
    parser = argparse.ArgumentParser("Mesh specifications and polynomial degree")
    parser.add_argument("--problem", choices=["taylorgreen", "kelvinhelmholtz", "shear", "cavity", "cylinder"], type=str, default="taylorgreen", help="model problem to solve")
    parser.add_argument("--nx", metavar="nx", type=int, default=8, help="number of grid cells in x-direction")
    parser.add_argument("--refinement", metavar="refinement", type=int, default=2, help="refinement level for unit disk mesh")
    parser.add_argument("--degree", metavar="degree", type=int, default=1, help="polynomial degree")
    parser.add_argument("--tfinal", metavar="tfinal", type=float, default=1.0, help="final time")
    parser.add_argument("--kappa", type=float, default=0.5, help="exponential decay factor")
    parser.add_argument("--dt", type=float, default=0.04, help="timestep size")
    parser.add_argument("--discretisation", choices=["conforming", "dg", "hdg"], type=str, default="hdg", help="discretisation method")
    parser.add_argument("--use_projection_method", action="store_true", default=False, help="use projection method for timestepping")
    parser.add_argument("--richardson", metavar="richardson", type=int, default=2, help="number of Richardson iterations")
    parser.add_argument("--flux", choices=["upwind", "centered"], type=str, default="upwind", help="numerical flux")
    parser.add_argument("--timestepper", choices=["implicit"] + list(TIMESTEPPERS), type=str, default="imex_ssp2_332", help="timestepper")
    parser.add_argument("--forcing", choices=["exponential", "constant"], type=str, default="exponential", help="forcing")
    parser.add_argument("--test_pressure_solver", action="store_true", default=False, help="carry out a single solve with the pressure solver for testing")
    parser.add_argument("--warmup", action="store_true", default=False, help="only perform one timestep")
    parser.add_argument("--animation", action="store_true", default=False,
                        help="save velocity and pressure fields at the end of each timestep as an animation")
    parser.add_argument("--tracer_advection", action="store_true", default=False, help="advect tracer field")
    parser.add_argument("--tracer_diffusivity", metavar="K", type=float, nargs="+", default=None,
                        help="molecular diffusivity of the tracers (with --tracer_advection): one value for all of them or "
                             "exactly --tracers values; explicit in time, see the printed diffusion number")
    parser.add_argument("--tracer_diffusion", choices=["explicit", "implicit"], default=None,
                        help="how the tracers diffuse (with --tracer_diffusivity): explicit in the stages (the default), or "
                             "implicit, one backward-Euler solve per step on the device: no limit on the diffusion number, first "
                             "order in dt; single GPU, structured meshes")
    parser.add_argument("--tracer_wall", metavar=("SIDE", "VALUE"), nargs="+", action="append", default=None,
                        help="SIDE VALUE [T]: hold tracer T (without T: every tracer) at VALUE on the wall SIDE (bottom, right, top, "
                             "left on the unit square; boundary with --problem kelvinhelmholtz); repeatable; acts through "
                             "--tracer_diffusivity; the wall flux of every tracer and side is printed at the end")
    parser.add_argument("--viscosity", metavar="NU", type=float, default=None,
                        help="kinematic viscosity: the momentum equation gains NU Laplace u, explicit in time (see the printed "
                             "viscous diffusion number); with --problem taylorgreen the forcing keeps the manufactured solution exact")
    parser.add_argument("--wall", choices=["free_slip", "no_slip"], default=None,
                        help="walls of the viscous term (with --viscosity; default free_slip)")
    parser.add_argument("--wall_velocity", metavar=("SIDE", "U"), nargs=2, action="append", default=None,
                        help="SIDE U: the no-slip wall SIDE (bottom, right, top, left) of the unit square moves along itself at the "
                             "constant speed U (repeatable; with --viscosity and --wall no_slip); the viscous force through every "
                             "side is printed at the end")
    parser.add_argument("--coriolis", metavar="F", type=float, nargs="+", default=None,
                        help="rotation F0 [BETA]: the momentum equation gains - (F0 + BETA y) k x u, explicit in time (see the "
                             "printed rotation number); with --problem taylorgreen the forcing keeps the manufactured solution exact")
    parser.add_argument("--drag", metavar="R", type=float, default=None,
                        help="uniform linear friction: the momentum equation gains - R u, explicit in time (see the printed drag "
                             "number); with --problem taylorgreen the forcing keeps the manufactured solution exact")
    parser.add_argument("--obstacle_drag", metavar="S", type=float, default=None,
                        help="with --problem cylinder: sigma inside the disc and at the crest of the fringe (default: the value that "
                             "puts (nu Lambda_u + S) dt at half the real-axis limit of the explicit tableau)")
    parser.add_argument("--stream", metavar="U", type=float, default=None, help="with --problem cylinder: the free stream (U, 0) (default 1)")
    parser.add_argument("--buoyancy", metavar="B", type=float, nargs="+", default=None,
                        help="Boussinesq buoyancy (with --tracer_advection): the momentum equation gains sum_t B_t q_t g; one "
                             "value for all tracers or exactly --tracers values, 0 keeps a tracer passive; explicit in time")
    parser.add_argument("--gravity", metavar=("GX", "GY"), type=float, nargs=2, default=None,
                        help="the constant g of --buoyancy (default 0 -1)")
    parser.add_argument("--tracers", metavar="N", type=int, default=1,
                        help="number of passive tracers advected through the one flow (with --tracer_advection); tracer m "
                             "starts from sin(2 pi (m+1) x) sin(2 pi (m+1) y)")
    # additions of the build
    parser.add_argument("--fused", action="store_true", default=False, help="run each timestep as one device-resident call")
    parser.add_argument("--output", type=str, default="solution.pvd",
                        help="VTK collection written at the end like the reference's solution.pvd ('' = no output)")
    parser.add_argument("--device", type=int, default=0, help="HIP device ordinal")
    parser.add_argument("--diagnostics", metavar="FILE", type=str, default=None,
                        help="record energy, enstrophy, divergence, jumps, integrals, maximum speed and CFL number of every "
                             "step on the device and write them to FILE (CSV); also prints the solver events")
    parser.add_argument("--probes", metavar="FILE", type=str, default=None,
                        help="record velocity, pressure, tracer and cell-local vorticity at the points of FILE (one 'x y' per "
                             "line, '#' starts a comment) after every step on the device")
    parser.add_argument("--probe_output", metavar="CSV", type=str, default="probes.csv",
                        help="CSV the --probes time series is written to")
    parser.add_argument("--particles", metavar="FILE", type=str, default=None,
                        help="advect Lagrangian particles seeded at the points of FILE (the format of --probes) through the "
                             "velocity of every step on the device")
    parser.add_argument("--particle_output", metavar="NPZ", type=str, default="particles.npz",
                        help="file the --particles positions are written to (t, xy (rows, n, 2), clamped, lost)")
    parser.add_argument("--particle_every", metavar="M", type=int, default=1,
                        help="record the particle positions every M-th step (they move every step)")
    parser.add_argument("--checkpoint", metavar="FILE", type=str, default=None,
                        help="write the engine's whole state to FILE after every --checkpoint_every-th step and after the last "
                             "one (--gpus N: FILE.<rank>)")
    parser.add_argument("--checkpoint_every", metavar="M", type=int, default=None,
                        help="with --checkpoint: write after every M-th step (default: after the last step only)")
    parser.add_argument("--restart", metavar="FILE", type=str, default=None,
                        help="continue the run whose --checkpoint FILE this is, to --tfinal")
    parser.add_argument("--start_from", metavar="FILE", type=str, default=None,
                        help="start at t = 0 from the state of the --checkpoint FILE of a run of another mesh size or degree, "
                             "projected onto this run's spaces (nested meshes; --problem shear)")
    parser.add_argument("--start_nx", metavar="N", type=int, default=None, help="with --start_from: the nx of the run that wrote FILE (default: --nx)")
    parser.add_argument("--start_degree", metavar="K", type=int, default=None,
                        help="with --start_from: the degree of the run that wrote FILE (default: --degree)")
    parser.add_argument("--start_dt", metavar="DT", type=float, default=None,
                        help="with --start_from: the timestep size of the run that wrote FILE (default: --dt)")
    parser.add_argument("--cfl", metavar="C", type=float, default=None,
                        help="adaptive time step: hold the CFL number dt max |u| / h at C; --dt is the first step size (and the "
                             "largest without --dt_max); not with --checkpoint / --restart")
    parser.add_argument("--dt_min", metavar="D", type=float, default=None, help="with --cfl: a proposed step size below D stops the run")
    parser.add_argument("--dt_max", metavar="D", type=float, default=None, help="with --cfl: the largest step size (default: --dt)")
    parser.add_argument("--adapt_every", metavar="M", type=int, default=None,
                        help="with --cfl: the controller decides before the first step and after every M-th one (default 1)")
    parser.add_argument("--max_steps", metavar="N", type=int, default=None,
                        help="with --cfl: stop the run with an error after N steps (default 10 ceil(tfinal / dt)); sizes the row logs")
    parser.add_argument("--streamfunction", action="store_true", default=False,
                        help="after the run print the extrema of the stream function, their positions, the defect "
                             "|u - ubar - curl psi| and the iteration count; with --animation psi is written next to the vorticity")
    parser.add_argument("--gpus", type=int, default=1,
                        help="number of ranks (strip partition of the square meshes, one process per rank)")
    return parser


def check_multi_gpu(args):
    """Refuse what the strip partition does not run, before any process is started or any engine is built."""
    if args.gpus < 1:
        raise RuntimeError(f"--gpus must be at least 1 (got {args.gpus})")
    if args.gpus == 1:
        return
    refused = [
        (args.tracer_advection, "--tracer_advection (the continuous space of the tracer is single-rank)"),
        (args.animation, "--animation (the vorticity's continuous space is single-rank)"),
        (args.test_pressure_solver, "--test_pressure_solver"),
        (args.discretisation == "dg", "--discretisation dg (single-rank)"),
        (args.problem == "kelvinhelmholtz", "--problem kelvinhelmholtz (general meshes are single-rank)"),
        (args.nx % args.gpus != 0, f"--nx {args.nx} not divisible by --gpus {args.gpus} (strips of equal height)"),
    ]
    for bad, what in refused:
        if bad:
            raise RuntimeError(f"--gpus {args.gpus} does not support {what}")


def check_streamfunction(args):
    """Refuse --streamfunction where the engine has no stream function, before any process is started or any engine is built."""
    if not args.streamfunction:
        return
    if args.gpus > 1:
        raise RuntimeError(f"--streamfunction does not support --gpus {args.gpus} (the continuous space is single-rank)")
    if args.problem == "kelvinhelmholtz":
        raise RuntimeError("--streamfunction does not support --problem kelvinhelmholtz (the stream function runs on the square meshes only)")


def report_streamfunction(timestepper):
    """One line: the extrema of psi of the current velocity and where they lie, the defect and the iteration count."""
    eng = timestepper._engine
    psi, info = eng.streamfunction()
    xy = eng.cg_coordinates()
    lo, hi = int(np.argmin(psi)), int(np.argmax(psi))
    print(f"stream function: min = {float(psi[lo])!r} at ({float(xy[lo, 0])!r}, {float(xy[lo, 1])!r}), "
          f"max = {float(psi[hi])!r} at ({float(xy[hi, 0])!r}, {float(xy[hi, 1])!r}), "
          f"defect = {info['defect']!r}, iterations = {info['iterations']}")
    print()


def check_particles(args):
    """Refuse --particles where the engine does not advect them, before any process is started or any engine is built."""
    if not args.particles:
        return
    if args.problem == "kelvinhelmholtz":
        raise RuntimeError("--particles does not support --problem kelvinhelmholtz (particles run on the square meshes only)")
    if args.particle_every < 1:
        raise RuntimeError(f"--particle_every must be at least 1 (got {args.particle_every})")


def check_tracers(args):
    """Refuse a tracer count the engine does not carry, before any process is started or any engine is built."""
    if not 1 <= args.tracers <= HDG_MAX_TRACERS:
        raise RuntimeError(f"--tracers must be in 1 .. {HDG_MAX_TRACERS} (got {args.tracers})")
    if args.tracers > 1 and not args.tracer_advection:
        raise RuntimeError(f"--tracers {args.tracers} needs --tracer_advection")
    kappa = args.tracer_diffusivity
    if kappa is not None:
        if not args.tracer_advection:
            raise RuntimeError("--tracer_diffusivity needs --tracer_advection")
        if len(kappa) not in (1, args.tracers):
            raise RuntimeError(f"--tracer_diffusivity takes one value or --tracers = {args.tracers} values (got {len(kappa)})")
        for m, x in enumerate(kappa):
            if not (np.isfinite(x) and x >= 0):
                raise RuntimeError(f"--tracer_diffusivity: value {m} ({x}) is not a finite number >= 0")
    if args.tracer_diffusion is not None:
        if kappa is None:
            raise RuntimeError("--tracer_diffusion needs --tracer_diffusivity")
        if args.tracer_diffusion == "implicit" and args.gpus > 1:
            raise RuntimeError(f"--tracer_diffusion implicit does not support --gpus {args.gpus} (the solve is single-rank)")
        if args.tracer_diffusion == "implicit" and args.problem == "kelvinhelmholtz":
            raise RuntimeError("--tracer_diffusion implicit: the disk of --problem kelvinhelmholtz is a general mesh "
                               "(structured meshes only)")
    tracer_walls(args)
    beta = args.buoyancy
    if args.gravity is not None and beta is None:
        raise RuntimeError("--gravity needs --buoyancy")
    if beta is not None:
        if not args.tracer_advection:
            raise RuntimeError("--buoyancy needs --tracer_advection")
        if len(beta) not in (1, args.tracers):
            raise RuntimeError(f"--buoyancy takes one value or --tracers = {args.tracers} values (got {len(beta)})")
        for m, x in enumerate(beta):
            if not np.isfinite(x):
                raise RuntimeError(f"--buoyancy: value {m} ({x}) is not a finite number")
        for m, x in enumerate(args.gravity or ()):
            if not np.isfinite(x):
                raise RuntimeError(f"--gravity: component {m} ({x}) is not a finite number")


def tracer_walls(args):
    """--tracer_wall SIDE VALUE [T] (repeatable) -> one dict {side: value} per tracer, or None without the flag; refuses what
    the engine would, before any engine exists."""
    if not args.tracer_wall:
        return None
    if not args.tracer_advection:
        raise RuntimeError("--tracer_wall needs --tracer_advection")
    if args.problem == "shear":
        raise RuntimeError("--tracer_wall: the doubly periodic square of --problem shear has no walls")
    sides = ("boundary",) if args.problem == "kelvinhelmholtz" else WALL_SIDES
    walls = [dict() for _ in range(args.tracers)]
    for item in args.tracer_wall:
        if len(item) not in (2, 3):
            raise RuntimeError(f"--tracer_wall takes SIDE VALUE [T] (got {len(item)} words: {' '.join(item)})")
        side = item[0]
        if side not in sides:
            raise RuntimeError(f"--tracer_wall: unknown side {side!r} for --problem {args.problem} (one of {', '.join(sides)})")
        try:
            value = float(item[1])
        except ValueError:
            value = float("nan")
        if not np.isfinite(value):
            raise RuntimeError(f"--tracer_wall {side}: value {item[1]} is not a finite number")
        if len(item) == 3:
            if not item[2].isdigit() or int(item[2]) >= args.tracers:
                raise RuntimeError(f"--tracer_wall {side}: tracer {item[2]} is not in 0 .. {args.tracers - 1}")
            walls[int(item[2])][side] = value
        else:
            for w in walls:
                w[side] = value
    return walls


def nodal_mean(coordinates, degree, values):
    """The mean over the domain of a broken nodal P_k field (k >= 1), on the host: `coordinates` (n_cells * n_p, 2) are the
    node positions cell by cell, every cell an affine image of one node set.  The weights of the node set (the cell mean of a
    polynomial as a combination of its node values) come from the moments of the barycentric monomials,
    mean(l1^a l2^b) = 2 a! b! / (a + b + 2)!."""
    from math import factorial

    n_p = (degree + 1) * (degree + 2) // 2
    X = np.asarray(coordinates, dtype=float).reshape(-1, n_p, 2)
    area2 = lambda A, B, C: (B[..., 0] - A[..., 0]) * (C[..., 1] - A[..., 1]) - (C[..., 0] - A[..., 0]) * (B[..., 1] - A[..., 1])
    x0 = X[0]
    corners = max(((i, j, m) for i in range(n_p) for j in range(i + 1, n_p) for m in range(j + 1, n_p)),
                  key=lambda t: abs(area2(x0[t[0]], x0[t[1]], x0[t[2]])))  # the vertices are among the nodes
    A, B, C = (x0[i] for i in corners)
    l1, l2 = area2(A, x0, C) / area2(A, B, C), area2(A, B, x0) / area2(A, B, C)
    powers = [(a, b) for a in range(degree + 1) for b in range(degree + 1 - a)]
    V = np.array([l1 ** a * l2 ** b for a, b in powers])
    w = np.linalg.solve(V, np.array([2.0 * factorial(a) * factorial(b) / factorial(a + b + 2) for a, b in powers]))
    area = np.abs(area2(X[:, corners[0]], X[:, corners[1]], X[:, corners[2]]))
    return float(np.sum(area * (np.asarray(values, dtype=float).reshape(-1, n_p) @ w)) / np.sum(area))


def check_viscosity(args):
    """--viscosity / --wall, before any engine exists"""
    if args.wall is not None and args.viscosity is None:
        raise RuntimeError("--wall needs --viscosity")
    if args.viscosity is not None and not (np.isfinite(args.viscosity) and args.viscosity >= 0):
        raise RuntimeError(f"--viscosity {args.viscosity} is not a finite number >= 0")


def wall_velocity(args):
    """--wall_velocity SIDE U (repeatable) -> {side: speed}, or None without the flag; refuses what the engine would, before
    any engine exists."""
    if not args.wall_velocity:
        return None
    if args.viscosity is None or args.wall != "no_slip":
        raise RuntimeError("--wall_velocity needs --viscosity and --wall no_slip")
    if args.problem == "shear":
        raise RuntimeError("--wall_velocity: the doubly periodic square of --problem shear has no walls")
    if args.problem == "kelvinhelmholtz":
        raise RuntimeError("--wall_velocity: the disk of --problem kelvinhelmholtz is a general mesh (the structured unit square only)")
    speeds = {}
    for side, word in args.wall_velocity:
        if side not in WALL_SIDES:
            raise RuntimeError(f"--wall_velocity: unknown side {side!r} (one of {', '.join(WALL_SIDES)})")
        try:
            u = float(word)
        except ValueError:
            u = float("nan")
        if not np.isfinite(u):
            raise RuntimeError(f"--wall_velocity {side}: speed {word} is not a finite number")
        speeds[side] = u
    return speeds


def coriolis_pair(args):
    """(f0, beta) of --coriolis F0 [BETA]"""
    return args.coriolis[0], args.coriolis[1] if len(args.coriolis) == 2 else 0.0


def check_coriolis(args):
    """--coriolis F0 [BETA], before any engine exists"""
    if args.coriolis is None:
        return
    if len(args.coriolis) > 2:
        raise RuntimeError(f"--coriolis takes F0 or F0 BETA ({len(args.coriolis)} values given)")
    for x in args.coriolis:
        if not np.isfinite(x):
            raise RuntimeError(f"--coriolis: {x} is not a finite number")
    if len(args.coriolis) == 2 and args.coriolis[1] != 0 and args.problem == "shear":
        raise RuntimeError("--coriolis: BETA != 0 is not available on the doubly periodic square of --problem shear "
                           "(f0 + beta y jumps at the wrap)")
    if args.problem == "taylorgreen" and args.forcing == "constant":
        raise RuntimeError("--coriolis with --problem taylorgreen needs --forcing exponential (with constant forcing the "
                           "manufactured forcing is not separable)")


def check_drag(args):
    """--drag R and --problem cylinder [--obstacle_drag S] [--stream U], before any engine exists"""
    if args.drag is not None:
        if not np.isfinite(args.drag) or args.drag < 0:
            raise RuntimeError(f"--drag {args.drag} is not a finite number >= 0")
        if args.problem == "taylorgreen" and args.forcing == "constant":
            raise RuntimeError("--drag with --problem taylorgreen needs --forcing exponential (with constant forcing the "
                               "manufactured forcing is not separable)")
        if args.problem == "taylorgreen" and args.coriolis is not None:
            raise RuntimeError("--drag with --coriolis: the manufactured forcing of --problem taylorgreen covers one of the two")
    if args.problem != "cylinder":
        for name in ("obstacle_drag", "stream"):
            if getattr(args, name) is not None:
                raise RuntimeError(f"--{name} needs --problem cylinder")
        return
    if args.viscosity is None or not args.viscosity > 0:
        raise RuntimeError("--problem cylinder needs --viscosity NU > 0 (the wake of a penalised body needs a viscous scale)")
    if args.discretisation == "dg":
        raise RuntimeError("--problem cylinder runs on the doubly periodic square, which the DG discretisation does not have")
    if args.tracer_wall or args.wall_velocity or args.wall == "no_slip":
        raise RuntimeError("--problem cylinder: the doubly periodic square has no walls")
    if args.coriolis is not None and len(args.coriolis) == 2 and args.coriolis[1] != 0:
        raise RuntimeError("--coriolis: BETA != 0 is not available on the doubly periodic square of --problem cylinder")
    if args.obstacle_drag is not None and (not np.isfinite(args.obstacle_drag) or args.obstacle_drag <= 0):
        raise RuntimeError(f"--obstacle_drag {args.obstacle_drag} is not a finite number > 0")
    if args.stream is not None and (not np.isfinite(args.stream) or args.stream == 0):
        raise RuntimeError(f"--stream {args.stream} is not a finite number != 0")


def cylinder_drag(args, timestepper):
    """The CylinderWake of the run and its obstacle_drag.  The default puts (nu Lambda_u + S) dt at half the real-axis limit of
    the explicit tableau; a viscous number that is above half the limit on its own is refused (before the first step)."""
    from .timesteppers.common import explicit_stability_limit

    eng = timestepper._engine
    s = eng.nstages
    limit = explicit_stability_limit(list(eng.cfg.a_expl)[:s * s], list(eng.cfg.b_expl)[:s])
    viscous = eng.viscosity_number()[1]
    if viscous >= 0.5 * limit:
        raise RuntimeError(f"--problem cylinder: the viscous diffusion number {viscous:.6g} alone is above half the stability limit "
                           f"{limit:.6g} of the explicit tableau, which leaves no room for the penalisation; reduce --dt or --viscosity")
    S = args.obstacle_drag if args.obstacle_drag is not None else (0.5 * limit - viscous) / args.dt
    L = 2 * np.pi
    return CylinderWake(timestepper._V_Q, timestepper._V_p, L, L / args.nx, S, stream=1.0 if args.stream is None else args.stream)


def check_checkpoint(args):
    """Refuse a checkpoint request that cannot be served, before any process is started or any engine is built."""
    if args.checkpoint_every is not None:
        if args.checkpoint_every < 1:
            raise RuntimeError(f"--checkpoint_every must be at least 1 (got {args.checkpoint_every})")
        if not args.checkpoint:
            raise RuntimeError("--checkpoint_every needs --checkpoint")
    if not args.restart:
        return
    for bad, what in ((args.warmup, "--warmup (one step from the initial condition)"),
                      (args.test_pressure_solver, "--test_pressure_solver (no time loop)")):
        if bad:
            raise RuntimeError(f"--restart does not go with {what}")
    files = [args.restart] if args.gpus == 1 else [f"{args.restart}.{r}" for r in range(args.gpus)]
    for path in files:
        if not os.path.isfile(path):
            raise RuntimeError(f"--restart: no checkpoint file {path}")


def check_adaptive(args):
    """--cfl and its options, before any process is started or any engine is built: what solve(cfl=...) refuses."""
    if args.cfl is None:
        for name in ("dt_min", "dt_max", "adapt_every", "max_steps"):
            if getattr(args, name) is not None:
                raise RuntimeError(f"--{name} needs --cfl")
        return
    if not (np.isfinite(args.cfl) and args.cfl > 0):
        raise RuntimeError(f"--cfl must be a finite number > 0 (got {args.cfl})")
    if args.adapt_every is not None and args.adapt_every < 1:
        raise RuntimeError(f"--adapt_every must be at least 1 (got {args.adapt_every})")
    if args.max_steps is not None and args.max_steps < 1:
        raise RuntimeError(f"--max_steps must be at least 1 (got {args.max_steps})")
    dt_min, dt_max = args.dt_min or 0.0, args.dt if args.dt_max is None else args.dt_max
    if not (np.isfinite(dt_min) and dt_min >= 0) or not (dt_max > 0) or dt_min > dt_max:
        raise RuntimeError(f"--dt_min and --dt_max must satisfy 0 <= dt_min <= dt_max, dt_max > 0 (got {dt_min}, {dt_max})")
    for bad, what in ((bool(args.checkpoint), "--checkpoint"), (bool(args.restart), "--restart"),
                      (args.test_pressure_solver, "--test_pressure_solver (no time loop)")):
        if bad:
            raise RuntimeError(f"--cfl does not go with {what}" + (": a checkpoint carries the step size of --dt in its fingerprint "
                               "and does not hold the time series of an adaptive run" if what in ("--checkpoint", "--restart") else ""))


def adaptive_keywords(args):
    """The keyword arguments of solve for --cfl and its options"""
    if args.cfl is None:
        return {}
    kw = {"cfl": args.cfl}
    for name in ("dt_min", "dt_max", "adapt_every", "max_steps"):
        if getattr(args, name) is not None:
            kw[name] = getattr(args, name)
    return kw


MAX_START_RATIO = 16  # csrc/hdg_transfer.hpp: MAX_RATIO


def check_start_from(args):
    """Refuse a --start_from request that cannot be served, before any process is started or any engine is built."""
    if not args.start_from:
        for name in ("start_nx", "start_degree", "start_dt"):
            if getattr(args, name) is not None:
                raise RuntimeError(f"--{name} needs --start_from")
        return
    refused = [
        (args.problem == "taylorgreen", "--problem taylorgreen (forcing and exact solution are tied to the absolute time)"),
        (args.problem == "kelvinhelmholtz", "--problem kelvinhelmholtz (general meshes are not transferred)"),
        (args.problem == "cavity", "--problem cavity (the source run is the periodic square's)"),
        (args.gpus > 1, f"--gpus {args.gpus} (the transfer is single-rank)"),
        (bool(args.restart), "--restart (a restart continues its own checkpoint)"),
        (args.warmup, "--warmup (one step from the initial condition)"),
        (args.test_pressure_solver, "--test_pressure_solver (no time loop)"),
    ]
    for bad, what in refused:
        if bad:
            raise RuntimeError(f"--start_from does not go with {what}")
    if not os.path.isfile(args.start_from):
        raise RuntimeError(f"--start_from: no checkpoint file {args.start_from}")
    nx0 = args.nx if args.start_nx is None else args.start_nx
    hi, lo = max(nx0, args.nx), min(nx0, args.nx)
    if lo < 1 or hi % lo != 0 or hi // lo > MAX_START_RATIO:
        raise RuntimeError(f"--start_nx {nx0} and --nx {args.nx} are not nested (one must be r times the other, "
                           f"1 <= r <= {MAX_START_RATIO})")


def tracer_initial(m):
    """Initial field of tracer m: sin(2 pi (m+1) x) sin(2 pi (m+1) y); m = 0 is driver.py:342."""
    return lambda x, y: np.sin(2 * (m + 1) * np.pi * x) * np.sin(2 * (m + 1) * np.pi * y)


def launch_ranks(argv, nranks):
    """Start the ranks as a fresh child process (torch.distributed.run) and wait for it; returns its exit status."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["PYTHONPATH"] = root + os.pathsep + env.get("PYTHONPATH", "")
    import socket

    with socket.socket() as so:  # a free rendezvous port: runs side by side do not meet
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nranks}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), "-m", "incompressibleeulerhdg_amd.driver", *argv]
    return subprocess.call(cmd, env=env)


class _Ranks:
    """This process's place in a --gpus run: rendezvous (gloo), device, transport and the timestepper keyword arguments."""

    def __init__(self, args):
        self.size = args.gpus
        self.rank = 0
        self.dist = None
        self.kwargs = {"device": args.device}
        if self.size == 1:
            return
        import torch
        import torch.distributed as dist

        from .distributed import comm_kwargs, make_comm_token

        self.rank = int(os.environ["RANK"])
        if int(os.environ["WORLD_SIZE"]) != self.size:
            raise RuntimeError(f"WORLD_SIZE {os.environ['WORLD_SIZE']} differs from --gpus {self.size}")
        dist.init_process_group("gloo")
        self.dist = dist
        ndev = max(torch.cuda.device_count(), 1)
        device = (args.device + int(os.environ.get("LOCAL_RANK", self.rank))) % ndev
        devices = [None] * self.size
        dist.all_gather_object(devices, device)
        backend = "rccl" if len(set(devices)) == self.size else "shm"  # RCCL refuses two ranks on one device

        def bcast(obj):
            lst = [obj]
            dist.broadcast_object_list(lst, src=0)
            return lst[0]

        token = make_comm_token(backend, self.rank, bcast)
        self.backend = backend
        self.kwargs = dict(device=device, **comm_kwargs(backend, self.rank, self.size, token))

    def gather(self, functions):
        """Rank 0: the given strip functions as functions on the global mesh (strips concatenate); None elsewhere."""
        if self.size == 1:
            return list(functions)
        mine = [(f.function_space().coordinates, np.asarray(f.dat.data), f.name()) for f in functions]
        got = [None] * self.size if self.rank == 0 else None
        self.dist.gather_object(mine, got, dst=0)
        if self.rank != 0:
            return None
        out = []
        for n, f in enumerate(functions):
            V = f.function_space()
            xy = np.concatenate([g[n][0] for g in got])
            Vg = FunctionSpace(V.mesh(), V.family, V.degree, xy, value_size=V.value_size)
            out.append(Function(Vg, np.concatenate([g[n][1] for g in got]), got[0][n][2]))
        return out

    def close(self):
        if self.dist is not None:
            self.dist.barrier()
            self.dist.destroy_process_group()
            self.dist = None


def report_solver_events(events):
    """Events of the condensed and tentative-velocity solves (hdg_get_solver_events); warns on rounding-floor exits."""
    print("solver events")
    print(40 * "-")
    for name, n in events.items():
        print(f"  {name:<27s} : {n:8d}")
    print()
    if events["cg_floor_exits"] > 0:
        print(f"WARNING: {events['cg_floor_exits']} condensed CG solve(s) ended at the rounding floor, not at the relative "
              "tolerance")
        print()


def write_diagnostics(path, diag):
    """CSV with one row per recorded state (step, t, the nine diagnostics); prints the first and the last row."""
    names = list(DIAGNOSTICS)
    n = len(diag["t"])
    with open(path, "w") as f:
        f.write(",".join(["step", "t"] + names) + "\n")
        for i in range(n):
            f.write(",".join([str(i), repr(float(diag["t"][i]))] + [repr(float(diag[c][i])) for c in names]) + "\n")
    print(f"diagnostics ({n} rows) written to {path}")
    for i in sorted({0, n - 1}):
        print(f"  step {i:6d}  t = {diag['t'][i]:.6g}  " + "  ".join(f"{c} = {diag[c][i]:.6e}" for c in names))
    print()


def read_probe_points(path):
    """Points of a --probes file: one 'x y' per line, '#' starts a comment, blank lines are skipped.  Returns (xy (n, 2),
    the line number of every point)."""
    pts, lines = [], []
    with open(path) as f:
        for lineno, line in enumerate(f, start=1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            fields = line.replace(",", " ").split()
            if len(fields) != 2:
                raise RuntimeError(f"{path}:{lineno}: expected 'x y', got {line!r}")
            pts.append((float(fields[0]), float(fields[1])))
            lines.append(lineno)
    if not pts:
        raise RuntimeError(f"{path}: no points")
    return np.array(pts, dtype=float), lines


def read_points_inside(path, eng, noun):
    """The points of a --probes / --particles file, every one inside the mesh: the first that is not stops the run, before
    its first step, with file:line and what the point is (`noun`)."""
    xy, lines = read_probe_points(path)
    _, located = eng.evaluate_points(xy)  # collective on strips
    if not np.all(located):
        bad = int(np.flatnonzero(~located)[0])
        raise RuntimeError(f"{path}:{lines[bad]}: {noun} ({xy[bad, 0]}, {xy[bad, 1]}) lies outside the mesh")
    return xy


def write_probes(path, probes):
    """CSV with one row per recorded state and point: step, t, point, x, y and the five point values."""
    t, xy = probes["t"], probes["xy"]
    with open(path, "w") as f:
        f.write(",".join(["step", "t", "point", "x", "y"] + list(POINT_COLUMNS)) + "\n")
        for i in range(len(t)):
            for n in range(len(xy)):
                vals = [probes["u"][i, n, 0], probes["u"][i, n, 1], probes["p"][i, n], probes["q"][i, n], probes["omega"][i, n]]
                f.write(",".join([str(i), repr(float(t[i])), str(n), repr(float(xy[n, 0])), repr(float(xy[n, 1]))]
                                 + [repr(float(v)) for v in vals]) + "\n")
    print(f"probes ({len(t)} rows x {len(xy)} points) written to {path}")
    print()


def write_particles(path, particles):
    """npz with t (rows,), xy (rows, n, 2) and the numbers of clamped updates and lost particles."""
    with open(path, "wb") as f:  # np.savez would append .npz to a name without it
        np.savez(f, t=particles["t"], xy=particles["xy"], clamped=particles["clamped"], lost=particles["lost"])
    rows, n = particles["xy"].shape[:2]
    print(f"particles ({rows} rows x {n} particles, {particles['clamped']} clamped updates, {particles['lost']} lost) "
          f"written to {path}")
    print()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    args = build_parser().parse_args(argv)
    if args.discretisation == "conforming":
        raise RuntimeError(f"discretisation '{args.discretisation}' is out of scope of the MI355X hot path")
    check_multi_gpu(args)
    check_streamfunction(args)
    check_particles(args)
    check_tracers(args)
    check_viscosity(args)
    wall_velocity(args)
    check_coriolis(args)
    check_drag(args)
    check_checkpoint(args)
    check_adaptive(args)
    check_start_from(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(argv, args.gpus)  # nothing here has touched the GPU
    ranks = _Ranks(args)
    try:
        # only rank 0 prints: the other ranks run the same (collective) calls with their output discarded
        with contextlib.redirect_stdout(sys.stdout if ranks.rank == 0 else io.StringIO()):
            return _run(args, ranks)
    finally:
        ranks.close()


def make_timestepper(args, ranks, mesh, degree, dt, callbacks):
    """The timestepper the arguments ask for, on the given mesh with the given degree and timestep size."""
    several = {"n_tracers": args.tracers} if args.tracers > 1 else {}
    if args.tracer_diffusivity is not None:
        kappa = args.tracer_diffusivity
        several["tracer_diffusivity"] = kappa[0] if len(kappa) == 1 else kappa
        if args.tracer_diffusion == "implicit":
            several["tracer_diffusion"] = "implicit"
    if args.tracer_wall:
        several["tracer_walls"] = tracer_walls(args)
    if args.buoyancy is not None:
        several["buoyancy"] = args.buoyancy[0] if len(args.buoyancy) == 1 else args.buoyancy
        several["gravity"] = tuple(args.gravity) if args.gravity is not None else (0.0, -1.0)
    if args.viscosity is not None:
        several["viscosity"] = args.viscosity
        several["wall"] = args.wall or "free_slip"
    if args.wall_velocity:
        several["wall_velocity"] = wall_velocity(args)
    if args.coriolis is not None:
        several["coriolis"] = coriolis_pair(args)
    if args.drag is not None and args.problem != "cylinder":  # the wake sets its own field once Lambda_u is known
        several["drag"] = args.drag
    if args.discretisation == "dg":
        # driver.py:203-213
        assert not args.use_projection_method, "Can not use projection method with DG discretsation"
        if args.timestepper != "implicit":
            raise RuntimeError(f"Invalid timestepping method for DG discretisation: '{args.timestepper}'")
        return IncompressibleEulerDGImplicit(mesh, degree, dt, flux=args.flux, callbacks=callbacks, device=args.device, **several)
    if args.timestepper == "implicit":
        return IncompressibleEulerHDGImplicit(  # driver.py:220-228 (passes n_richardson: SURVEY C-1)
            mesh, degree, dt, flux=args.flux, use_projection_method=args.use_projection_method,
            n_richardson=args.richardson, callbacks=callbacks, **ranks.kwargs, **several)
    if args.timestepper in TIMESTEPPERS:
        return TIMESTEPPERS[args.timestepper](
            mesh, degree, dt, flux=args.flux, use_projection_method=args.use_projection_method,
            n_richardson=args.richardson, callbacks=callbacks, **ranks.kwargs, **several)
    raise RuntimeError(f"Invalid timestepping method for HDG discretisation: '{args.timestepper}'")


def start_from(args, ranks, timestepper):
    """--start_from: (Q, p, q) on the run's spaces from the checkpoint of a run of another mesh size and degree.  A second
    timestepper with the start values (otherwise the run's arguments) loads the file, its state is transferred on the device,
    and it is closed again."""
    nx0 = args.nx if args.start_nx is None else args.start_nx
    k0 = args.degree if args.start_degree is None else args.start_degree
    dt0 = args.dt if args.start_dt is None else args.start_dt
    mesh0 = PeriodicSquareMesh(nx0, nx0, L=2 * np.pi, quadrilateral=False)
    source = make_timestepper(args, ranks, mesh0, k0, dt0, None)
    try:
        with open(args.start_from, "rb") as f:
            _, t0 = source._engine.load_checkpoint(f.read())
        fields = timestepper.state_from(source)
    finally:
        source._engine.close()
    print(f"start: transferred nx = {nx0}, degree = {k0}, t = {t0!r} -> nx = {args.nx}, degree = {args.degree}")
    print()
    return fields


def _run(args, ranks):
    callbacks = None
    if args.animation:  # driver.py:187
        callbacks = [AnimationCallback("evolution.pvd", streamfunction=True) if args.streamfunction else AnimationCallback("evolution.pvd")]
    if args.problem in ("shear", "cylinder"):
        mesh = PeriodicSquareMesh(args.nx, args.nx, L=2 * np.pi, quadrilateral=False)  # driver.py:182-183
    elif args.problem == "kelvinhelmholtz":
        mesh = UnitDiskMesh(refinement_level=args.refinement)  # driver.py:184-185
    else:
        mesh = UnitSquareMesh(args.nx, args.nx, quadrilateral=False)  # driver.py:181
    timestepper = make_timestepper(args, ranks, mesh, args.degree, args.dt, callbacks)
    wake = None
    if args.problem == "cylinder":
        wake = cylinder_drag(args, timestepper)
        r = args.drag or 0.0
        timestepper.set_drag((lambda x, y: wake.sigma(x, y) + r) if r else wake.sigma, wake.target, wake.region)

    print("+-------------------------------------------------+")
    print("! timesteppers for incompressible Euler equations !")
    print("+-------------------------------------------------+")
    print()
    print(f"model problem = {args.problem}")
    if args.problem == "kelvinhelmholtz":
        print(f"refinement level = {args.refinement}")
    else:
        print(f"mesh size = {args.nx} x {args.nx}")
    print(f"forcing = {args.forcing}")
    print(f"kappa = {args.kappa}")
    print(f"polynomial degree = {args.degree}")
    print(f"final time = {args.tfinal}")
    print(f"timestep size = {args.dt}")
    print(f"discretisation = {args.discretisation}")
    print(f"numerical flux = {args.flux}")
    print(f"number of Richardson iterations = {args.richardson}")
    print(f"use projection method = {args.use_projection_method}")
    print(f"advect tracer = {args.tracer_advection}")
    if args.tracers > 1:
        print(f"number of tracers = {args.tracers}")
    if args.tracer_diffusivity is not None:
        print(f"tracer diffusivity = {' '.join(repr(x) for x in args.tracer_diffusivity)}")
        if args.tracer_diffusion == "implicit":
            print("tracer diffusion = implicit")
            print(f"tracer diffusion number = {timestepper._engine.tracer_diffusion_number()[1]:.6g}")
        else:
            print(f"tracer diffusion number = {timestepper._engine.tracer_diffusion_number()[1]:.6g} (limit {timestepper.diffusion_limit:.6g})")
    if args.tracer_wall:
        for t, w in enumerate(timestepper._engine.tracer_walls() or []):
            print(f"tracer wall = tracer {t}: " + (", ".join(f"{side} {value!r}" for side, value in w.items()) or "no flux"))
    if args.viscosity is not None:
        print(f"viscosity = {args.viscosity!r}")
        print(f"wall = {args.wall or 'free_slip'}")
        print(f"viscous diffusion number = {timestepper._engine.viscosity_number()[1]:.6g} (limit {timestepper.viscosity_limit:.6g})")
    if args.wall_velocity:
        print("wall velocity = " + ", ".join(f"{side} {float(u)!r}" for side, u in zip(WALL_SIDES, timestepper._engine.wall_velocity()) if u != 0.0))
    if args.coriolis is not None:
        number = timestepper._engine.coriolis_number()[1]
        print(f"coriolis = {' '.join(repr(x) for x in args.coriolis)}")
        print(f"rotation number F dt = {number:.6g} (growth per inertial period "
              f"{(timestepper.rotation_growth * 2 * np.pi / number if number > 0 else 0.0):.6g})")
    if args.drag is not None:
        print(f"drag = {args.drag!r}")
    if wake is not None:
        print(f"obstacle drag = {wake.S!r}")
        print(f"stream = {wake.U!r}")
    if args.drag is not None or wake is not None:
        S, number = timestepper._engine.drag_number()
        print(f"drag: S = {S:.6g}, S dt = {number:.6g}")
    print(f"timestepping method = {timestepper.label}")
    print()

    eng = timestepper._engine
    if args.test_pressure_solver:
        # working equivalent of driver.py:308-324 (the reference's call is stale, SURVEY C-4): random
        # velocity-row right-hand side with seed 123456789, untimed first solve, timed second solve
        if args.timestepper == "implicit" or args.discretisation == "dg":
            raise RuntimeError("--test_pressure_solver needs an IMEX timestepper")
        rng = np.random.default_rng(123456789)
        f_Q = rng.standard_normal(eng.shape_Q)
        print("=== Testing pressure solver")
        print()
        eng.set_field(0, Q=f_Q, p=np.zeros(eng.shape_p), lam=np.zeros(eng.shape_l))
        for i in range(eng.nstages + 1):
            eng.set_forcing_scale(i, 0.0)
        eng.begin_step()
        for i in range(1, eng.nstages):  # stage iterates := the same random field, so r^{n+1} = (f_Q, w)
            eng.set_field(i, Q=f_Q)
        _ = timestepper.pressure_solve("final_stage")
        eng.set_field(0, lam=np.zeros(eng.shape_l))
        t_start = time.perf_counter()
        its = timestepper.pressure_solve("final_stage")
        t_finish = time.perf_counter()
        print(f"    solve time           = {t_finish-t_start:12.4f} s")
        print(f"    number of iterations = {its}")
        return 0

    if args.warmup:
        print("WARNING: performing a single timestep only!")
        print()
    if args.problem == "shear":
        model_problem = DoubleLayerShearFlow(timestepper._V_Q, timestepper._V_p)  # driver.py:334-335
    elif args.problem == "kelvinhelmholtz":
        model_problem = KelvinHelmholtz(timestepper._V_Q, timestepper._V_p)  # driver.py:336-337
    elif args.problem == "cavity":
        model_problem = Cavity(timestepper._V_Q, timestepper._V_p)
    elif args.problem == "cylinder":
        model_problem = wake
    elif args.drag is not None:
        model_problem = DraggedTaylorGreen(timestepper._V_Q, timestepper._V_p, args.forcing, args.kappa,
                                           viscosity=args.viscosity or 0.0, drag=args.drag)
    else:
        if args.coriolis is not None:
            model_problem = RotatingTaylorGreen(timestepper._V_Q, timestepper._V_p, args.forcing, args.kappa,
                                                viscosity=args.viscosity or 0.0, coriolis=coriolis_pair(args))
        else:
            model_problem = TaylorGreen(timestepper._V_Q, timestepper._V_p, args.forcing, args.kappa, viscosity=args.viscosity or 0.0)
    Q_0, p_0 = model_problem.initial_condition()
    # driver.py:340-344
    q_0 = (lambda x, y: np.sin(2 * np.pi * x) * np.sin(2 * np.pi * y)) if args.tracer_advection else None
    if args.tracers > 1:
        q_0 = [tracer_initial(m) for m in range(args.tracers)]
    if args.problem == "cavity" and args.tracer_advection:  # every tracer starts from 0: the walls set it going
        zero = lambda x, y: 0.0 * x
        q_0 = [zero] * args.tracers if args.tracers > 1 else zero
    if args.start_from:
        Q_0, p_0, q_start = start_from(args, ranks, timestepper)
        if args.tracer_advection and q_start is not None:
            q_0 = q_start
    if args.buoyancy is not None:
        # the mean force of the initial state, sum_t beta_t mean(q_t) g: on the periodic square a uniform acceleration
        beta = args.buoyancy * (args.tracers if len(args.buoyancy) == 1 else 1)
        grav = args.gravity if args.gravity is not None else [0.0, -1.0]
        V_q = timestepper._V_q
        fields = q_0 if isinstance(q_0, (list, tuple)) else [q_0]
        mean = sum(b * nodal_mean(V_q.coordinates, V_q.degree, timestepper._as_nodal_pressure(q)) for b, q in zip(beta, fields))
        print(f"buoyancy = {' '.join(repr(x) for x in args.buoyancy)}")
        print(f"gravity = {' '.join(repr(float(x)) for x in grav)}")
        print(f"buoyancy mean force = {mean * grav[0]:.6g} {mean * grav[1]:.6g}")
        print()
    kw = {"fused": True} if (args.fused and args.timestepper != "implicit") else {}
    if args.diagnostics:
        kw["diagnostics"] = True
    if args.probes:
        kw["probes"] = read_points_inside(args.probes, eng, "probe point")
    if args.particles:
        kw["particles"] = read_points_inside(args.particles, eng, "particle seed")
        kw["particle_every"] = args.particle_every
    if args.checkpoint:
        kw["checkpoint"], kw["checkpoint_every"] = args.checkpoint, args.checkpoint_every or 0
    if args.restart:
        kw["restart"] = args.restart
    kw.update(adaptive_keywords(args))
    Q, p = timestepper.solve(Q_0, p_0, q_0, model_problem.f_rhs(), args.tfinal, warmup=args.warmup, **kw)
    state_digest = eng.state_digest()  # of this rank's strip
    if timestepper.step_sizes is not None:  # --cfl (not with --warmup, whose one step is --dt)
        dts = timestepper.step_sizes[:, 1]
        print(f"steps = {len(dts)}, dt in [{float(dts.min())!r}, {float(dts.max())!r}], last dt = {float(dts[-1])!r}" if len(dts) else "steps = 0")
        print()
    if args.diagnostics:
        report_solver_events(eng.solver_events())
        if ranks.rank == 0:
            write_diagnostics(args.diagnostics, timestepper.diagnostics)
    if args.probes and ranks.rank == 0:
        write_probes(args.probe_output, timestepper.probes)
    if args.particles and ranks.rank == 0:
        write_particles(args.particle_output, timestepper.particles)
    if args.tracers > 1:
        for q in timestepper.q_tracers:
            integral = eng.integrate_pressure(q.dat.data)
            half_sq = timestepper.compute_diagnostics(Q, p, q)["tracer_half_sq"]
            print(f"{q.name()}: integral = {integral!r}, half square integral = {half_sq!r}")
        print()
    if args.tracer_diffusion == "implicit":
        rows = np.asarray(timestepper.tracer_diffusion_iterations or [np.zeros(args.tracers)], dtype=float)
        print("tracer diffusion iterations per solve (mean) = " + " ".join(f"{x:.1f}" for x in rows.mean(axis=0)))
        print()
    if args.tracer_wall:
        sides = ("boundary",) if args.problem == "kelvinhelmholtz" else WALL_SIDES
        for t, row in enumerate(eng.tracer_wall_flux()):
            print(f"tracer wall flux = tracer {t}: " + ", ".join(f"{side} {float(row[w])!r}" for w, side in enumerate(sides)))
        print()
    if args.wall_velocity:
        for side, row in zip(WALL_SIDES, eng.wall_force()):
            print(f"wall force {side} = {float(row[0])!r} {float(row[1])!r}")
        print()
    if wake is not None:  # the force on the body is the negative of the term's force on the fluid of region 1
        force = eng.drag_force()[1]
        cd, cl = wake.coefficients(force)
        print(f"disc: force on the body = {float(-force[0])!r} {float(-force[1])!r}, C_D = {float(cd)!r}, C_L = {float(cl)!r}")
        print()
    if args.streamfunction:
        report_streamfunction(timestepper)
    log_summary()
    print(f"state digest = {state_digest[0]:016x}{state_digest[1]:016x}")
    print()
    if args.problem in ("shear", "kelvinhelmholtz", "cavity", "cylinder"):
        # no exact solution (the reference's driver calls model_problem.solution, which these problems lack: it stops here
        # with an AttributeError); write the final fields
        if args.output:
            Q.rename("velocity")
            p.rename("pressure")
            divQ = Function(timestepper._V_p, eng.apply_weak_divergence(Q.dat.data, broken=True), "divergence")
            fields = ranks.gather([Q, p, divQ])
            if fields is not None:
                VTKFile(args.output).write(*fields)
        return 0
    if not args.warmup:
        Q.rename("velocity")
        p.rename("pressure")
        Q_exact, p_exact = model_problem.solution(args.tfinal, eng.integrate_pressure)
        Q_error = Function(timestepper._V_Q, Q.dat.data - Q_exact.dat.data, "velocity_error")
        p_error = Function(timestepper._V_p, p.dat.data - p_exact.dat.data, "pressure_error")
        Q_error_nrm, p_error_nrm = eng.l2_norms(Q_error.dat.data, p_error.dat.data)  # driver.py:376-377
        print()
        print(f"velocity error = {Q_error_nrm}")
        print(f"pressure error = {p_error_nrm}")
        print()
        if args.output:
            # driver.py:356-385: L2 projection of the (broken) divergence onto the pressure space, then
            # velocity, pressure, divergence, exact fields and errors into solution.pvd
            divQ = Function(timestepper._V_p, eng.apply_weak_divergence(Q.dat.data, broken=True), "divergence")
            Q_exact.rename("velocity_exact")
            p_exact.rename("pressure_exact")
            fields = ranks.gather([Q, p, divQ, Q_exact, Q_error, p_exact, p_error])
            if fields is not None:
                VTKFile(args.output).write(*fields)
    return 0


if __name__ == "__main__":
    sys.exit(main())
