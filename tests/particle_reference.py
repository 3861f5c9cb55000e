"""CPU checker of Lagrangian particles (helper of the particle tests, not a test module).

Heun's method (include/hdg_mi355x.h: hdg_set_particles) restated in numpy on top of
tests/probe_reference.py, which supplies the ownership rule and the point values of nodal fields:

    k1 = u^n(X^n),  X* = X^n + dt k1,  k2 = u^{n+1}(X*),  X^{n+1} = X^n + dt/2 (k1 + k2)

with every coordinate clamped to [0, L] after each of the two updates on the unit square, and positions left unwrapped on the
periodic square.  The integrator also returns how close each evaluation point came to a cell edge, in units of h: a point
within rounding of an edge may be owned by either neighbour, and the broken velocity jumps there.
"""
import math

import numpy as np

import probe_reference as pr


def edge_margin(xy, nx, L, periodic):
    """Distance of every point (n, 2) to the nearest cell edge (horizontal, vertical, diagonal), in units of h = L / nx."""
    h = L / nx
    out = np.empty(len(xy))
    for t, (x, y) in enumerate(np.asarray(xy, dtype=float)):
        o = pr.owner_square(x, y, nx, nx, L, periodic)
        if o is None:
            out[t] = np.nan
            continue
        i, j, _, xw, yw = o
        fx, fy = xw / h - i, yw / h - j
        out[t] = min(fx, 1.0 - fx, fy, 1.0 - fy, abs(fx + fy - 1.0) / math.sqrt(2.0))
    return out


def clamp(xy, L):
    """(clamped positions, number of particles with a coordinate moved); NaN stays NaN."""
    c = np.where(xy < 0.0, 0.0, np.where(xy > L, L, xy))
    return c, int(np.any(c != xy, axis=1).sum() - np.any(np.isnan(xy), axis=1).sum())


def heun(velocity, xy0, dt, nt, L=None, square=None, frozen=False):
    """Positions (nt + 1, n, 2) of the particles seeded at xy0 over nt steps of size dt, the number of clamped updates and
    the margins (2 nt, n) of the evaluation points X^0, X*^0, X^1, X*^1, ... (NaN without `square`).

    velocity(step, xy) -> (n, 2): the field of flow state `step` (0 .. nt) at the points; frozen: state 0 throughout.
    L: clamp every coordinate to [0, L] after each update (the unit square); square = (nx, L, periodic) for the margins."""
    X = np.array(xy0, dtype=float).reshape(-1, 2)
    rows, margins, nclamp = [X.copy()], [], 0

    def margin(P):
        return edge_margin(P, *square) if square is not None else np.full(len(P), np.nan)

    for n in range(nt):
        margins.append(margin(X))
        k1 = velocity(0 if frozen else n, X)
        Xs = X + dt * k1
        if L is not None:
            Xs, c = clamp(Xs, L)
            nclamp += c
        margins.append(margin(Xs))
        k2 = velocity(0 if frozen else n + 1, Xs)
        X = X + 0.5 * dt * (k1 + k2)
        if L is not None:
            X, c = clamp(X, L)
            nclamp += c
        rows.append(X.copy())
    return np.array(rows), nclamp, np.array(margins).reshape(-1, len(X))


def heun_fields(ev, fields, xy0, dt, frozen=False, nt=None):
    """heun through nodal velocity fields (layout of hdg_set_state) fields[0 .. nt] by the PointEvaluator `ev` of a square
    mesh."""
    nx, _, L, periodic = ev.square

    def velocity(step, xy):
        vals, located = ev.evaluate(xy, Q=fields[step])
        assert located.all(), "a particle left the mesh"
        return vals[:, 0:2]

    nt = len(fields) - 1 if nt is None else nt
    return heun(velocity, xy0, dt, nt, L=None if periodic else L, square=(nx, L, periodic), frozen=frozen)
