"""Reference of the adaptive time step: the numpy twin of the rule of csrc/hdg_step_control.hpp, and
reference loops that run the oracle's existing steppers through a given list of step sizes -- one oracle stepper per distinct
dt, the state handed on.  Nothing here touches the GPU."""
import numpy as np

DEFAULTS = {"dt_min": 0.0, "dt_max": np.inf, "grow": 1.25, "band": 0.1}
INF = float("inf")


def propose(A, dt, t, t_final, cfl, dt_min=0.0, dt_max=0.0, grow=0.0, band=0.0, caps=(0.0, 0.0, 0.0)):
    """(verdict, p) of the rule: one IEEE double operation per statement, in the order of the header.  A zero means the default.
    Every number passes through np.float64, so nothing is evaluated in another precision."""
    f = np.float64
    A, dt, t, t_final, cfl, dt_min, dt_max, grow, band = (f(x) for x in (A, dt, t, t_final, cfl, dt_min, dt_max, grow, band))
    caps = [f(c) for c in caps]
    ok = cfl > 0 and dt_min >= 0 and dt_max >= 0 and grow >= 0 and band >= 0 and all(c >= 0 for c in caps)
    if not ok:
        return "bad_control", f("nan")
    if not (A >= 0) or A == INF:
        return "not_finite", f("nan")
    dt_max = f(INF) if dt_max == 0 else dt_max
    grow = f(1.25) if grow == 0 else grow
    band = f(0.1) if band == 0 else band
    caps = [f(INF) if c == 0 else c for c in caps]
    with np.errstate(over="ignore", divide="ignore"):
        q = f(INF) if A == 0 else cfl / A
        p = dt_max
        for x in caps + [q]:
            p = x if x < p else p
        g = grow * dt
        p = g if g < p else p
        b1 = f(1.0) + band
        hi = b1 * dt
        if dt <= p and p <= hi:
            p = dt
        rem = t_final - t
        if p >= rem:
            p = rem
        elif p < dt_min:
            return "below_min", p
    return "ok", p


def replay(rates, dt0, t_final, every=1, **control):
    """The dt of every step of a controlled run from the rates the controller saw at its decisions (in order): the loop of
    timesteppers/common.py with the twin in the place of the library's rule.  Returns (dt per step, proposals)."""
    f = np.float64
    t, dt, k, dts, props, it = f(0.0), f(dt0), 0, [], [], iter(rates)
    while t_final - t > 1.0e-12 * t_final:
        if k % every == 0:
            verdict, p = propose(next(it), dt, t, t_final, **control)
            assert verdict == "ok", (verdict, t)
            props.append(p)
            dt = p
        dts.append(dt)
        t, k = t + dt, k + 1
    return np.array(dts), np.array(props)


# ---- reference loops: the oracle's steppers fed a list of step sizes
_IMEX_STATE = ("stage_Q", "stage_p", "stage_l", "Qstar", "Q_tent", "b_rhs", "Q", "p", "lam")


def imex_loop(make, dts, Q0, p0, f_rhs, tracer=None, q0=None):
    """make(dt) -> an OracleHDGIMEX; one stepper per distinct dt, every state vector (the persistent stage vectors are the
    start of the Richardson iteration) handed on where dt changes.  Returns the last stepper: .Q, .p, .lam.
    With tracer (an oracle.tracer_oracle.TracerOracle) and q0 a passive tracer is carried along as
    oracle.tracer_oracle.imex_with_tracer carries it, with the dt of each step; the last stepper then has .q too."""
    from oracle.tracer_oracle import _step_with_hook

    steppers, cur, t = {}, None, 0.0
    q = None if q0 is None else q0.copy()
    for dt in dts:
        o = steppers.get(dt)
        if o is None:
            o = steppers[dt] = make(dt)
        if cur is None:
            o.set_initial_condition(Q0, p0)
        elif o is not cur:
            for name in _IMEX_STATE:
                v = getattr(cur, name)
                setattr(o, name, [x.copy() for x in v] if isinstance(v, list) else v.copy())
        cur = o
        if q is None:
            o.step(f_rhs, t)
        else:
            qs = [q.copy()] + [None] * (o.nstages - 1)

            def after_stage(i):
                ui = tracer.cg_project(o.stage_Q[i])
                acc = qs[0].copy()
                for j in range(i):
                    if o.a_expl[i, j] != 0:
                        acc = acc + dt * o.a_expl[i, j] * tracer._lu_mp.solve(tracer.tracer_form(qs[j], ui))
                qs[i] = acc

            _step_with_hook(o, f_rhs, t, after_stage)
            q = qs[0].copy()
            for i in range(o.nstages):
                if o.b_expl[i] != 0:
                    q = q + dt * o.b_expl[i] * tracer._lu_mp.solve(tracer.tracer_form(qs[i], tracer.cg_project(o.stage_Q[i])))
        t = t + dt
    cur.q = q
    return cur


def one_step_loop(step, dts, Q0, p0, f_rhs, tracer=None, q0=None):
    """step(dt, Q, p, f) -> (Q, p) takes ONE step of size dt with the forcing f(t'), t' counted from the start of the step (the
    implicit HDG and DG steppers of the oracle: solve(..., T_final = dt)); the state is handed on.  With tracer and q0 the
    tracer takes a forward Euler step of the same dt with the velocity at the START of the step, as
    oracle.tracer_oracle.implicit_with_tracer and dg_reference.dg_solve do.  Returns (Q, p, q); q None without a tracer."""
    Q, p, t = Q0, p0, 0.0
    q = None if q0 is None else q0.copy()
    for dt in dts:
        dq = dt * tracer.tracer_tendency(q, Q) if q is not None else None
        Q, p = step(dt, Q, p, lambda s, t0=t: f_rhs(t0 + s))
        if q is not None:
            q = q + dq
        t = t + dt
    return Q, p, q
