"""Stiff test problems for the extrapolated linearly implicit Euler integrator (csrc/ode_stiff.hpp, membrane.integrate_batch_stiff):
the fast-gate Hodgkin-Huxley membrane of examples/custom_membrane_model/mm_hh_fastgate.py in the project's SI units, Robertson's
chemical kinetics and the Prothero-Robinson problem, each with a numpy `rhs` in the vectorised module protocol; the two that run on
the device carry HIP_RHS as well.  Also the reference solutions (scipy's Radau at rtol 1e-12) the tests compare against."""
import hashlib
import os
import sys

import numpy as np

import rtc_models

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EX = os.path.join(ROOT, "examples", "custom_membrane_model")
if _EX not in sys.path:
    sys.path.insert(0, _EX)

import mm_hh_fastgate as fastgate                     # noqa: E402

# the membrane's surroundings as the idealized examples initialise them (examples/idealized_geometries/idealized_common.py)
HH_ENV = dict(Cm=0.02, K_e=3.3236967382705265, Na_i=12.838513108648856, E_K=-0.0936, E_Na=0.0533)
WINDOW = 1.0e-4                                       # [s] = 0.1 ms, the PDE time step of the idealized examples
STIM = 40.0                                           # stim_amplitude while the stimulus is on [S/m^2]


def hh_rows(ode, n_rows=8, seed=5, **fixed):
    """(states, parameters) of n_rows distinct membrane nodes of an HH-type model module: initial potentials, gates and surroundings
    spread around the resting state."""
    rng = np.random.default_rng(seed)
    s = np.tile(np.asarray(ode.init_state_values(), dtype=np.float64), (n_rows, 1))
    p = np.tile(np.asarray(ode.init_parameter_values(**dict(HH_ENV, **fixed)), dtype=np.float64), (n_rows, 1))
    s[:, ode.state_indices("V")] += 4e-3 * rng.uniform(-1, 1, n_rows)
    for g in ("m", "h", "n"):
        s[:, ode.state_indices(g)] *= 1 + 0.05 * rng.uniform(-1, 1, n_rows)
    for name, spread in (("K_e", 0.1), ("Na_i", 0.1), ("E_K", 0.02), ("E_Na", 0.02), ("g_Na_bar", 0.05)):
        p[:, ode.parameter_indices(name)] *= 1 + spread * rng.uniform(-1, 1, n_rows)
    return s, p


def stim_schedule(k, first_on=10):
    """stim_amplitude of window k: off until window `first_on`, on from there (the switch sits on a window boundary)."""
    return STIM if k >= first_on else 0.0


_radau_memo = {}
# Radau solutions recorded for the inputs the tests use (2 s per row otherwise), keyed by a hash of everything that goes in;
# `python tests/stiff_models.py` solves them again and rewrites the file.  Other inputs are solved on the spot.
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ode_stiff_radau.npz")
_recorded = None


def radau_windows(ode, s0, p0, windows, stim_rows=None, dt=WINDOW, first_on=10):
    """States [rows, ns] after `windows` windows and the per-state maximum of |y| along the trajectory, from scipy's Radau at
    rtol 1e-12 / atol 1e-14, one row at a time, the stimulus parameter switched where the integrators under test switch it.
    Memoised per process (read-only arrays), and read from tests/golden/ode_stiff_radau.npz where these very inputs were solved before."""
    from scipy.integrate import solve_ivp
    n = s0.shape[0]
    stim_rows = np.ones(n, dtype=bool) if stim_rows is None else np.asarray(stim_rows, dtype=bool)
    key = hashlib.sha256(repr((ode.__name__.rsplit(".", 1)[-1], s0.tobytes(), p0.tobytes(), windows, stim_rows.tobytes(), dt,
                               first_on)).encode()).hexdigest()[:16]
    if key in _radau_memo:
        return _radau_memo[key]
    if _recorded is None and os.path.exists(GOLDEN):
        with np.load(GOLDEN) as z:
            globals()["_recorded"] = {name: z[name] for name in z.files}
    if _recorded and key + "_y" in _recorded:              # solved before for exactly these inputs
        out, ymax = _recorded[key + "_y"], _recorded[key + "_max"]
        out.setflags(write=False)
        ymax.setflags(write=False)
        _radau_memo[key] = (out, ymax)
        return out, ymax
    out = np.empty_like(s0)
    ymax = np.abs(s0).copy()
    col = ode.parameter_indices("stim_amplitude")
    for i in range(n):
        y = s0[i].copy()
        p = p0[i:i + 1].copy()
        amps = [stim_schedule(k, first_on) if stim_rows[i] else p[0, col] for k in range(windows)]
        edges = [0] + [k for k in range(1, windows) if amps[k] != amps[k - 1]] + [windows]
        for k0, k1 in zip(edges[:-1], edges[1:]):         # one solve per stretch of windows with the same stimulus: the right-hand
            p[0, col] = amps[k0]                           # side is smooth inside it, so the windows need no restart

            def fun(t, Y):                                 # vectorised: Radau's difference Jacobian costs one call
                return ode.rhs(np.full(Y.shape[1], t), Y.T, np.repeat(p, Y.shape[1], axis=0)).T
            sol = solve_ivp(fun, (k0 * dt, k1 * dt), y, method="Radau", rtol=1e-12, atol=1e-14, vectorized=True)
            assert sol.success
            y = sol.y[:, -1]
            ymax[i] = np.maximum(ymax[i], np.abs(sol.y).max(axis=1))
        out[i] = y
    out.setflags(write=False)
    ymax.setflags(write=False)
    _radau_memo[key] = (out, ymax)
    return out, ymax


# --- Robertson's problem (Hairer & Wanner, Solving ODEs II, section IV.1): three species, rate constants 0.04, 3e7, 1e4
ROBERTSON_BODY = r"""
const double r1 = p[P_k1] * y[S_a], r2 = p[P_k2] * y[S_b] * y[S_b], r3 = p[P_k3] * y[S_b] * y[S_c];
dy[S_a] = -r1 + r3;
dy[S_b] = r1 - r3 - r2;
dy[S_c] = r2;
"""


def robertson_rhs(t, states, parameters):
    a, b, c = states[:, 0], states[:, 1], states[:, 2]
    p = parameters
    r1, r2, r3 = p[:, 0] * a, p[:, 1] * b * b, p[:, 2] * b * c
    out = np.empty_like(states)
    out[:, 0] = -r1 + r3
    out[:, 1] = r1 - r3 - r2
    out[:, 2] = r2
    return out


def robertson():
    return rtc_models.make_model("mm_robertson", ROBERTSON_BODY, states=("a", "b", "c"), params=("k1", "k2", "k3"),
                                 s0=[1.0, 0.0, 0.0], p0=[0.04, 3.0e7, 1.0e4], rhs=robertson_rhs)


# --- Prothero-Robinson: y' = lambda (y - cos t) - sin t, y(0) = 1; the solution is cos t whatever lambda is
def prothero_robinson_rhs(t, states, parameters):
    return parameters[:, :1] * (states - np.cos(t)[:, None]) - np.sin(t)[:, None]


# --- smooth non-stiff problems with known solutions, for the order measurement: the plane rotation  y1' = -y2, y2' = y1  ->
# (cos t, sin t), and a nonlinear non-autonomous system built around the same solution
def rotation_rhs(t, states, parameters):
    return np.stack([-states[:, 1], states[:, 0]], axis=1)


def smooth_rhs(t, states, parameters):
    y1, y2 = states[:, 0], states[:, 1]
    out = np.empty_like(states)
    e2 = y2 - np.sin(t)
    out[:, 0] = -(y1 - np.cos(t)) - np.sin(t) + e2 * e2 + y1 * e2
    out[:, 1] = -e2 + np.cos(t) - 0.5 * (y1 - np.cos(t)) * y2
    return out


def reference_inputs():
    """(ode, s0, p0, windows, stim_rows, first_on) of every Radau reference the tests ask for."""
    from knpemidg.models import mm_hh
    every_third = np.arange(8) % 3 == 0
    cases = [(fastgate,) + hh_rows(fastgate, 1, tau_q=tau) + (50, None, 10) for tau in (1e-7, 1e-9)]
    cases.append((fastgate,) + hh_rows(fastgate, 8, tau_q=1e-9) + (20, every_third, 5))
    cases.append((mm_hh,) + hh_rows(mm_hh, 8) + (20, every_third, 5))
    return cases


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(ROOT, "knp-emi-dg_amd"))
    _recorded = {}                                         # solve, do not read
    rec = {}
    for ode, s0, p0, windows, rows, first_on in reference_inputs():
        y, ymax = radau_windows(ode, s0, p0, windows, stim_rows=rows, first_on=first_on)
        key = [k for k, v in _radau_memo.items() if v[0] is y][0]
        rec[key + "_y"], rec[key + "_max"] = y, ymax
    np.savez(GOLDEN, **rec)
    print("wrote %s: %d references" % (GOLDEN, len(rec) // 2))
