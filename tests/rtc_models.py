"""Membrane model modules for the runtime-compiled device path (knpemidg/ode_rtc.py): a FitzHugh-Nagumo-type membrane with
sizes no built-in device model has (2 states, 9 parameters) and a factory for deliberately broken HIP_RHS modules."""
import types

import numpy as np


def make_model(name, body, states=("v", "w"), params=("a", "b", "tau", "Cm", "stim_amplitude", "I_ch_Na", "I_ch_K", "I_ch_Cl", "g"),
               s0=None, p0=None, rhs=None):
    """A model module built in memory: STATE_IND / PARAM_IND from the name lists, HIP_RHS = body."""
    m = types.ModuleType(name)
    m.STATE_IND = {s: i for i, s in enumerate(states)}
    m.PARAM_IND = {q: i for i, q in enumerate(params)}
    s0 = np.zeros(len(states)) if s0 is None else np.asarray(s0, dtype=np.float64)
    p0 = np.ones(len(params)) if p0 is None else np.asarray(p0, dtype=np.float64)
    m.init_state_values = lambda **kw: s0.copy()
    m.init_parameter_values = lambda **kw: p0.copy()
    m.state_indices = lambda *a: [m.STATE_IND[x] for x in a] if len(a) > 1 else m.STATE_IND[a[0]]
    m.parameter_indices = lambda *a: [m.PARAM_IND[x] for x in a] if len(a) > 1 else m.PARAM_IND[a[0]]
    m.HIP_RHS = body
    if rhs is not None:
        m.rhs = rhs
    return m


FHN_BODY = r"""
const double v = y[S_v], w = y[S_w];
const double i_stim = p[P_stim_amplitude] * exp(-t / 2.0);
const double i_Na = p[P_g] * (v * v * v / 3.0 - v) - i_stim;
const double i_K = p[P_g] * w;
p[P_I_ch_Na] = i_Na;
p[P_I_ch_K] = i_K;
p[P_I_ch_Cl] = 0.0;
dy[S_v] = -(i_Na + i_K) / p[P_Cm];
dy[S_w] = (v + p[P_a] - p[P_b] * w) / p[P_tau];
"""


def fhn_rhs(t, states, parameters):
    v, w = states[:, 0], states[:, 1]
    p = parameters
    i_stim = p[:, 4] * np.exp(-t / 2.0)
    i_Na = p[:, 8] * (v * v * v / 3.0 - v) - i_stim
    i_K = p[:, 8] * w
    p[:, 5] = i_Na
    p[:, 6] = i_K
    p[:, 7] = 0.0
    out = np.empty_like(states)
    out[:, 0] = -(i_Na + i_K) / p[:, 3]
    out[:, 1] = (v + p[:, 0] - p[:, 1] * w) / p[:, 2]
    return out


def fhn():
    """FitzHugh-Nagumo membrane in its own dimensionless units, resting near (v, w) = (-1.2, -0.625)."""
    return make_model("mm_fhn", FHN_BODY, s0=[-1.1994, -0.6243], p0=[0.7, 0.8, 12.5, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0], rhs=fhn_rhs)
