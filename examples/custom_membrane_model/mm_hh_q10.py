"""A membrane model that is not one of the built-in device models: Hodgkin-Huxley kinetics with Q10 temperature scaling of the
gate rates, plus a persistent (non-inactivating) Na current, with the leak, Na/K pump and synaptic stimulus of the idealized
examples' mm_hh.  SI units (V, s, S/m^2, mol/m^3), same state / parameter names as mm_hh for everything the solver exchanges
(V, E_*, K_e, Na_i, I_ch_*, Cm, stim_amplitude), so it drops into any idealized-geometry run.

It carries its right-hand side twice: `rhs` (numpy, all rows at once) for the host integrator, and `HIP_RHS` (C++, one row)
which the device integrator compiles at run time (knpemidg/ode_rtc.py).  Both state the same formulas."""
import numpy as np

STATE_IND = dict(m=0, h=1, n=2, V=3)
PARAM_IND = dict(g_Na_bar=0, g_K_bar=1, g_leak_Na=2, g_leak_K=3, E_Na=4, E_K=5, Cm=6, stim_amplitude=7,
                 I_ch_Na=8, I_ch_K=9, I_ch_Cl=10, K_e=11, Na_i=12, m_K=13, m_Na=14, I_max=15, E_Cl=16,
                 g_NaP=17, temperature=18, T_ref=19, Q10=20)


def init_state_values(**values):
    init = np.array([0.016648440745822956, 0.8542015627820805, 0.1882020248041632, -0.07438609374462003])
    for name, value in values.items():
        if name not in STATE_IND:
            raise ValueError("{0} is not a state.".format(name))
        init[STATE_IND[name]] = value
    return init


def init_parameter_values(**values):
    init = np.zeros(len(PARAM_IND))
    init[[0, 1, 2, 3]] = [1200.0, 360.0, 2.0 * 0.5, 8.0 * 0.5]       # conductances as mm_hh
    init[[13, 14, 15]] = [2.0, 7.7, 0.449]                            # pump m_K, m_Na, I_max
    init[[17, 18, 19, 20]] = [2.0, 9.3, 6.3, 3.0]                     # g_NaP [S/m^2], T [deg C], T_ref [deg C], Q10
    for name, value in values.items():
        if name not in PARAM_IND:
            raise ValueError("{0} is not a parameter.".format(name))
        init[PARAM_IND[name]] = value
    return init


def _indices(table, what, names):
    out = []
    for n in names:
        if n not in table:
            raise ValueError("Unknown {0}: '{1}'".format(what, n))
        out.append(table[n])
    return out if len(out) > 1 else out[0]


def state_indices(*states):
    return _indices(STATE_IND, "state", states)


def parameter_indices(*params):
    return _indices(PARAM_IND, "param", params)


def rhs(t, states, parameters):
    m, h, n, V = states[:, 0], states[:, 1], states[:, 2], states[:, 3]
    p = parameters
    phi = p[:, 20] ** ((p[:, 18] - p[:, 19]) / 10.0)                # Q10 factor of every gate rate
    u = 1.0e3 * (V + 65.0e-3)
    values = np.empty_like(states)
    alpha_m = 0.1e3 * (25.0 - u) / (np.exp((25.0 - u) / 10.0) - 1.0)
    beta_m = 4.0e3 * np.exp(-u / 18.0)
    values[:, 0] = phi * ((1 - m) * alpha_m - m * beta_m)
    alpha_h = 0.07e3 * np.exp(-u / 20.0)
    beta_h = 1.0e3 / (np.exp((30.0 - u) / 10.0) + 1.0)
    values[:, 1] = phi * ((1 - h) * alpha_h - h * beta_h)
    alpha_n = 0.01e3 * (10.0 - u) / (np.exp((10.0 - u) / 10.0) - 1.0)
    beta_n = 0.125e3 * np.exp(-u / 80.0)
    values[:, 2] = phi * ((1 - n) * alpha_n - n * beta_n)
    m_p = 1.0 / (1.0 + np.exp(-(1.0e3 * V + 52.0) / 5.0))          # persistent Na activation, instantaneous
    i_pump = p[:, 15] / ((1 + p[:, 13] / p[:, 11]) ** 2 * (1 + p[:, 14] / p[:, 12]) ** 3)
    g_stim = p[:, 7] * np.exp(-np.mod(t, 0.03) / 0.002) * (t < 125e-3)
    i_Na = (p[:, 2] + p[:, 0] * h * m ** 3 + p[:, 17] * m_p + g_stim) * (V - p[:, 4]) + 3 * i_pump
    i_K = (p[:, 3] + p[:, 1] * n ** 4) * (V - p[:, 5]) - 2 * i_pump
    p[:, 8] = i_Na
    p[:, 9] = i_K
    p[:, 10] = 0.0
    values[:, 3] = (-i_K - i_Na) / p[:, 6]
    return values


HIP_RHS = r"""
const double m = y[S_m], h = y[S_h], n = y[S_n], V = y[S_V];
const double phi = pow(p[P_Q10], (p[P_temperature] - p[P_T_ref]) / 10.0);
const double u = 1.0e3 * (V + 65.0e-3);
const double alpha_m = 0.1e3 * (25.0 - u) / (exp((25.0 - u) / 10.0) - 1.0);
const double beta_m = 4.0e3 * exp(-u / 18.0);
dy[S_m] = phi * ((1 - m) * alpha_m - m * beta_m);
const double alpha_h = 0.07e3 * exp(-u / 20.0);
const double beta_h = 1.0e3 / (exp((30.0 - u) / 10.0) + 1.0);
dy[S_h] = phi * ((1 - h) * alpha_h - h * beta_h);
const double alpha_n = 0.01e3 * (10.0 - u) / (exp((10.0 - u) / 10.0) - 1.0);
const double beta_n = 0.125e3 * exp(-u / 80.0);
dy[S_n] = phi * ((1 - n) * alpha_n - n * beta_n);
const double m_p = 1.0 / (1.0 + exp(-(1.0e3 * V + 52.0) / 5.0));
const double a = 1 + p[P_m_K] / p[P_K_e], b = 1 + p[P_m_Na] / p[P_Na_i];
const double i_pump = p[P_I_max] / (a * a * b * b * b);
const double g_stim = (t < 125e-3) ? p[P_stim_amplitude] * exp(-fmod(t, 0.03) / 0.002) : 0.0;
const double i_Na = (p[P_g_leak_Na] + p[P_g_Na_bar] * h * m * m * m + p[P_g_NaP] * m_p + g_stim) * (V - p[P_E_Na]) + 3 * i_pump;
const double n2 = n * n;
const double i_K = (p[P_g_leak_K] + p[P_g_K_bar] * n2 * n2) * (V - p[P_E_K]) - 2 * i_pump;
p[P_I_ch_Na] = i_Na;
p[P_I_ch_K] = i_K;
p[P_I_ch_Cl] = 0.0;
dy[S_V] = (-i_K - i_Na) / p[P_Cm];
"""
