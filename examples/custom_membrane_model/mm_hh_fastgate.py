"""A stiff membrane model: the Hodgkin-Huxley membrane of the idealized examples (knpemidg.models.mm_hh) plus a persistent Na
current whose activation gate q relaxes to its steady state with a time constant tau_q far below every other time scale,

    q' = (q_inf(V) - q) / tau_q,    q_inf(V) = 1 / (1 + exp(-(V + 52 mV) / 5 mV)),    I_NaP = g_NaP q (V - E_Na).

SI units (V, s, S/m^2, mol/m^3) and the state / parameter names of mm_hh for everything the solver exchanges.  tau_q is a
parameter [s]; at 1e-7 s and below the explicit Dormand-Prince integrator is held to steps of about 3 tau_q by stability alone, so
the module asks for the stiff integrator (ODE_METHOD; Solver.setup_membrane_model(..., ode_method=) overrides it).

Like every user-written model it carries its right-hand side twice: `rhs` (numpy, all rows at once) for the host integrator and
`HIP_RHS` (C++, one row) for the device integrator (knpemidg/ode_rtc.py)."""
import numpy as np

ODE_METHOD = "stiff"

STATE_IND = dict(m=0, h=1, n=2, V=3, q=4)
PARAM_IND = dict(g_Na_bar=0, g_K_bar=1, g_leak_Na=2, g_leak_K=3, E_Na=4, E_K=5, Cm=6, stim_amplitude=7,
                 I_ch_Na=8, I_ch_K=9, I_ch_Cl=10, K_e=11, Na_i=12, m_K=13, m_Na=14, I_max=15, E_Cl=16,
                 g_NaP=17, tau_q=18)


def _q_inf(V):
    return 1.0 / (1.0 + np.exp(-(1.0e3 * V + 52.0) / 5.0))


def init_state_values(**values):
    V0 = -0.07438609374462003
    init = np.array([0.016648440745822956, 0.8542015627820805, 0.1882020248041632, V0, _q_inf(V0)])
    for name, value in values.items():
        if name not in STATE_IND:
            raise ValueError("{0} is not a state.".format(name))
        init[STATE_IND[name]] = value
    return init


def init_parameter_values(**values):
    init = np.zeros(len(PARAM_IND))
    init[[0, 1, 2, 3]] = [1200.0, 360.0, 2.0 * 0.5, 8.0 * 0.5]       # conductances as mm_hh
    init[[13, 14, 15]] = [2.0, 7.7, 0.449]                            # pump m_K, m_Na, I_max
    init[[17, 18]] = [2.0, 1.0e-9]                                    # g_NaP [S/m^2], tau_q [s]
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
    m, h, n, V, q = states[:, 0], states[:, 1], states[:, 2], states[:, 3], states[:, 4]
    p = parameters
    u = 1.0e3 * (V + 65.0e-3)
    values = np.empty_like(states)
    alpha_m = 0.1e3 * (25.0 - u) / (np.exp((25.0 - u) / 10.0) - 1.0)
    beta_m = 4.0e3 * np.exp(-u / 18.0)
    values[:, 0] = (1 - m) * alpha_m - m * beta_m
    alpha_h = 0.07e3 * np.exp(-u / 20.0)
    beta_h = 1.0e3 / (np.exp((30.0 - u) / 10.0) + 1.0)
    values[:, 1] = (1 - h) * alpha_h - h * beta_h
    alpha_n = 0.01e3 * (10.0 - u) / (np.exp((10.0 - u) / 10.0) - 1.0)
    beta_n = 0.125e3 * np.exp(-u / 80.0)
    values[:, 2] = (1 - n) * alpha_n - n * beta_n
    values[:, 4] = (_q_inf(V) - q) / p[:, 18]
    i_pump = p[:, 15] / ((1 + p[:, 13] / p[:, 11]) ** 2 * (1 + p[:, 14] / p[:, 12]) ** 3)
    g_stim = p[:, 7] * np.exp(-np.mod(t, 0.03) / 0.002) * (t < 125e-3)
    i_Na = (p[:, 2] + p[:, 0] * h * m ** 3 + p[:, 17] * q + g_stim) * (V - p[:, 4]) + 3 * i_pump
    i_K = (p[:, 3] + p[:, 1] * n ** 4) * (V - p[:, 5]) - 2 * i_pump
    p[:, 8] = i_Na
    p[:, 9] = i_K
    p[:, 10] = 0.0
    values[:, 3] = (-i_K - i_Na) / p[:, 6]
    return values


HIP_RHS = r"""
const double m = y[S_m], h = y[S_h], n = y[S_n], V = y[S_V], q = y[S_q];
const double u = 1.0e3 * (V + 65.0e-3);
const double alpha_m = 0.1e3 * (25.0 - u) / (exp((25.0 - u) / 10.0) - 1.0);
const double beta_m = 4.0e3 * exp(-u / 18.0);
dy[S_m] = (1 - m) * alpha_m - m * beta_m;
const double alpha_h = 0.07e3 * exp(-u / 20.0);
const double beta_h = 1.0e3 / (exp((30.0 - u) / 10.0) + 1.0);
dy[S_h] = (1 - h) * alpha_h - h * beta_h;
const double alpha_n = 0.01e3 * (10.0 - u) / (exp((10.0 - u) / 10.0) - 1.0);
const double beta_n = 0.125e3 * exp(-u / 80.0);
dy[S_n] = (1 - n) * alpha_n - n * beta_n;
const double q_inf = 1.0 / (1.0 + exp(-(1.0e3 * V + 52.0) / 5.0));
dy[S_q] = (q_inf - q) / p[P_tau_q];
const double a = 1 + p[P_m_K] / p[P_K_e], b = 1 + p[P_m_Na] / p[P_Na_i];
const double i_pump = p[P_I_max] / (a * a * b * b * b);
const double g_stim = (t < 125e-3) ? p[P_stim_amplitude] * exp(-fmod(t, 0.03) / 0.002) : 0.0;
const double i_Na = (p[P_g_leak_Na] + p[P_g_Na_bar] * h * m * m * m + p[P_g_NaP] * q + g_stim) * (V - p[P_E_Na]) + 3 * i_pump;
const double n2 = n * n;
const double i_K = (p[P_g_leak_K] + p[P_g_K_bar] * n2 * n2) * (V - p[P_E_K]) - 2 * i_pump;
p[P_I_ch_Na] = i_Na;
p[P_I_ch_K] = i_K;
p[P_I_ch_Cl] = 0.0;
dy[S_V] = (-i_K - i_Na) / p[P_Cm];
"""
