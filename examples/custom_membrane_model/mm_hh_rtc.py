"""The Hodgkin-Huxley membrane of the idealized examples (knpemidg.models.mm_hh) written the way a user writes a model of their
own: no built-in device id (MODEL_ID), its right-hand side as HIP_RHS, which the device integrator compiles at run time
(knpemidg/ode_rtc.py).  The text follows the built-in kernel's (csrc/ode.hip: hh_rhs<true>) operation by operation, so both
give the same numbers; tools/ode_rtc_bench.py and tests/test_gpu_ode_rtc.py compare them."""
from knpemidg.models._hh_core import (STATE_IND, PARAM_IND, init_state_values, init_parameter_values, state_indices,
                                      parameter_indices, rhs_impl)


def rhs(t, states, parameters):
    return rhs_impl(t, states, parameters, True)


HIP_RHS = r"""
const double m = y[S_m], h = y[S_h], n = y[S_n], V = y[S_V];
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
const double a = 1 + p[P_m_K] / p[P_K_e], b = 1 + p[P_m_Na] / p[P_Na_i];
const double i_pump = p[P_I_max] / (a * a * b * b * b);
const double g_stim = (t < 125e-3) ? p[P_stim_amplitude] * exp(-fmod(t, 0.03) / 0.002) : 0.0;
const double i_Na = (p[P_g_leak_Na] + p[P_g_Na_bar] * h * m * m * m + g_stim) * (V - p[P_E_Na]) + 3 * i_pump;
const double n2 = n * n;
const double i_K = (p[P_g_leak_K] + p[P_g_K_bar] * n2 * n2) * (V - p[P_E_K]) - 2 * i_pump;
p[P_I_ch_Na] = i_Na;
p[P_I_ch_K] = i_K;
p[P_I_ch_Cl] = 0.0;
dy[S_V] = (-i_K - i_Na) / p[P_Cm];
"""
