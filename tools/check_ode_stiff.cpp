// CPU check of the per-node core of the stiff membrane-ODE integrator (knp-emi-dg_amd/csrc/ode_stiff.hpp: ode_stiff_node with its
// unrolled Jacobian, pivoted LU and extrapolation table), compiled for the host with the device qualifiers defined away.  It runs
// the three test problems of tests/stiff_models.py -- the fast-gate Hodgkin-Huxley membrane (5 states, tau_q 1e-7 s and 1e-9 s,
// 50 windows of 0.1 ms with the stimulus switched on at window 10), Robertson's problem on [0, 40] and Prothero-Robinson with
// lambda = -1e6 on [0, 10] -- plus an 11-state system at the cap.  No GPU call is made; meant to be built with the host sanitizers:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -I knp-emi-dg_amd/csrc tools/check_ode_stiff.cpp \
//       -o /tmp/check_ode_stiff && /tmp/check_ode_stiff
// Exit status 0 and "ode_stiff ok" = every check holds (and the sanitizers had nothing to report).
#include <cmath>
#include <cstdint>
#include <cstdio>
using std::fabs;
using std::fmax;
using std::fmin;
using std::isinf;
using std::pow;
#define __device__
#define __forceinline__ inline
#define ODE_STIFF_HOST_ONLY
#include "ode_stiff.hpp"

static int failures = 0;
#define EXPECT(cond, what)                                  \
    do {                                                    \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
    } while (0)

// examples/custom_membrane_model/mm_hh_fastgate.py: states m h n V q, parameters as mm_hh + 17 g_NaP, 18 tau_q
struct FastGateRhs {
    void operator()(double t, const double* y, double* p, double* dy) const {
        const double m = y[0], h = y[1], n = y[2], V = y[3], q = y[4];
        const double u = 1.0e3 * (V + 65.0e-3);
        const double alpha_m = 0.1e3 * (25.0 - u) / (exp((25.0 - u) / 10.0) - 1.0);
        const double beta_m = 4.0e3 * exp(-u / 18.0);
        dy[0] = (1 - m) * alpha_m - m * beta_m;
        const double alpha_h = 0.07e3 * exp(-u / 20.0);
        const double beta_h = 1.0e3 / (exp((30.0 - u) / 10.0) + 1.0);
        dy[1] = (1 - h) * alpha_h - h * beta_h;
        const double alpha_n = 0.01e3 * (10.0 - u) / (exp((10.0 - u) / 10.0) - 1.0);
        const double beta_n = 0.125e3 * exp(-u / 80.0);
        dy[2] = (1 - n) * alpha_n - n * beta_n;
        const double q_inf = 1.0 / (1.0 + exp(-(1.0e3 * V + 52.0) / 5.0));
        dy[4] = (q_inf - q) / p[18];
        const double a = 1 + p[13] / p[11], b = 1 + p[14] / p[12];
        const double i_pump = p[15] / (a * a * b * b * b);
        const double g_stim = (t < 125e-3) ? p[7] * exp(-fmod(t, 0.03) / 0.002) : 0.0;
        const double i_Na = (p[2] + p[0] * h * m * m * m + p[17] * q + g_stim) * (V - p[4]) + 3 * i_pump;
        const double n2 = n * n;
        const double i_K = (p[3] + p[1] * n2 * n2) * (V - p[5]) - 2 * i_pump;
        p[8] = i_Na;
        p[9] = i_K;
        p[10] = 0.0;
        dy[3] = (-i_K - i_Na) / p[6];
    }
};

struct RobertsonRhs {
    void operator()(double, const double* y, double* p, double* dy) const {
        const double r1 = p[0] * y[0], r2 = p[1] * y[1] * y[1], r3 = p[2] * y[1] * y[2];
        dy[0] = -r1 + r3;
        dy[1] = r1 - r3 - r2;
        dy[2] = r2;
    }
};

struct ProtheroRobinsonRhs {
    void operator()(double t, const double* y, double* p, double* dy) const { dy[0] = p[0] * (y[0] - cos(t)) - sin(t); }
};

// 11 relaxations towards a common, slowly moving mean with rates spread over nine decades: every state couples to every other
struct ChainRhs {
    void operator()(double t, const double* y, double* p, double* dy) const {
        double mean = 0.0;
        for (int s = 0; s < 11; ++s) mean += y[s] / 11;
        for (int s = 0; s < 11; ++s) dy[s] = -p[0] * pow(10.0, (double)s - 1.0) * (y[s] - mean - 0.1 * sin(t + s));
    }
};

static void fast_gate(double tau) {
    double y[5] = {0.016648440745822956, 0.8542015627820805, 0.1882020248041632, -0.07438609374462003, 0.0};
    y[4] = 1.0 / (1.0 + exp(-(1.0e3 * y[3] + 52.0) / 5.0));
    double p[19] = {1200.0, 360.0, 1.0, 4.0, 0.0533, -0.0936, 0.02, 0.0, 0, 0, 0, 3.3236967382705265, 12.838513108648856, 2.0, 7.7,
                    0.449, 0.0, 2.0, tau};
    double h = 0.0, vmax = y[3];
    OdeStiffCount cnt = {0, 0, 0, 0};
    bool ok = true;
    for (int k = 0; k < 50; ++k) {
        p[7] = k >= 10 ? 40.0 : 0.0;
        ok = ok && ode_stiff_node<5, 19>(FastGateRhs(), k * 1e-4, (k + 1) * 1e-4, 1e-8, 0.0, 100000, y, p, h, cnt);
        vmax = fmax(vmax, y[3]);
    }
    std::printf("fast gate tau %.0e: V %.10g (max %.4g), q - q_inf %.3g, steps %d + %d rejected, %d rhs calls, %d Jacobians\n", tau, y[3],
                vmax, y[4] - 1.0 / (1.0 + exp(-(1.0e3 * y[3] + 52.0) / 5.0)), cnt.acc, cnt.rej, cnt.rhs, cnt.jac);
    EXPECT(ok, "fast gate reaches every window end");
    EXPECT(vmax > 0.0 && y[3] < -0.06, "fast gate fires and repolarises");
    EXPECT(cnt.acc >= 50 && cnt.acc < 2000, "fast gate step count");
    EXPECT(cnt.rhs == cnt.jac * (1 + 5 + ODE_STIFF_K * (ODE_STIFF_K + 1) / 2) + 50, "fast gate rhs count");
    EXPECT(h > 0.0, "fast gate step size carried");
}

int main() {
    fast_gate(1e-7);
    fast_gate(1e-9);
    {
        double y[3] = {1.0, 0.0, 0.0}, p[3] = {0.04, 3.0e7, 1.0e4}, h = 0.0;
        OdeStiffCount cnt = {0, 0, 0, 0};
        const bool ok = ode_stiff_node<3, 3>(RobertsonRhs(), 0.0, 40.0, 1e-8, 0.0, 100000, y, p, h, cnt);
        std::printf("Robertson at 40: %.10g %.10g %.10g, steps %d + %d rejected, %d rhs calls\n", y[0], y[1], y[2], cnt.acc, cnt.rej, cnt.rhs);
        // the solution at t = 40
        EXPECT(ok && fabs(y[0] - 0.7158270688) < 1e-8 && fabs(y[1] - 9.185534765e-6) < 1e-12 && fabs(y[2] - 0.2841637457) < 1e-8, "Robertson at 40");
        EXPECT(fabs(y[0] + y[1] + y[2] - 1.0) < 1e-12, "Robertson conserves mass");
    }
    {
        double y[1] = {1.0}, p[1] = {-1.0e6}, h = 0.0;
        OdeStiffCount cnt = {0, 0, 0, 0};
        const bool ok = ode_stiff_node<1, 1>(ProtheroRobinsonRhs(), 0.0, 10.0, 1e-8, 0.0, 100000, y, p, h, cnt);
        std::printf("Prothero-Robinson at 10: error %.3g, steps %d + %d rejected\n", y[0] - cos(10.0), cnt.acc, cnt.rej);
        EXPECT(ok && fabs(y[0] - cos(10.0)) < 1e-6 && cnt.acc <= 30000, "Prothero-Robinson");
    }
    {
        double y[11], p[1] = {1.0}, h = 0.0;
        for (int s = 0; s < 11; ++s) y[s] = 0.1 * s;
        OdeStiffCount cnt = {0, 0, 0, 0};
        const bool ok = ode_stiff_node<11, 1>(ChainRhs(), 0.0, 5.0, 1e-8, 1e-12, 100000, y, p, h, cnt);
        double mean = 0.0;
        for (int s = 0; s < 11; ++s) mean += y[s] / 11;
        std::printf("11 states at 5: mean %.10g, fastest state off its target by %.3g, steps %d + %d rejected\n", mean,
                    y[10] - mean - 0.1 * sin(5.0 + 10), cnt.acc, cnt.rej);
        EXPECT(ok && fabs(y[10] - mean - 0.1 * sin(5.0 + 10)) < 1e-6 && cnt.acc < 5000, "11 states");
    }
    if (failures) { std::printf("%d check(s) failed\n", failures); return 1; }
    std::printf("ode_stiff ok\n");
    return 0;
}
