// One membrane-ODE step of one facet: adaptive Dormand-Prince 5(4) from t0 to t1 with the right-hand side given as a functor
// (same pair, step controller and tolerances as knpemidg/membrane.py:integrate_batch).  The single text of the integrator:
// ode.hip instantiates it for the built-in models 1-6 (k_ode_step<MODEL, NS, NP>), and knpemidg/ode_rtc.py pastes it into the
// translation unit it hands to hipRTC for a model module that carries its right-hand side as HIP_RHS.  So it compiles under
// both: no includes at all (hipRTC has no <cstdint>; the including file supplies int64_t / uint8_t) and device code only.
#ifndef KNPEMI_ODE_DP5_HPP
#define KNPEMI_ODE_DP5_HPP

#define ODE_MAX_STIM 4

// the stimulus entries travel by value with every launch: the built-in and the runtime-compiled kernels share this layout
struct StimArgs { int n; int col[ODE_MAX_STIM]; double val[ODE_MAX_STIM]; };

// Rhs: any callable `void (double t, const double* y, double* p, double* dy)`; it may write outputs (I_ch_k) into p
template <int NS, int NP, class Rhs>
__device__ __forceinline__ void ode_dp5_step(const Rhs& rhs, int64_t n, double t0, double t1, double rtol, double atol,
                                             int max_steps, double* __restrict__ states, double* __restrict__ params,
                                             double* __restrict__ hstore, int* __restrict__ fail,
                                             const uint8_t* __restrict__ stim_mask, StimArgs stim) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double y[NS], p[NP], k[7][NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) y[s] = states[i * NS + s];
#pragma unroll
    for (int q = 0; q < NP; ++q) p[q] = params[i * NP + q];
    // the stimulus overwrites its parameters on the masked rows at the start of EVERY step (membrane.py:102-104), whatever a
    // hook or a parameter upload wrote there in between
    if (stim.n > 0 && stim_mask[i]) {
        for (int e = 0; e < stim.n; ++e)
#pragma unroll
            for (int q = 0; q < NP; ++q)
                if (q == stim.col[e]) p[q] = stim.val[e];
    }
    // Dormand-Prince 5(4)
    const double C[7] = {0, 1.0 / 5, 3.0 / 10, 4.0 / 5, 8.0 / 9, 1, 1};
    const double A[7][6] = {{0, 0, 0, 0, 0, 0},
                            {1.0 / 5, 0, 0, 0, 0, 0},
                            {3.0 / 40, 9.0 / 40, 0, 0, 0, 0},
                            {44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0},
                            {19372.0 / 6561, -25360.0 / 2187, 64448.0 / 6561, -212.0 / 729, 0, 0},
                            {9017.0 / 3168, -355.0 / 33, 46732.0 / 5247, 49.0 / 176, -5103.0 / 18656, 0},
                            {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84}};
    const double B5[7] = {35.0 / 384, 0, 500.0 / 1113, 125.0 / 192, -2187.0 / 6784, 11.0 / 84, 0};
    const double B4[7] = {5179.0 / 57600, 0, 7571.0 / 16695, 393.0 / 640, -92097.0 / 339200, 187.0 / 2100, 1.0 / 40};
    double t = t0;
    double h = hstore[i];
    if (!(h > 0.0)) h = (t1 - t0) / 16;
    const double tiny = 1e-14 * fmax(fabs(t1), 1e-30);
    rhs(t, y, p, k[0]);
    int steps = 0;
    bool done = false;
    while (!done && steps < max_steps) {
        const double hh = fmin(h, t1 - t);
#pragma unroll
        for (int s = 1; s < 7; ++s) {
            double ys[NS];
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < 6; ++j)
                    if (j < s) acc += A[s][j] * k[j][q];
                ys[q] = y[q] + hh * acc;
            }
            rhs(t + C[s] * hh, ys, p, k[s]);
        }
        double e = 0.0, y5[NS];
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            double a5 = 0.0, ae = 0.0;
#pragma unroll
            for (int j = 0; j < 7; ++j) { a5 += B5[j] * k[j][q]; ae += (B5[j] - B4[j]) * k[j][q]; }
            y5[q] = y[q] + hh * a5;
            const double scale = fmax(atol + rtol * fmax(fabs(y[q]), fabs(y5[q])), 1e-300);   // atol = 0 is the reference's (membrane.py:112)
            e = fmax(e, fabs(hh * ae) / scale);
        }
        if (!(e == e) || isinf(e)) e = 1e10;
        ++steps;
        if (e <= 1.0 || hh < tiny) {
            t += hh;
#pragma unroll
            for (int q = 0; q < NS; ++q) { y[q] = y5[q]; k[0][q] = k[6][q]; }
            if (t >= t1 - 1e-15 * fabs(t1)) done = true;
        }
        const double fac = fmin(5.0, fmax(0.2, 0.9 * pow(1.0 / fmax(e, 1e-10), 0.2)));
        if (!done) h = hh * fac;
    }
    if (!done) atomicExch(fail, 1);
    rhs(t1, y, p, k[0]);                              // leave I_ch_k evaluated at the end state
#pragma unroll
    for (int s = 0; s < NS; ++s) states[i * NS + s] = y[s];
#pragma unroll
    for (int q = 0; q < NP; ++q) params[i * NP + q] = p[q];
    hstore[i] = h;
}

#endif
