// One membrane-ODE step of one facet with a STIFF integrator: the extrapolated linearly implicit Euler method from t0 to t1, right-
// hand side given as a functor -- the counterpart of ode_dp5.hpp (same launch contract: one thread per node, states and parameters in
// registers, the stimulus imposed at the start of every call, hstore carrying the step size, the failure flag, a final rhs(t1, ..)
// that leaves I_ch_k at the end state) for models DP5 can only follow by shrinking its step to the fastest time constant.
// knpemidg/membrane.py:integrate_batch_stiff restates the same arithmetic in numpy.
//
// One basic step H from (t, y):
//   J  = forward-difference Jacobian of f at (t, y): column c from f(t, y + d_c e_c), d_c = sqrt(eps) max(|y_c|, ODE_STIFF_FD_FLOOR)
//   for the substep counts n = 1 .. K (harmonic sequence), h = H / n:  LU of I - h J (partial pivoting), then n times
//        (I - h J) d = h f(t_m + h, y_m),   y_{m+1} = y_m + d                       -> T_n1
//   Aitken-Neville:  T_{n,k+1} = T_{n,k} + (T_{n,k} - T_{n-1,k}) / (n / (n - k) - 1)       -> T_KK, of order K
//   err = max_s |T_KK - T_K,K-1|_s / (atol + rtol max(|y_s|, |T_KK|_s));  accept if err <= 1;  H <- H clip(0.9 err^(-1/K), 0.2, 5)
// The extrapolation weights follow from the substep counts, the method has no other coefficients.  Every table entry has R(inf) = 0
// and is A(alpha)-stable with alpha above 89 degrees (Hairer & Wanner, Solving ODEs II, section IV.9).  The Jacobian only has to be
// approximately right: the order of the extrapolated value does not depend on it, only the stability does.
//
// NS is a compile-time constant and every loop over states is unrolled with compile-time indices (row swaps of the pivoting and the
// writes of a Jacobian column are selects, not indexed stores), so J, LU and the table live in registers while they fit: 2 NS^2 +
// (K + 5) NS doubles.  The loops over Jacobian columns, table columns and substeps stay rolled: four inlined copies of the right-hand
// side in all.  ODE_STIFF_MAX_STATES caps NS; at 11 (the calibration system) the arrays exceed the 512 VGPRs of a wave and spill.
//
// Like ode_dp5.hpp: no includes (hipRTC pastes this text; the including file supplies int64_t / uint8_t) and device code only.
// ode_stiff_node, the per-node core, touches neither blockIdx nor global memory, so a host program can compile it with __device__ and
// __forceinline__ defined away and ODE_STIFF_HOST_ONLY set (tools/check_ode_stiff.cpp).
#ifndef KNPEMI_ODE_STIFF_HPP
#define KNPEMI_ODE_STIFF_HPP

#ifndef ODE_MAX_STIM                 // the launch layout of ode_dp5.hpp, for a translation unit that holds this header alone
#define ODE_MAX_STIM 4
struct StimArgs { int n; int col[ODE_MAX_STIM]; double val[ODE_MAX_STIM]; };
#endif

#define ODE_STIFF_K 8                // table columns = order; 8 took fewer right-hand-side calls than 6 on both test models
#define ODE_STIFF_MAX_STATES 11
#define ODE_STIFF_FD_REL 1.4901161193847656e-08      // 2^-26 = sqrt(eps) of a double
#define ODE_STIFF_FD_FLOOR 1.0e-5                    // smallest |y_c| the increment is scaled by (gates and concentrations near 0)

// per node and launch: accepted steps, rejected steps, right-hand-side calls (Jacobian columns included), Jacobians
struct OdeStiffCount { int acc, rej, rhs, jac; };

// A <- its LU factors (unit lower triangle below the diagonal), piv[c] = row swapped with row c
template <int NS> __device__ __forceinline__ void ode_stiff_lu(double (&A)[NS][NS], int (&piv)[NS]) {
#pragma unroll
    for (int c = 0; c < NS; ++c) {
        int pr = c;
        double big = fabs(A[c][c]);
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const double v = fabs(A[r][c]);
            if (v > big) { big = v; pr = r; }
        }
        piv[c] = pr;
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const bool sw = r == pr;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const double a = A[c][q], b = A[r][q];
                A[c][q] = sw ? b : a;
                A[r][q] = sw ? a : b;
            }
        }
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const double l = A[r][c] / A[c][c];
            A[r][c] = l;
#pragma unroll
            for (int q = c + 1; q < NS; ++q) A[r][q] -= l * A[c][q];
        }
    }
}

// b <- solution of (L U) x = P b
template <int NS> __device__ __forceinline__ void ode_stiff_solve(const double (&A)[NS][NS], const int (&piv)[NS], double (&b)[NS]) {
#pragma unroll
    for (int c = 0; c < NS; ++c)
#pragma unroll
        for (int r = c + 1; r < NS; ++r) {
            const bool sw = r == piv[c];
            const double u = b[c], v = b[r];
            b[c] = sw ? v : u;
            b[r] = sw ? u : v;
        }
#pragma unroll
    for (int r = 1; r < NS; ++r)
#pragma unroll
        for (int c = 0; c < r; ++c) b[r] -= A[r][c] * b[c];
#pragma unroll
    for (int r = NS - 1; r >= 0; --r) {
#pragma unroll
        for (int c = r + 1; c < NS; ++c) b[r] -= A[r][c] * b[c];
        b[r] /= A[r][r];
    }
}

// Rhs: any callable `void (double t, const double* y, double* p, double* dy)`; it may write outputs (I_ch_k) into p.
// Integrates y from t0 to t1 (h: step size in and out), ends with rhs(t1, y, ..); false if t1 was not reached within max_steps.
template <int NS, int NP, class Rhs>
__device__ __forceinline__ bool ode_stiff_node(const Rhs& rhs, double t0, double t1, double rtol, double atol, int max_steps,
                                               double (&y)[NS], double (&p)[NP], double& h, OdeStiffCount& cnt) {
    static_assert(NS >= 1 && NS <= ODE_STIFF_MAX_STATES, "ode_stiff: 1..ODE_STIFF_MAX_STATES states");
    double J[NS][NS] = {}, T[ODE_STIFF_K][NS] = {};      // written through selects, so they start defined
    double A[NS][NS], f0[NS], f[NS], yy[NS];
    int piv[NS];
    double t = t0;
    if (!(h > 0.0)) h = (t1 - t0) / 16;
    const double tiny = 1e-14 * fmax(fabs(t1), 1e-30);
    int steps = 0;
    bool done = false;
    while (!done && steps < max_steps) {
        const double hh = fmin(h, t1 - t);
        rhs(t, y, p, f0);
#pragma unroll 1
        for (int c = 0; c < NS; ++c) {
            double d = 0.0;
#pragma unroll
            for (int q = 0; q < NS; ++q) {
                const double dq = ODE_STIFF_FD_REL * fmax(fabs(y[q]), ODE_STIFF_FD_FLOOR);
                yy[q] = q == c ? y[q] + dq : y[q];
                d = q == c ? dq : d;
            }
            rhs(t, yy, p, f);
#pragma unroll
            for (int r = 0; r < NS; ++r) {
                const double v = (f[r] - f0[r]) / d;
#pragma unroll
                for (int q = 0; q < NS; ++q) J[r][q] = q == c ? v : J[r][q];
            }
        }
#pragma unroll 1
        for (int j = 0; j < ODE_STIFF_K; ++j) {
            const double hs = hh / (j + 1);
#pragma unroll
            for (int r = 0; r < NS; ++r)
#pragma unroll
                for (int q = 0; q < NS; ++q) A[r][q] = (r == q ? 1.0 : 0.0) - hs * J[r][q];
            ode_stiff_lu<NS>(A, piv);
#pragma unroll
            for (int q = 0; q < NS; ++q) yy[q] = y[q];
#pragma unroll 1
            for (int m = 0; m <= j; ++m) {
                rhs(t + (m + 1) * hs, yy, p, f);
#pragma unroll
                for (int q = 0; q < NS; ++q) f[q] *= hs;
                ode_stiff_solve<NS>(A, piv, f);
#pragma unroll
                for (int q = 0; q < NS; ++q) yy[q] += f[q];
            }
            // T[k] <- T_{j,j-k+1} in place, from the new T_j1 down: T[k] still holds the row above when it is read
#pragma unroll
            for (int k = 0; k < ODE_STIFF_K; ++k)
#pragma unroll
                for (int q = 0; q < NS; ++q) T[k][q] = k == j ? yy[q] : T[k][q];
#pragma unroll
            for (int k = ODE_STIFF_K - 2; k >= 0; --k)
                if (k < j) {
                    const double w = (j + 1.0) / (k + 1.0) - 1.0;
#pragma unroll
                    for (int q = 0; q < NS; ++q) T[k][q] = T[k + 1][q] + (T[k + 1][q] - T[k][q]) / w;
                }
        }
        double e = 0.0;
        bool nan = false;                            // fmax drops a NaN operand: a step that produced one must not pass as e = 0
#pragma unroll
        for (int q = 0; q < NS; ++q) {
            const double scale = fmax(atol + rtol * fmax(fabs(y[q]), fabs(T[0][q])), 1e-300);
            const double r = fabs(T[0][q] - T[1][q]) / scale;
            nan = nan || !(r == r);
            e = fmax(e, r);
        }
        if (nan || isinf(e)) e = 1e10;
        ++steps;
        ++cnt.jac;
        cnt.rhs += 1 + NS + ODE_STIFF_K * (ODE_STIFF_K + 1) / 2;
        if (e <= 1.0 || hh < tiny) {
            t += hh;
#pragma unroll
            for (int q = 0; q < NS; ++q) y[q] = T[0][q];
            if (t >= t1 - 1e-15 * fabs(t1)) done = true;
            ++cnt.acc;
        } else {
            ++cnt.rej;
        }
        const double fac = fmin(5.0, fmax(0.2, 0.9 * pow(1.0 / fmax(e, 1e-10), 1.0 / ODE_STIFF_K)));
        if (!done) h = hh * fac;
    }
    rhs(t1, y, p, f0);                               // leave I_ch_k evaluated at the end state
    ++cnt.rhs;
    return done;
}

#ifndef ODE_STIFF_HOST_ONLY                     // a host program that checks ode_stiff_node defines it
// the launch side of ode_dp5_step, plus stats[4]: the block's counters, reduced over the wave, one vector atomic per counter
template <int NS, int NP, class Rhs>
__device__ __forceinline__ void ode_stiff_step(const Rhs& rhs, int64_t n, double t0, double t1, double rtol, double atol,
                                               int max_steps, double* __restrict__ states, double* __restrict__ params,
                                               double* __restrict__ hstore, int* __restrict__ fail,
                                               const uint8_t* __restrict__ stim_mask, StimArgs stim,
                                               unsigned long long* __restrict__ stats) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    OdeStiffCount cnt = {0, 0, 0, 0};
    if (i < n) {                                     // no early return: every lane takes part in the reduction below
        double y[NS], p[NP];
#pragma unroll
        for (int s = 0; s < NS; ++s) y[s] = states[i * NS + s];
#pragma unroll
        for (int q = 0; q < NP; ++q) p[q] = params[i * NP + q];
        if (stim.n > 0 && stim_mask[i]) {
            for (int e = 0; e < stim.n; ++e)
#pragma unroll
                for (int q = 0; q < NP; ++q)
                    if (q == stim.col[e]) p[q] = stim.val[e];
        }
        double h = hstore[i];
        if (!ode_stiff_node<NS, NP>(rhs, t0, t1, rtol, atol, max_steps, y, p, h, cnt)) atomicExch(fail, 1);
#pragma unroll
        for (int s = 0; s < NS; ++s) states[i * NS + s] = y[s];
#pragma unroll
        for (int q = 0; q < NP; ++q) params[i * NP + q] = p[q];
        hstore[i] = h;
    }
    int v[4] = {cnt.acc, cnt.rej, cnt.rhs, cnt.jac};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        for (int off = warpSize / 2; off > 0; off >>= 1) v[q] += __shfl_down(v[q], off);
        if (threadIdx.x % warpSize == 0 && v[q]) atomicAdd(&stats[q], (unsigned long long)v[q]);
    }
}
#endif

#endif
