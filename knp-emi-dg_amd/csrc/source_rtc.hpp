// Load vector of a space- and time-dependent ion source on the device: text of the runtime-compiled translation units that
// knpemidg/expression.py generates (one per Expression, mesh dimension and basis size), never compiled into the library itself.
//
// The generated text in front of this header defines
//     struct UserSource { double operator()(const double* x, const double* knp_params) const; };
// (the user's scalar expression over x[0 .. DIM-1] and the named parameters), and behind it one extern "C" kernel that calls
// source_load_vector<DIM, ND>.  For every selected cell K (the context's ECS cells, device order) and local basis function a
//     out[K * ND + a] = vol_K * sum_q w_q f(x_q) B[q][a],      x_q = sum_l bary[q][l] X_l,
// with the rule and the basis values tabulated on the host (quadrature.simplex_rule(dim, mms_terms.QDEG), dgtab.tabulate), so host
// and device integrate with the same numbers.
//
// Shape: one lane per cell, the ND sums in registers, q in ascending order -- no atomics, no cross-lane step, so two runs give the
// same bits, and the row is overwritten, not accumulated.  q is the same in every lane: the table reads (bary, w, B) and the
// parameters are wave-uniform and travel through the scalar unit; per lane there are DIM + 1 vertex ids, DIM + 1 coordinate rows and
// ND stores.  The kernel is bound by the nq evaluations of the user's expression, not by bytes.
#ifndef KNP_SOURCE_RTC_HPP          // a guard, not `#pragma once`: this text is also the main file of a runtime compile
#define KNP_SOURCE_RTC_HPP

#define KNP_SOURCE_MAX_PARAMS 32
#define KNP_SOURCE_BLOCK 64

struct SourceParams { double v[KNP_SOURCE_MAX_PARAMS]; };   // by value in the kernel arguments: an evaluation copies nothing to the device

// coords: [nv][4] in 3D (padded rows), [nv][2] in 2D; cells: [nc][DIM + 1]; sel: [n] cells to integrate over
template <int DIM, int ND, typename F>
__device__ __forceinline__ void source_load_vector(const F f, int64_t n, const int32_t* __restrict__ sel, const double* __restrict__ coords,
                                                   const int32_t* __restrict__ cells, int nq, const double* __restrict__ bary,
                                                   const double* __restrict__ w, const double* __restrict__ B, const SourceParams& p,
                                                   double* __restrict__ out) {
    constexpr int NV = DIM + 1;
    constexpr int CS = DIM == 3 ? 4 : 2;
    const int64_t i = (int64_t)blockIdx.x * KNP_SOURCE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t cell = sel[i];
    double X[NV][DIM];
    for (int l = 0; l < NV; ++l) {
        const int64_t v = cells[cell * NV + l];
        for (int d = 0; d < DIM; ++d) X[l][d] = coords[v * CS + d];
    }
    double J[DIM][DIM];
    for (int l = 0; l < DIM; ++l)
        for (int d = 0; d < DIM; ++d) J[l][d] = X[l + 1][d] - X[0][d];
    double det;
    if constexpr (DIM == 2) det = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    else det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
               J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    const double vol = (det < 0.0 ? -det : det) * (DIM == 2 ? 0.5 : 1.0 / 6.0);
    double acc[ND];
    for (int a = 0; a < ND; ++a) acc[a] = 0.0;
    for (int q = 0; q < nq; ++q) {
        double x[DIM];
        for (int d = 0; d < DIM; ++d) {
            double s = 0.0;
            for (int l = 0; l < NV; ++l) s += bary[q * NV + l] * X[l][d];
            x[d] = s;
        }
        const double wf = w[q] * f(x, p.v);
        for (int a = 0; a < ND; ++a) acc[a] += wf * B[q * ND + a];
    }
    for (int a = 0; a < ND; ++a) out[cell * ND + a] = vol * acc[a];
}

#endif
