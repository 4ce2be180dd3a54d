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

// ---- sources that read the solution (knpemidg.FieldExpression) ---------------------------------------------------------------
// The functor takes a third argument,
//     struct UserSource { double operator()(const double* x, const double* knp_fields, const double* knp_params) const; };
// knp_fields[i] being the value at x of the i-th of NF nodal fields (phi or a concentration, [nc][ND] in device cell order):
//     u_i(x_q) = sum_a U[i][a] B[q][a],
// with the same B the test functions are tabulated with.  Same shape as above -- one lane per cell of the kernel's own list, q
// ascending, the ND sums in registers, no atomics, no LDS, no cross-lane step -- plus NF * ND nodal values per lane, loaded once
// in front of the q loop.  A cell's ND values are contiguous; ND * 8 bytes is a multiple of 16 for every basis but the 2D P1 one,
// so the rows are read 16 bytes at a time where ND is even (the host refuses a field pointer that is not 16-byte aligned then) and
// value by value where it is odd.  Live doubles per lane in the q loop, (3D, P2, NF = 4): 40 nodal values + 10 sums + 12
// coordinates; the compile log of the test expression shows 162 of the 512 VGPRs a block of one wave may hold.
#define KNP_SOURCE_MAX_FIELDS 9     // KNP_MAX_IONS + 1: phi and every ion

struct SourceFields { const double* v[KNP_SOURCE_MAX_FIELDS]; };    // by value in the kernel arguments; the first NF are set

typedef double knp_source_d2 __attribute__((ext_vector_type(2)));

template <int DIM, int ND, int NF, typename F>
__device__ __forceinline__ void source_load_vector_fields(const F f, int64_t n, const int32_t* __restrict__ sel,
                                                          const double* __restrict__ coords, const int32_t* __restrict__ cells, int nq,
                                                          const double* __restrict__ bary, const double* __restrict__ w,
                                                          const double* __restrict__ B, const SourceFields& fld, const SourceParams& p,
                                                          double* __restrict__ out) {
    static_assert(NF >= 0 && NF <= KNP_SOURCE_MAX_FIELDS, "phi and at most KNP_MAX_IONS concentrations");
    constexpr int NV = DIM + 1;
    constexpr int CS = DIM == 3 ? 4 : 2;
    const int64_t i = (int64_t)blockIdx.x * KNP_SOURCE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t cell = sel[i];
    double U[NF > 0 ? NF : 1][ND];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const double* __restrict__ row = fld.v[k] + cell * ND;
        if constexpr (ND % 2 == 0) {
#pragma unroll
            for (int a = 0; a < ND; a += 2) {
                const knp_source_d2 pair = *reinterpret_cast<const knp_source_d2*>(row + a);
                U[k][a] = pair.x;
                U[k][a + 1] = pair.y;
            }
        } else {
#pragma unroll
            for (int a = 0; a < ND; ++a) U[k][a] = row[a];
        }
    }
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
        double u[NF > 0 ? NF : 1];
#pragma unroll
        for (int k = 0; k < NF; ++k) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < ND; ++a) s += U[k][a] * B[q * ND + a];
            u[k] = s;
        }
        const double wf = w[q] * f(x, u, p.v);
        for (int a = 0; a < ND; ++a) acc[a] += wf * B[q * ND + a];
    }
    for (int a = 0; a < ND; ++a) out[cell * ND + a] = vol * acc[a];
}

#endif
