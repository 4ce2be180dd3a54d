// Shared by the two DG-p (p >= 2) sources over tabulated rules, tab_rhs.hip and tab_assembled.hip: the ion valences as a kernel argument, the
// facet frame of a cell and of an interior facet pair, small nodal helpers, and the launch helpers.  The reference basis is tabulated
// on the host (knpemidg/dgtab.py) at the quadrature points of each integral class and uploaded once (knp_set_tabulation, tab_rhs.hip),
// so these kernels are generic in the polynomial degree.
#pragma once
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "cell_geom.hpp"
#include <cstdlib>

struct IonZ { int n; double z[KNP_MAX_IONS]; };
static inline IonZ ion_z(const knp_ctx* c) {
    IonZ a; a.n = c->p.n_ions;
    for (int i = 0; i < KNP_MAX_IONS; ++i) a.z[i] = i < c->p.n_ions ? c->p.z[i] : 1.0;
    return a;
}

// area of facet i of cell K
template <int D> __device__ __forceinline__ double facet_area(const CellGeom<D>& K, int i) {
    return (double)D * K.vol * sqrt(dotD<D>(K.g[i], K.g[i]));
}

// facet i of cell K: gn[l] = grad lambda_l . n (n = outward unit normal = -g_i/|g_i|), returns the facet area
template <int D> __device__ __forceinline__ double facet_frame(const CellGeom<D>& K, int i, double* nrm, double* gn) {
    const double gi2 = dotD<D>(K.g[i], K.g[i]);
    const double gl = sqrt(gi2);
#pragma unroll
    for (int k = 0; k < D; ++k) nrm[k] = -K.g[i][k] / gl;
#pragma unroll
    for (int l = 0; l <= D; ++l) gn[l] = dotD<D>(K.g[l], nrm);
    return facet_area<D>(K, i);
}

// interior facet i of cell K with the cell K2 behind it: the own normal derivatives gn[l] of the barycentric coordinates, the
// neighbour's gn2[l] = grad lambda'_l . n with the SAME normal (the own outward one), and the facet area
template <int D> struct TabPair { double gn[D + 1], gn2[D + 1], area; };
template <int D> __device__ __forceinline__ void tab_pair(const CellGeom<D>& K, const CellGeom<D>& K2, int i, TabPair<D>& P) {
    double nrm[D];
    P.area = facet_frame<D>(K, i, nrm, P.gn);
#pragma unroll
    for (int l = 0; l <= D; ++l) P.gn2[l] = dotD<D>(K2.g[l], nrm);
}

template <int NV> __device__ __forceinline__ double dotNV(const double* a, const double* b) {
    double s = a[0] * b[0];
#pragma unroll
    for (int l = 1; l < NV; ++l) s = fma(a[l], b[l], s);
    return s;
}

template <int ND> __device__ __forceinline__ void ld(const double* __restrict__ p, int64_t c, double* v) {
#pragma unroll
    for (int a = 0; a < ND; ++a) v[a] = p[c * ND + a];
}

// ---- launch helpers --------------------------------------------------------------------------------------------
static inline int need_tabs(knp_ctx* c, std::initializer_list<int> slots) {
    for (int s : slots)
        if (!c->tab[s].w) { c->err = "DG-p path: tabulation slot " + std::to_string(s) + " not set (knp_set_tabulation)"; return -1; }
    return 0;
}

#define TAB_DISPATCH(c, KERN, grid, block, ...)                                                              \
    do {                                                                                                     \
        if ((c)->m.dim == 3) hipLaunchKernelGGL((KERN<3, 10>), grid, block, 0, (c)->stream, __VA_ARGS__);      \
        else hipLaunchKernelGGL((KERN<2, 6>), grid, block, 0, (c)->stream, __VA_ARGS__);                       \
        HIPCHK(c, hipGetLastError());                                                                        \
    } while (0)

static inline dim3 cells_grid(knp_ctx* c, int block, int ny = 1) {
    return dim3((unsigned)((c->m.nc_owned + block - 1) / block), (unsigned)ny);
}
static inline dim3 rows_grid(knp_ctx* c, int block, int ny = 1) {
    return dim3((unsigned)((c->m.nc_owned * c->nd + block - 1) / block), (unsigned)ny);
}
