// What a matrix-free DG-P2 facet kernel is made of (device code only; the formulation is in the header of apply_p2.hip):
//  * P2<D>: index arithmetic of the FACET FRAME [apex | facet vertices | facet edges | apex edges], frame_packed: its nibble-packed permutations;
//  * nodal_gradients / project_gradients / pair_matrix (cells), dn_vertices / back_project (facets), the monomial-product helpers;
//  * StageP2 + stage_block_p2: the workgroup's two nodal vectors and the class table in LDS; load_frame, load_cellvec / store_cellvec;
//  * cell_geometry_p2, facet_geometry, facet_neighbour, facet_normals: geometry and neighbour of one facet in Gram form (cell_geom.hpp).
#pragma once
#include "cell_geom.hpp"
#include "p2_tables.hpp"
#include "p2_mono_tables.hpp"

template <int D> struct P2 {
    static constexpr int NV = D + 1, ND = NV * (NV + 1) / 2, NFE = D * (D - 1) / 2, NF = D + NFE;
    static constexpr int edge(int a, int b) {                 // cell dof of edge (a, b)
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        int k = NV;
        for (int i = 0; i < lo; ++i) k += NV - 1 - i;
        return k + (hi - lo - 1);
    }
    static constexpr int fe(int m, int mp) {                  // frame slot of the facet edge (m, mp)
        const int lo = m < mp ? m : mp, hi = m < mp ? mp : m;
        int k = 1 + D;
        for (int i = 0; i < lo; ++i) k += D - 1 - i;
        return k + (hi - lo - 1);
    }
    static constexpr int ae(int m) { return 1 + D + NFE + m; } // frame slot of the edge (apex, facet vertex m)
    // cell dof behind frame slot s of local facet I (= P2Tab<D>::FRAME_SLOTS[I][s], as arithmetic so that it folds to a
    // register index at compile time; loads from the table would be run-time loads + dynamic register indexing)
    static constexpr int fs(int I, int s) {
        if (s == 0) return I;
        if (s <= D) return (s - 1) + ((s - 1) >= I ? 1 : 0);
        if (s <= D + NFE) {
            int k = 1 + D;
            for (int a = 0; a < D; ++a)
                for (int b = a + 1; b < D; ++b) {
                    if (k == s) return edge(a + (a >= I ? 1 : 0), b + (b >= I ? 1 : 0));
                    ++k;
                }
        }
        const int mm = s - 1 - D - NFE;
        return edge(I, mm + (mm >= I ? 1 : 0));
    }
    static constexpr uint64_t packed(int j) {                 // nibble s = fs(j, s)
        uint64_t p = 0;
        for (int s = 0; s < ND; ++s) p |= (uint64_t)fs(j, s) << (4 * s);
        return p;
    }
    static constexpr int pair(int a, int b) {                 // index of the unordered vertex pair in M3
        const int lo = a < b ? a : b, hi = a < b ? b : a;
        int k = 0;
        for (int i = 0; i < lo; ++i) k += NV - i;
        return k + (hi - lo);
    }
};

#define CLS_MAX_P2 32

// U[l][v] = d u / d lambda_l at vertex v
template <int D> __device__ __forceinline__ void nodal_gradients(const double* x, double (*U)[D + 1]) {
#pragma unroll
    for (int v = 0; v <= D; ++v)
#pragma unroll
        for (int l = 0; l <= D; ++l) U[l][v] = (l == v) ? 3.0 * x[v] : fma(4.0, x[P2<D>::edge(v, l)], -x[l]);
}

// y[a] (+)= sum_{l, v} H[l][v] * d phi_a / d lambda_l (v)
template <int D, bool ADD> __device__ __forceinline__ void project_gradients(const double (*H)[D + 1], double* y) {
    constexpr int NV = D + 1;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        double s = 3.0 * H[a][a];
#pragma unroll
        for (int v = 0; v < NV; ++v)
            if (v != a) s -= H[a][v];
        y[a] = ADD ? y[a] + s : s;
    }
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int b = a + 1; b < NV; ++b) {
            const double s = 4.0 * (H[a][b] + H[b][a]);
            y[P2<D>::edge(a, b)] = ADD ? y[P2<D>::edge(a, b)] + s : s;
        }
}

// W[v][v'] = sum_b coef[b] M3[b][pair(v, v')]
template <int D> __device__ __forceinline__ void pair_matrix(const double* coef, double (*W)[D + 1]) {
    constexpr int NV = D + 1, ND = P2<D>::ND;
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int b = a; b < NV; ++b) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < ND; ++k) s = fma(coef[k], P2Tab<D>::M3[k][P2<D>::pair(a, b)], s);
            W[a][b] = s;
            W[b][a] = s;
        }
}

// normal derivative at the D facet vertices from a frame vector F = [apex | fv | fe | ae]
template <int D> __device__ __forceinline__ void dn_vertices(const double* F, double gnA, const double* gnV, double* out) {
#pragma unroll
    for (int m = 0; m < D; ++m) {
        double s = 3.0 * gnV[m] * F[1 + m];
        s = fma(gnA, fma(4.0, F[P2<D>::ae(m)], -F[0]), s);
#pragma unroll
        for (int mp = 0; mp < D; ++mp)
            if (mp != m) s = fma(gnV[mp], fma(4.0, F[P2<D>::fe(m, mp)], -F[1 + mp]), s);
        out[m] = s;
    }
}

// y (cell dofs) += sum_m T[m] * (normal derivative of the own basis functions at facet vertex m); frame of local facet I
template <int D, int I> __device__ __forceinline__ void back_project(const double* T, double gnA, const double* gnV, double* y) {
#pragma unroll
    for (int m = 0; m < D; ++m) {
        y[P2<D>::fs(I, 1 + m)] = fma(3.0 * gnV[m], T[m], y[P2<D>::fs(I, 1 + m)]);
        y[P2<D>::fs(I, 0)] = fma(-gnA, T[m], y[P2<D>::fs(I, 0)]);
        y[P2<D>::fs(I, P2<D>::ae(m))] = fma(4.0 * gnA, T[m], y[P2<D>::fs(I, P2<D>::ae(m))]);
#pragma unroll
        for (int mp = 0; mp < D; ++mp)
            if (mp != m) {
                y[P2<D>::fs(I, 1 + mp)] = fma(-gnV[mp], T[m], y[P2<D>::fs(I, 1 + mp)]);
                y[P2<D>::fs(I, P2<D>::fe(m, mp))] = fma(4.0 * gnV[mp], T[m], y[P2<D>::fs(I, P2<D>::fe(m, mp))]);
            }
    }
}

template <int D> __device__ __forceinline__ uint64_t frame_packed(int j) {
    constexpr uint64_t p0 = P2<D>::packed(0), p1 = P2<D>::packed(1), p2 = P2<D>::packed(2), p3 = P2<D>::packed(D == 3 ? 3 : 0);
    static_assert(p0 == P2Tab<D>::FRAME_PACKED[0] && p1 == P2Tab<D>::FRAME_PACKED[1] && p2 == P2Tab<D>::FRAME_PACKED[2] &&
                  p3 == P2Tab<D>::FRAME_PACKED[D == 3 ? 3 : 0], "frame permutation disagrees with the generated table");
    uint64_t p = p0;
    if (j == 1) p = p1;
    if (j == 2) p = p2;
    if (D == 3 && j == 3) p = p3;
    return p;
}

// Workgroup staging: the block's own nodal vectors in LDS ([cell][ND]); vectors A and B (x and kappa | x and phi)
template <int D> struct StageP2 {
    const lds_double* a;
    const lds_double* b;
    int64_t c0;
    unsigned nvalid;        // 0: nothing staged (setup kernels)
};

// neighbour's vector in its facet frame, slots [S0, S1): LDS for in-block neighbours, exec-masked global gather otherwise
template <int D, int S0, int S1>
__device__ __forceinline__ void load_frame(const lds_double* l, const double* __restrict__ g, bool in_block, uint64_t packed, double* out) {
    double vg[S1 - S0];
#pragma unroll
    for (int s = S0; s < S1; ++s) {
        const unsigned dof = (unsigned)(packed >> (4 * s)) & 15u;
        out[s - S0] = l[dof];
        vg[s - S0] = 0.0;
    }
    if (!in_block) {
#pragma unroll
        for (int s = S0; s < S1; ++s) vg[s - S0] = g[(unsigned)(packed >> (4 * s)) & 15u];
    }
#pragma unroll
    for (int s = S0; s < S1; ++s) out[s - S0] = in_block ? out[s - S0] : vg[s - S0];
}

// per-facet geometry: own barycentric coordinates of the neighbour's apex, |g_i|, 2 / (h + h')
template <int D, int I, bool CLS>
__device__ __forceinline__ void facet_geometry(const MeshDev& m, const CellGeom<D>& K, const lds_double* rec, int64_t c, int64_t Kp, int j,
                                               double* L, double& sqG, double& hinv) {
    constexpr int NV = D + 1;
    if (CLS) {
#pragma unroll
        for (int a = 0; a < NV; ++a) L[a] = rec[11 + 6 * I + a];
        sqG = rec[11 + 6 * I + 4];
        hinv = rec[11 + 6 * I + 5];
    } else {
        double Xo[D];
        load_vertex<D>(m.coords, m.cells[Kp * NV + j], Xo);
        apex_bary<D>(K, Xo, L);
        sqG = fast_sqrt(K.G[I][I]);
        hinv = fast_rcp(0.5 * (m.h[c] + m.h[Kp]));
    }
}

// the cell behind local facet I, decoded from the facet's flag byte fb: its local facet index, its frame permutation and where its
// vectors are found.  MODE 0: apply; MODE 1: cell-diagonal block (nothing staged)
template <int D> struct NeighbourP2 { int j; int64_t Kp; uint64_t packed; bool in_block; unsigned loc; };
template <int D, int I, int MODE> __device__ __forceinline__ NeighbourP2<D> facet_neighbour(uint32_t fb, const int* nb, const StageP2<D>& st) {
    NeighbourP2<D> n;
    n.j = (int)(fb & 3u);
    n.Kp = nb[I];
    n.packed = frame_packed<D>(n.j);
    const unsigned loc0 = (unsigned)(n.Kp - st.c0);
    n.in_block = MODE == 0 && loc0 < st.nvalid;
    n.loc = n.in_block ? loc0 : 0u;
    return n;
}

// area of local facet I (sqG = |g_I|) and the normal derivatives of the barycentric coordinates on both sides of it:
// n = -g_I / |g_I|:  grad(lambda_l) . n = -G_lI / |g_I|;  neighbour basis through the apex coordinates L (cell_geom.hpp).
// gnA / gnV[m]: own apex / facet vertex m;  gr / gnVn[m]: the neighbour's.  area_only: all a membrane facet needs
template <int D> struct FacetNormals { double area, gnA, gr, gnV[D], gnVn[D]; };
template <int D, int I>
__device__ __forceinline__ void facet_normals(const CellGeom<D>& K, const double* L, double sqG, bool area_only, FacetNormals<D>& N) {
    N.area = sqG * (double)D * K.vol;
    if (area_only) return;
    const double rs = fast_rcp(sqG);
    N.gnA = -sqG;
    N.gr = N.gnA * fast_rcp(L[I]);
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        N.gnV[mm] = -K.G[mm + (mm >= I)][I] * rs;
        N.gnVn[mm] = fma(-L[mm + (mm >= I)], N.gr, N.gnV[mm]);
    }
}

// ---- monomial-product form of the triangle-facet integrals (p2_mono_tables.hpp; tools/gen_p2_tables.py: mono_tables) --------------
// a P2 trace given by its six facet-node values (v0 v1 v2 e01 e02 e12) as a polynomial in the facet's barycentric coordinates:
// coefficients of l0^2 l1^2 l2^2 l0l1 l0l2 l1l2  (Lagrange P2 with 1 = l0 + l1 + l2 folded in)
__device__ __forceinline__ void p2_to_mono(const double* u, double* a) {
    a[0] = u[0]; a[1] = u[1]; a[2] = u[2];
    a[3] = fma(4.0, u[3], -(u[0] + u[1]));
    a[4] = fma(4.0, u[4], -(u[0] + u[2]));
    a[5] = fma(4.0, u[5], -(u[1] + u[2]));
}
// q (degree 4, 15 coefficients) = a * b for two degree-2 polynomials; the index map is a compile-time table, so every q[.] is a register
__device__ __forceinline__ void mono_mul22(const double* a, const double* b, double* q) {
#pragma unroll
    for (int k = 0; k < P2Mono::N4; ++k) q[k] = 0.0;
#pragma unroll
    for (int i = 0; i < P2Mono::N2; ++i)
#pragma unroll
        for (int j = 0; j < P2Mono::N2; ++j) q[P2Mono::IDX22[i][j]] = fma(a[i], b[j], q[P2Mono::IDX22[i][j]]);
}
// c (degree 3, 10 coefficients) += a (degree 2) * sum_m d[m] l_m
__device__ __forceinline__ void mono_mul21_add(const double* a, const double* d, double* c) {
#pragma unroll
    for (int i = 0; i < P2Mono::N2; ++i)
#pragma unroll
        for (int m = 0; m < 3; ++m) c[P2Mono::IDX21[i][m]] = fma(a[i], d[m], c[P2Mono::IDX21[i][m]]);
}

template <int ND> __device__ __forceinline__ void load_cellvec(const double* __restrict__ p, int64_t c, double* v) {
    const double2* q = reinterpret_cast<const double2*>(p + (int64_t)ND * c);
#pragma unroll
    for (int k = 0; k < ND / 2; ++k) { const double2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
}
template <int ND> __device__ __forceinline__ void store_cellvec(double* __restrict__ p, int64_t c, const double* v) {
    double2* q = reinterpret_cast<double2*>(p + (int64_t)ND * c);
#pragma unroll
    for (int k = 0; k < ND / 2; ++k) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
}

template <int D, bool CLS> __device__ __forceinline__ void cell_geometry_p2(const MeshDev& m, int64_t c, const lds_double* rec, CellGeom<D>& K) {
    if (CLS) class_gram<D>(rec, K);
    else load_cell_geometry<D>(m, c, K);
}

// Prologue of the two apply kernels for the block whose first cell is c0 (the kernel has returned if that lies past the range): thread t takes
// cell c = c0 + t, loads its neighbours, flags, class and its nodal vectors av / bv, stages the two vectors in s_a / s_b ([BLK][ND]) and the
// class table in s_tab, and fills st.  Returns whether c is a cell; the caller's __syncthreads() follows.
template <int D, int BLK, bool CLS>
__device__ __forceinline__ bool stage_block_p2(const MeshDev& m, int64_t c0, const double* __restrict__ a, const double* __restrict__ b, double* s_a,
                                               double* s_b, double* s_tab, int64_t& c, int* nb, uint32_t& flags, unsigned& cls, double* av,
                                               double* bv, StageP2<D>& st) {
    constexpr int ND = P2<D>::ND;
    c = c0 + threadIdx.x;
    const bool valid = c < m.c_end;
    if (CLS)
        for (int i = threadIdx.x; i < m.ncls * KNP_CLS_STRIDE; i += BLK) s_tab[i] = m.cls_table[i];
    flags = 0;
    cls = 0;
    if (valid) {
        load_cell_ints<D>(m.nbr, c, nb);
        flags = m.fflag[c];
        if (CLS) cls = m.cls[c];
        load_cellvec<ND>(a, c, av);
        load_cellvec<ND>(b, c, bv);
        const unsigned t = threadIdx.x;
#pragma unroll
        for (int k = 0; k < ND; ++k) { s_a[t * ND + k] = av[k]; s_b[t * ND + k] = bv[k]; }
    }
    st = StageP2<D>{TO_LDS(s_a), TO_LDS(s_b), c0, (unsigned)((m.c_end - c0 < BLK) ? (m.c_end - c0) : BLK)};
    return valid;
}
