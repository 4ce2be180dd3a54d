// Matrix-free DG-P2 operator applies (EMI potential operator, KNP species operator) and their cell-diagonal blocks.
//
// Replaces, for Solver(degree_emi=2, degree_knp=2) (reference: tests/run_MMS_space.py:194-195, src/knpemidg/solver.py:157-175):
//   dolfin.assemble(a_emi) + PETSc MatMult   src/knpemidg/solver.py:325-328, 346, 477, 509
//   dolfin.assemble(A_knp) + PETSc MatMult   src/knpemidg/solver.py:586-594, 730, 771
// Round 1 integrated these forms into dense cell blocks once per time step (4 KB per cell and operator, 12 GB at 10^6 tets)
// and streamed them in every Krylov iteration: HBM-bound on 16-20x the algorithmic bytes.  Here nothing is assembled:
//
//  * cells:  grad u is P1, so  int coef grad u . grad v  =  vol sum_{ll'} G_ll' sum_{vv'} W_vv' U_l(v) V_l'(v')  with the nodal
//            gradient values U_l(v) = d u / d lambda_l at vertex v and  W_vv' = sum_b coef_b M3[b][vv']  (reference tensor
//            M3 = int phi_b lambda_v lambda_v', p2_tables.hpp): exact, 300 FMAs per cell instead of a 27-point rule;
//  * facets: everything is evaluated in the FACET FRAME [apex | facet vertices | facet edges | apex edges]: the own cell's
//            frame is a compile-time permutation of its registers, the neighbour's 10 dofs are gathered through a nibble-
//            packed permutation selected by its local facet index, after which both sides share the same facet basis:
//            traces are P2 on the facet (D(D+1)/2 nodes), normal derivatives are P1 (D vertex values), and the integrals
//            run over the facet rule of p2_tables.hpp (degree 6 for a_emi: exact; degree 5 = FIAT's points for a_knp, whose
//            upwind speed |D grad(phi).n| is not a polynomial);
//  * geometry in Gram form (cell_geom.hpp): class records on (block-)structured meshes, vertex coordinates otherwise.
//
// One thread per cell (EMI) / per (cell, species) (KNP); the workgroup's own x and coefficient live in LDS, where ~83 % of the
// facet neighbours of a Morton-ordered block are found.  FP64 vector FMAs: on MI355X the FP64 matrix rate equals the vector
// rate, the facet contractions are 12 x 6 / 7 x 6 (padding to 16 x 16 x 4 MFMA tiles wastes > 40 %), and the sparse P2
// gradient structure (4 of 40 entries per point) is exploited here; see DESIGN.md section 4b for the measured comparison.
// The numpy restatement of exactly this formulation is tests/p2_formulation.py (checked against the oracle on the CPU: tests/test_p2_formulation_host.py).
#include "../../include/knpemi_hip.h"
#include "p2_frame.hpp"
#include <cstdlib>

namespace {

// ------------------------------------------------------------------------------------------------------------------
// EMI:  y = A(kappa) x     (forms: apply_p1.hip header; reference solver.py:325-328, 346)
// ------------------------------------------------------------------------------------------------------------------
// MODE 0: apply; MODE 1: cell-diagonal block (neighbour values 0, neighbour coefficient from global memory)
template <int D, int I, bool CLS, int MODE>
__device__ __forceinline__ void emi_facet_p2(const MeshDev& m, const CellGeom<D>& K, const lds_double* rec, int64_t c, const int* nb,
                                             uint32_t flags, const double* xv, const double* kv, const double* __restrict__ x,
                                             const double* __restrict__ kappa, const StageP2<D>& st, double C_phi, double tau,
                                             double* y) {
    constexpr int NV = D + 1, ND = P2<D>::ND, NF = P2<D>::NF;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    const uint32_t kind = (fb >> 2) & 3u;
    if (kind >= FK_EXTERIOR) return;
    const NeighbourP2<D> n2 = facet_neighbour<D, I, MODE>(fb, nb, st);
    double Fn[ND], Kn[NF];
    if (MODE == 0) {
        load_frame<D, 0, ND>(st.a + n2.loc * ND, x + n2.Kp * ND, n2.in_block, n2.packed, Fn);
        load_frame<D, 1, 1 + NF>(st.b + n2.loc * ND, kappa + n2.Kp * ND, n2.in_block, n2.packed, Kn);
    } else {
#pragma unroll
        for (int s = 0; s < ND; ++s) Fn[s] = 0.0;
#pragma unroll
        for (int s = 0; s < NF; ++s) Kn[s] = kappa[n2.Kp * ND + ((unsigned)(n2.packed >> (4 * (1 + s))) & 15u)];
    }
    double ju[NF];
#pragma unroll
    for (int n = 0; n < NF; ++n) ju[n] = xv[P2<D>::fs(I, 1 + n)] - Fn[1 + n];
    double L[NV], sqG, hinv;
    facet_geometry<D, I, CLS>(m, K, rec, c, n2.Kp, n2.j, L, sqG, hinv);
    FacetNormals<D> N;
    facet_normals<D, I>(K, L, sqG, kind == FK_MEMBRANE, N);
    if (kind == FK_MEMBRANE) {
        const double w = C_phi * N.area;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < NF; ++k) s = fma(P2Tab<D>::FMASS[n][k], ju[k], s);
            y[P2<D>::fs(I, 1 + n)] = fma(w, s, y[P2<D>::fs(I, 1 + n)]);
        }
        return;
    }
    double Fo[ND];
#pragma unroll
    for (int s = 0; s < ND; ++s) Fo[s] = xv[P2<D>::fs(I, s)];
    double dno[D], dnn[D];
    dn_vertices<D>(Fo, N.gnA, N.gnV, dno);
    dn_vertices<D>(Fn, N.gr, N.gnVn, dnn);
    const double pen = 0.5 * tau * hinv;
    double r[NF], T[D];
#pragma unroll
    for (int n = 0; n < NF; ++n) r[n] = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) T[mm] = 0.0;
    if constexpr (D == 3) {
        // Round 4: every integrand of a_emi is a polynomial of degree <= 6 on the facet (kappa, [u] P2; d_n u P1; test function P2 / P1), so
        // the traces are multiplied AS POLYNOMIALS in the facet's barycentric coordinates and the products integrated exactly
        // against the test functions (tables of p2_mono_tables.hpp) instead of being sampled at the 12 points of the degree-6 rule:
        //   flux = pen (ko + kn) [u] - 1/2 (ko d_n u + kn d_n u')    degree 4 (the cubic part times 1 = l0 + l1 + l2)
        //   t    = -1/2 ko [u]                                          degree 4
        // 327 instead of 480 FP64 instructions per facet (profiles/r04_p2_mono.txt); same numbers to rounding (any exact rule gives them).
        double kon[NF], kom[NF], knm[NF], jm[NF], sm[NF];
#pragma unroll
        for (int n = 0; n < NF; ++n) kon[n] = kv[P2<D>::fs(I, 1 + n)];
        p2_to_mono(kon, kom);
        p2_to_mono(Kn, knm);
        p2_to_mono(ju, jm);
#pragma unroll
        for (int n = 0; n < NF; ++n) sm[n] = kom[n] + knm[n];
        double q4[P2Mono::N4], t4[P2Mono::N4], c3[P2Mono::N3];
        mono_mul22(sm, jm, q4);
        mono_mul22(kom, jm, t4);
        double hdo[D], hdn[D];
#pragma unroll
        for (int mm = 0; mm < D; ++mm) { hdo[mm] = -0.5 * dno[mm]; hdn[mm] = -0.5 * dnn[mm]; }
#pragma unroll
        for (int k = 0; k < P2Mono::N3; ++k) c3[k] = 0.0;
        mono_mul21_add(kom, hdo, c3);
        mono_mul21_add(knm, hdn, c3);
        // g = pen q4 + (l0 + l1 + l2) c3, held in q4's registers
#pragma unroll
        for (int k = 0; k < P2Mono::N4; ++k) q4[k] *= pen;
#pragma unroll
        for (int k = 0; k < P2Mono::N3; ++k)
#pragma unroll
            for (int mm = 0; mm < 3; ++mm) q4[P2Mono::IDX31[k][mm]] += c3[k];
#pragma unroll
        for (int k = 0; k < P2Mono::N4; ++k) {
#pragma unroll
            for (int n = 0; n < NF; ++n) r[n] = fma(q4[k], P2Mono::I4[k][n], r[n]);
#pragma unroll
            for (int mm = 0; mm < D; ++mm) T[mm] = fma(t4[k], P2Mono::I4L[k][mm], T[mm]);
        }
        const double ht = -0.5 * N.area;
#pragma unroll
        for (int n = 0; n < NF; ++n) r[n] *= N.area;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) T[mm] *= ht;
    } else {
#pragma unroll
    for (int q = 0; q < P2Tab<D>::NQE; ++q) {
        double ko = 0.0, kn = 0.0, jq = 0.0, do_ = 0.0, dn_ = 0.0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const double p = P2Tab<D>::PSIE[q][n];
            ko = fma(kv[P2<D>::fs(I, 1 + n)], p, ko);
            kn = fma(Kn[n], p, kn);
            jq = fma(ju[n], p, jq);
        }
#pragma unroll
        for (int mm = 0; mm < D; ++mm) {
            do_ = fma(dno[mm], P2Tab<D>::LAME[q][mm], do_);
            dn_ = fma(dnn[mm], P2Tab<D>::LAME[q][mm], dn_);
        }
        const double w = P2Tab<D>::WE[q] * N.area;
        const double flux = w * fma(pen * (ko + kn), jq, -0.5 * fma(ko, do_, kn * dn_));
        const double t = -0.5 * w * ko * jq;
#pragma unroll
        for (int n = 0; n < NF; ++n) r[n] = fma(flux, P2Tab<D>::PSIE[q][n], r[n]);
#pragma unroll
        for (int mm = 0; mm < D; ++mm) T[mm] = fma(t, P2Tab<D>::LAME[q][mm], T[mm]);
    }
    }
#pragma unroll
    for (int n = 0; n < NF; ++n) y[P2<D>::fs(I, 1 + n)] += r[n];
    back_project<D, I>(T, N.gnA, N.gnV, y);
}

template <int D, bool CLS, int MODE>
__device__ __forceinline__ void emi_cell_p2(const MeshDev& m, const CellGeom<D>& K, const lds_double* rec, int64_t c, const int* nb,
                                            uint32_t flags, const double* xv, const double* kv, const double* __restrict__ x,
                                            const double* __restrict__ kappa, const StageP2<D>& st, double C_phi, double tau,
                                            double* y) {
    constexpr int NV = D + 1;
    {
        double U[NV][NV], W[NV][NV], H[NV][NV];
        nodal_gradients<D>(xv, U);
        pair_matrix<D>(kv, W);
        // T = G U (in U's place would need a copy: H holds T, then H <- vol T W)
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < NV; ++l) s = fma(K.G[k][l], U[l][v], s);
                H[k][v] = s * K.vol;
            }
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double row[NV];
#pragma unroll
            for (int w = 0; w < NV; ++w) {
                double s = 0.0;
#pragma unroll
                for (int v = 0; v < NV; ++v) s = fma(H[k][v], W[v][w], s);
                row[w] = s;
            }
#pragma unroll
            for (int w = 0; w < NV; ++w) U[k][w] = row[w];
        }
        project_gradients<D, false>(U, y);
    }
    emi_facet_p2<D, 0, CLS, MODE>(m, K, rec, c, nb, flags, xv, kv, x, kappa, st, C_phi, tau, y);
    emi_facet_p2<D, 1, CLS, MODE>(m, K, rec, c, nb, flags, xv, kv, x, kappa, st, C_phi, tau, y);
    emi_facet_p2<D, 2, CLS, MODE>(m, K, rec, c, nb, flags, xv, kv, x, kappa, st, C_phi, tau, y);
    if (D == 3) emi_facet_p2<D, (D == 3 ? 3 : 0), CLS, MODE>(m, K, rec, c, nb, flags, xv, kv, x, kappa, st, C_phi, tau, y);
}

template <int D, int BLK, bool CLS>
__global__ __launch_bounds__(BLK) void k_emi_apply_p2(MeshDev m, const double* __restrict__ x, const double* __restrict__ kappa,
                                                      double* __restrict__ y, double C_phi, double tau) {
    constexpr int NV = D + 1, ND = P2<D>::ND;
    __shared__ __attribute__((aligned(16))) double s_x[BLK * ND];
    __shared__ __attribute__((aligned(16))) double s_k[BLK * ND];
    __shared__ __attribute__((aligned(16))) double s_tab[CLS ? CLS_MAX_P2 * KNP_CLS_STRIDE : 2];
    const int64_t c0 = m.c_begin + xcd_block(blockIdx.x, gridDim.x) * BLK;
    if (c0 >= m.c_end) return;
    int64_t c;
    int nb[NV];
    uint32_t flags;
    unsigned cls;
    double xv[ND], kv[ND], yv[ND];
    StageP2<D> st;
    const bool valid = stage_block_p2<D, BLK, CLS>(m, c0, x, kappa, s_x, s_k, s_tab, c, nb, flags, cls, xv, kv, st);
    __syncthreads();
    if (!valid) return;
    const lds_double* rec = TO_LDS(s_tab) + cls * KNP_CLS_STRIDE;
    CellGeom<D> K;
    cell_geometry_p2<D, CLS>(m, c, rec, K);
    emi_cell_p2<D, CLS, 0>(m, K, rec, c, nb, flags, xv, kv, x, kappa, st, C_phi, tau, yv);
    store_cellvec<ND>(y, c, yv);
}

// ------------------------------------------------------------------------------------------------------------------
// KNP:  y_k = A_k x_k, one species per blockIdx.y    (reference solver.py:586-594)
//   cells:  1/dt M + D K + z psi D int u grad(phi).grad(v);   facets dS(0): consistency, adjoint consistency, penalty on
//   jump(D u), upwind drift  -z psi jump(v) jump(un u),  un = max(D grad(phi).n_own, 0) sampled at the degree-5 facet points
// ------------------------------------------------------------------------------------------------------------------
template <int D, int I, bool CLS, int MODE>
__device__ __forceinline__ void knp_facet_p2(const MeshDev& m, const CellGeom<D>& K, const lds_double* rec, int64_t c, const int* nb,
                                             uint32_t flags, const double* xv, const double* pv, double Dc, double zp,
                                             const double* __restrict__ x, const double* __restrict__ phi,
                                             const double* __restrict__ Dspec, const StageP2<D>& st, double tau, double* y) {
    constexpr int NV = D + 1, ND = P2<D>::ND, NF = P2<D>::NF;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    if (((fb >> 2) & 3u) != FK_SIPG) return;
    const NeighbourP2<D> n2 = facet_neighbour<D, I, MODE>(fb, nb, st);
    double L[NV], sqG, hinv;
    facet_geometry<D, I, CLS>(m, K, rec, c, n2.Kp, n2.j, L, sqG, hinv);
    FacetNormals<D> N;
    facet_normals<D, I>(K, L, sqG, false, N);
    const double D2 = Dspec[n2.Kp];
    // upwind speeds at the facet vertices (P1 along the facet): own side with n, neighbour side with -n
    double sp[D], sm[D];
    {
        double Po[ND], Pn[ND];
#pragma unroll
        for (int s = 0; s < ND; ++s) Po[s] = pv[P2<D>::fs(I, s)];
        if (MODE == 0) load_frame<D, 0, ND>(st.b + n2.loc * ND, phi + n2.Kp * ND, n2.in_block, n2.packed, Pn);
        else {
#pragma unroll
            for (int s = 0; s < ND; ++s) Pn[s] = phi[n2.Kp * ND + ((unsigned)(n2.packed >> (4 * s)) & 15u)];
        }
        dn_vertices<D>(Po, N.gnA, N.gnV, sp);
        dn_vertices<D>(Pn, N.gr, N.gnVn, sm);
#pragma unroll
        for (int mm = 0; mm < D; ++mm) { sp[mm] *= Dc; sm[mm] *= -D2; }
    }
    double Fo[ND], Fn[ND];
#pragma unroll
    for (int s = 0; s < ND; ++s) Fo[s] = xv[P2<D>::fs(I, s)];
    if (MODE == 0) load_frame<D, 0, ND>(st.a + n2.loc * ND, x + n2.Kp * ND, n2.in_block, n2.packed, Fn);
    else {
#pragma unroll
        for (int s = 0; s < ND; ++s) Fn[s] = 0.0;
    }
    double dno[D], dnn[D];
    dn_vertices<D>(Fo, N.gnA, N.gnV, dno);
    dn_vertices<D>(Fn, N.gr, N.gnVn, dnn);
    const double pen = tau * hinv;
    double r[NF], T[D];
#pragma unroll
    for (int n = 0; n < NF; ++n) r[n] = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) T[mm] = 0.0;
#pragma unroll
    for (int q = 0; q < P2Tab<D>::NQK; ++q) {
        double uo = 0.0, un = 0.0, do_ = 0.0, dn_ = 0.0, so = 0.0, sn = 0.0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const double p = P2Tab<D>::PSIK[q][n];
            uo = fma(Fo[1 + n], p, uo);
            un = fma(Fn[1 + n], p, un);
        }
#pragma unroll
        for (int mm = 0; mm < D; ++mm) {
            const double l = P2Tab<D>::LAMK[q][mm];
            do_ = fma(dno[mm], l, do_);
            dn_ = fma(dnn[mm], l, dn_);
            so = fma(sp[mm], l, so);
            sn = fma(sm[mm], l, sn);
        }
        const double upo = fmax(so, 0.0), upn = fmax(sn, 0.0);
        const double w = P2Tab<D>::WK[q] * N.area;
        // -1/2 (D dn u + D' dn u') + pen (D u - D' u') - z psi (un u - un' u')
        const double flux = w * (fma(fma(pen, Dc, -zp * upo), uo, -fma(pen, D2, -zp * upn) * un) - 0.5 * fma(Dc, do_, D2 * dn_));
        const double t = -0.5 * w * Dc * (uo - un);
#pragma unroll
        for (int n = 0; n < NF; ++n) r[n] = fma(flux, P2Tab<D>::PSIK[q][n], r[n]);
#pragma unroll
        for (int mm = 0; mm < D; ++mm) T[mm] = fma(t, P2Tab<D>::LAMK[q][mm], T[mm]);
    }
#pragma unroll
    for (int n = 0; n < NF; ++n) y[P2<D>::fs(I, 1 + n)] += r[n];
    back_project<D, I>(T, N.gnA, N.gnV, y);
}

template <int D, bool CLS, int MODE>
__device__ __forceinline__ void knp_cell_p2(const MeshDev& m, const CellGeom<D>& K, const lds_double* rec, int64_t c, const int* nb,
                                            uint32_t flags, const double* xv, const double* pv, double Dc, double zp, double inv_dt,
                                            const double* __restrict__ x, const double* __restrict__ phi,
                                            const double* __restrict__ Dspec, const StageP2<D>& st, double tau, double* y) {
    constexpr int NV = D + 1, ND = P2<D>::ND;
    {
        // H[k][w] = D vol ( sum_l G_kl Z_l(w) + z psi sum_v (G P)_k(v) Q[v][w] ),  Z = M1 U,  Q = pair matrix of x
        double U[NV][NV], Q[NV][NV], H[NV][NV];
        nodal_gradients<D>(xv, U);
        constexpr double m1 = 1.0 / (double)((D + 1) * (D + 2));
#pragma unroll
        for (int l = 0; l < NV; ++l) {
            double su = 0.0;
#pragma unroll
            for (int v = 0; v < NV; ++v) su += U[l][v];
#pragma unroll
            for (int v = 0; v < NV; ++v) U[l][v] = m1 * (U[l][v] + su);
        }
        const double dv = Dc * K.vol;
#pragma unroll
        for (int k = 0; k < NV; ++k)
#pragma unroll
            for (int w = 0; w < NV; ++w) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < NV; ++l) s = fma(K.G[k][l], U[l][w], s);
                H[k][w] = dv * s;
            }
        pair_matrix<D>(xv, Q);
        nodal_gradients<D>(pv, U);                      // U <- nodal gradients of phi
        const double dz = dv * zp;
#pragma unroll
        for (int k = 0; k < NV; ++k) {
            double gp[NV];                              // grad(phi) . grad(lambda_k) at the vertices
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < NV; ++l) s = fma(K.G[k][l], U[l][v], s);
                gp[v] = s * dz;
            }
#pragma unroll
            for (int w = 0; w < NV; ++w) {
                double s = H[k][w];
#pragma unroll
                for (int v = 0; v < NV; ++v) s = fma(gp[v], Q[v][w], s);
                H[k][w] = s;
            }
        }
        project_gradients<D, false>(H, y);
        const double mw = inv_dt * K.vol;
#pragma unroll
        for (int a = 0; a < ND; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < ND; ++b) s = fma(P2Tab<D>::MASS[a][b], xv[b], s);
            y[a] = fma(mw, s, y[a]);
        }
    }
    knp_facet_p2<D, 0, CLS, MODE>(m, K, rec, c, nb, flags, xv, pv, Dc, zp, x, phi, Dspec, st, tau, y);
    knp_facet_p2<D, 1, CLS, MODE>(m, K, rec, c, nb, flags, xv, pv, Dc, zp, x, phi, Dspec, st, tau, y);
    knp_facet_p2<D, 2, CLS, MODE>(m, K, rec, c, nb, flags, xv, pv, Dc, zp, x, phi, Dspec, st, tau, y);
    if (D == 3) knp_facet_p2<D, (D == 3 ? 3 : 0), CLS, MODE>(m, K, rec, c, nb, flags, xv, pv, Dc, zp, x, phi, Dspec, st, tau, y);
}

template <int D, int BLK, bool CLS>
__global__ __launch_bounds__(BLK) void k_knp_apply_p2(MeshDev m, const double* __restrict__ x_all, const double* __restrict__ phi,
                                                      const double* __restrict__ Dall, double* __restrict__ y_all, KnpOpArgs ka) {
    constexpr int NV = D + 1, ND = P2<D>::ND;
    __shared__ __attribute__((aligned(16))) double s_x[BLK * ND];
    __shared__ __attribute__((aligned(16))) double s_p[BLK * ND];
    __shared__ __attribute__((aligned(16))) double s_tab[CLS ? CLS_MAX_P2 * KNP_CLS_STRIDE : 2];
    const int64_t c0 = m.c_begin + xcd_block(blockIdx.x, gridDim.x) * BLK;
    if (c0 >= m.c_end) return;
    const int sp = blockIdx.y;
    const double* x = x_all + (int64_t)sp * m.nc * ND;
    const double* Dspec = Dall + (int64_t)sp * m.nc;
    int64_t c;
    int nb[NV];
    uint32_t flags;
    unsigned cls;
    double xv[ND], pv[ND], yv[ND];
    StageP2<D> st;
    const bool valid = stage_block_p2<D, BLK, CLS>(m, c0, x, phi, s_x, s_p, s_tab, c, nb, flags, cls, xv, pv, st);
    __syncthreads();
    if (!valid) return;
    const double Dc = Dspec[c];
    const lds_double* rec = TO_LDS(s_tab) + cls * KNP_CLS_STRIDE;
    CellGeom<D> K;
    cell_geometry_p2<D, CLS>(m, c, rec, K);
    knp_cell_p2<D, CLS, 0>(m, K, rec, c, nb, flags, xv, pv, Dc, ka.z[sp] * ka.psi, ka.inv_dt, x, phi, Dspec, st, ka.tau, yv);
    store_cellvec<ND>(y_all + (int64_t)sp * m.nc * ND, c, yv);
}

// ------------------------------------------------------------------------------------------------------------------
// Cell-diagonal blocks and their inverses (block-Jacobi).  ND threads per cell: thread (cell, b) applies the cell-local
// operator to the unit vector e_b (neighbour values 0), the block is transposed through LDS so that thread r holds row r,
// and the ND threads of a cell run an in-register Gauss-Jordan with the pivot row broadcast through LDS.
// ------------------------------------------------------------------------------------------------------------------
template <int D, bool EMI, int CPB>
__global__ __launch_bounds__(CPB * P2<D>::ND) void k_p2_blockjacobi(MeshDev m, const double* __restrict__ coef, const double* __restrict__ Dall,
                                                                    bjreal* __restrict__ binv_all, double C_phi, double tau, KnpOpArgs ka) {
    constexpr int NV = D + 1, ND = P2<D>::ND;
    __shared__ double M[CPB][ND][ND + 1];
    __shared__ double prow[CPB][ND];
    const int ci = threadIdx.x / ND, b = threadIdx.x % ND;
    const int64_t c = (int64_t)blockIdx.x * CPB + ci;
    const int sp = blockIdx.y;
    const bool valid = c < m.nc_owned;
    double col[ND];
    if (valid) {
        int nb[NV];
        load_cell_ints<D>(m.nbr, c, nb);
        const uint32_t flags = m.fflag[c];
        CellGeom<D> K;
        cell_geometry_p2<D, false>(m, c, nullptr, K);
        double e[ND], cv[ND];
#pragma unroll
        for (int a = 0; a < ND; ++a) e[a] = (a == b) ? 1.0 : 0.0;
        load_cellvec<ND>(coef, c, cv);
        StageP2<D> st{nullptr, nullptr, 0, 0u};
        if (EMI) {
            emi_cell_p2<D, false, 1>(m, K, nullptr, c, nb, flags, e, cv, nullptr, coef, st, C_phi, tau, col);
        } else {
            const double* Dspec = Dall + (int64_t)sp * m.nc;
            knp_cell_p2<D, false, 1>(m, K, nullptr, c, nb, flags, e, cv, Dspec[c], ka.z[sp] * ka.psi, ka.inv_dt, nullptr, coef, Dspec, st,
                                     ka.tau, col);
        }
#pragma unroll
        for (int a = 0; a < ND; ++a) M[ci][a][b] = col[a];
    }
    __syncthreads();
    double row[ND];
#pragma unroll
    for (int k = 0; k < ND; ++k) row[k] = valid ? M[ci][b][k] : (k == b ? 1.0 : 0.0);
#pragma unroll
    for (int p = 0; p < ND; ++p) {
        if (b == p) {
            const double inv = 1.0 / row[p];
            row[p] = 1.0;
#pragma unroll
            for (int k = 0; k < ND; ++k) { row[k] *= inv; prow[ci][k] = row[k]; }
        }
        __syncthreads();
        if (b != p) {
            const double f = row[p];
            row[p] = 0.0;
#pragma unroll
            for (int k = 0; k < ND; ++k) row[k] = fma(-f, prow[ci][k], row[k]);
        }
        __syncthreads();
    }
    bjreal* dst = binv_all + (int64_t)sp * m.nc * ND * ND + c * ND * ND + b * ND;
    if (EMI) {                                         // exactly symmetric after rounding to fp32 (PCG needs an SPD preconditioner)
#pragma unroll
        for (int k = 0; k < ND; ++k) M[ci][b][k] = row[k];
        __syncthreads();
        if (valid) {
#pragma unroll
            for (int k = 0; k < ND; ++k) dst[k] = (bjreal)(0.5 * (row[k] + M[ci][k][b]));
        }
    } else if (valid) {
#pragma unroll
        for (int k = 0; k < ND; ++k) dst[k] = (bjreal)row[k];
    }
}

}  // namespace

// ---- launchers ---------------------------------------------------------------------------------------------------------
static inline unsigned grid8_for(int64_t n, int blk) { return (unsigned)((((n + blk - 1) / blk + 7) / 8) * 8); }

#define P2_BLK 256

// geometry classes (MeshDev::cls) serve the 3D applies while the class table fits in their LDS copy
static inline bool p2_classed(const knp_ctx* c) { return c->m.cls && c->m.dim == 3 && c->m.ncls <= CLS_MAX_P2; }

// KERN<D, P2_BLK, CLS> over the context's cell range, ny grid rows
#define P2_DISPATCH(c, KERN, ny, ...)                                                                                        \
    do {                                                                                                                     \
        if ((c)->m.c_end <= (c)->m.c_begin) return 0;                                                                        \
        const dim3 g(grid8_for((c)->m.c_end - (c)->m.c_begin, P2_BLK), (unsigned)(ny)), b(P2_BLK);                           \
        if ((c)->m.dim == 3 && p2_classed(c)) hipLaunchKernelGGL((KERN<3, P2_BLK, true>), g, b, 0, (c)->stream, __VA_ARGS__); \
        else if ((c)->m.dim == 3) hipLaunchKernelGGL((KERN<3, P2_BLK, false>), g, b, 0, (c)->stream, __VA_ARGS__);           \
        else hipLaunchKernelGGL((KERN<2, P2_BLK, false>), g, b, 0, (c)->stream, __VA_ARGS__);                                \
        HIPCHK(c, hipGetLastError());                                                                                        \
    } while (0)

int p2_emi_apply(knp_ctx* c, const double* x, const double* kappa, double* y) {
    P2_DISPATCH(c, k_emi_apply_p2, 1, c->m, x, kappa, y, c->p.C_phi, c->p.tau_emi);
    return 0;
}

int p2_knp_apply(knp_ctx* c, const double* x, const double* phi, double* y) {
    P2_DISPATCH(c, k_knp_apply_p2, c->p.n_sys, c->m, x, phi, (const double*)c->D, y, knp_op_args(c));
    return 0;
}

template <int D, int CPB> static void launch_blockjacobi(knp_ctx* c, int which, const double* coef, bjreal* binv) {
    const dim3 g((unsigned)((c->m.nc_owned + CPB - 1) / CPB), (unsigned)(which == 0 ? 1 : c->p.n_sys)), b(CPB * P2<D>::ND);
    if (which == 0) hipLaunchKernelGGL((k_p2_blockjacobi<D, true, CPB>), g, b, 0, c->stream, c->m, coef, (const double*)c->D, binv, c->p.C_phi, c->p.tau_emi, knp_op_args(c));
    else hipLaunchKernelGGL((k_p2_blockjacobi<D, false, CPB>), g, b, 0, c->stream, c->m, coef, (const double*)c->D, binv, c->p.C_phi, c->p.tau_emi, knp_op_args(c));
}

// which 0: EMI blocks from kappa; 1: KNP blocks (all species) from phi
int p2_block_inverse(knp_ctx* c, int which, const double* coef, bjreal* binv) {
    if (c->m.dim == 3) launch_blockjacobi<3, 25>(c, which, coef, binv);
    else launch_blockjacobi<2, 42>(c, which, coef, binv);
    HIPCHK(c, hipGetLastError());
    return 0;
}
