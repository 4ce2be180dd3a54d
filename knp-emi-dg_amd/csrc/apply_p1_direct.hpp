// Coordinate-path kernels of the matrix-free P1 applies (apply_p1.hip): every neighbour access is a global (L1/L2) gather and the
// geometry comes from the vertex coordinates, so they run on any mesh (2D, 3D, with or without geometry classes).  Also the setup
// kernels built from the same cell functions: the block-Jacobi inverses, gphi and the neighbour-material table.
#pragma once
#include "cell_geom.hpp"

// grad(w') . g_i for the neighbour's P1 function w' (values wn[], neighbour local facet j)
template <int D, int I>
__device__ __forceinline__ double nb_grad_dot(const CellGeom<D>& K, const double* L, double rLi, const double* wn, int j) {
    const double gr = K.G[I][I] * rLi;
    double s = pick_apex<D>(wn, j) * gr;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        const int a = mm + (mm >= I);
        s = fma(pick_facet<D>(wn, mm, j), fma(-L[a], gr, K.G[a][I]), s);
    }
    return s;
}

// ------------------------------------------------------------------------------------------
// EMI:  y = A(kappa) x
//   A(u,v) = int kappa grad u.grad v - int_dS0 avg(kappa grad u).n jump(v) - int_dS0 avg(kappa grad v).n jump(u)
//          + int_dS0 tau/avg(h) avg(kappa) jump(u) jump(v) + C_phi int_dS(mem) jump(u) jump(v)
// With s(w) = grad w . g_i:   area * (grad w . n_i) = -D vol s(w),   area = sqrt(G_ii) D vol.
// ------------------------------------------------------------------------------------------
template <int D, int I, int MODE>
__device__ __forceinline__ void emi_facet(const MeshDev& m, const CellGeom<D>& K, const int* nb, uint32_t flags,
                                          const double* xv, const double* kv, double hK,
                                          const double* __restrict__ x, const double* __restrict__ kappa,
                                          double C_phi, double tau, double* y) {
    // MODE 0: apply (neighbour data gathered from global memory); MODE 1: cell-diagonal block (neighbour values 0)
    constexpr int NV = D + 1;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    const uint32_t kind = (fb >> 2) & 3u;
    if (kind >= FK_EXTERIOR) return;
    const int j = (int)(fb & 3u);
    const int64_t Kp = nb[I];
    double xn[NV];
    if (MODE == 1) {
#pragma unroll
        for (int a = 0; a < NV; ++a) xn[a] = 0.0;
    } else {
        load_nodal<D>(x, Kp, xn);
    }
    double du[D], sdu = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        du[mm] = xv[mm + (mm >= I)] - pick_facet<D>(xn, mm, j);
        sdu += du[mm];
    }
    const double DV = (double)D * K.vol;
    const double sqG = fast_sqrt(K.G[I][I]);
    if (kind == FK_MEMBRANE) {
        const double w = C_phi * sqG * DV * FacetConst<D>::mass;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) y[mm + (mm >= I)] = fma(w, sdu + du[mm], y[mm + (mm >= I)]);
        return;
    }
    double kn[NV], Xo[D], L[NV];
    load_nodal<D>(kappa, Kp, kn);
    const double hN = m.h[Kp];
    load_vertex<D>(m.coords, m.cells[Kp * NV + j], Xo);
    apex_bary<D>(K, Xo, L);
    const double rLi = fast_rcp(L[I]);
    // s = grad u . g_i on both sides
    double s_own = 0.0;
#pragma unroll
    for (int a = 0; a < NV; ++a) s_own = fma(xv[a], K.G[a][I], s_own);
    const double s_nb = nb_grad_dot<D, I>(K, L, rLi, xn, j);
    double kf[D], knf[D], sk = 0.0, skn = 0.0, q = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        kf[mm] = kv[mm + (mm >= I)];
        knf[mm] = pick_facet<D>(kn, mm, j);
        sk += kf[mm];
        skn += knf[mm];
        q = fma(kf[mm], sdu + du[mm], q);
    }
    const double hm = 0.5 * DV * FacetConst<D>::mass;
    // consistency: -1/2 int (k grad u.n + k' grad u'.n) v   ->  +hm (s_own (sk+kf_m) + s_nb (skn+knf_m))
    // adjoint consistency: -1/2 (grad v_a.n) int k jump(u)  ->  +hm G_ai q
    q *= hm;
#pragma unroll
    for (int a = 0; a < NV; ++a) y[a] = fma(K.G[a][I], q, y[a]);
    // penalty: tau/avg(h) int avg(k) jump(u) v
    const double pw = tau * fast_rcp(0.5 * (hK + hN)) * sqG * DV * FacetConst<D>::trip;
    double kb[D], skb = 0.0, skd = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        kb[mm] = 0.5 * (kf[mm] + knf[mm]);
        skb += kb[mm];
        skd = fma(kb[mm], du[mm], skd);
    }
    const double base = fma(skb, sdu, skd);
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        const double t1 = hm * fma(s_own, sk + kf[mm], s_nb * (skn + knf[mm]));
        const double t3 = pw * (base + fma(kb[mm], sdu, du[mm] * fma(2.0, kb[mm], skb)));
        y[mm + (mm >= I)] += t1 + t3;
    }
}

template <int D, int MODE>
__device__ __forceinline__ void emi_cell(const MeshDev& m, const CellGeom<D>& K, const int* nb, uint32_t flags,
                                         const double* xv, const double* kv, double hK,
                                         const double* __restrict__ x, const double* __restrict__ kappa,
                                         double C_phi, double tau, double* y) {
    constexpr int NV = D + 1;
    double kbar = 0.0;
#pragma unroll
    for (int a = 0; a < NV; ++a) kbar += kv[a];
    kbar *= K.vol / (double)NV;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < NV; ++b) s = fma(K.G[a][b], xv[b], s);
        y[a] = kbar * s;
    }
    emi_facet<D, 0, MODE>(m, K, nb, flags, xv, kv, hK, x, kappa, C_phi, tau, y);
    emi_facet<D, 1, MODE>(m, K, nb, flags, xv, kv, hK, x, kappa, C_phi, tau, y);
    emi_facet<D, 2, MODE>(m, K, nb, flags, xv, kv, hK, x, kappa, C_phi, tau, y);
    if (D == 3) emi_facet<D, (D == 3 ? 3 : 0), MODE>(m, K, nb, flags, xv, kv, hK, x, kappa, C_phi, tau, y);
}

// direct variant: every neighbour access is a global (L1/L2) gather
template <int D>
__global__ __launch_bounds__(KNP_BLOCK) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_emi_apply(MeshDev m, const double* __restrict__ x, const double* __restrict__ kappa, double* __restrict__ y,
                 double C_phi, double tau) {
    constexpr int NV = D + 1;
    const int64_t c = m.c_begin + xcd_block(blockIdx.x, gridDim.x) * KNP_BLOCK + threadIdx.x;
    if (c >= m.c_end) return;
    int verts[NV], nb[NV];
    load_cell_ints<D>(m.cells, c, verts);
    load_cell_ints<D>(m.nbr, c, nb);
    const uint32_t flags = m.fflag[c];
    double xv[NV], kv[NV], yv[NV];
    load_nodal<D>(x, c, xv);
    load_nodal<D>(kappa, c, kv);
    const double hK = m.h[c];
    CellGeom<D> K;
    load_cell_geometry<D>(m, verts, K);
    emi_cell<D, 0>(m, K, nb, flags, xv, kv, hK, x, kappa, C_phi, tau, yv);
    store_nodal<D>(y, c, yv);
}

// in-register inverse of a small dense matrix (Gauss-Jordan, no pivoting: the blocks are SPD
// for EMI and diagonally dominant M/dt + diffusion blocks for KNP)
template <int N> __device__ __forceinline__ void invert_small(double (*A)[N]) {
#pragma unroll
    for (int p = 0; p < N; ++p) {
        const double ip = 1.0 / A[p][p];
        A[p][p] = 1.0;
#pragma unroll
        for (int k = 0; k < N; ++k) A[p][k] *= ip;
#pragma unroll
        for (int r = 0; r < N; ++r) {
            if (r == p) continue;
            const double f = A[r][p];
            A[r][p] = 0.0;
#pragma unroll
            for (int k = 0; k < N; ++k) A[r][k] -= f * A[p][k];
        }
    }
}

// inverse of the cell-diagonal block of A_emi (block-Jacobi preconditioner), stored [c][row][col]
template <int D>
__global__ __launch_bounds__(KNP_BLOCK) void k_emi_blockjacobi(MeshDev m, const double* __restrict__ kappa,
                                                               bjreal* __restrict__ binv, double C_phi, double tau,
                                                               double shift) {
    constexpr int NV = D + 1;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= m.nc_owned) return;
    int verts[NV], nb[NV];
    load_cell_ints<D>(m.cells, c, verts);
    load_cell_ints<D>(m.nbr, c, nb);
    const uint32_t flags = m.fflag[c];
    CellGeom<D> K;
    load_cell_geometry<D>(m, verts, K);
    double kv[NV];
    load_nodal<D>(kappa, c, kv);
    const double hK = m.h[c];
    double A[NV][NV];
#pragma unroll
    for (int b = 0; b < NV; ++b) {
        double e[NV], col[NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) e[a] = (a == b) ? 1.0 : 0.0;
        emi_cell<D, 1>(m, K, nb, flags, e, kv, hK, nullptr, kappa, C_phi, tau, col);
#pragma unroll
        for (int a = 0; a < NV; ++a) A[a][b] = col[a];
    }
    // B_emi's mass shift kappa/Lp^2 int u v (reference: solver.py:390-395), lumped with mean kappa
    if (shift != 0.0) {
        double kbar = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) kbar += kv[a];
        kbar /= (double)NV;
        const double w = shift * kbar * K.vol / (double)((D + 1) * (D + 2));
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
            for (int b = 0; b < NV; ++b) A[a][b] += w * ((a == b) ? 2.0 : 1.0);
    }
    invert_small<NV>(A);
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int b = 0; b < NV; ++b) binv[(c * NV + a) * NV + b] = (bjreal)(0.5 * (A[a][b] + A[b][a]));   // exactly symmetric in fp32
}

// ------------------------------------------------------------------------------------------
// KNP: y_k = A_k x_k for all solved species k at once (shared mesh / geometry / phi data)
//   A_k(u,v) = 1/dt int u v + int D grad u.grad v - int_dS0 avg(D grad u).n jump(v)
//            - int_dS0 avg(D grad v).n jump(u) + int_dS0 tau/avg(h) jump(D u) jump(v)
//            + z psi int D u grad(phi).grad v - z psi int_dS0 jump(v) jump(un u),
//   un = max(D grad(phi).n_own, 0).   `gphi[c][a]` = grad(phi)_c . grad(lambda_a) is precomputed
//   once per KNP solve (phi is frozen during the solve):  area * grad(phi).n_i = -D vol gphi_i.
// ------------------------------------------------------------------------------------------

template <int D, int NS, int I, bool DIAG>
__device__ __forceinline__ void knp_facet(const MeshDev& m, const CellGeom<D>& K, const int* nb, uint32_t flags,
                                          const double (*xv)[D + 1], const double* gp, const double* Dk, double hK,
                                          const double* __restrict__ x, const double* __restrict__ gphi,
                                          const double* __restrict__ Dall, const KnpArgs& ka, double (*y)[D + 1]) {
    constexpr int NV = D + 1;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    const uint32_t kind = (fb >> 2) & 3u;
    if (kind != FK_SIPG) return;
    const int j = (int)(fb & 3u);
    const int64_t Kp = nb[I];
    double Xo[D], L[NV];
    load_vertex<D>(m.coords, m.cells[Kp * NV + j], Xo);
    const double hN = m.h[Kp];
    const double gp_nb = gphi[Kp * NV + j];
    apex_bary<D>(K, Xo, L);
    const double rLi = fast_rcp(L[I]);
    const double DV = (double)D * K.vol;
    // upwind speeds times area: un*area = D_k max(-gphi_i, 0) D vol ; neighbour: vol' = -L_i vol
    const double up_own = fmax(-gp[I], 0.0) * DV;
    const double up_nb = fmax(-gp_nb, 0.0) * DV * (-L[I]);
    const double penA = ka.tau * fast_rcp(0.5 * (hK + hN)) * fast_sqrt(K.G[I][I]) * DV;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const double Dn = Dall[(int64_t)k * m.nc + Kp];
        double xn[NV];
        if (DIAG) {
#pragma unroll
            for (int a = 0; a < NV; ++a) xn[a] = 0.0;
        } else {
            load_nodal<D>(x + (int64_t)k * m.nc * NV, Kp, xn);
        }
        double s_own = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) s_own = fma(xv[k][a], K.G[a][I], s_own);
        const double s_nb = nb_grad_dot<D, I>(K, L, rLi, xn, j);
        const double zp = ka.z[k] * ka.psi;
        // per facet-vertex weight of the mass-like terms:  pen (D u - D' u') - z psi (un u - un' u')
        const double c_own = penA * Dk[k] - zp * Dk[k] * up_own;
        const double c_nb = penA * Dn - zp * Dn * up_nb;
        double sdu = 0.0, w[D], sw = 0.0;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) {
            const double xo = xv[k][mm + (mm >= I)];
            const double xnb = pick_facet<D>(xn, mm, j);
            sdu += xo - xnb;
            w[mm] = fma(c_own, xo, -c_nb * xnb);
            sw += w[mm];
        }
        // consistency: +1/2 vol (D s_own + D' s_nb) ; adjoint: +1/2 D G_ai vol sum(du)
        const double t1 = 0.5 * K.vol * fma(Dk[k], s_own, Dn * s_nb);
        const double t2 = 0.5 * Dk[k] * K.vol * sdu;
#pragma unroll
        for (int a = 0; a < NV; ++a) y[k][a] = fma(K.G[a][I], t2, y[k][a]);
#pragma unroll
        for (int mm = 0; mm < D; ++mm)
            y[k][mm + (mm >= I)] += t1 + FacetConst<D>::mass * (sw + w[mm]);
    }
}

template <int D, int NS, bool DIAG>
__device__ __forceinline__ void knp_cell(const MeshDev& m, const CellGeom<D>& K, const int* nb, uint32_t flags,
                                         const double (*xv)[D + 1], const double* gp, const double* Dk, double hK,
                                         const double* __restrict__ x, const double* __restrict__ gphi,
                                         const double* __restrict__ Dall, const KnpArgs& ka, double (*y)[D + 1]) {
    constexpr int NV = D + 1;
    const double mw = ka.inv_dt * K.vol / (double)((D + 1) * (D + 2));
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double sx = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) sx += xv[k][a];
        const double drift = ka.z[k] * ka.psi * Dk[k] * K.vol * sx / (double)NV;
        const double dv = Dk[k] * K.vol;
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < NV; ++b) s = fma(K.G[a][b], xv[k][b], s);
            y[k][a] = fma(mw, sx + xv[k][a], fma(dv, s, drift * gp[a]));
        }
    }
    knp_facet<D, NS, 0, DIAG>(m, K, nb, flags, xv, gp, Dk, hK, x, gphi, Dall, ka, y);
    knp_facet<D, NS, 1, DIAG>(m, K, nb, flags, xv, gp, Dk, hK, x, gphi, Dall, ka, y);
    knp_facet<D, NS, 2, DIAG>(m, K, nb, flags, xv, gp, Dk, hK, x, gphi, Dall, ka, y);
    if (D == 3) knp_facet<D, NS, (D == 3 ? 3 : 0), DIAG>(m, K, nb, flags, xv, gp, Dk, hK, x, gphi, Dall, ka, y);
}

template <int D, int NS>
__global__ __launch_bounds__(KNP_BLOCK) void k_knp_apply(MeshDev m, const double* __restrict__ x,
                                                         const double* __restrict__ gphi,
                                                         const double* __restrict__ Dall, double* __restrict__ yout,
                                                         KnpArgs ka) {
    constexpr int NV = D + 1;
    const int64_t c = m.c_begin + xcd_block(blockIdx.x, gridDim.x) * KNP_BLOCK + threadIdx.x;
    if (c >= m.c_end) return;
    int verts[NV], nb[NV];
    load_cell_ints<D>(m.cells, c, verts);
    load_cell_ints<D>(m.nbr, c, nb);
    const uint32_t flags = m.fflag[c];
    double xv[NS][NV], y[NS][NV], gp[NV], Dk[NS];
    load_nodal<D>(gphi, c, gp);
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        load_nodal<D>(x + (int64_t)k * m.nc * NV, c, xv[k]);
        Dk[k] = Dall[(int64_t)k * m.nc + c];
    }
    const double hK = m.h[c];
    CellGeom<D> K;
    load_cell_geometry<D>(m, verts, K);
    knp_cell<D, NS, false>(m, K, nb, flags, xv, gp, Dk, hK, x, gphi, Dall, ka, y);
#pragma unroll
    for (int k = 0; k < NS; ++k) store_nodal<D>(yout + (int64_t)k * m.nc * NV, c, y[k]);
}

// material id of the neighbour behind every facet (once per knp_set_params)
__global__ void k_neighbour_materials(int64_t nc, const int32_t* __restrict__ nbr, const uint8_t* __restrict__ mat, uint8_t* __restrict__ nmat4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc * 4) return;
    const int32_t nb = nbr[i];
    nmat4[i] = nb >= 0 ? mat[nb] : (uint8_t)0;
}

// one species per launch dimension (setup only, once per KNP solve)
template <int D>
__global__ __launch_bounds__(KNP_BLOCK) void k_knp_blockjacobi(MeshDev m, const double* __restrict__ gphi,
                                                               const double* __restrict__ Dall,
                                                               bjreal* __restrict__ binv, KnpArgs ka) {
    constexpr int NV = D + 1;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    const int k = blockIdx.y;
    if (c >= m.nc_owned) return;
    int verts[NV], nb[NV];
    load_cell_ints<D>(m.cells, c, verts);
    load_cell_ints<D>(m.nbr, c, nb);
    const uint32_t flags = m.fflag[c];
    CellGeom<D> K;
    load_cell_geometry<D>(m, verts, K);
    double gp[NV], Dk[1];
    load_nodal<D>(gphi, c, gp);
    Dk[0] = Dall[(int64_t)k * m.nc + c];
    const double hK = m.h[c];
    KnpArgs k1 = ka;
    k1.z[0] = ka.z[k];
    double A[NV][NV];
#pragma unroll
    for (int b = 0; b < NV; ++b) {
        double e[1][NV], col[1][NV];
#pragma unroll
        for (int a = 0; a < NV; ++a) e[0][a] = (a == b) ? 1.0 : 0.0;
        knp_cell<D, 1, true>(m, K, nb, flags, e, gp, Dk, hK, nullptr, gphi, Dall + (int64_t)k * m.nc, k1, col);
#pragma unroll
        for (int a = 0; a < NV; ++a) A[a][b] = col[0][a];
    }
    invert_small<NV>(A);
    bjreal* out = binv + ((int64_t)k * m.nc + c) * NV * NV;
#pragma unroll
    for (int a = 0; a < NV; ++a)
#pragma unroll
        for (int b = 0; b < NV; ++b) out[a * NV + b] = (bjreal)A[a][b];
}

// gphi[c][a] = grad(phi)_c . grad(lambda_a) = sum_b phi_b G_ab
template <int D>
__global__ __launch_bounds__(KNP_BLOCK) void k_gphi(MeshDev m, const double* __restrict__ phi, double* __restrict__ out) {
    constexpr int NV = D + 1;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= m.nc) return;
    int verts[NV];
    load_cell_ints<D>(m.cells, c, verts);
    CellGeom<D> K;
    load_cell_geometry<D>(m, verts, K);
    double pv[NV], s[NV];
    load_nodal<D>(phi, c, pv);
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        double t = 0.0;
#pragma unroll
        for (int b = 0; b < NV; ++b) t = fma(K.G[a][b], pv[b], t);
        s[a] = t;
    }
    store_nodal<D>(out, c, s);
}
