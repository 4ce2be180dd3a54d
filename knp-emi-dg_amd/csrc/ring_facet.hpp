// Arithmetic of the ring-staged P1 applies (apply_ring.hip, apply_ring_u.hip), once for both families: the cell terms, the facet
// terms and the two places the geometric coefficients of a facet come from -- the class record of a structured mesh, or the staged
// vertex coordinates of any mesh.  Forms and notation: apply_p1.hip (emi_facet_cls, k_knp_apply_halo).  The thread-per-cell kernels
// keep facet functions of their own: they associate some products differently, and sharing them would change result bits.
#pragma once
#include "ring_common.hpp"

namespace ring {

// ---- coefficient sources ---------------------------------------------------------------------------------------------------------
// What the facet terms need from the geometry of facet I, offered by both sources through the same two operations:
//   area<I>(K)      the facet area sqrt(G_II) D vol (all a membrane facet needs);
//   coef<I>(K, ..)  gr = G_II / L_I, cf = the neighbour-gradient weights G_{a_m I} - L_{a_m} gr, pen_geo = 2 / (h + h') area,
//                   nLI_DV = the neighbour-volume factor -L_I D vol.
// coef fills plain doubles: handing the six numbers over in a struct cost k_knp_apply_ring<2, 1> four VGPRs.

// structured meshes: the derived per-class coefficients (MeshDev::cls_ext, 8 per facet) in LDS.  A kernel pays only for the entries
// it uses: the loads of the others are dead.
struct ClassCoef {
    const lds_double* ft;
    template <int I> __device__ __forceinline__ double area(const CellGeom<3>&) const { return ft[8 * I + 6]; }
    template <int I> __device__ __forceinline__ void coef(const CellGeom<3>&, double& gr, double* cf, double& pen_geo, double& nLI_DV) const {
        gr = ft[8 * I];
        pen_geo = ft[8 * I + 4];
        nLI_DV = ft[8 * I + 5];
#pragma unroll
        for (int mm = 0; mm < 3; ++mm) cf[mm] = ft[8 * I + 1 + mm];
    }
};

__device__ __forceinline__ void lds_vertex(const lds_double* co, unsigned v, double* X) {
    typedef double __attribute__((ext_vector_type(2))) vdouble2;
    typedef __attribute__((address_space(3))) vdouble2 lds_vdouble2;
    const vdouble2 a = *(const lds_vdouble2*)(co + 4 * v);
    X[0] = a.x; X[1] = a.y; X[2] = co[4 * v + 2];
}
// any mesh: the same numbers from the cell's geometry, the staged coordinates co, the position vapex of the neighbour's apex vertex
// in them and hinv = 2 / (h + h') of the facet
struct CoordCoef {
    const lds_double* co;
    unsigned vapex;
    double hinv;
    template <int I> __device__ __forceinline__ double area(const CellGeom<3>& K) const { return fast_sqrt(K.G[I][I]) * (3.0 * K.vol); }
    template <int I> __device__ __forceinline__ void coef(const CellGeom<3>& K, double& gr, double* cf, double& pen_geo, double& nLI_DV) const {
        double Xo[3], L[4];
        lds_vertex(co, vapex, Xo);
        apex_bary<3>(K, Xo, L);
        gr = K.G[I][I] * fast_rcp(L[I]);
#pragma unroll
        for (int mm = 0; mm < 3; ++mm) cf[mm] = fma(-L[mm + (mm >= I)], gr, K.G[mm + (mm >= I)][I]);
        const double DV = 3.0 * K.vol;
        pen_geo = hinv * area<I>(K);
        nLI_DV = -L[I] * DV;
    }
};

// ================================================================================================================================
// EMI:  y = A(kappa) x
// ================================================================================================================================
// cell term; gx = G x is kept for the facets ((G x)_I = grad(u) . g_I)
__device__ __forceinline__ void emi_cell_term(const CellGeom<3>& K, const double* xv, const double* kv, double* gx, double* y) {
    constexpr int NV = 4;
    double kbar = 0.0;
#pragma unroll
    for (int a = 0; a < NV; ++a) kbar += kv[a];
    kbar *= K.vol / (double)NV;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        double sa = 0.0;
#pragma unroll
        for (int bb = 0; bb < NV; ++bb) sa = fma(xv[bb], K.G[bb][a], sa);
        gx[a] = sa;
        y[a] = kbar * sa;
    }
}

// facet I of a cell; loc = LDS entry of the neighbour's rows in X (x) and KA (kappa)
template <int I, typename Coef>
__device__ __forceinline__ void emi_facet_ring(const CellGeom<3>& K, uint32_t flags, unsigned loc, const Coef& src, const double* xv, const double* gx,
                                               const double* kv, double C_phi, double tau, const lds_double* X, const lds_double* KA, double* y) {
    constexpr int D = 3, NV = 4;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    const uint32_t kind = (fb >> 2) & 3u;
    if (kind >= FK_EXTERIOR) return;
    const unsigned j = fb & 3u;
    double xr[NV], kr[NV], xf[D], knf[D];
    lds_row(X, loc, xr);
    lds_row(KA, loc, kr);
    const double xap = pick_apex<D>(xr, (int)j);
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        xf[mm] = pick_facet<D>(xr, mm, (int)j);
        knf[mm] = pick_facet<D>(kr, mm, (int)j);
    }
    double du[D], sdu = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        du[mm] = xv[mm + (mm >= I)] - xf[mm];
        sdu += du[mm];
    }
    if (kind == FK_MEMBRANE) {
        const double w = C_phi * src.template area<I>(K) * FacetConst<D>::mass;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) y[mm + (mm >= I)] = fma(w, sdu + du[mm], y[mm + (mm >= I)]);
        return;
    }
    double gr, cf[D], pen_geo, nLI_DV;
    src.template coef<I>(K, gr, cf, pen_geo, nLI_DV);
    const double s_own = gx[I];                                            // (G x)_I from the cell term
    double s_nb = xap * gr;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) s_nb = fma(xf[mm], cf[mm], s_nb);
    double kf[D], sk = 0.0, skn = 0.0, q = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        kf[mm] = kv[mm + (mm >= I)];
        sk += kf[mm];
        skn += knf[mm];
        q = fma(kf[mm], sdu + du[mm], q);
    }
    const double hm = 0.5 * (double)D * K.vol * FacetConst<D>::mass;
    q *= hm;
#pragma unroll
    for (int a = 0; a < NV; ++a) y[a] = fma(K.G[a][I], q, y[a]);
    const double pw = tau * pen_geo * FacetConst<D>::trip;
    double kb[D], skb = 0.0, skd = 0.0;
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        kb[mm] = 0.5 * (kf[mm] + knf[mm]);
        skb += kb[mm];
        skd = fma(kb[mm], du[mm], skd);
    }
    const double bs = fma(skb, sdu, skd);
#pragma unroll
    for (int mm = 0; mm < D; ++mm) {
        const double t1 = hm * fma(s_own, sk + kf[mm], s_nb * (skn + knf[mm]));
        const double t3 = pw * (bs + fma(kb[mm], sdu, du[mm] * fma(2.0, kb[mm], skb)));
        y[mm + (mm >= I)] += t1 + t3;
    }
}

// ================================================================================================================================
// KNP:  y_k = A_k x_k for NS species
// ================================================================================================================================
// cell terms (mass, diffusion, drift); gx[k] = G x_k and hvD[k] = vol D_k / 2 are kept for the facets
template <int NS>
__device__ __forceinline__ void knp_cell_term(const CellGeom<3>& K, const double (*xv)[4], const double* gp, const double* Dk, const double* zpsi,
                                              double inv_dt, double (*gx)[4], double* hvD, double (*y)[4]) {
    constexpr int NV = 4;
    const double mw = inv_dt * K.vol / 20.0;
#pragma unroll
    for (int k = 0; k < NS; ++k) hvD[k] = 0.5 * K.vol * Dk[k];
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double sx = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) sx += xv[k][a];
        const double drift = zpsi[k] * Dk[k] * K.vol * sx / (double)NV;
        const double dv = Dk[k] * K.vol;
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            double sacc = 0.0;
#pragma unroll
            for (int bb = 0; bb < NV; ++bb) sacc = fma(xv[k][bb], K.G[bb][a], sacc);
            gx[k][a] = sacc;
            y[k][a] = fma(mw, sx + xv[k][a], fma(dv, sacc, drift * gp[a]));
        }
    }
}

// facet I of a cell; loc = LDS entry of the neighbour's rows in X (species k at X + k XS) and in G (gphi), dsel = its material,
// sD = the material table [NS][KNP_MAX_MAT]
template <int NS, int I, int XS, typename Coef>
__device__ __forceinline__ void knp_facet_ring(const CellGeom<3>& K, uint32_t flags, unsigned loc, const Coef& src, unsigned dsel, const double (*xv)[4],
                                               const double (*gx)[4], const double* gp, const double* Dk, const double* hvD, const double* zpsi,
                                               double tau, const lds_double* X, const lds_double* G, const lds_double* sD, double (*y)[4]) {
    constexpr int D = 3, NV = 4;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    if (((fb >> 2) & 3u) != FK_SIPG) return;
    const unsigned j = fb & 3u;
    double gr, cf[D], pen_geo, nLI_DV;
    src.template coef<I>(K, gr, cf, pen_geo, nLI_DV);
    double gp_nb;
    {   // the 16-byte half that holds component j of the neighbour's gphi row: own rows (swizzled image) or the halo's [entry][2].
        // Kept in line: as a function of its own the same statements cost every KNP ring kernel one VGPR.
        typedef double __attribute__((ext_vector_type(2))) vdouble2;
        typedef __attribute__((address_space(3))) vdouble2 lds_vdouble2;
        const unsigned idx = loc < (unsigned)RB ? loc * NV + 2u * (((j >> 1) ^ (loc >> 3)) & 1u) : (unsigned)(RB * NV) + (loc - RB) * 2u;
        const vdouble2 g2 = *(const lds_vdouble2*)(G + idx);
        gp_nb = (j & 1u) ? g2.y : g2.x;
    }
    const double DV = (double)D * K.vol;
    const double up_own = fmax(-gp[I], 0.0) * DV;
    const double up_nb = fmax(-gp_nb, 0.0) * nLI_DV;
    const double penA = tau * pen_geo;
    const double hv = 0.5 * K.vol;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        double xr[NV], xf[D];
        lds_row(X + (unsigned)k * XS, loc, xr);
        const double xap = pick_apex<D>(xr, (int)j);
#pragma unroll
        for (int mm = 0; mm < D; ++mm) xf[mm] = pick_facet<D>(xr, mm, (int)j);
        const double Dn = sD[(unsigned)k * KNP_MAX_MAT + dsel];
        const double s_own = gx[k][I];                                             // (G x)_I = grad(u) . g_I, from the cell term
        double s_nb = xap * gr;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) s_nb = fma(xf[mm], cf[mm], s_nb);
        // penalty and upwind weights of the two traces:  D (pen - z psi un),  written so that each costs one FMA and one product
        const double zp = zpsi[k];
        const double c_own = Dk[k] * fma(-zp, up_own, penA);
        const double c_nb = Dn * fma(-zp, up_nb, penA);
        double sdu = 0.0, w[D], sw = 0.0;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) {
            const double xo = xv[k][mm + (mm >= I)];
            sdu += xo - xf[mm];
            w[mm] = fma(c_own, xo, -c_nb * xf[mm]);
            sw += w[mm];
        }
        const double t1m = fma(FacetConst<D>::mass, sw, hv * fma(Dk[k], s_own, Dn * s_nb));
        const double t2 = hvD[k] * sdu;
#pragma unroll
        for (int a = 0; a < NV; ++a) y[k][a] = fma(K.G[a][I], t2, y[k][a]);
#pragma unroll
        for (int mm = 0; mm < D; ++mm) y[k][mm + (mm >= I)] += fma(FacetConst<D>::mass, w[mm], t1m);
    }
}

}  // namespace ring
