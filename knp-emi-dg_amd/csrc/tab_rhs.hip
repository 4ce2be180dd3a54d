// DG-p path for p >= 2 ("tabulated" path): the per-step kernels every degree-2 run uses, reached from the degree dispatch in rhs_p1.hip.
//  * nodal coefficient fields: kappa, the eliminated concentration (exact: combinations of DG-p functions with cell-wise constant factors);
//  * right-hand sides L_emi and L_knp, one thread per cell, by quadrature over the rules tabulated on the host (knpemidg/dgtab.py) and
//    uploaded once by knp_set_tabulation below: generic in the polynomial degree;
//  * step III on the membrane facets (phi_M, Nernst potentials) and facet traces.
// The OPERATORS of these runs are matrix-free: apply_p2.hip.  Only under KNP_P2_ASSEMBLED=1 (A/B runs) tab_kappa also has the a_emi blocks
// assembled from the kappa it has just formed (tab_assembled.hip).
//
// Reference forms restated here: L_emi  src/knpemidg/solver.py:270-403, L_knp :534-663, step III :808-845, facet projector utils.py:100-124.
#include "tab_common.hpp"

namespace {

// out[b] = sum_k w_k D_k(cell) src_k[cell][b] over all ions, src_k = c_k for the solved species and the eliminated concentration for the
// last one; w_k = z_k^2 (squared) or F z_k
template <int ND>
__device__ __forceinline__ void ion_sum(int64_t nc, const double* __restrict__ cc, const double* __restrict__ celim, const double* __restrict__ Dk,
                                        const IonZ& ia, double F, bool squared, int64_t cell, double* out) {
#pragma unroll
    for (int b = 0; b < ND; ++b) out[b] = 0.0;
    for (int k = 0; k < ia.n; ++k) {
        const double* src = (k < ia.n - 1) ? cc + (int64_t)k * nc * ND : celim;
        const double f = (squared ? ia.z[k] : F) * ia.z[k] * Dk[(int64_t)k * nc + cell];
#pragma unroll
        for (int b = 0; b < ND; ++b) out[b] = fma(f, src[cell * ND + b], out[b]);
    }
}

// ------------------------------------------------------------------------------------------------------------
// nodal coefficient fields (exact: linear combinations of DG-p functions with cell-wise constant factors)
// ------------------------------------------------------------------------------------------------------------
__global__ void k_tab_kappa(int64_t nc, int nd, const double* __restrict__ cc, const double* __restrict__ celim,
                            const double* __restrict__ Dk, IonZ ia, double F, double psi, double* __restrict__ kappa) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nc * nd) return;
    const int64_t c = t / nd;
    double s = 0.0;
    for (int i = 0; i < ia.n; ++i) {
        const double v = (i < ia.n - 1) ? cc[(int64_t)i * nc * nd + t] : celim[t];
        s += F * ia.z[i] * ia.z[i] * psi * Dk[(int64_t)i * nc + c] * v;
    }
    kappa[t] = s;
}

__global__ void k_tab_celim(int64_t nc, int nd, const double* __restrict__ cc, const double* __restrict__ rho, IonZ ia,
                            double* __restrict__ celim) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nc * nd) return;
    const double zN = ia.z[ia.n - 1];
    double acc = 0.0;
    for (int i = 0; i < ia.n - 1; ++i) acc += -(1.0 / zN) * ia.z[i] * cc[(int64_t)i * nc * nd + t];
    acc += -(1.0 / zN) * rho[t / nd];
    celim[t] = acc;
}

// ------------------------------------------------------------------------------------------------------------
// L_emi: one thread per CELL, all ND rows (round 3; rounds 1-2 ran one thread per (cell, row): every row recomputed the cell's
// geometry, the nodal combination S, the neighbour's data and every quadrature-point flux -- 419 us per step for 124 416 P2 cells)
// ------------------------------------------------------------------------------------------------------------
template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_emi_rhs(MeshDev m, TabRule rc, TabRule rf, TabRule rm, const double* __restrict__ cc,
                                                     const double* __restrict__ celim, const double* __restrict__ Dk,
                                                     const double* __restrict__ phiM, const double* __restrict__ Ich, IonZ ia,
                                                     double F, double C_phi, int splitting, const double* __restrict__ extra,
                                                     double* __restrict__ out) {
    constexpr int NV = D + 1;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m.nc_owned) return;
    CellGeom<D> K;
    load_cell_gradients<D>(m, c, K);
    // S = sum_k F z_k D_k c_k is a DG-p function (D_k is cell-wise constant): nodal combination
    double S[ND], acc[ND];
#pragma unroll
    for (int b = 0; b < ND; ++b) acc[b] = 0.0;
    ion_sum<ND>(m.nc, cc, celim, Dk, ia, F, false, c, S);
    for (int q = 0; q < rc.nq; ++q) {
        const double* dB = rc.dB + (int64_t)q * ND * NV;
        double gS[D];
#pragma unroll
        for (int k = 0; k < D; ++k) gS[k] = 0.0;
#pragma unroll
        for (int l = 0; l < NV; ++l) {
            double sl = 0.0;
#pragma unroll
            for (int b = 0; b < ND; ++b) sl = fma(S[b], dB[b * NV + l], sl);
#pragma unroll
            for (int k = 0; k < D; ++k) gS[k] = fma(sl, K.g[l][k], gS[k]);
        }
        // grad(S) . grad(lambda_l), then each row's gradient is a combination of those
        double gl[NV];
#pragma unroll
        for (int l = 0; l < NV; ++l) gl[l] = dotD<D>(gS, K.g[l]);
        const double wv = rc.w[q] * K.vol;
#pragma unroll
        for (int a = 0; a < ND; ++a) acc[a] -= wv * dotNV<NV>(dB + a * NV, gl);
    }
    const uint32_t flags = m.fflag[c];
    for (int i = 0; i < NV; ++i) {
        const uint32_t fb = (flags >> (8 * i)) & 0xffu;
        const uint32_t kind = (fb >> 2) & 3u;
        const int j = (int)(fb & 3u);
        const int64_t nb = m.nbr[c * NV + i];
        if (nb < 0) continue;
        if (kind == FK_SIPG) {
            CellGeom<D> K2;
            load_cell_gradients<D>(m, nb, K2);
            double S2[ND];
            ion_sum<ND>(m.nc, cc, celim, Dk, ia, F, false, nb, S2);
            TabPair<D> P;
            tab_pair<D>(K, K2, i, P);
            for (int q = 0; q < rf.nq; ++q) {
                const double* Bi = rf.B + ((int64_t)i * rf.nq + q) * ND;
                const double* dBi = rf.dB + ((int64_t)i * rf.nq + q) * ND * NV;
                const double* dBj = rf.dB + ((int64_t)j * rf.nq + q) * ND * NV;
                double flux = 0.0;
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    flux = fma(S[b], dotNV<NV>(dBi + b * NV, P.gn), flux);
                    flux = fma(S2[b], dotNV<NV>(dBj + b * NV, P.gn2), flux);
                }
                const double wf = rf.w[q] * P.area * 0.5 * flux;
#pragma unroll
                for (int a = 0; a < ND; ++a) acc[a] = fma(wf, Bi[a], acc[a]);
            }
        } else if (kind == FK_MEMBRANE && splitting != 2) {    // MMS: Robin data arrives as host-integrated extra RHS
            const int64_t f = m.cfacet[c * NV + i];
            double g = phiM[f];
            if (!splitting) {
                double It = 0.0;
                for (int k = 0; k < ia.n; ++k) It += Ich[(int64_t)k * m.nf + f];
                g -= It / C_phi;
            }
            const double sgn = ((fb >> 4) & 1u) ? -1.0 : 1.0;      // e (plus) side carries -v_e
            const double area = facet_area<D>(K, i);
            const double wm = sgn * C_phi * g * area;
            for (int q = 0; q < rm.nq; ++q) {
                const double* Bi = rm.B + ((int64_t)i * rm.nq + q) * ND;
                const double wq = wm * rm.w[q];
#pragma unroll
                for (int a = 0; a < ND; ++a) acc[a] = fma(wq, Bi[a], acc[a]);
            }
        }
    }
#pragma unroll
    for (int a = 0; a < ND; ++a) out[c * ND + a] = acc[a] + (extra ? extra[c * ND + a] : 0.0);
}

// ------------------------------------------------------------------------------------------------------------
// L_knp of species s = blockIdx.y: one thread per CELL, all ND rows (round 3, as above)
// ------------------------------------------------------------------------------------------------------------
struct KnpRhsTab { double F, C_M, dt; int splitting; const double* mms_C; const double* extra; };

template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_knp_rhs(MeshDev m, TabRule rc, TabRule rm, const double* __restrict__ cc,
                                                     const double* __restrict__ cprev, const double* __restrict__ celim,
                                                     const double* __restrict__ phi, const double* __restrict__ Dk,
                                                     const double* __restrict__ phiM, const double* __restrict__ Ich,
                                                     const double* __restrict__ fsrc, IonZ ia, KnpRhsTab ra,
                                                     double* __restrict__ out_all) {
    constexpr int NV = D + 1;
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m.nc_owned) return;
    const int s = blockIdx.y;
    CellGeom<D> K;
    load_cell_gradients<D>(m, c, K);
    const double z = ia.z[s];
    const double Dc = Dk[(int64_t)s * m.nc + c];
    double cp[ND], acc[ND];
    ld<ND>(cprev + (int64_t)s * m.nc * ND, c, cp);
#pragma unroll
    for (int a = 0; a < ND; ++a) acc[a] = 0.0;
    const double fs = fsrc ? fsrc[(int64_t)s * m.nc + c] : 0.0;
    for (int q = 0; q < rc.nq; ++q) {
        const double* B = rc.B + (int64_t)q * ND;
        double cq = 0.0;
#pragma unroll
        for (int b = 0; b < ND; ++b) cq = fma(B[b], cp[b], cq);
        const double wq = rc.w[q] * K.vol * (cq / ra.dt + fs);
#pragma unroll
        for (int a = 0; a < ND; ++a) acc[a] = fma(wq, B[a], acc[a]);
    }
    const uint32_t flags = m.fflag[c];
    for (int i = 0; i < NV; ++i) {
        const uint32_t fb = (flags >> (8 * i)) & 0xffu;
        if (((fb >> 2) & 3u) != FK_MEMBRANE) continue;
        const int64_t nb = m.nbr[c * NV + i];
        if (nb < 0) continue;
        const int j = (int)(fb & 3u);
        const int64_t f = m.cfacet[c * NV + i];
        const bool is_e = (fb >> 4) & 1u;
        // own-side nodal fields: c_k (current iterate), alpha_sum = sum_k D_k z_k^2 c_k, phi on both sides
        double ck[ND], as[ND], po[ND], pn[ND];
        ld<ND>(cc + (int64_t)s * m.nc * ND, c, ck);
        ld<ND>(phi, c, po);
        ld<ND>(phi, nb, pn);
        ion_sum<ND>(m.nc, cc, celim, Dk, ia, 0.0, true, c, as);
        const double area = facet_area<D>(K, i);
        const double sgn = is_e ? -1.0 : 1.0;
        if (ra.splitting == 2) {
            // MMS (solver.py:649-650): -(phi_i - phi_e)(C_i v_i - C_e v_e) with the DG0 coupling coefficient C
            const double Cown = ra.mms_C[(int64_t)s * m.nc + c];
            for (int q = 0; q < rm.nq; ++q) {
                const double* Bi = rm.B + ((int64_t)i * rm.nq + q) * ND;
                const double* Bj = rm.B + ((int64_t)j * rm.nq + q) * ND;
                double pq = 0.0, pq2 = 0.0;
#pragma unroll
                for (int b = 0; b < ND; ++b) { pq = fma(Bi[b], po[b], pq); pq2 = fma(Bj[b], pn[b], pq2); }
                const double jump = is_e ? (pq2 - pq) : (pq - pq2);
                const double wq = rm.w[q] * area * sgn * Cown * jump;
#pragma unroll
                for (int a = 0; a < ND; ++a) acc[a] -= wq * Bi[a];
            }
            continue;
        }
        const double I_k = Ich[(int64_t)s * m.nf + f];
        double I_tot = 0.0;
        for (int k = 0; k < ia.n; ++k) I_tot += Ich[(int64_t)k * m.nf + f];
        const double pM = phiM[f];
        for (int q = 0; q < rm.nq; ++q) {
            const double* Bi = rm.B + ((int64_t)i * rm.nq + q) * ND;
            const double* Bj = rm.B + ((int64_t)j * rm.nq + q) * ND;
            double cq = 0.0, aq = 0.0, pq = 0.0, pq2 = 0.0;
#pragma unroll
            for (int b = 0; b < ND; ++b) {
                cq = fma(Bi[b], ck[b], cq);
                aq = fma(Bi[b], as[b], aq);
                pq = fma(Bi[b], po[b], pq);
                pq2 = fma(Bj[b], pn[b], pq2);
            }
            const double alpha = Dc * z * z * cq / aq;
            const double C = alpha * ra.C_M / (ra.F * z * ra.dt);
            double g = pM - ra.dt / (ra.C_M * alpha) * I_k;
            if (ra.splitting) g += (ra.dt / ra.C_M) * I_tot;
            const double jump = is_e ? (pq2 - pq) : (pq - pq2);       // phi_i - phi_e
            const double wq = rm.w[q] * area * sgn * C * (g - jump);
#pragma unroll
            for (int a = 0; a < ND; ++a) acc[a] = fma(wq, Bi[a], acc[a]);
        }
    }
    double* out = out_all + (int64_t)s * m.nc * ND;
    const double* ex = ra.extra ? ra.extra + (int64_t)s * m.nc * ND : nullptr;
#pragma unroll
    for (int a = 0; a < ND; ++a) out[c * ND + a] = acc[a] + (ex ? ex[c * ND + a] : 0.0);
}

// ------------------------------------------------------------------------------------------------------------
// step III per membrane facet: phi_M = avg(phi_i - phi_e), E_k = RT/(F z_k) avg ln(c_e / c_i)
// ------------------------------------------------------------------------------------------------------------
template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_facet_updates(MeshDev m, TabRule ra, TabRule rn, const double* __restrict__ cc,
                                                           const double* __restrict__ celim, const double* __restrict__ phi,
                                                           double* __restrict__ phiM, double* __restrict__ E, IonZ ia,
                                                           double RT_over_F) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.nmf) return;
    const int32_t* row = m.mf + 6 * t;
    if (!row[5]) return;
    const int64_t ce = row[0], ci = row[1];
    const int le = row[2], li = row[3];
    const int64_t f = row[4];
    double ve[ND], vi[ND];
    if (phi) {
        ld<ND>(phi, ce, ve);
        ld<ND>(phi, ci, vi);
        double s = 0.0;
        for (int q = 0; q < ra.nq; ++q) {
            const double* Be = ra.B + ((int64_t)le * ra.nq + q) * ND;
            const double* Bi = ra.B + ((int64_t)li * ra.nq + q) * ND;
            double pe = 0.0, pi = 0.0;
#pragma unroll
            for (int b = 0; b < ND; ++b) { pe = fma(Be[b], ve[b], pe); pi = fma(Bi[b], vi[b], pi); }
            s += ra.w[q] * (pi - pe);
        }
        phiM[f] = s;
    }
    for (int k = 0; k < ia.n; ++k) {
        const double* src = (k < ia.n - 1) ? cc + (int64_t)k * m.nc * ND : celim;
        ld<ND>(src, ce, ve);
        ld<ND>(src, ci, vi);
        double s = 0.0;
        for (int q = 0; q < rn.nq; ++q) {
            const double* Be = rn.B + ((int64_t)le * rn.nq + q) * ND;
            const double* Bi = rn.B + ((int64_t)li * rn.nq + q) * ND;
            double xe = 0.0, xi = 0.0;
#pragma unroll
            for (int b = 0; b < ND; ++b) { xe = fma(Be[b], ve[b], xe); xi = fma(Bi[b], vi[b], xi); }
            s += rn.w[q] * log(xe / xi);
        }
        E[(int64_t)k * m.nf + f] = RT_over_F / ia.z[k] * s;
    }
}

template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_facet_trace(MeshDev m, TabRule ra, const double* __restrict__ nodal, int side,
                                                         double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.nmf) return;
    const int32_t* row = m.mf + 6 * t;
    const int64_t cell = row[side];
    const int lf = row[2 + side];
    double v[ND];
    ld<ND>(nodal, cell, v);
    double s = 0.0;
    for (int q = 0; q < ra.nq; ++q) {
        const double* B = ra.B + ((int64_t)lf * ra.nq + q) * ND;
        double x = 0.0;
#pragma unroll
        for (int b = 0; b < ND; ++b) x = fma(B[b], v[b], x);
        s += ra.w[q] * x;
    }
    out[row[4]] = s;
}

}  // namespace

// ---- launchers (called from the degree dispatch in rhs_p1.hip) -------------------------------------------------
int tab_kappa(knp_ctx* c, const double* cc, const double* celim, double* kappa) {
    const int64_t n = c->m.nc * c->nd;
    hipLaunchKernelGGL(k_tab_kappa, dim3((unsigned)grid_for(n)), dim3(KNP_BLOCK), 0, c->stream, c->m.nc, c->nd, cc, celim,
                       (const double*)c->D, ion_z(c), c->p.F, c->p.psi, kappa);
    HIPCHK(c, hipGetLastError());
    return p2_assembled(c) ? tab_assemble_emi(c, kappa) : 0;   // the matrix-free applies read kappa directly (apply_p2.hip)
}

int tab_emi_rhs(knp_ctx* c, const double* cc, const double* celim, const double* phiM, const double* Ich, double* b) {
    if (need_tabs(c, {KNP_TAB_CELL_RHS_EMI, KNP_TAB_FACET_RHS_EMI, KNP_TAB_FACET_MEM_LIN})) return -1;
    TAB_DISPATCH(c, k_tab_emi_rhs, cells_grid(c, 128), dim3(128), c->m, c->tab[KNP_TAB_CELL_RHS_EMI], c->tab[KNP_TAB_FACET_RHS_EMI],
                 c->tab[KNP_TAB_FACET_MEM_LIN], cc, celim, (const double*)c->D, phiM, Ich, ion_z(c), c->p.F, c->p.C_phi,
                 c->p.splitting, (const double*)c->extra_emi, b);
    return 0;
}

int tab_knp_rhs(knp_ctx* c, const double* cc, const double* cprev, const double* celim, const double* phi, const double* phiM,
                const double* Ich, double* b) {
    if (need_tabs(c, {KNP_TAB_CELL_MASS, KNP_TAB_FACET_MEM_KNP})) return -1;
    KnpRhsTab ra{c->p.F, c->p.C_M, c->p.dt, c->p.splitting, (const double*)c->mms_C, (const double*)c->extra_knp};
    TAB_DISPATCH(c, k_tab_knp_rhs, cells_grid(c, 128, c->p.n_sys), dim3(128), c->m, c->tab[KNP_TAB_CELL_MASS],
                 c->tab[KNP_TAB_FACET_MEM_KNP], cc, cprev, celim, phi, (const double*)c->D, phiM, Ich, (const double*)c->fsrc,
                 ion_z(c), ra, b);
    return 0;
}

int tab_step_updates(knp_ctx* c, const double* cc, double* celim, const double* phi, double* phiM, double* E, bool do_celim) {
    if (need_tabs(c, {KNP_TAB_FACET_AVG, KNP_TAB_FACET_NERNST})) return -1;
    if (do_celim) {
        const int64_t n = c->m.nc * c->nd;
        hipLaunchKernelGGL(k_tab_celim, dim3((unsigned)grid_for(n)), dim3(KNP_BLOCK), 0, c->stream, c->m.nc, c->nd, cc,
                           (const double*)c->rho, ion_z(c), celim);
    }
    if (c->m.nmf > 0)
        TAB_DISPATCH(c, k_tab_facet_updates, dim3((unsigned)((c->m.nmf + 127) / 128)), dim3(128), c->m, c->tab[KNP_TAB_FACET_AVG],
                     c->tab[KNP_TAB_FACET_NERNST], cc, (const double*)celim, phi, phiM, E, ion_z(c), c->p.R * c->p.T / c->p.F);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int tab_facet_trace(knp_ctx* c, const double* nodal, int side, double* out) {
    if (need_tabs(c, {KNP_TAB_FACET_AVG})) return -1;
    if (c->m.nmf > 0)
        TAB_DISPATCH(c, k_tab_facet_trace, dim3((unsigned)((c->m.nmf + 127) / 128)), dim3(128), c->m, c->tab[KNP_TAB_FACET_AVG], nodal,
                     side, out);
    return 0;
}

void tab_free(knp_ctx* c) {
    for (int s = 0; s < KNP_TAB_COUNT; ++s) {
        hipFree(c->tab_mem[s]);
        c->tab_mem[s] = nullptr;
        c->tab[s] = TabRule();
    }
    tab_free_blocks(c);
}

extern "C" int knp_set_tabulation(knp_ctx* c, int slot, int nloc, int nq, const double* w, const double* B, const double* dB) {
    if (!c || slot < 0 || slot >= KNP_TAB_COUNT || !w || !B || !dB) return -1;
    const int NV = c->m.dim + 1;
    const bool facet = slot >= KNP_TAB_FACET_EMI;
    if (nq < 1 || nq > 256 || nloc != (facet ? NV : 1)) { c->err = "set_tabulation: nloc must be 1 (cell rules) or dim+1 (facet rules)"; return -1; }
    const size_t nB = (size_t)nloc * nq * c->nd, ndB = nB * NV;
    hipFree(c->tab_mem[slot]);
    c->tab_mem[slot] = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->tab_mem[slot], sizeof(double) * (nq + nB + ndB)));
    double* base = c->tab_mem[slot];
    HIPCHK(c, host_memcpy(c, base, w, sizeof(double) * nq, hipMemcpyHostToDevice));
    HIPCHK(c, host_memcpy(c, base + nq, B, sizeof(double) * nB, hipMemcpyHostToDevice));
    HIPCHK(c, host_memcpy(c, base + nq + nB, dB, sizeof(double) * ndB, hipMemcpyHostToDevice));
    TabRule r;
    r.nq = nq; r.w = base; r.B = base + nq; r.dB = base + nq + nB;
    c->tab[slot] = r;
    return 0;
}
