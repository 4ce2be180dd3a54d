// Assembled DG-p (p >= 2) operator blocks: the round-1 form of the P2 operators, kept for A/B runs under KNP_P2_ASSEMBLED=1 only.
// The operators of every other degree-2 run are the matrix-free applies of apply_p2.hip, which stream no matrix at all.
// Here the quadrature of a_emi / a_knp (reference src/knpemidg/solver.py:270-403, :534-663) runs ONCE per time step, exactly when the
// reference re-assembles (solver.py:477-479, 730-731), over the tabulated rules (tab_common.hpp) into dense (nd x nd) cell blocks:
// blk[c][0] the diagonal block of cell c, blk[c][1+i] its coupling to the neighbour behind local facet i.  They stay in HBM (4 KB per
// cell and operator in 3D), and an apply is the block-sparse gather  y_c = sum_j blk[c][j] x_{nbr_j(c)}: HBM-bound on 16-20x the bytes
// the matrix-free applies move, which is what the A/B runs measure.
#include "tab_common.hpp"

namespace {

// physical gradient of basis function b from its tabulated reference gradient: out[k] = sum_l dB[b][l] (grad lambda_l)_k
template <int D> __device__ __forceinline__ void grad_basis(const double* dB, int b, const CellGeom<D>& K, double* out) {
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double s = 0.0;
#pragma unroll
        for (int l = 0; l <= D; ++l) s = fma(dB[b * (D + 1) + l], K.g[l][k], s);
        out[k] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------
// a_emi blocks: one thread per (cell, row a)
// ------------------------------------------------------------------------------------------------------------
template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_assemble_emi(MeshDev m, TabRule rc, TabRule rf, TabRule rm,
                                                          const double* __restrict__ kappa, double tau, double C_phi,
                                                          double* __restrict__ blk) {
    constexpr int NV = D + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.nc_owned * ND) return;
    const int64_t c = t / ND;
    const int a = (int)(t % ND);
    CellGeom<D> K;
    load_cell_gradients<D>(m, c, K);
    double kap[ND];
    ld<ND>(kappa, c, kap);
    double diag[ND];
#pragma unroll
    for (int b = 0; b < ND; ++b) diag[b] = 0.0;

    // cells: int kappa grad u . grad v
    for (int q = 0; q < rc.nq; ++q) {
        const double* B = rc.B + (int64_t)q * ND;
        const double* dB = rc.dB + (int64_t)q * ND * NV;
        double kq = 0.0;
#pragma unroll
        for (int b = 0; b < ND; ++b) kq = fma(B[b], kap[b], kq);
        double ga[D];
        grad_basis<D>(dB, a, K, ga);
        const double w = rc.w[q] * K.vol * kq;
#pragma unroll
        for (int b = 0; b < ND; ++b) {
            double gb[D], s = 0.0;
            grad_basis<D>(dB, b, K, gb);
#pragma unroll
            for (int k = 0; k < D; ++k) s = fma(ga[k], gb[k], s);
            diag[b] = fma(w, s, diag[b]);
        }
    }

    const uint32_t flags = m.fflag[c];
    const double hc = m.h[c];
    for (int i = 0; i < NV; ++i) {
        const uint32_t fb = (flags >> (8 * i)) & 0xffu;
        const uint32_t kind = (fb >> 2) & 3u;
        const int j = (int)(fb & 3u);
        const int64_t nb = m.nbr[c * NV + i];
        double off[ND];
#pragma unroll
        for (int b = 0; b < ND; ++b) off[b] = 0.0;
        if (nb >= 0 && kind == FK_SIPG) {
            CellGeom<D> K2;
            load_cell_gradients<D>(m, nb, K2);
            double kap2[ND];
            ld<ND>(kappa, nb, kap2);
            TabPair<D> P;
            tab_pair<D>(K, K2, i, P);
            const double pen0 = tau / (0.5 * (hc + m.h[nb]));
            for (int q = 0; q < rf.nq; ++q) {
                const double* Bi = rf.B + ((int64_t)i * rf.nq + q) * ND;
                const double* dBi = rf.dB + ((int64_t)i * rf.nq + q) * ND * NV;
                const double* Bj = rf.B + ((int64_t)j * rf.nq + q) * ND;
                const double* dBj = rf.dB + ((int64_t)j * rf.nq + q) * ND * NV;
                double kq = 0.0, kq2 = 0.0;
#pragma unroll
                for (int b = 0; b < ND; ++b) { kq = fma(Bi[b], kap[b], kq); kq2 = fma(Bj[b], kap2[b], kq2); }
                const double w = rf.w[q] * P.area;
                const double pen = pen0 * 0.5 * (kq + kq2);
                const double Ba = Bi[a];
                const double dna = dotNV<NV>(dBi + a * NV, P.gn);
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    const double Bb = Bi[b], B2b = Bj[b];
                    const double dnb = dotNV<NV>(dBi + b * NV, P.gn);
                    const double dn2b = dotNV<NV>(dBj + b * NV, P.gn2);
                    diag[b] += w * (-0.5 * kq * dnb * Ba - 0.5 * kq * dna * Bb + pen * Ba * Bb);
                    off[b] += w * (-0.5 * kq2 * dn2b * Ba + 0.5 * kq * dna * B2b - pen * Ba * B2b);
                }
            }
        } else if (nb >= 0 && kind == FK_MEMBRANE) {
            const double area = facet_area<D>(K, i);
            for (int q = 0; q < rm.nq; ++q) {
                const double* Bi = rm.B + ((int64_t)i * rm.nq + q) * ND;
                const double* Bj = rm.B + ((int64_t)j * rm.nq + q) * ND;
                const double w = rm.w[q] * area * C_phi * Bi[a];
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    diag[b] = fma(w, Bi[b], diag[b]);
                    off[b] = fma(-w, Bj[b], off[b]);
                }
            }
        }
        double* o = blk + ((c * (NV + 1) + 1 + i) * ND + a) * ND;
#pragma unroll
        for (int b = 0; b < ND; ++b) o[b] = off[b];
    }
    double* o = blk + ((c * (NV + 1)) * ND + a) * ND;
#pragma unroll
    for (int b = 0; b < ND; ++b) o[b] = diag[b];
}

// ------------------------------------------------------------------------------------------------------------
// a_knp blocks of species s = blockIdx.y
// ------------------------------------------------------------------------------------------------------------
template <int D, int ND>
__global__ __launch_bounds__(128) void k_tab_assemble_knp(MeshDev m, TabRule rc, TabRule rf, const double* __restrict__ phi,
                                                          const double* __restrict__ Dk, KnpOpArgs ka,
                                                          double* __restrict__ blk_all) {
    constexpr int NV = D + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.nc_owned * ND) return;
    const int s = blockIdx.y;
    const int64_t c = t / ND;
    const int a = (int)(t % ND);
    double* blk = blk_all + (int64_t)s * m.nc * (NV + 1) * ND * ND;
    const double z = ka.z[s];
    const double Dc = Dk[(int64_t)s * m.nc + c];
    CellGeom<D> K;
    load_cell_gradients<D>(m, c, K);
    double ph[ND];
    ld<ND>(phi, c, ph);
    double diag[ND];
#pragma unroll
    for (int b = 0; b < ND; ++b) diag[b] = 0.0;

    // cells: 1/dt u v + D grad u . grad v + z psi D u grad(phi) . grad v     (row v = a, column u = b)
    for (int q = 0; q < rc.nq; ++q) {
        const double* B = rc.B + (int64_t)q * ND;
        const double* dB = rc.dB + (int64_t)q * ND * NV;
        double ga[D], gphi[D];
        grad_basis<D>(dB, a, K, ga);
#pragma unroll
        for (int k = 0; k < D; ++k) gphi[k] = 0.0;
#pragma unroll
        for (int b = 0; b < ND; ++b) {
            double gb[D];
            grad_basis<D>(dB, b, K, gb);
#pragma unroll
            for (int k = 0; k < D; ++k) gphi[k] = fma(ph[b], gb[k], gphi[k]);
        }
        const double w = rc.w[q] * K.vol;
        const double drift = z * ka.psi * Dc * dotD<D>(gphi, ga);
#pragma unroll
        for (int b = 0; b < ND; ++b) {
            double gb[D], s2 = 0.0;
            grad_basis<D>(dB, b, K, gb);
#pragma unroll
            for (int k = 0; k < D; ++k) s2 = fma(ga[k], gb[k], s2);
            diag[b] += w * (ka.inv_dt * B[a] * B[b] + Dc * s2 + drift * B[b]);
        }
    }

    const uint32_t flags = m.fflag[c];
    const double hc = m.h[c];
    for (int i = 0; i < NV; ++i) {
        const uint32_t fb = (flags >> (8 * i)) & 0xffu;
        const uint32_t kind = (fb >> 2) & 3u;
        const int j = (int)(fb & 3u);
        const int64_t nb = m.nbr[c * NV + i];
        double off[ND];
#pragma unroll
        for (int b = 0; b < ND; ++b) off[b] = 0.0;
        if (nb >= 0 && kind == FK_SIPG) {
            CellGeom<D> K2;
            load_cell_gradients<D>(m, nb, K2);
            double ph2[ND];
            ld<ND>(phi, nb, ph2);
            const double D2 = Dk[(int64_t)s * m.nc + nb];
            TabPair<D> P;
            tab_pair<D>(K, K2, i, P);
            const double pen = ka.tau / (0.5 * (hc + m.h[nb]));
            for (int q = 0; q < rf.nq; ++q) {
                const double* Bi = rf.B + ((int64_t)i * rf.nq + q) * ND;
                const double* dBi = rf.dB + ((int64_t)i * rf.nq + q) * ND * NV;
                const double* Bj = rf.B + ((int64_t)j * rf.nq + q) * ND;
                const double* dBj = rf.dB + ((int64_t)j * rf.nq + q) * ND * NV;
                // upwind speeds: own side with its outward normal n, neighbour side with -n
                double sp = 0.0, sm = 0.0;
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    sp = fma(ph[b], dotNV<NV>(dBi + b * NV, P.gn), sp);
                    sm = fma(ph2[b], dotNV<NV>(dBj + b * NV, P.gn2), sm);
                }
                sp *= Dc;
                sm *= -D2;
                const double un = 0.5 * (sp + fabs(sp)), un2 = 0.5 * (sm + fabs(sm));
                const double w = rf.w[q] * P.area;
                const double Ba = Bi[a];
                const double dna = dotNV<NV>(dBi + a * NV, P.gn);
#pragma unroll
                for (int b = 0; b < ND; ++b) {
                    const double Bb = Bi[b], B2b = Bj[b];
                    const double dnb = dotNV<NV>(dBi + b * NV, P.gn);
                    const double dn2b = dotNV<NV>(dBj + b * NV, P.gn2);
                    diag[b] += w * (-0.5 * Dc * dnb * Ba - 0.5 * Dc * dna * Bb + pen * Dc * Ba * Bb - z * ka.psi * un * Ba * Bb);
                    off[b] += w * (-0.5 * D2 * dn2b * Ba + 0.5 * Dc * dna * B2b - pen * D2 * Ba * B2b + z * ka.psi * un2 * Ba * B2b);
                }
            }
        }
        double* o = blk + ((c * (NV + 1) + 1 + i) * ND + a) * ND;
#pragma unroll
        for (int b = 0; b < ND; ++b) o[b] = off[b];
    }
    double* o = blk + ((c * (NV + 1)) * ND + a) * ND;
#pragma unroll
    for (int b = 0; b < ND; ++b) o[b] = diag[b];
}

// ------------------------------------------------------------------------------------------------------------
// y_c = sum_j blk[c][j] x_{nbr_j(c)}     one thread per (cell, row); blockIdx.y = system
// ------------------------------------------------------------------------------------------------------------
template <int D, int ND>
__global__ __launch_bounds__(256) void k_tab_apply(MeshDev m, const double* __restrict__ blk_all, const double* __restrict__ x_all,
                                                   double* __restrict__ y_all) {
    constexpr int NV = D + 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m.nc_owned * ND) return;
    const int s = blockIdx.y;
    const int64_t c = t / ND;
    const int a = (int)(t % ND);
    const double* blk = blk_all + (int64_t)s * m.nc * (NV + 1) * ND * ND;
    const double* x = x_all + (int64_t)s * m.nc * ND;
    const double* row = blk + ((c * (NV + 1)) * ND + a) * ND;
    double acc = 0.0;
#pragma unroll
    for (int b = 0; b < ND; ++b) acc = fma(row[b], x[c * ND + b], acc);
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int64_t nb = m.nbr[c * NV + i];
        if (nb < 0) continue;
        const double* r2 = row + (int64_t)(1 + i) * ND * ND;
        double s2 = 0.0;
#pragma unroll
        for (int b = 0; b < ND; ++b) s2 = fma(r2[b], x[nb * ND + b], s2);
        acc += s2;
    }
    y_all[(int64_t)s * m.nc * ND + t] = acc;
}

// inverse of the diagonal blocks (block-Jacobi): one thread per cell, its block in LDS (column index strided by the
// 64 lanes -> conflict free), in-place Gauss-Jordan without pivoting (blocks are SPD resp. mass-dominated)
template <int D, int ND>
__global__ __launch_bounds__(64) void k_tab_block_inverse(MeshDev m, const double* __restrict__ blk_all, bjreal* __restrict__ binv_all, int symmetric) {
    constexpr int NV = D + 1;
    __shared__ double M[ND * ND * 64];
    const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int s = blockIdx.y;
    const int tid = threadIdx.x;
    if (c >= m.nc_owned) return;
    const double* src = blk_all + (int64_t)s * m.nc * (NV + 1) * ND * ND + c * (NV + 1) * ND * ND;
    for (int k = 0; k < ND * ND; ++k) M[k * 64 + tid] = src[k];
    for (int p = 0; p < ND; ++p) {
        const double piv = 1.0 / M[(p * ND + p) * 64 + tid];
        M[(p * ND + p) * 64 + tid] = 1.0;
        for (int k = 0; k < ND; ++k) M[(p * ND + k) * 64 + tid] *= piv;
        for (int r = 0; r < ND; ++r) {
            if (r == p) continue;
            const double f = M[(r * ND + p) * 64 + tid];
            M[(r * ND + p) * 64 + tid] = 0.0;
            for (int k = 0; k < ND; ++k) M[(r * ND + k) * 64 + tid] -= f * M[(p * ND + k) * 64 + tid];
        }
    }
    bjreal* dst = binv_all + (int64_t)s * m.nc * ND * ND + c * ND * ND;
    if (symmetric) {                                   // EMI: exactly symmetric after rounding to fp32
        for (int a = 0; a < ND; ++a)
            for (int b = 0; b < ND; ++b) dst[a * ND + b] = (bjreal)(0.5 * (M[(a * ND + b) * 64 + tid] + M[(b * ND + a) * 64 + tid]));
    } else {
        for (int k = 0; k < ND * ND; ++k) dst[k] = (bjreal)M[k * 64 + tid];
    }
}

}  // namespace

// ---- launchers (called from the degree dispatch in apply_p1.hip, and from tab_kappa) ---------------------------
static int ensure_blocks(knp_ctx* c) {
    const size_t per = (size_t)c->m.nc * (c->m.dim + 2) * c->nd * c->nd;
    if (!c->blk_emi) HIPCHK(c, hipMalloc((void**)&c->blk_emi, sizeof(double) * per));
    if (!c->blk_knp) HIPCHK(c, hipMalloc((void**)&c->blk_knp, sizeof(double) * per * c->p.n_sys));
    return 0;
}

int tab_assemble_emi(knp_ctx* c, const double* kappa) {
    if (need_tabs(c, {KNP_TAB_CELL_STIFF, KNP_TAB_FACET_EMI, KNP_TAB_FACET_MEM}) || ensure_blocks(c)) return -1;
    TAB_DISPATCH(c, k_tab_assemble_emi, rows_grid(c, 128), dim3(128), c->m, c->tab[KNP_TAB_CELL_STIFF], c->tab[KNP_TAB_FACET_EMI],
                 c->tab[KNP_TAB_FACET_MEM], kappa, c->p.tau_emi, c->p.C_phi, c->blk_emi);
    return 0;
}

int tab_assemble_knp(knp_ctx* c, const double* phi) {
    if (need_tabs(c, {KNP_TAB_CELL_STIFF, KNP_TAB_FACET_KNP}) || ensure_blocks(c)) return -1;
    TAB_DISPATCH(c, k_tab_assemble_knp, rows_grid(c, 128, c->p.n_sys), dim3(128), c->m, c->tab[KNP_TAB_CELL_STIFF],
                 c->tab[KNP_TAB_FACET_KNP], phi, (const double*)c->D, knp_op_args(c), c->blk_knp);
    return 0;
}

int tab_apply(knp_ctx* c, int which, const double* x, double* y) {
    const double* blk = which == 0 ? c->blk_emi : c->blk_knp;
    if (!blk) { c->err = "DG-p path: operator blocks not assembled (update_kappa / update_dnphi first)"; return -1; }
    TAB_DISPATCH(c, k_tab_apply, rows_grid(c, 256, which == 0 ? 1 : c->p.n_sys), dim3(256), c->m, blk, x, y);
    return 0;
}

int tab_block_inverse(knp_ctx* c, int which, bjreal* binv) {
    const double* blk = which == 0 ? c->blk_emi : c->blk_knp;
    if (!blk) { c->err = "DG-p path: operator blocks not assembled"; return -1; }
    const dim3 g((unsigned)((c->m.nc_owned + 63) / 64), (unsigned)(which == 0 ? 1 : c->p.n_sys));
    TAB_DISPATCH(c, k_tab_block_inverse, g, dim3(64), c->m, blk, binv, which == 0 ? 1 : 0);
    return 0;
}

void tab_free_blocks(knp_ctx* c) {
    hipFree(c->blk_emi); hipFree(c->blk_knp);
    c->blk_emi = c->blk_knp = nullptr;
}
