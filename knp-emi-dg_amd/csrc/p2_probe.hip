// FP64 MFMA probe: the one genuinely dense, cell-independent contraction of the P2 path -- the facet quadrature
//   forward  [NQ x NF] . {jump(u), kappa, kappa'}  and  [NQ x D] . {dn u, dn u'},   pointwise flux,
//   backward [NF x NQ] . flux  and  [D x NQ] . t
// -- once as v_mfma_f64_16x16x4_f64 tiles (columns = 16 cell-facets per wave, the 4 lane groups hold the K index) and once
// as the per-thread FMA chain of the sampled rule (the one the 2D apply runs, apply_p2.hip: emi_facet_p2), on identical synthetic
// inputs [ncol][26] -> outputs [ncol][9].
// knp_probe_facet_contraction times both; tests check that they agree.  Measured (profiles/r02_mfma_probe.md): the MFMA
// form pads 12 x 6 / 6 x 12 / 3 x 12 to 16 x 16 x 4 tiles and runs at the same FP64 rate as the vector pipe, so it loses.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "p2_tables.hpp"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

struct ProbeTabs { double psi[16][8]; double lam[16][4]; double w[16]; };   // zero padded: [q][n], [q][m], [q]

__global__ __launch_bounds__(256) void k_probe_valu(int64_t ncol, const double* __restrict__ in, double* __restrict__ out) {
    constexpr int D = 3, NF = 6, NQ = P2Tab<3>::NQE;
    const int64_t col = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= ncol) return;
    const double* p = in + col * 26;
    double ju[NF], ko[NF], kn[NF], dno[D], dnn[D];
#pragma unroll
    for (int n = 0; n < NF; ++n) { ju[n] = p[n]; ko[n] = p[6 + n]; kn[n] = p[12 + n]; }
#pragma unroll
    for (int m = 0; m < D; ++m) { dno[m] = p[18 + m]; dnn[m] = p[21 + m]; }
    const double area = p[24], pen = p[25];
    double r[NF] = {0, 0, 0, 0, 0, 0}, T[D] = {0, 0, 0};
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        double a = 0.0, b = 0.0, j = 0.0, d0 = 0.0, d1 = 0.0;
#pragma unroll
        for (int n = 0; n < NF; ++n) {
            const double ps = P2Tab<3>::PSIE[q][n];
            a = fma(ko[n], ps, a); b = fma(kn[n], ps, b); j = fma(ju[n], ps, j);
        }
#pragma unroll
        for (int m = 0; m < D; ++m) { d0 = fma(dno[m], P2Tab<3>::LAME[q][m], d0); d1 = fma(dnn[m], P2Tab<3>::LAME[q][m], d1); }
        const double w = P2Tab<3>::WE[q] * area;
        const double flux = w * fma(pen * (a + b), j, -0.5 * fma(a, d0, b * d1));
        const double t = -0.5 * w * a * j;
#pragma unroll
        for (int n = 0; n < NF; ++n) r[n] = fma(flux, P2Tab<3>::PSIE[q][n], r[n]);
#pragma unroll
        for (int m = 0; m < D; ++m) T[m] = fma(t, P2Tab<3>::LAME[q][m], T[m]);
    }
    double* o = out + col * 9;
#pragma unroll
    for (int n = 0; n < NF; ++n) o[n] = r[n];
#pragma unroll
    for (int m = 0; m < D; ++m) o[6 + m] = T[m];
}

// one wave = 16 columns; lane (g = lane >> 4, n = lane & 15): B operand element [k = g][col n], A operand element [row n][k = g],
// C/D registers i = 0..3 hold rows g + 4 i of column n (cdna_hip_programming.md section 3, f64 layout)
__global__ __launch_bounds__(256) void k_probe_mfma(int64_t ncol, const double* __restrict__ in, const ProbeTabs* __restrict__ tabs,
                                                    double* __restrict__ out) {
    const int lane = threadIdx.x & 63, g = lane >> 4, n = lane & 15;
    const int64_t col0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * 16;
    if (col0 >= ncol) return;                                   // whole wave
    const int64_t col = (col0 + n < ncol) ? col0 + n : ncol - 1;
    const double* p = in + col * 26;
    // A operands: forward  A[q = n][k]  with k = g (step 0), 4 + g (step 1);  backward  A[m = n][q = g + 4 i]
    const double aP0 = tabs->psi[n][g], aP1 = tabs->psi[n][4 + g], aL = tabs->lam[n][g];
    double bP[3], bL[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { bP[i] = n < 8 ? tabs->psi[g + 4 * i][n] : 0.0; bL[i] = n < 4 ? tabs->lam[g + 4 * i][n] : 0.0; }
    const double4_t z = {0.0, 0.0, 0.0, 0.0};
    double4_t Dj = z, Da = z, Db = z, D0 = z, D1 = z;
    // B operands: nodal values k = g and 4 + g of this column (k >= 6 / k >= 3 are padding)
    Dj = __builtin_amdgcn_mfma_f64_16x16x4f64(aP0, p[g], Dj, 0, 0, 0);
    Da = __builtin_amdgcn_mfma_f64_16x16x4f64(aP0, p[6 + g], Da, 0, 0, 0);
    Db = __builtin_amdgcn_mfma_f64_16x16x4f64(aP0, p[12 + g], Db, 0, 0, 0);
    const bool k1 = g < 2;
    Dj = __builtin_amdgcn_mfma_f64_16x16x4f64(aP1, k1 ? p[4 + g] : 0.0, Dj, 0, 0, 0);
    Da = __builtin_amdgcn_mfma_f64_16x16x4f64(aP1, k1 ? p[10 + g] : 0.0, Da, 0, 0, 0);
    Db = __builtin_amdgcn_mfma_f64_16x16x4f64(aP1, k1 ? p[16 + g] : 0.0, Db, 0, 0, 0);
    const bool k3 = g < 3;
    D0 = __builtin_amdgcn_mfma_f64_16x16x4f64(aL, k3 ? p[18 + g] : 0.0, D0, 0, 0, 0);
    D1 = __builtin_amdgcn_mfma_f64_16x16x4f64(aL, k3 ? p[21 + g] : 0.0, D1, 0, 0, 0);
    const double area = p[24], pen = p[25];
    double4_t R = z, T = z;
#pragma unroll
    for (int i = 0; i < 3; ++i) {                                // quadrature points q = g + 4 i of this column
        const double w = tabs->w[g + 4 * i] * area;
        const double a = Da[i], b = Db[i], j = Dj[i];
        const double flux = w * fma(pen * (a + b), j, -0.5 * fma(a, D0[i], b * D1[i]));
        const double t = -0.5 * w * a * j;
        R = __builtin_amdgcn_mfma_f64_16x16x4f64(bP[i], flux, R, 0, 0, 0);
        T = __builtin_amdgcn_mfma_f64_16x16x4f64(bL[i], t, T, 0, 0, 0);
    }
    if (col0 + n < ncol) {
        double* o = out + (col0 + n) * 9;
        o[g] = R[0];                                            // rows m = g
        if (g < 2) o[4 + g] = R[1];                             // rows m = 4 + g
        if (g < 3) o[6 + g] = T[0];
    }
}

}  // namespace

extern "C" int knp_probe_facet_contraction(knp_ctx* c, int variant, int64_t ncol, int reps, const double* in_host, double* out_host,
                                           float* avg_ms) {
    if (!c || ncol < 1 || reps < 1 || !in_host || !out_host || !avg_ms || (variant != 0 && variant != 1)) return -1;
    double *in = nullptr, *out = nullptr;
    ProbeTabs h{};
    for (int q = 0; q < P2Tab<3>::NQE; ++q) {
        for (int n = 0; n < 6; ++n) h.psi[q][n] = P2Tab<3>::PSIE[q][n];
        for (int m = 0; m < 3; ++m) h.lam[q][m] = P2Tab<3>::LAME[q][m];
        h.w[q] = P2Tab<3>::WE[q];
    }
    ProbeTabs* tabs = nullptr;
    HIPCHK(c, hipMalloc((void**)&in, sizeof(double) * 26 * ncol));
    HIPCHK(c, hipMalloc((void**)&out, sizeof(double) * 9 * ncol));
    HIPCHK(c, hipMalloc((void**)&tabs, sizeof(ProbeTabs)));
    HIPCHK(c, host_memcpy(c, in, in_host, sizeof(double) * 26 * ncol, hipMemcpyHostToDevice));
    HIPCHK(c, host_memcpy(c, tabs, &h, sizeof(ProbeTabs), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemset(out, 0, sizeof(double) * 9 * ncol));
    auto launch = [&]() {
        if (variant == 0)
            hipLaunchKernelGGL(k_probe_valu, dim3((unsigned)((ncol + 255) / 256)), dim3(256), 0, c->stream, ncol, (const double*)in, out);
        else
            hipLaunchKernelGGL(k_probe_mfma, dim3((unsigned)((ncol + 63) / 64)), dim3(256), 0, c->stream, ncol, (const double*)in,
                               (const ProbeTabs*)tabs, out);
    };
    launch();
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    for (int i = 0; i < reps; ++i) launch();
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, host_event_sync(c, c->ev1));
    HIPCHK(c, hipGetLastError());
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / (float)reps;
    HIPCHK(c, host_memcpy(c, out_host, out, sizeof(double) * 9 * ncol, hipMemcpyDeviceToHost));
    hipFree(in); hipFree(out); hipFree(tabs);
    return 0;
}
