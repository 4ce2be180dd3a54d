// Reduction primitives and cell-vector helpers of the Krylov solvers (krylov.hip): wavefront / block sums, the per-block partial
// rows, the fixed-order second stage k_reduce, loads / stores of one cell's dofs, the block-Jacobi block product and the residual
// measure of the stopping tests.
#pragma once
#include "cell_geom.hpp"
#include "krylov_scalar.hpp"

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// block-level sum of NR values per thread; result valid in thread 0
template <int NR> __device__ __forceinline__ void block_sum(double* v, double* out) {
    __shared__ double lds[KNP_BLOCK / 64][NR];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double s = wave_sum(v[r]);
        if (lane == 0) lds[wv][r] = s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double s = lds[0][r];
#pragma unroll
            for (int w = 1; w < KNP_BLOCK / 64; ++w) s += lds[w][r];
            out[r] = s;
        }
    }
}

template <int NR> __device__ __forceinline__ void write_partials(double* partial, int nsys, double* v) {
    double out[NR];
    block_sum<NR>(v, out);
    if (threadIdx.x == 0) {
        double* p = partial + ((int64_t)blockIdx.x * nsys + blockIdx.y) * KNP_MAX_RED;
#pragma unroll
        for (int r = 0; r < NR; ++r) p[r] = out[r];
    }
}

// NV = dofs per cell: 3 / 4 (P1 triangles / tets), 6 / 10 (P2)
template <int NV> __device__ __forceinline__ void ldv(const double* p, int64_t c, double* v) {
    if constexpr (NV <= 4) {
        load_nodal<NV - 1>(p, c, v);
    } else {
        static_assert(NV % 2 == 0, "P2 cell vectors are read as double2");
        const double2* q = reinterpret_cast<const double2*>(p + (int64_t)NV * c);
#pragma unroll
        for (int k = 0; k < NV / 2; ++k) { const double2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
    }
}
template <int NV> __device__ __forceinline__ void stv(double* p, int64_t c, const double* v) {
    if constexpr (NV <= 4) {
        store_nodal<NV - 1>(p, c, v);
    } else {
        double2* q = reinterpret_cast<double2*>(p + (int64_t)NV * c);
#pragma unroll
        for (int k = 0; k < NV / 2; ++k) q[k] = make_double2(v[2 * k], v[2 * k + 1]);
    }
}

template <int NV> __device__ __forceinline__ void block_matvec(const bjreal* __restrict__ binv, int64_t c, const double* r, double* z) {
    const bjreal* B = binv + c * NV * NV;
#pragma unroll
    for (int a = 0; a < NV; ++a) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < NV; ++b) s += (double)B[a * NV + b] * r[b];
        z[a] = s;
    }
}

struct VecDims {
    int64_t nc_owned, nc;   // vectors are [nsys][nc*NV]; only owned cells are updated / reduced
    int nsys;
    // block-Jacobi table (KNP on structured meshes, solve.hip: build_bj_table): the cell's inverse block is entry bj_idx[c] of a small
    // table instead of 4 NV^2 bytes per cell and species read from HBM in every vector kernel; null -> per-cell inverses
    const uint16_t* bj_idx;
    const bjreal* bj_tab;   // [n_entries][nsys][NV*NV]
    // Residual norms of the stopping tests are weighted with 1 / cell volume: ||r||_w^2 = sum_K |r_K|^2 / vol_K ~ r^T M^-1 r, the L2
    // norm of the residual's Riesz representative.  r and b are load vectors (int f v_i): their plain 2-norm is dominated by the
    // largest cells, so that on a mesh with slivers (EMIx: cell volumes over 6 decades) a tolerance on it says nothing about the
    // small cells, where the max-norm error of the concentrations sits.  On a uniform mesh the weight is a constant factor.
    const float* ivol;      // [nc], or null (weight 1)
    // KNP stopping test (d8 != 0): order-8 norms of the residual and load DENSITIES, ||r / vol||_8 <= rtol' ||b / vol||_8, a sum-type
    // stand-in for  max_K ||r_K|| / vol_K  <=  rtol' max_K ||b_K|| / vol_K.  The concentrations are asked for in the MAX norm, and
    // the measurement behind this choice (tools/knp_norm_experiment.py, profiles/r03_knp_norms_*.txt: BiCGStab stopped after k
    // iterations, true max-norm error against the converged solution next to four residual measures) shows the max-norm error at
    // 0.03-0.055 of this ratio on BOTH mesh families -- the idealized BoxMesh and the EMIx reconstruction, whose cell volumes span
    // 3.5 decades -- while the (weighted) 2-norm ratio sits 5x above the error on the first and 10x BELOW it on the second (round
    // 2's per-mesh factor 0.03 on rtol_knp).  Sums of 8th powers ride the same deterministic reduction / all-reduce as the inner
    // products.
    int d8;
};
__device__ __forceinline__ double cell_weight(const VecDims& d, int64_t c) { return d.ivol ? (double)d.ivol[c] : 1.0; }
// this cell's term of the residual measure the stopping tests sum: |r_K|^2 / vol_K (weighted 2-norm) or (|r_K| / vol_K)^8 (d8)
__device__ __forceinline__ double residual_measure(const VecDims& d, int64_t c, double rr) {
    const double w = cell_weight(d, c);
    if (!d.d8) return rr * w;
    const double q = rr * w * w;
    return (q * q) * (q * q);
}

// inverse block of system s, cell c: from the table when there is one, else from the per-cell array binv [nsys][nc][NV*NV]
template <int NV> __device__ __forceinline__ const bjreal* bj_block(const VecDims& d, const bjreal* __restrict__ binv, int s, int64_t c) {
    return d.bj_idx ? d.bj_tab + ((int64_t)d.bj_idx[c] * d.nsys + s) * (NV * NV) : binv + ((int64_t)s * d.nc + c) * (NV * NV);
}

// op > 0: the block's thread 0 also runs the scalar recurrence of its system (single-GPU: saves one launch per reduction
// point; with a communicator the all-reduce sits between the two and k_scalar_op runs separately).
// Eight partial rows per thread are in flight at a time: with one row per loop trip the 15 trips of the r=2 mesh were 15 dependent
// L2 round trips (11 us for a kernel that moves 250 KB).
#define KNP_REDUCE_BLOCK 1024
template <int NR, int UR = 4>
__global__ __launch_bounds__(KNP_REDUCE_BLOCK) void k_reduce(const double* __restrict__ partial, int64_t nblocks, int nsys, double* red, int op,
                                                             double* scal, int* status, StopTest st, int aux) {
    // one block per system; deterministic order
    const int s = blockIdx.x;
    __shared__ double lds[KNP_REDUCE_BLOCK / 64][NR];
    // thread 0 runs the scalar recurrence at the end: its operands travel with the partial sums instead of behind them
    double S[KS_N];
    int flag = 0, iter = 0;
    if (threadIdx.x == 0 && op > 0) {
#pragma unroll
        for (int i = 0; i < KS_N; ++i) S[i] = scal_row(scal, s)[i];
        flag = status[2 * s];
        iter = status[2 * s + 1];
    }
    double acc[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = 0.0;
    for (int64_t b0 = threadIdx.x; b0 < nblocks; b0 += UR * KNP_REDUCE_BLOCK) {
        double v[UR][NR];
#pragma unroll
        for (int u = 0; u < UR; ++u) {
            const int64_t b = b0 + (int64_t)u * KNP_REDUCE_BLOCK;
            const double* p = partial + (b * nsys + s) * KNP_MAX_RED;
#pragma unroll
            for (int r = 0; r < NR; ++r) v[u][r] = b < nblocks ? p[r] : 0.0;
        }
#pragma unroll
        for (int u = 0; u < UR; ++u)
#pragma unroll
            for (int r = 0; r < NR; ++r) acc[r] += v[u][r];
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        const double v = wave_sum(acc[r]);
        if (lane == 0) lds[wv][r] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double R[KNP_MAX_RED];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            double v = lds[0][r];
#pragma unroll
            for (int w = 1; w < KNP_REDUCE_BLOCK / 64; ++w) v += lds[w][r];
            R[r] = v;
            red[s * KNP_MAX_RED + r] = v;
        }
        if (op > 0) {
            scalar_op(op, S, R, &flag, &iter, st, scal_gm(scal, s), aux);
#pragma unroll
            for (int i = 0; i < KS_N; ++i) scal_row(scal, s)[i] = S[i];
            status[2 * s] = flag;
            status[2 * s + 1] = iter;
        }
    }
}
