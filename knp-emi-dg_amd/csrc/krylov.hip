// Device-resident Krylov solvers: PCG for the (singular, consistent) EMI system and a batched
// per-species BiCGStab for the KNP systems, both with a cell-block-Jacobi preconditioner.
// All Krylov scalars live in device memory; the host only launches kernels and polls a status
// word every `check_every` iterations, so there is no per-iteration host round trip.
// Inner products: 64-lane wavefront shuffle -> per-block LDS -> per-block partial in HBM ->
// fixed-order second stage (bitwise reproducible), all-reduced over RCCL when nranks > 1.
//
// Replaces PETSc KSP cg / gmres + hypre (reference: src/knpemidg/solver.py:425-444,509,684-701,771).
#include "krylov_reduce.hpp"
#include <cstdlib>
#include <cstring>

// conforming-space correction e gathered into the DG dofs of cell c: dg2cg[c][a] is the conforming dof of DG dof (c, a)
// (P1: membrane-broken vertex dofs; P2: vertex + edge dofs of the conforming P2 space) -- pure injection
template <int NV> __device__ __forceinline__ void prolong_cell(const int32_t* __restrict__ dg2cg, const double* __restrict__ e,
                                                                int64_t c, double* add, int nil = 1) {
    // nil: interleaved right-hand-side columns of the level vector (amg_vcycle.hip); e points at this column's first entry
#pragma unroll
    for (int a = 0; a < NV; ++a) add[a] = e[(int64_t)dg2cg[c * NV + a] * nil];
}

#define SYS_PTR(p, s) ((p) + (int64_t)(s) * d.nc * NV)

// ---- PCG kernels ----------------------------------------------------------------------------
// r = b - w(=A x);  z = Binv r;  p = z;  partials: r.z, z.z, (Binv b).(Binv b)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_cg_init(VecDims d, const double* __restrict__ b, const double* __restrict__ w,
                                                       const bjreal* __restrict__ binv, double* __restrict__ r,
                                                       double* __restrict__ z, double* __restrict__ p, double* __restrict__ partial) {
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < d.nc_owned) {
        double bv[NV], wv[NV], rv[NV], zv[NV], zb[NV];
        ldv<NV>(b, c, bv);
        ldv<NV>(w, c, wv);
#pragma unroll
        for (int a = 0; a < NV; ++a) rv[a] = bv[a] - wv[a];
        block_matvec<NV>(binv, c, rv, zv);
        block_matvec<NV>(binv, c, bv, zb);
        stv<NV>(r, c, rv);
        stv<NV>(z, c, zv);
        stv<NV>(p, c, zv);
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            acc[0] += rv[a] * zv[a];
            acc[1] += zv[a] * zv[a];
            acc[2] += zb[a] * zb[a];
            acc[3] += rv[a] * rv[a];
        }
        acc[3] = residual_measure(d, c, acc[3]);
    }
    write_partials<4>(partial, 1, acc);
}

template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_dot2(VecDims d, const double* __restrict__ u, const double* __restrict__ v,
                                                    const double* __restrict__ u2, const double* __restrict__ v2,
                                                    double* __restrict__ partial, const int* __restrict__ status) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[2] = {0.0, 0.0};
    if (c < d.nc_owned) {
        double a[NV], b[NV];
        ldv<NV>(SYS_PTR(u, s), c, a);
        ldv<NV>(SYS_PTR(v, s), c, b);
#pragma unroll
        for (int k = 0; k < NV; ++k) acc[0] += a[k] * b[k];
        if (u2) {
            ldv<NV>(SYS_PTR(u2, s), c, a);
            ldv<NV>(SYS_PTR(v2, s), c, b);
#pragma unroll
            for (int k = 0; k < NV; ++k) acc[1] += a[k] * b[k];
        }
    }
    write_partials<2>(partial, d.nsys, acc);
}

// x += alpha p ; r -= alpha w ; z = Binv r ; partials r.z, z.z
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_cg_update(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                         const double* __restrict__ p, const double* __restrict__ w,
                                                         const bjreal* __restrict__ binv, double* __restrict__ x,
                                                         double* __restrict__ r, double* __restrict__ z, double* __restrict__ partial) {
    if (status[0]) return;
    const double alpha = scal[KS_ALPHA];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    if (c < d.nc_owned) {
        double pv[NV], wv[NV], xv[NV], rv[NV], zv[NV];
        ldv<NV>(p, c, pv);
        ldv<NV>(w, c, wv);
        ldv<NV>(x, c, xv);
        ldv<NV>(r, c, rv);
#pragma unroll
        for (int a = 0; a < NV; ++a) { xv[a] += alpha * pv[a]; rv[a] -= alpha * wv[a]; }
        block_matvec<NV>(binv, c, rv, zv);
        stv<NV>(x, c, xv);
        stv<NV>(r, c, rv);
        stv<NV>(z, c, zv);
#pragma unroll
        for (int a = 0; a < NV; ++a) { acc[0] += rv[a] * zv[a]; acc[1] += zv[a] * zv[a]; acc[2] += rv[a] * rv[a]; }
        acc[2] = residual_measure(d, c, acc[2]);
    }
    write_partials<3>(partial, 1, acc);
}

// The same update fused with stage 1 of the tile-wise restriction of the auxiliary-space correction (amg_restrict.hip: k_restrict_tiles), for
// preconditioners WITHOUT the DG-level Chebyshev step (large uniform meshes, knp_set_emi_dg_smoother): the restricted vector is the new
// residual, which this kernel has in registers -- one pass over r less per PCG iteration (r=3: 104 us).  No partial sums: with a
// hierarchy k_prolong_dot forms them from the corrected z.  grid = tiles of tile_cells consecutive owned cells.
template <int NV>
__global__ __launch_bounds__(256) void k_cg_update_restrict(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                            const double* __restrict__ p, const double* __restrict__ w,
                                                            const bjreal* __restrict__ binv, double* __restrict__ x, double* __restrict__ r,
                                                            double* __restrict__ z, TileTables T, double* __restrict__ part) {
    extern __shared__ double s_r[];
    if (status[0]) return;                                     // converged: the V-cycle's output is not used either
    const double alpha = scal[KS_ALPHA];
    const int64_t c0 = (int64_t)blockIdx.x * T.tile_cells;
    const int ncell = (int)((d.nc_owned - c0 < T.tile_cells) ? (d.nc_owned - c0) : T.tile_cells);
    for (int i = threadIdx.x; i < ncell; i += 256) {
        const int64_t c = c0 + i;
        double pv[NV], wv[NV], xv[NV], rv[NV], zv[NV];
        ldv<NV>(p, c, pv);
        ldv<NV>(w, c, wv);
        ldv<NV>(x, c, xv);
        ldv<NV>(r, c, rv);
#pragma unroll
        for (int a = 0; a < NV; ++a) { xv[a] += alpha * pv[a]; rv[a] -= alpha * wv[a]; s_r[i * NV + a] = rv[a]; }
        block_matvec<NV>(binv, c, rv, zv);
        stv<NV>(x, c, xv);
        stv<NV>(r, c, rv);
        stv<NV>(z, c, zv);
    }
    __syncthreads();
    tile_slot_sums(s_r, T.tile_off, T.slot_ptr, T.slot_idx, part);
}

// z += P e (conforming correction, gathered through dg2cg) ; partials r.z, z.z, ||r||_w^2 (NR = 3)  |  on init (NR = 4): r.z, z.z,
// (Minv b).(Minv b), ||r||_w^2
template <int NV, int NR>
__global__ __launch_bounds__(KNP_BLOCK) void k_prolong_dot(VecDims d, const int* __restrict__ status, int use_status,
                                                           const int32_t* __restrict__ dg2cg, const double* __restrict__ e,
                                                           const double* __restrict__ r, double* __restrict__ z,
                                                           const double* __restrict__ e2, double* __restrict__ z2,
                                                           double* __restrict__ partial) {
    if (use_status && status[0]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[NR];
#pragma unroll
    for (int k = 0; k < NR; ++k) acc[k] = 0.0;
    if (c < d.nc_owned) {
        double rv[NV], zv[NV];
        ldv<NV>(r, c, rv);
        ldv<NV>(z, c, zv);
        double ad[NV];
        prolong_cell<NV>(dg2cg, e, c, ad);
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            zv[a] += ad[a];
            acc[0] += rv[a] * zv[a];
            acc[1] += zv[a] * zv[a];
            acc[NR - 1] += rv[a] * rv[a];
        }
        acc[NR - 1] = residual_measure(d, c, acc[NR - 1]);
        stv<NV>(z, c, zv);
        if (NR == 4) {
            double bv[NV];
            ldv<NV>(z2, c, bv);
            prolong_cell<NV>(dg2cg, e2, c, ad);
#pragma unroll
            for (int a = 0; a < NV; ++a) {
                bv[a] += ad[a];
                acc[2] += bv[a] * bv[a];
            }
        }
    }
    write_partials<NR>(partial, 1, acc);
}

// y += P e for a PAIR of species whose corrections sit interleaved in the shared hierarchy's level vector (grid.y = pair): one
// 16-byte gather per DG dof serves both
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_prolong_add_pair(VecDims d, const int* __restrict__ status, const int32_t* __restrict__ dg2cg,
                                                                const double* __restrict__ e, int64_t ncg, double* __restrict__ y) {
    const int s0 = 2 * blockIdx.y;
    const bool on0 = !status[2 * s0], on1 = !status[2 * (s0 + 1)];
    if (!on0 && !on1) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    const double2* e2 = reinterpret_cast<const double2*>(e + (int64_t)s0 * ncg);
    double2 ad[NV];
#pragma unroll
    for (int a = 0; a < NV; ++a) ad[a] = e2[dg2cg[c * NV + a]];
    double* y0 = y + (int64_t)s0 * d.nc * NV;
    double* y1 = y0 + d.nc * NV;
    double yv[NV];
    if (on0) {
        ldv<NV>(y0, c, yv);
#pragma unroll
        for (int a = 0; a < NV; ++a) yv[a] += ad[a].x;
        stv<NV>(y0, c, yv);
    }
    if (on1) {
        ldv<NV>(y1, c, yv);
#pragma unroll
        for (int a = 0; a < NV; ++a) yv[a] += ad[a].y;
        stv<NV>(y1, c, yv);
    }
}

// y += P e for one species block (BiCGStab preconditioner application)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_prolong_add(VecDims d, const int* __restrict__ status, int sys,
                                                           const int32_t* __restrict__ dg2cg, const double* __restrict__ e,
                                                           int64_t ncg, double* __restrict__ y) {
    int nil = 1;
    if (sys < 0) {                                   // batched: grid.y = species, y is [nsys][nc*NV]; e is the shared hierarchy's level
        sys = blockIdx.y;                            // vector: columns interleaved in pairs when nsys is even (amg_vcycle.hip)
        nil = (d.nsys % 2 == 0) ? 2 : 1;
        e += (int64_t)(sys / nil) * nil * ncg + (sys % nil);
        y += (int64_t)sys * d.nc * NV;
    }
    if (status[2 * sys]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double yv[NV];
    ldv<NV>(y, c, yv);
    double ad[NV];
    prolong_cell<NV>(dg2cg, e, c, ad, nil);
#pragma unroll
    for (int a = 0; a < NV; ++a) yv[a] += ad[a];
    stv<NV>(y, c, yv);
}

// z = Binv r (plain block-Jacobi apply, used to precondition b on init when the AMG term is active)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_bj_apply(VecDims d, const bjreal* __restrict__ binv, const double* __restrict__ r,
                                                        double* __restrict__ z, int s = 0) {
    // binv: the [nsys][nc][NV*NV] array (system s is selected here); r, z: the system's own vectors
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double rv[NV], zv[NV];
    ldv<NV>(r, c, rv);
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, rv, zv);
    stv<NV>(z, c, zv);
}

// p = z + beta p
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_cg_p(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                    const double* __restrict__ z, double* __restrict__ p) {
    if (status[0]) return;
    const double beta = scal[KS_BETA];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double zv[NV], pv[NV];
    ldv<NV>(z, c, zv);
    ldv<NV>(p, c, pv);
#pragma unroll
    for (int a = 0; a < NV; ++a) pv[a] = zv[a] + beta * pv[a];
    stv<NV>(p, c, pv);
}

// ---- BiCGStab kernels (system = blockIdx.y) ------------------------------------------------------
// r = b - w ; rhat = r ; p = v = 0 (ZPV; BiCGStab leaves them alone and runs its first k_bi_p in the FIRST form) ; partials r.r, b.b
template <int NV, bool ZPV = true>
__global__ __launch_bounds__(KNP_BLOCK) void k_bi_init(VecDims d, const double* __restrict__ b, const double* __restrict__ w,
                                                       double* __restrict__ r, double* __restrict__ rhat, double* __restrict__ p,
                                                       double* __restrict__ v, double* __restrict__ partial) {
    const int s = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};                 // r.r (= rho_1, plain), ||r||_w^2 | ||r/vol||_8^8, ||b||_w^2 | ||b/vol||_8^8
    if (c < d.nc_owned) {
        double bv[NV], wv[NV], rv[NV], zero[NV];
        ldv<NV>(SYS_PTR(b, s), c, bv);
        ldv<NV>(SYS_PTR(w, s), c, wv);
#pragma unroll
        for (int a = 0; a < NV; ++a) { rv[a] = bv[a] - wv[a]; zero[a] = 0.0; acc[0] += rv[a] * rv[a]; acc[2] += bv[a] * bv[a]; }
        acc[1] = residual_measure(d, c, acc[0]);
        acc[2] = residual_measure(d, c, acc[2]);
        stv<NV>(SYS_PTR(r, s), c, rv);
        stv<NV>(SYS_PTR(rhat, s), c, rv);
        if (ZPV) {
            stv<NV>(SYS_PTR(p, s), c, zero);
            stv<NV>(SYS_PTR(v, s), c, zero);
        }
    }
    write_partials<3>(partial, d.nsys, acc);
}

// p = r + beta (p - omega v) ; y = Binv p.  FIRST (iteration 0, p = v = 0): p = r, and p, v are not read
template <int NV, bool FIRST = false>
__global__ __launch_bounds__(KNP_BLOCK) void k_bi_p(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                    const double* __restrict__ r, const double* __restrict__ v,
                                                    const bjreal* __restrict__ binv, double* __restrict__ p, double* __restrict__ y) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const double beta = scal_row(scal, s)[KS_BETA], omega = scal_row(scal, s)[KS_OMEGA];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double rv[NV], vv[NV], pv[NV], yv[NV];
    ldv<NV>(SYS_PTR(r, s), c, rv);
    if (FIRST) {
#pragma unroll
        for (int a = 0; a < NV; ++a) pv[a] = rv[a] + 0.0;        // beta = 0, omega = 1 after OP_BI_INIT: + 0.0 keeps the sign of a zero r as before
    } else {
        ldv<NV>(SYS_PTR(v, s), c, vv);
        ldv<NV>(SYS_PTR(p, s), c, pv);
#pragma unroll
        for (int a = 0; a < NV; ++a) pv[a] = rv[a] + beta * (pv[a] - omega * vv[a]);
    }
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, pv, yv);
    stv<NV>(SYS_PTR(p, s), c, pv);
    stv<NV>(SYS_PTR(y, s), c, yv);
}

// s = r - alpha v (in place in r) ; z = Binv s
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_bi_s(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                    const double* __restrict__ v, const bjreal* __restrict__ binv,
                                                    double* __restrict__ r, double* __restrict__ z) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const double alpha = scal_row(scal, s)[KS_ALPHA];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double rv[NV], vv[NV], zv[NV];
    ldv<NV>(SYS_PTR(r, s), c, rv);
    ldv<NV>(SYS_PTR(v, s), c, vv);
#pragma unroll
    for (int a = 0; a < NV; ++a) rv[a] -= alpha * vv[a];
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, rv, zv);
    stv<NV>(SYS_PTR(r, s), c, rv);
    stv<NV>(SYS_PTR(z, s), c, zv);
}

// second step of the two-step Chebyshev iteration on Binv A (zero initial guess), given t = A y0 with y0 = Binv r:
//   y = ca y0 + cb Binv (r - ct t) = Binv ((ca + cb) r - cb ct t)        (Binv is linear: y0 need not be read back)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_bj_cheb2(VecDims d, const int* __restrict__ status, const bjreal* __restrict__ binv,
                                                        const double* __restrict__ r, const double* __restrict__ t,
                                                        double* __restrict__ y, double cr, double ctt) {
    const int s = blockIdx.y;
    if (status && status[2 * s]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double rv[NV], tv[NV], yv[NV];
    ldv<NV>(SYS_PTR(r, s), c, rv);
    ldv<NV>(SYS_PTR(t, s), c, tv);
#pragma unroll
    for (int a = 0; a < NV; ++a) rv[a] = cr * rv[a] - ctt * tv[a];
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, rv, yv);
    stv<NV>(SYS_PTR(y, s), c, yv);
}

// The same step fused with stage 1 of the tile-wise restriction of the coarse correction (amg_restrict.hip: k_restrict_tiles): both read r and
// t = A Binv r, and the restricted vector r - ct t (hybrid form; ct = 0: r itself) is formed from the values already in registers.
// One pass over r and t instead of two (128 MB per preconditioner application at r=2).  grid = (tiles, systems).
template <int NV>
__global__ __launch_bounds__(256) void k_bj_cheb2_restrict(VecDims d, const int* __restrict__ status, const bjreal* __restrict__ binv,
                                                           const double* __restrict__ r, const double* __restrict__ t, double* __restrict__ y,
                                                           double cr, double ctt, TileTables T, double* __restrict__ part, double ct) {
    extern __shared__ double s_r[];
    const int s = blockIdx.y;
    if (status && status[2 * s]) return;                       // converged system: its V-cycle output is not used either
    const int64_t c0 = (int64_t)blockIdx.x * T.tile_cells;
    const int ncell = (int)((d.nc_owned - c0 < T.tile_cells) ? (d.nc_owned - c0) : T.tile_cells);
    for (int i = threadIdx.x; i < ncell; i += 256) {
        const int64_t c = c0 + i;
        double rv[NV], tv[NV], yv[NV];
        ldv<NV>(SYS_PTR(r, s), c, rv);
        ldv<NV>(SYS_PTR(t, s), c, tv);
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            s_r[i * NV + a] = fma(-ct, tv[a], rv[a]);
            rv[a] = cr * rv[a] - ctt * tv[a];
        }
        block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, rv, yv);
        stv<NV>(SYS_PTR(y, s), c, yv);
    }
    __syncthreads();
    tile_slot_sums(s_r, T.tile_off, T.slot_ptr, T.slot_idx, part + (int64_t)s * T.nslots);
}

// out = alpha[s] * in  (per system)
__global__ void k_scale_sys(int64_t n_owned, int64_t stride, const double* __restrict__ in, double a0, double a1, double a2, double a3,
                            double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_owned) return;
    const int s = blockIdx.y;
    const double a = s == 0 ? a0 : (s == 1 ? a1 : (s == 2 ? a2 : a3));
    out[(int64_t)s * stride + i] = a * in[(int64_t)s * stride + i];
}

// x += alpha y + omega z ; r = s - omega t ; partials rhat.r, ||r||_w^2
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_bi_x(VecDims d, const double* __restrict__ scal, const int* __restrict__ status,
                                                    const double* __restrict__ y, const double* __restrict__ z,
                                                    const double* __restrict__ t, const double* __restrict__ rhat,
                                                    double* __restrict__ x, double* __restrict__ r, double* __restrict__ partial) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const double alpha = scal_row(scal, s)[KS_ALPHA], omega = scal_row(scal, s)[KS_OMEGA];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[2] = {0.0, 0.0};
    if (c < d.nc_owned) {
        double yv[NV], zv[NV], tv[NV], hv[NV], xv[NV], rv[NV];
        ldv<NV>(SYS_PTR(y, s), c, yv);
        ldv<NV>(SYS_PTR(z, s), c, zv);
        ldv<NV>(SYS_PTR(t, s), c, tv);
        ldv<NV>(SYS_PTR(rhat, s), c, hv);
        ldv<NV>(SYS_PTR(x, s), c, xv);
        ldv<NV>(SYS_PTR(r, s), c, rv);
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            xv[a] += alpha * yv[a] + omega * zv[a];
            rv[a] -= omega * tv[a];
            acc[0] += hv[a] * rv[a];
            acc[1] += rv[a] * rv[a];
        }
        acc[1] = residual_measure(d, c, acc[1]);
        stv<NV>(SYS_PTR(x, s), c, xv);
        stv<NV>(SYS_PTR(r, s), c, rv);
    }
    write_partials<2>(partial, d.nsys, acc);
}

// inf-norm of a - b over the owned part of an [nsys][nc*NV] field (Picard stopping test, solver.py:879-880)
__global__ __launch_bounds__(KNP_BLOCK) void k_max_abs_diff(int64_t n_owned, int64_t stride, int nsys, const double* __restrict__ a,
                                                            const double* __restrict__ b, double* __restrict__ partial) {
    __shared__ double lds[KNP_BLOCK / 64];
    double v = 0.0;
    for (int s = 0; s < nsys; ++s)
        for (int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x; i < n_owned; i += (int64_t)gridDim.x * KNP_BLOCK)
            v = fmax(v, fabs(a[s * stride + i] - b[s * stride + i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KNP_BLOCK / 64; ++w) v = fmax(v, lds[w]);
        partial[blockIdx.x] = v;
    }
}

int max_abs_diff(knp_ctx* c, const double* a, const double* b, int nsys, double* out) {
    const int nb = 256;
    const int64_t n_owned = c->m.nc_owned * c->nd, stride = c->m.nc * c->nd;
    hipLaunchKernelGGL(k_max_abs_diff, dim3(nb), dim3(KNP_BLOCK), 0, c->stream, n_owned, stride, nsys, a, b, c->partial);
    HIPCHK(c, hipGetLastError());
    std::vector<double> h(nb);
    HIPCHK(c, hipMemcpyAsync(h.data(), c->partial, sizeof(double) * nb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    double m = 0.0;
    for (double v : h) m = v > m ? v : m;
    if (c->dist) {
        int rc = allreduce_max(c, &m);
        if (rc) return rc;
    }
    *out = m;
    return 0;
}

// ---- host drivers ---------------------------------------------------------------------------------

// f(std::integral_constant<int, NV>) for the context's dofs per cell; `unsupported` (may be null) becomes the error text otherwise
template <typename F> static int dispatch_nd(knp_ctx* c, const char* unsupported, F&& f) {
    switch (c->nd) {
        case 3: return f(std::integral_constant<int, 3>());
        case 4: return f(std::integral_constant<int, 4>());
        case 6: return f(std::integral_constant<int, 6>());
        case 10: return f(std::integral_constant<int, 10>());
    }
    if (unsupported) c->err = unsupported;
    return -1;
}

static int finalize(knp_ctx* c, int op, int nsys, int nred, const StopTest& st, int aux = 0) {
    const int64_t nb = grid_for(c->m.nc_owned);
    double* red = krylov_red(c);
    const int dop = c->dist ? 0 : op;
    // partial rows in flight per thread: 4 up to 8 192 producer blocks (r=2: 3 888), 8 beyond (r=3: 31 104 blocks were eight
    // dependent trips = 64 us)
    const bool deep = nb > 8192;
#define KNP_REDUCE(NR_)                                                                                                                  \
    do {                                                                                                                                 \
        if (deep) hipLaunchKernelGGL((k_reduce<NR_, 8>), dim3(nsys), dim3(KNP_REDUCE_BLOCK), 0, c->stream, c->partial, nb, nsys, red, dop,  \
                                     c->scal, c->status, st, aux);                                                                       \
        else hipLaunchKernelGGL((k_reduce<NR_, 4>), dim3(nsys), dim3(KNP_REDUCE_BLOCK), 0, c->stream, c->partial, nb, nsys, red, dop,       \
                                c->scal, c->status, st, aux);                                                                            \
    } while (0)
    switch (nred) {
        case 1: KNP_REDUCE(1); break;
        case 2: KNP_REDUCE(2); break;
        case 3: KNP_REDUCE(3); break;
        case 4: KNP_REDUCE(4); break;
        case 8: KNP_REDUCE(8); break;
        default: c->err = "finalize: unsupported number of partial sums"; return -1;
    }
#undef KNP_REDUCE
    if (c->dist) {
        int rc = allreduce_red(c, red, nsys * KNP_MAX_RED);
        if (rc) return rc;
        hipLaunchKernelGGL(k_scalar_op, dim3(1), dim3(64), 0, c->stream, op, nsys, red, c->scal, c->status, st, aux);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// One look at the device: the head of the status block (status words and every system's scalar row, KNP_LOOK_BYTES) to the pinned
// mirror with one copy and one wait -- one host round trip
int status_look(knp_ctx* c) {
    HIPCHK(c, hipMemcpyAsync(c->pinned, c->status, KNP_LOOK_BYTES, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    return 0;
}

static int poll_status(knp_ctx* c, int nsys, int* host_status) {
    { const int rc = status_look(c); if (rc) return rc; }
    for (int i = 0; i < 2 * nsys; ++i) host_status[i] = ((int*)c->pinned)[i];
    { int bits = ((int*)c->pinned)[KNP_PECLET_SLOT]; float pe; memcpy(&pe, &bits, sizeof(pe)); c->last_peclet = pe; }
    if (((int*)c->pinned)[KNP_ODE_FAIL_SLOT]) {      // raised by k_ode_step earlier in this time step (`assert success`, membrane.py:113)
        hipMemsetAsync(c->status + KNP_ODE_FAIL_SLOT, 0, sizeof(int), c->stream);
        c->err = "ODE integrator did not reach the end time";
        return -4;
    }
    return 0;
}

// How many iterations to enqueue before the next look at the device's convergence flag.  Kernels of iterations past
// convergence are no-ops only for the vector updates -- operator applies and V-cycles still run -- so a fixed chunk of
// 25 wastes up to a whole solve's worth of work (17 useful + 8 wasted iterations at r=2).  Iteration counts are stable
// from one time step to the next: enqueue (previous count - 1) iterations without looking, then look after every iteration.
// A look costs one status read and the host's re-enqueue (about 30 us of idle GPU); an iteration enqueued past convergence
// costs its applies and V-cycles (r=2: about 0.75 ms for KNP, 0.2 ms for EMI), so past the prediction looking every time wins
// (profiles/r05_poll_tail.txt).  KNP_POLL_TAIL=0 restores the previous rule (every 2, every 1 for 1-2 iteration solves).
static int poll_tail() {
    return env_int("KNP_POLL_TAIL", 1);                    // read per call: tests switch it inside one process
}
// The look behind a solve's init kernel is dropped when the previous solve of the kind iterated (predicted >= 1): a system that is
// converged at entry is rare (KNP has an iteration floor, the EMI target test needs an iteration), every kernel and scalar
// recurrence of an iteration either returns on a set status word or writes scratch only, and the first regular look sees whatever
// the dropped one would have seen -- convergence at entry, the ODE failure word -- one chunk of no-op launches later.  Without a
// prediction, and with maxit = 0 (no look would follow), the look stays.  KNP_POLL_FIRST=1 restores it everywhere.
static bool skip_first_look(int predicted, int maxit) {
    return predicted >= 1 && maxit > 0 && !env_flag("KNP_POLL_FIRST", false);   // read per call, like KNP_POLL_TAIL
}
// The scalar rows of the first ns systems at the end of a solve.  They were final when the last look ran and nothing was enqueued
// since, so the look's host copy holds them.  KNP_FOLD_EPILOGUE=0 (read per call): a blocking copy of their own, as before.
static int epilogue_scalars(knp_ctx* c, int ns, double* hscal) {
    if (env_flag("KNP_FOLD_EPILOGUE", true)) { memcpy(hscal, look_scal(c), sizeof(double) * KS_N * ns); return 0; }
    HIPCHK(c, host_memcpy(c, hscal, krylov_scal(c), sizeof(double) * KS_N * ns, hipMemcpyDeviceToHost));
    return 0;
}
static inline int next_chunk(int it, int maxit, int check_every, int predicted) {
    int chunk = check_every;
    if (predicted > 0) {
        const int ahead = predicted - 1 - it;
        const int tail = poll_tail();
        chunk = ahead > 0 ? (ahead < 4 * check_every ? ahead : 4 * check_every)
                          : (tail > 0 ? tail : (predicted <= 2 ? 1 : 2));   // old rule: 1-2 iteration solves look every time
    }
    return (maxit - it < chunk) ? (maxit - it) : chunk;
}

// KNP (BiCGStab takes any preconditioner): HYBRID two-level form -- the coarse correction acts on r1 = r - t / theta, the residual left
// by the FIRST step of the DG-level Chebyshev smoother (t = A Binv r is the operator product that smoother computes anyway), instead of
// on r:  z = S2(r) + P Ac^+ P^T r1.  Same cost per application (the restriction reads t next to r), fewer iterations: 15 instead
// of 19 BiCGStab iterations to 1e-6 on the oracle's KNP matrix at the r=2 diffusion number (tools/precond_experiment.py).  The EMI
// system keeps the additive (symmetric) form PCG needs.  KNP_HYBRID=0 restores the additive form.
static bool knp_hybrid() {
    static const bool on = env_flag("KNP_HYBRID", true);
    return on;
}
template <bool EMI> static double bj_lmin_frac() {
    // lower end of the Chebyshev interval as a fraction of lambda_max(Binv A): 0.05 measured best over 30 steps at r=2 for the additive
    // form (0.03..0.06) and for the hybrid one (0.05: 9.06, 0.08: 9.13, 0.12: 9.44 ms/step; profiles/r03_hybrid_ab.txt)
    static const double v = getenv("KNP_BJ_LMIN") ? atof(getenv("KNP_BJ_LMIN")) : 0.05;
    return v;
}
template <bool EMI> static double bj_theta(const KrylovVecs& kv) { return 0.5 * (1.0 + bj_lmin_frac<EMI>()) * kv.bj_lmax; }

// y (= Binv r on entry) <- two-step Chebyshev block-Jacobi of r:  costs one operator apply and one fused vector kernel
// Hfuse != null: the coarse correction's restriction of (r - ct_restrict t) into Hfuse is done in the same pass (k_bj_cheb2_restrict +
// the remaining restriction stages); the caller then skips amg_restrict_from_dg
template <int NV, bool EMI>
static int bj_cheb2(knp_ctx* c, const VecDims& d, const KrylovVecs& kv, const double* r, double* y, bool use_status = true,
                    AmgHierarchy* Hfuse = nullptr, double ct_restrict = 0.0) {
    int rc;
    if ((rc = dist_apply(c, EMI ? 0 : 1, y, kv.coef, kv.tmp))) return rc;
    const double lmin_frac = bj_lmin_frac<EMI>();
    const double lmax = kv.bj_lmax, lmin = lmin_frac * lmax;
    const double theta = 0.5 * (lmax + lmin), delta = 0.5 * (lmax - lmin), sigma = theta / delta, rho0 = 1.0 / sigma;
    const double rho1 = 1.0 / (2.0 * sigma - rho0);
    const double cr = (1.0 + rho1 * rho0) / theta + 2.0 * rho1 / delta, ctt = (2.0 * rho1 / delta) / theta;
    const int* st = use_status ? (const int*)c->status : (const int*)nullptr;
    if (Hfuse) {
        AmgHierarchy& H = *Hfuse;
        if ((rc = amg_restrict_tiles_prepare(c, H))) return rc;
        hipLaunchKernelGGL(k_bj_cheb2_restrict<NV>, dim3((unsigned)H.tiles.ntiles, (unsigned)d.nsys), dim3(256),
                           sizeof(double) * H.tiles.tile_cells * NV, c->stream, d, st, kv.binv, r, (const double*)kv.tmp, y, cr, ctt, H.tiles,
                           H.part, ct_restrict);
        return amg_restrict_finish(c, H);
    }
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)d.nsys), b(KNP_BLOCK);
    hipLaunchKernelGGL(k_bj_cheb2<NV>, g, b, 0, c->stream, d, st, kv.binv, r, (const double*)kv.tmp, y, cr, ctt);
    return 0;
}
// whether the second Chebyshev step and the restriction into H can share one pass (KNP_FUSE_RESTRICT=0: two passes, A/B runs)
static bool fuse_restrict(const KrylovVecs& kv, const AmgHierarchy& H, int nsys) {
    const bool on = env_flag("KNP_FUSE_RESTRICT", true);    // read per call: tests switch it inside one process
    return on && kv.bj_lmax > 0.0 && H.ready && H.tiles.usable() && H.ncol == nsys;
}

static bool fuse_update_restrict(const AmgHierarchy& H) {
    // KNP_FUSE_CG_RESTRICT is read per call: tests switch it inside one process
    return env_flag("KNP_FUSE_CG_RESTRICT", true) && H.ready && H.tiles.usable() && H.ncol == 1;
}

// power iteration for lambda_max(Binv A) of the batched KNP operator (inf-norm normalisation; max over the species)
template <int NV, bool EMI>
static int bj_lambda_max_impl(knp_ctx* c, KrylovVecs& kv, int iters, double* out) {
    const int ns = EMI ? 1 : c->p.n_sys;
    if (ns > 4) { *out = 0.0; return 0; }
    VecDims d{c->m.nc_owned, c->m.nc, ns, EMI ? nullptr : kv.bj_idx, EMI ? nullptr : kv.bj_tab, kv.ivol, 0};
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)ns), b(KNP_BLOCK);
    const int64_t n_owned = c->m.nc_owned * NV, stride = c->m.nc * NV;
    const dim3 gs((unsigned)((n_owned + 255) / 256), (unsigned)ns);
    int rc;
    HIPCHK(c, hipMemsetAsync(kv.z, 0, sizeof(double) * ns * stride, c->stream));
    HIPCHK(c, hipMemcpyAsync(kv.v, kv.b, sizeof(double) * ns * stride, hipMemcpyDeviceToDevice, c->stream));
    double lam = 0.0, nv = 0.0;
    if ((rc = max_abs_diff(c, kv.v, kv.z, ns, &nv))) return rc;
    if (!(nv > 0.0)) { *out = 0.0; return 0; }
    for (int it = 0; it < iters; ++it) {
        if ((rc = dist_apply(c, EMI ? 0 : 1, kv.v, kv.coef, kv.w))) return rc;
        for (int s = 0; s < ns; ++s)
            hipLaunchKernelGGL(k_bj_apply<NV>, dim3(g.x), b, 0, c->stream, d, (const bjreal*)kv.binv,
                               (const double*)(kv.w + (int64_t)s * stride), kv.y + (int64_t)s * stride, s);
        double ny = 0.0;
        if ((rc = max_abs_diff(c, kv.y, kv.z, ns, &ny))) return rc;
        lam = ny / nv;
        if (!(ny > 0.0)) break;
        const double a = 1.0 / ny;
        hipLaunchKernelGGL(k_scale_sys, gs, dim3(256), 0, c->stream, n_owned, stride, (const double*)kv.y, a, a, a, a, kv.v);
        nv = 1.0;
    }
    *out = lam;
    return 0;
}

int knp_bj_lambda_max(knp_ctx* c, KrylovVecs& kv, int iters, double* out, bool emi) {
    return dispatch_nd(c, nullptr, [&](auto nv) {
        constexpr int NV = decltype(nv)::value;
        return emi ? bj_lambda_max_impl<NV, true>(c, kv, iters, out) : bj_lambda_max_impl<NV, false>(c, kv, iters, out);
    });
}

// One PCG iteration's  x += alpha p ; r -= alpha w ; z = M^-1 r  with the partial sums r.z, z.z, ||r||_w^2 behind it (H = the EMI hierarchy,
// or null: block-Jacobi alone).  Three sequences of launches:
//   no DG-level Chebyshev step, tiles: update fused with stage 1 of the restriction of the new residual (KNP_FUSE_CG_RESTRICT=0: two passes)
//   Chebyshev step, tiles:             update ; Chebyshev step fused with stage 1 of the restriction (KNP_FUSE_RESTRICT=0: two passes)
//   otherwise:                         update ; Chebyshev step if there is one ; restriction
// each followed by the V-cycle and k_prolong_dot, which forms the partial sums from the corrected z (without H: k_cg_update's own)
template <int NV>
static int emi_precondition_residual(knp_ctx* c, const VecDims& d, const KrylovVecs& kv, AmgHierarchy* H) {
    const dim3 g((unsigned)grid_for(c->m.nc_owned)), b(KNP_BLOCK);
    const bool cheb = kv.bj_lmax > 0.0;
    int rc;
    if (H && !cheb && fuse_update_restrict(*H)) {
        if ((rc = amg_restrict_tiles_prepare(c, *H))) return rc;
        hipLaunchKernelGGL(k_cg_update_restrict<NV>, dim3((unsigned)H->tiles.ntiles), dim3(256), sizeof(double) * H->tiles.tile_cells * NV,
                           c->stream, d, c->scal, c->status, kv.p, kv.w, kv.binv, kv.x, kv.r, kv.z, H->tiles, H->part);
        if ((rc = amg_restrict_finish(c, *H))) return rc;
    } else {
        hipLaunchKernelGGL(k_cg_update<NV>, g, b, 0, c->stream, d, c->scal, c->status, kv.p, kv.w, kv.binv, kv.x, kv.r, kv.z, c->partial);
        if (!H) return 0;
        if (fuse_restrict(kv, *H, 1)) {
            if ((rc = bj_cheb2<NV, true>(c, d, kv, kv.r, kv.z, true, H, 0.0))) return rc;
        } else {
            if (cheb && (rc = bj_cheb2<NV, true>(c, d, kv, kv.r, kv.z))) return rc;
            if ((rc = amg_restrict_from_dg(c, *H, kv.r))) return rc;
        }
    }
    if ((rc = amg_vcycle(c, *H))) return rc;
    hipLaunchKernelGGL((k_prolong_dot<NV, 3>), g, b, 0, c->stream, d, c->status, 1, H->dg2cg, H->levels[0].x, kv.r, kv.z,
                       (const double*)nullptr, (double*)nullptr, c->partial);
    return 0;
}

template <int NV>
static int pcg_impl(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int check_every, int* niter, double* res) {
    VecDims d{c->m.nc_owned, c->m.nc, 1, nullptr, nullptr, kv.ivol, (kv.d8 && kv.ivol) ? 1 : 0};
    const StopTest stop{rtol, atol, kv.r_abs, 0, d.d8};
    const dim3 g((unsigned)grid_for(c->m.nc_owned)), b(KNP_BLOCK);
    int rc;
    if ((rc = dist_apply(c, 0, kv.x, kv.coef, kv.w))) return rc;
    AmgHierarchy* H = (c->amg.size() && c->amg[0].ready) ? &c->amg[0] : nullptr;
    hipLaunchKernelGGL(k_cg_init<NV>, g, b, 0, c->stream, d, kv.b, kv.w, kv.binv, kv.r, kv.z, kv.p, c->partial);
    if (H) {
        // z = Binv r + P V(P^T r) ; reference norm uses the same preconditioner on b (stored in y)
        hipLaunchKernelGGL(k_bj_apply<NV>, g, b, 0, c->stream, d, kv.binv, kv.b, kv.y);
        if (kv.bj_lmax > 0.0) {                  // same DG-level smoother on b (reference norm) and on r
            if ((rc = bj_cheb2<NV, true>(c, d, kv, kv.b, kv.y, false))) return rc;
            if ((rc = bj_cheb2<NV, true>(c, d, kv, kv.r, kv.z, false))) return rc;
        }
        if ((rc = amg_restrict_from_dg(c, *H, kv.b))) return rc;
        if ((rc = amg_vcycle(c, *H))) return rc;
        HIPCHK(c, hipMemcpyAsync(kv.v, H->levels[0].x, sizeof(double) * H->ncg, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = amg_restrict_from_dg(c, *H, kv.r))) return rc;
        if ((rc = amg_vcycle(c, *H))) return rc;
        hipLaunchKernelGGL((k_prolong_dot<NV, 4>), g, b, 0, c->stream, d, c->status, 0, H->dg2cg, H->levels[0].x, kv.r, kv.z,
                           kv.v, kv.y, c->partial);
        HIPCHK(c, hipMemcpyAsync(kv.p, kv.z, sizeof(double) * c->m.nc * NV, hipMemcpyDeviceToDevice, c->stream));
    }
    if ((rc = finalize(c, OP_CG_INIT, 1, 4, stop))) return rc;
    if (kv.r_abs > 0.0) {               // ||x0||_A^2 = x0 . A x0: the scale of the energy-norm test (w = A x0 is still intact)
        hipLaunchKernelGGL(k_dot2<NV>, dim3(g.x, 1), b, 0, c->stream, d, kv.x, kv.w, (const double*)nullptr, (const double*)nullptr, c->partial,
                           c->status);
        if ((rc = finalize(c, OP_CG_XA, 1, 1, stop))) return rc;
    }
    int hs[2] = {0, 0};
    int it = 0;
    if (!skip_first_look(c->last_it_emi, maxit) && (rc = poll_status(c, 1, hs))) return rc;
    while (!hs[0] && it < maxit) {
        const int chunk = next_chunk(it, maxit, check_every, c->last_it_emi);
        for (int k = 0; k < chunk; ++k) {
            if ((rc = dist_apply(c, 0, kv.p, kv.coef, kv.w))) return rc;
            hipLaunchKernelGGL(k_dot2<NV>, dim3(g.x, 1), b, 0, c->stream, d, kv.p, kv.w, (const double*)nullptr,
                               (const double*)nullptr, c->partial, c->status);
            if ((rc = finalize(c, OP_CG_ALPHA, 1, 1, stop))) return rc;
            if ((rc = emi_precondition_residual<NV>(c, d, kv, H))) return rc;
            if ((rc = finalize(c, OP_CG_BETA, 1, 3, stop))) return rc;
            hipLaunchKernelGGL(k_cg_p<NV>, g, b, 0, c->stream, d, c->scal, c->status, kv.z, kv.p);
        }
        it += chunk;
        if ((rc = poll_status(c, 1, hs))) return rc;
    }
    double hscal[KS_N];
    if ((rc = epilogue_scalars(c, 1, hscal))) return rc;
    *niter = hs[1];
    c->last_it_emi = hs[1];
    // the norm the stopping test looked at: the true residual (order-8 density norm) with a residual target, else PETSc's preconditioned norm
    res[0] = kv.r_abs > 0.0 ? hscal[KS_CG_RN0] : hscal[KS_RES0];
    res[1] = kv.r_abs > 0.0 ? hscal[KS_RNORM] : hscal[KS_RES];
    res[2] = kv.r_abs > 0.0 ? hscal[KS_CG_EST] / sqrt(fmax(fmax(hscal[KS_CG_XA], hscal[KS_CG_SUM]), 1.0e-300)) : hscal[KS_BNORM];
    if (hs[0] == KS_NAN) { c->err = "EMI PCG: NaN residual"; return -4; }
    if (hs[0] != KS_CONVERGED) { c->err = "EMI PCG did not converge"; return -3; }
    return 0;
}

int pcg_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int check_every, int* niter, double* res) {
    if (check_every < 1) check_every = 1;
    return dispatch_nd(c, "pcg: unsupported dofs per cell",
                       [&](auto nv) { return pcg_impl<decltype(nv)::value>(c, kv, rtol, atol, maxit, check_every, niter, res); });
}

// out_s += P_s V_s(P_s^T in_s) for every species s with an armed hierarchy (slot 1 + s).  The species' V-cycles are
// independent chains of tiny latency-bound kernels: species 0 runs on the context's stream, every further species
// on its own auxiliary stream (fork / join with events), so the chains overlap.
template <int NV>
static int knp_coarse_correction(knp_ctx* c, const VecDims& d, const double* in, double* out, const double* t = nullptr, double ct = 0.0,
                                 bool restricted = false) {
    const dim3 g1((unsigned)grid_for(c->m.nc_owned)), b(KNP_BLOCK);
    int active[KNP_MAX_SYS], na = 0;
    for (int s = 0; s < d.nsys; ++s)
        if ((int)c->amg.size() > 1 + s && c->amg[1 + s].ready) active[na++] = s;
    if (!na) return 0;
    int rc;
    if (c->amg[1].ready && c->amg[1].ncol == d.nsys) {
        // shared hierarchy: one restriction, one V-cycle and one prolongation carry all species as right-hand-side columns
        AmgHierarchy& H = c->amg[1];
        if (!restricted && (rc = amg_restrict_from_dg(c, H, in, nullptr, d.nc * NV, t, ct))) return rc;     // restricted: done by bj_cheb2's fused pass
        if ((rc = amg_vcycle(c, H))) return rc;
        if (d.nsys % 2 == 0)
            hipLaunchKernelGGL(k_prolong_add_pair<NV>, dim3(g1.x, (unsigned)(d.nsys / 2)), b, 0, c->stream, d, c->status, H.dg2cg,
                               H.levels[0].x, H.ncg, out);
        else
            hipLaunchKernelGGL(k_prolong_add<NV>, dim3(g1.x, (unsigned)d.nsys), b, 0, c->stream, d, c->status, -1, H.dg2cg, H.levels[0].x,
                               H.ncg, out);
        return 0;
    }
    // every species is an independent chain  restrict -> V-cycle -> prolong  of short latency-bound kernels writing
    // disjoint slices: species 0 runs on the context's stream, every further species on its own auxiliary stream
    // (fork / join with events).  With a communicator the restriction ends in an all-reduce on the context's stream, so
    // only the V-cycles fork.
    // (partitioned runs keep every species on the context's stream: the row-distributed level 0 exchanges its shared dofs on the
    // main communicator, whose calls must be enqueued in ONE order on every rank -- DESIGN.md section 6)
    const bool fork = na > 1 && !c->dist && c->amg[1 + active[0]].graph_tried && c->amg[1 + active[0]].graph_exec;
    if (!fork) {
        for (int i = 0; i < na; ++i) {
            const int s = active[i];
            if ((rc = amg_restrict_from_dg(c, c->amg[1 + s], in + (int64_t)s * d.nc * NV, nullptr, 0, t ? t + (int64_t)s * d.nc * NV : nullptr, ct))) return rc;
        }
    } else {
        while ((int)c->aux_streams.size() < na - 1) {
            hipStream_t st; hipEvent_t ev;
            HIPCHK(c, hipStreamCreate(&st));
            HIPCHK(c, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
            c->aux_streams.push_back(st);
            c->aux_events.push_back(ev);
        }
        if (!c->fork_event) HIPCHK(c, hipEventCreateWithFlags(&c->fork_event, hipEventDisableTiming));
        HIPCHK(c, hipEventRecord(c->fork_event, c->stream));
    }
    // aux streams first, so that their chains are already running while the host enqueues species 0
    for (int i = na - 1; i >= 0; --i) {
        const int s = active[i];
        AmgHierarchy& H = c->amg[1 + s];
        hipStream_t st = nullptr;
        if (fork && i > 0 && H.graph_exec) {
            st = c->aux_streams[i - 1];
            HIPCHK(c, hipStreamWaitEvent(st, c->fork_event, 0));
        }
        if (fork && (rc = amg_restrict_from_dg(c, H, in + (int64_t)s * d.nc * NV, st, 0, t ? t + (int64_t)s * d.nc * NV : nullptr, ct))) return rc;
        if ((rc = amg_vcycle(c, H, st))) return rc;
        hipLaunchKernelGGL(k_prolong_add<NV>, g1, b, 0, st ? st : c->stream, d, c->status, s, H.dg2cg, H.levels[0].x, H.ncg,
                           out + (int64_t)s * d.nc * NV);
        if (st) HIPCHK(c, hipEventRecord(c->aux_events[i - 1], st));
    }
    for (int i = 1; i < na; ++i)
        if (fork && c->amg[1 + active[i]].graph_exec) HIPCHK(c, hipStreamWaitEvent(c->stream, c->aux_events[i - 1], 0));
    return 0;
}

// out (= Binv in on entry) <- M^-1 in for the batched KNP systems: the two-step Chebyshev block-Jacobi smoother when there is one
// (kv.bj_lmax > 0), then the auxiliary-space coarse correction -- in the hybrid form on the residual the smoother's first step leaves,
// and with the restriction done in the smoother's pass where the two can share it (fuse_restrict)
template <int NV>
static int knp_precondition(knp_ctx* c, const VecDims& d, const KrylovVecs& kv, const double* in, double* out) {
    int rc;
    const bool hyb = kv.bj_lmax > 0.0 && knp_hybrid();
    const double ct = hyb ? 1.0 / bj_theta<false>(kv) : 0.0;
    const bool fuse = (int)c->amg.size() > 1 && fuse_restrict(kv, c->amg[1], d.nsys);
    if (kv.bj_lmax > 0.0 && (rc = bj_cheb2<NV, false>(c, d, kv, in, out, true, fuse ? &c->amg[1] : nullptr, ct))) return rc;
    return knp_coarse_correction<NV>(c, d, in, out, hyb ? kv.tmp : nullptr, ct, fuse);
}

// end of a KNP solve: iteration counts and residual norms of every system out, the prediction for the next solve's status polls, and
// the error text when a system did not converge
static int knp_solve_epilogue(knp_ctx* c, int ns, const int* hs, int* niter, double* res, const char* method) {
    double hscal[KNP_MAX_SYS * KS_N];
    { const int rc = epilogue_scalars(c, ns, hscal); if (rc) return rc; }
    int bad = 0;
    for (int s = 0; s < ns; ++s) {
        const double* S = scal_row(hscal, s);
        niter[s] = hs[2 * s + 1];
        if (s == 0 || niter[s] > c->last_it_knp) c->last_it_knp = niter[s];
        res[3 * s + 0] = S[KS_RES0];
        res[3 * s + 1] = S[KS_RES];
        res[3 * s + 2] = S[KS_BNORM];
        if (hs[2 * s] != KS_CONVERGED) bad = hs[2 * s] ? hs[2 * s] : -1;
    }
    if (bad) { c->err = std::string("KNP ") + method + " did not converge (status " + std::to_string(bad) + ")"; return -3; }
    return 0;
}

// BiCGStab's first iteration with p = v = 0 folded in: k_bi_init does not write the two zero vectors and the first k_bi_p does not
// read them (same bits: r + beta (0 - omega 0) = r).  KNP_FUSE_BI_FIRST=0: zeros written and read as before.
static bool bi_first_form() {
    return env_flag("KNP_FUSE_BI_FIRST", true);             // read per call: tests switch it inside one process
}

template <int NV>
static int bicgstab_impl(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every,
                         int* niter, double* res) {
    const int ns = c->p.n_sys;
    VecDims d{c->m.nc_owned, c->m.nc, ns, kv.bj_idx, kv.bj_tab, kv.ivol, (kv.d8 && kv.ivol) ? 1 : 0};
    const StopTest stop{rtol, atol, c->knp_early, min_it, d.d8};
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)ns), b(KNP_BLOCK);
    int rc;
    if ((rc = dist_apply(c, 1, kv.x, kv.coef, kv.w))) return rc;
    const bool first_form = bi_first_form();
    if (first_form) hipLaunchKernelGGL((k_bi_init<NV, false>), g, b, 0, c->stream, d, kv.b, kv.w, kv.r, kv.rhat, kv.p, kv.v, c->partial);
    else hipLaunchKernelGGL((k_bi_init<NV, true>), g, b, 0, c->stream, d, kv.b, kv.w, kv.r, kv.rhat, kv.p, kv.v, c->partial);
    if ((rc = finalize(c, OP_BI_INIT, ns, 3, stop))) return rc;
    int hs[2 * KNP_MAX_SYS] = {0};
    auto all_done = [&]() { for (int s = 0; s < ns; ++s) if (!hs[2 * s]) return false; return true; };
    if (!skip_first_look(c->last_it_knp, maxit) && (rc = poll_status(c, ns, hs))) return rc;
    int it = 0;
    while (!all_done() && it < maxit) {
        const int chunk = next_chunk(it, maxit, check_every, c->last_it_knp);
        for (int k = 0; k < chunk; ++k) {
            if (first_form && it + k == 0)
                hipLaunchKernelGGL((k_bi_p<NV, true>), g, b, 0, c->stream, d, c->scal, c->status, kv.r, kv.v, kv.binv, kv.p, kv.y);
            else
                hipLaunchKernelGGL((k_bi_p<NV, false>), g, b, 0, c->stream, d, c->scal, c->status, kv.r, kv.v, kv.binv, kv.p, kv.y);
            if ((rc = knp_precondition<NV>(c, d, kv, kv.p, kv.y))) return rc;
            if ((rc = dist_apply(c, 1, kv.y, kv.coef, kv.v))) return rc;
            hipLaunchKernelGGL(k_dot2<NV>, g, b, 0, c->stream, d, kv.rhat, kv.v, (const double*)nullptr, (const double*)nullptr,
                               c->partial, c->status);
            if ((rc = finalize(c, OP_BI_ALPHA, ns, 1, stop))) return rc;
            hipLaunchKernelGGL(k_bi_s<NV>, g, b, 0, c->stream, d, c->scal, c->status, kv.v, kv.binv, kv.r, kv.z);
            if ((rc = knp_precondition<NV>(c, d, kv, kv.r, kv.z))) return rc;
            if ((rc = dist_apply(c, 1, kv.z, kv.coef, kv.w))) return rc;
            hipLaunchKernelGGL(k_dot2<NV>, g, b, 0, c->stream, d, kv.w, kv.r, kv.w, kv.w, c->partial, c->status);
            if ((rc = finalize(c, OP_BI_OMEGA, ns, 2, stop))) return rc;
            hipLaunchKernelGGL(k_bi_x<NV>, g, b, 0, c->stream, d, c->scal, c->status, kv.y, kv.z, kv.w, kv.rhat, kv.x, kv.r,
                               c->partial);
            if ((rc = finalize(c, OP_BI_RHO, ns, 2, stop))) return rc;
        }
        it += chunk;
        if ((rc = poll_status(c, ns, hs))) return rc;
    }
    return knp_solve_epilogue(c, ns, hs, niter, res, "BiCGStab");
}

// ---- restarted GMRES (right preconditioning) ------------------------------------------------------------------------------------
// The reference solves the KNP system with PETSc GMRES(30) + BoomerAMG (solver.py:684-701, 767-771).  Same preconditioner and same
// stopping test on the true residual as bicgstab_solve; classical Gram-Schmidt with up to eight inner products per pass over w; the
// preconditioned basis Z = M^-1 V is kept (flexible-GMRES storage), so a cycle ends with x += Z y and no extra preconditioner call.
// Systems (species) run in lockstep; a system whose cycle is complete (status 4) idles until the others are, then all of them
// update x, look at their true residual and either stop or start the next cycle from it.

// y = Binv v
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_binv(VecDims d, const int* __restrict__ status, const bjreal* __restrict__ binv,
                                                       const double* __restrict__ v, double* __restrict__ y) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double vv[NV], yv[NV];
    ldv<NV>(SYS_PTR(v, s), c, vv);
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, vv, yv);
    stv<NV>(SYS_PTR(y, s), c, yv);
}

// v *= scal[slot] (the normalisation of the newest basis vector) ; y = Binv v : one pass instead of two
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_scale_binv(VecDims d, const int* __restrict__ status, const double* __restrict__ scal, int slot,
                                                             const bjreal* __restrict__ binv, double* __restrict__ v, double* __restrict__ y) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const double a = scal_row(scal, s)[slot];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double vv[NV], yv[NV];
    ldv<NV>(SYS_PTR(v, s), c, vv);
#pragma unroll
    for (int a_ = 0; a_ < NV; ++a_) vv[a_] *= a;
    block_matvec<NV>(bj_block<NV>(d, binv, s, c), 0, vv, yv);
    stv<NV>(SYS_PTR(v, s), c, vv);
    stv<NV>(SYS_PTR(y, s), c, yv);
}

// partial[r] = w . V_{j0 + r}, r < cnt <= 8 (the rest zero)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_dots(VecDims d, const int* __restrict__ status, const double* __restrict__ w,
                                                       const double* __restrict__ V, int64_t vstride, int j0, int cnt,
                                                       double* __restrict__ partial) {
    const int s = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (!status[2 * s] && c < d.nc_owned) {
        double wv[NV], vv[NV];
        ldv<NV>(SYS_PTR(w, s), c, wv);
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r < cnt) {
                ldv<NV>(SYS_PTR(V + (int64_t)(j0 + r) * vstride, s), c, vv);
                double t = 0.0;
#pragma unroll
                for (int a = 0; a < NV; ++a) t += wv[a] * vv[a];
                acc[r] = t;
            }
    }
    write_partials<8>(partial, d.nsys, acc);
}

// w -= sum_{i <= j} H[i, j] V_i ;  partial[0] = ||w||^2
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_update(VecDims d, const int* __restrict__ status, const double* __restrict__ scal,
                                                         double* __restrict__ w, const double* __restrict__ V, int64_t vstride, int j, int jlo,
                                                         double* __restrict__ partial) {
    const int s = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[1] = {0.0};
    if (!status[2 * s] && c < d.nc_owned) {
        const double* h = &GmState(scal_gm(scal, s)).H(0, j);
        double wv[NV], vv[NV];
        ldv<NV>(SYS_PTR(w, s), c, wv);
        for (int i = jlo; i <= j; ++i) {
            const double hi = h[i];
            ldv<NV>(SYS_PTR(V + (int64_t)i * vstride, s), c, vv);
#pragma unroll
            for (int a = 0; a < NV; ++a) wv[a] -= hi * vv[a];
        }
#pragma unroll
        for (int a = 0; a < NV; ++a) acc[0] += wv[a] * wv[a];
        stv<NV>(SYS_PTR(w, s), c, wv);
    }
    write_partials<1>(partial, d.nsys, acc);
}

// u += sum_{i < k} y_i Z_i  (k = the system's column count; u = x, Z_i = M^-1 V_i)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_lincomb(VecDims d, const int* __restrict__ status, const double* __restrict__ scal,
                                                          const double* __restrict__ V, int64_t vstride, double* __restrict__ u) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    const int k = (int)scal_row(scal, s)[KS_GM_K];
    const double* y = GmState(scal_gm(scal, s)).y();
    double uv[NV], vv[NV];
    ldv<NV>(SYS_PTR(u, s), c, uv);
    for (int i = 0; i < k; ++i) {
        const double yi = y[i];
        ldv<NV>(SYS_PTR(V + (int64_t)i * vstride, s), c, vv);
#pragma unroll
        for (int a = 0; a < NV; ++a) uv[a] += yi * vv[a];
    }
    stv<NV>(SYS_PTR(u, s), c, uv);
}

// x += z
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_gm_xpy(VecDims d, const int* __restrict__ status, const double* __restrict__ z,
                                                      double* __restrict__ x) {
    const int s = blockIdx.y;
    if (status[2 * s]) return;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (c >= d.nc_owned) return;
    double zv[NV], xv[NV];
    ldv<NV>(SYS_PTR(z, s), c, zv);
    ldv<NV>(SYS_PTR(x, s), c, xv);
#pragma unroll
    for (int a = 0; a < NV; ++a) xv[a] += zv[a];
    stv<NV>(SYS_PTR(x, s), c, xv);
}

template <int NV>
static int gmres_impl(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every, int* niter, double* res) {
    const int ns = c->p.n_sys, m = kv.gm_m;
    VecDims d{c->m.nc_owned, c->m.nc, ns, kv.bj_idx, kv.bj_tab, kv.ivol, (kv.d8 && kv.ivol) ? 1 : 0};
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)ns), b(KNP_BLOCK);
    const int64_t vstride = (int64_t)ns * c->m.nc * NV;
    double* V = kv.gm_V;
    double* Z = kv.gm_V + (int64_t)(m + 1) * vstride;      // Z_j = M^-1 V_j, kept (flexible-GMRES storage): the update x += Z y needs no further preconditioner application
    const StopTest stop{rtol, atol, 0.0, min_it, d.d8};
    int rc;
    static const int trunc = env_int("KNP_GMRES_TRUNC", 0);
    // out = M^-1 in (knp_precondition behind this method's own block-Jacobi pass)
    // slot >= 0: `in` is the newest, still unnormalised basis vector; it is scaled by scal[slot] in the same pass
    auto precond = [&](double* in, double* out, int slot) -> int {
        if (slot >= 0) hipLaunchKernelGGL(k_gm_scale_binv<NV>, g, b, 0, c->stream, d, (const int*)c->status, (const double*)c->scal, slot, kv.binv, in, out);
        else hipLaunchKernelGGL(k_gm_binv<NV>, g, b, 0, c->stream, d, (const int*)c->status, kv.binv, (const double*)in, out);
        return knp_precondition<NV>(c, d, kv, in, out);
    };
    // r = b - A x into V_0 (unnormalised), norms of the true residual -> convergence test / next cycle
    auto residual = [&](int op) -> int {
        int r;
        if ((r = dist_apply(c, 1, kv.x, kv.coef, kv.w))) return r;
        hipLaunchKernelGGL(k_bi_init<NV>, g, b, 0, c->stream, d, kv.b, kv.w, V, kv.rhat, kv.p, kv.v, c->partial);
        return finalize(c, op, ns, 3, stop);
    };
    if ((rc = residual(OP_GM_INIT))) return rc;
    int hs[2 * KNP_MAX_SYS] = {0};
    auto any_running = [&]() { for (int s = 0; s < ns; ++s) if (hs[2 * s] == KS_RUNNING) return true; return false; };
    auto all_done = [&]() { for (int s = 0; s < ns; ++s) if (hs[2 * s] == KS_RUNNING || hs[2 * s] == KS_CYCLE_DONE) return false; return true; };
    if (!skip_first_look(c->last_it_knp, maxit) && (rc = poll_status(c, ns, hs))) return rc;
    int it = 0;
    while (!all_done() && it < maxit) {
        // one restart cycle
        int j = 0;
        while (j < m && any_running() && it < maxit) {
            int chunk = next_chunk(it, maxit, check_every, c->last_it_knp);
            if (chunk > m - j) chunk = m - j;
            for (int k = 0; k < chunk; ++k, ++j) {
                double* w = V + (int64_t)(j + 1) * vstride;
                double* zj = Z + (int64_t)j * vstride;
                if ((rc = precond(V + (int64_t)j * vstride, zj, j == 0 ? (int)KS_ALPHA : (int)KS_OMEGA))) return rc;
                if ((rc = dist_apply(c, 1, zj, kv.coef, w))) return rc;
                // KNP_GMRES_TRUNC = t > 0: incomplete orthogonalisation against the last t basis vectors only (IOM / quasi-minimal
                // residual: the cycle's estimate is then a quasi-residual, the true residual at the cycle's end still decides)
                const int jlo = trunc > 0 ? std::max(0, j + 1 - trunc) : 0;
                for (int j0 = jlo; j0 <= j; j0 += 8) {
                    const int cnt = std::min(8, j + 1 - j0);
                    hipLaunchKernelGGL(k_gm_dots<NV>, g, b, 0, c->stream, d, (const int*)c->status, (const double*)w, (const double*)V, vstride, j0,
                                       cnt, c->partial);
                    if ((rc = finalize(c, OP_GM_H, ns, 8, stop, gm_aux_pack(j0, j, cnt)))) return rc;
                }
                hipLaunchKernelGGL(k_gm_update<NV>, g, b, 0, c->stream, d, (const int*)c->status, (const double*)c->scal, w, (const double*)V,
                                   vstride, j, jlo, c->partial);
                if ((rc = finalize(c, OP_GM_NORM, ns, 1, stop, gm_aux_pack(j, m, jlo)))) return rc;
            }
            it += chunk;
            if ((rc = poll_status(c, ns, hs))) return rc;
        }
        // x += M^-1 (V y) for every system that iterated in this cycle; then its true residual decides
        hipLaunchKernelGGL(k_scalar_op, dim3(1), dim3(64), 0, c->stream, (int)OP_GM_SOLVE, ns, (const double*)krylov_red(c), c->scal, c->status,
                           stop, 0);
        hipLaunchKernelGGL(k_gm_lincomb<NV>, g, b, 0, c->stream, d, (const int*)c->status, (const double*)c->scal, (const double*)Z, vstride, kv.x);
        if ((rc = residual(OP_GM_RESTART))) return rc;
        if ((rc = poll_status(c, ns, hs))) return rc;
    }
    return knp_solve_epilogue(c, ns, hs, niter, res, "GMRES");
}

int gmres_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every, int* niter, double* res) {
    if (check_every < 1) check_every = 1;
    if (!kv.gm_V || kv.gm_m < 2 || kv.gm_m > KNP_GM_MAX) { c->err = "gmres: no basis storage"; return -1; }
    return dispatch_nd(c, "gmres: unsupported dofs per cell",
                       [&](auto nv) { return gmres_impl<decltype(nv)::value>(c, kv, rtol, atol, maxit, min_it, check_every, niter, res); });
}

// partial sums of the load measure the stopping tests use (residual_measure: (|b_K| / vol_K)^8, or |b_K|^2 / vol_K without d8)
template <int NV>
__global__ __launch_bounds__(KNP_BLOCK) void k_load_measure(VecDims d, const double* __restrict__ b, double* __restrict__ partial) {
    const int s = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    double acc[1] = {0.0};
    if (c < d.nc_owned) {
        double bv[NV], bb = 0.0;
        ldv<NV>(SYS_PTR(b, s), c, bv);
#pragma unroll
        for (int a = 0; a < NV; ++a) bb += bv[a] * bv[a];
        acc[0] = residual_measure(d, c, bb);
    }
    write_partials<1>(partial, d.nsys, acc);
}

// out[s] = sum over this rank's owned cells of the load measure of species s' right-hand side b [nsys][nc][nd] (NOT all-reduced: the caller
// sums over the ranks and takes the 8th / square root)
int load_measure(knp_ctx* c, const double* b, const float* ivol, bool d8, double* out) {
    const int ns = c->p.n_sys;
    VecDims d{c->m.nc_owned, c->m.nc, ns, nullptr, nullptr, ivol, (d8 && ivol) ? 1 : 0};
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)ns), blk(KNP_BLOCK);
    const int rc = dispatch_nd(c, "load_measure: unsupported dofs per cell", [&](auto nv) {
        hipLaunchKernelGGL(k_load_measure<decltype(nv)::value>, g, blk, 0, c->stream, d, b, c->partial);
        return 0;
    });
    if (rc) return rc;
    // second stage without the all-reduce and without a scalar recurrence behind it
    const int64_t nb = grid_for(c->m.nc_owned);
    double* red = krylov_red(c);
    hipLaunchKernelGGL((k_reduce<1, 8>), dim3(ns), dim3(KNP_REDUCE_BLOCK), 0, c->stream, c->partial, nb, ns, red, 0, c->scal, c->status, StopTest{}, 0);
    HIPCHK(c, hipGetLastError());
    double h[KNP_MAX_SYS * KNP_MAX_RED];
    HIPCHK(c, hipMemcpyAsync(h, red, sizeof(double) * (size_t)ns * KNP_MAX_RED, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    for (int s = 0; s < ns; ++s) out[s] = h[s * KNP_MAX_RED];
    return 0;
}

int bicgstab_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every, int* niter,
                   double* res) {
    if (check_every < 1) check_every = 1;
    return dispatch_nd(c, "bicgstab: unsupported dofs per cell",
                       [&](auto nv) { return bicgstab_impl<decltype(nv)::value>(c, kv, rtol, atol, maxit, min_it, check_every, niter, res); });
}
