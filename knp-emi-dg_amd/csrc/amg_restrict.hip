// DG -> conforming-P1 restriction of the auxiliary-space preconditioner (gather forms, deterministic): tile-wise in two stages where the
// hierarchy has tile tables (amg_tables.hpp; stage 1 may instead be done by a fused kernel of krylov.hip), else one gather per conforming
// dof; behind either the tail: a transfer-only level 0 goes down to level 1 at once, a partitioned run all-reduces.  The way back
// (k_prolong_*) is fused with the Krylov dot products and lives in krylov.hip.
#include "knpemi_internal.hpp"
#include "amg.hpp"

namespace {

// rc[v] = sum over the DG dofs mapped to conforming dof v (CSR list, fixed order -> deterministic)
// G lanes per conforming dof (a vertex is shared by ~24 tets); fixed summation tree -> deterministic
template <int G>
__global__ __launch_bounds__(256) void k_dg_restrict(int64_t ncg, const int32_t* __restrict__ ptr, const int32_t* __restrict__ idx,
                                                     const double* __restrict__ r, double* __restrict__ rc, int64_t r_stride, int nil,
                                                     const double* __restrict__ t, double ct) {
    r += (int64_t)blockIdx.y * r_stride;
    if (t) t += (int64_t)blockIdx.y * r_stride;
    rc += (int64_t)(blockIdx.y / nil) * nil * ncg + (blockIdx.y % nil);          // column blockIdx.y of the interleaved level vector
    const int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    double s = 0.0;
    if (v < ncg) {
        const int e = ptr[v + 1];
        for (int k = ptr[v] + lane; k < e; k += G) s += t ? fma(-ct, t[idx[k]], r[idx[k]]) : r[idx[k]];
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) s += __shfl_down(s, off, G);
    if (v < ncg && lane == 0) rc[v * nil] = s;
}

// Tile-wise restriction, stage 1: the tile's DG values (consecutive cells: one coalesced read of r) go to LDS; every slot (= one
// conforming dof touched by the tile) is summed by one thread in a fixed order.  The gather form above reads 8 bytes out of every
// 32-byte cell record four times over (once per vertex): 38 us at r=2 against 64 MB of input.
__global__ __launch_bounds__(256) void k_restrict_tiles(int64_t ndof_owned, int tile_dofs, TileTables T, const double* __restrict__ r,
                                                        int64_t r_stride, double* __restrict__ part, const double* __restrict__ t, double ct) {
    // t != null: the restricted vector is r - ct t (the residual left by the first step of the DG-level Chebyshev smoother, whose
    // operator product t = A Binv r exists anyway: krylov.hip, hybrid two-level preconditioner)
    extern __shared__ double s_r[];
    r += (int64_t)blockIdx.y * r_stride;
    if (t) t += (int64_t)blockIdx.y * r_stride;
    part += (int64_t)blockIdx.y * T.nslots;
    const int64_t d0 = (int64_t)blockIdx.x * tile_dofs;
    const int n = (int)((ndof_owned - d0 < tile_dofs) ? (ndof_owned - d0) : tile_dofs);
    const double* src = r + d0;
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {                        // 16-byte aligned column: pairs (tile_dofs is even)
        const double2* src2 = reinterpret_cast<const double2*>(src);
        if (t) {
            const double2* t2 = reinterpret_cast<const double2*>(t + d0);
            for (int i = threadIdx.x; 2 * i + 1 < n; i += 256) {
                const double2 v = src2[i], w = t2[i];
                s_r[2 * i] = fma(-ct, w.x, v.x);
                s_r[2 * i + 1] = fma(-ct, w.y, v.y);
            }
            if ((n & 1) && threadIdx.x == 0) s_r[n - 1] = fma(-ct, t[d0 + n - 1], src[n - 1]);
        } else {
            for (int i = threadIdx.x; 2 * i + 1 < n; i += 256) {
                const double2 v = src2[i];
                s_r[2 * i] = v.x;
                s_r[2 * i + 1] = v.y;
            }
            if ((n & 1) && threadIdx.x == 0) s_r[n - 1] = src[n - 1];
        }
    } else {
        for (int i = threadIdx.x; i < n; i += 256) s_r[i] = t ? fma(-ct, t[d0 + i], src[i]) : src[i];
    }
    __syncthreads();
    tile_slot_sums(s_r, T.tile_off, T.slot_ptr, T.slot_idx, part);
}

// stage 2: rc[v] = sum of the slots of conforming dof v (fixed order); with dinv also the zero-guess first Chebyshev update of level 0
// (r = rc ; d = x = dinv rc / theta: one launch less per V-cycle; AmgHierarchy::fuse_first0)
__global__ __launch_bounds__(256) void k_restrict_sum(int64_t ncg, TileTables T, const double* __restrict__ part, double* __restrict__ rc,
                                                      int nil, const double* __restrict__ dinv, double inv_theta, double* __restrict__ r0,
                                                      double* __restrict__ d0, double* __restrict__ x0) {
    part += (int64_t)blockIdx.y * T.nslots;
    const int64_t o = (int64_t)(blockIdx.y / nil) * nil * ncg + (blockIdx.y % nil);   // column blockIdx.y of the interleaved level vector
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= ncg) return;
    double s = 0.0;
    const int e = T.part_ptr[v + 1];
    for (int k = T.part_ptr[v]; k < e; ++k) s += part[T.part_idx[k]];
    rc[o + v * nil] = s;
    if (dinv) {
        const double w = dinv[v] * s * inv_theta;
        r0[o + v * nil] = s;
        d0[o + v * nil] = w;
        x0[o + v * nil] = w;
    }
}

// Everything behind the restriction onto level 0.  Multi-GPU: the conforming hierarchy is replicated on every rank; the restricted
// residual is the sum of the ranks' owned-cell contributions (one all-reduce), after which every rank runs the same V-cycle.  When the
// finest level is transfer-only (EMI) the restriction to level 1 is linear in b, so it is applied to the LOCAL vector first and the
// all-reduce moves the 6.5x shorter level-1 vector (29 k instead of 188 k doubles at r=2).
int restrict_tail(knp_ctx* c, AmgHierarchy& H, hipStream_t st) {
    if (H.levels.size() > 1 && H.levels[0].cheb_degree == 0) {
        AmgLevel& L = H.levels[0];
        amg_csr_apply(H, L.R, L.b, H.levels[1].b, st);
        if (c->dist) return allreduce_red(c, H.levels[1].b, (int)(H.levels[1].n * H.ncol));
        return 0;
    }
    if (c->dist && !H.dist0) return allreduce_red(c, H.levels[0].b, (int)(H.ncg * H.ncol));
    return 0;                                                       // dist0: b stays the rank's partial sums (amg_vcycle_dist0)
}

}  // namespace

int amg_restrict_from_dg(knp_ctx* c, AmgHierarchy& H, const double* r_dg, hipStream_t on_stream, int64_t r_stride, const double* t_dg,
                         double ct) {
    if (on_stream && c->dist) { c->err = "amg: the all-reduced restriction runs on the context's stream"; return -1; }
    hipStream_t st = on_stream ? on_stream : c->stream;
    if (H.tiles.usable()) {
        const int tile_dofs = H.tiles.tile_cells * c->nd;
        int rc = amg_restrict_tiles_prepare(c, H);
        if (rc) return rc;
        hipLaunchKernelGGL(k_restrict_tiles, dim3((unsigned)H.tiles.ntiles, (unsigned)H.ncol), dim3(256), sizeof(double) * tile_dofs, st,
                           c->m.nc_owned * c->nd, tile_dofs, H.tiles, r_dg, r_stride, H.part, t_dg, ct);
        return amg_restrict_finish(c, H, on_stream);
    }
    const AmgCols cols = H.cols();
    hipLaunchKernelGGL(k_dg_restrict<8>, cols.per_column((H.ncg * 8 + 255) / 256), dim3(256), 0, st, H.ncg, H.cg_ptr, H.cg_idx, r_dg,
                       H.levels[0].b, r_stride, cols.nil, t_dg, ct);
    return restrict_tail(c, H, st);
}

// the per-tile partial sums buffer [ncol][nslots] of the tile-wise restriction, sized at the first use
int amg_restrict_tiles_prepare(knp_ctx* c, AmgHierarchy& H) {
    if (!H.tiles.usable()) return -1;
    if (!H.part || H.part_cols != H.ncol) {
        hipFree(H.part);
        H.part = nullptr;
        HIPCHK(c, hipMalloc((void**)&H.part, sizeof(double) * (size_t)H.ncol * (size_t)(H.tiles.nslots ? H.tiles.nslots : 1)));
        H.part_cols = H.ncol;
    }
    return 0;
}

// everything behind stage 1 of the tile-wise restriction (H.part filled by k_restrict_tiles or by the fused Chebyshev / restriction
// kernel of krylov.hip): stage 2, the transfer-only finest level, the all-reduce of a partitioned run
int amg_restrict_finish(knp_ctx* c, AmgHierarchy& H, hipStream_t on_stream) {
    if (on_stream && c->dist) { c->err = "amg: the all-reduced restriction runs on the context's stream"; return -1; }
    hipStream_t st = on_stream ? on_stream : c->stream;
    const AmgCols cols = H.cols();
    AmgLevel& L0 = H.levels[0];
    const bool fuse = H.fuse_first0;                                // (amg_vcycle_eager then skips level 0's k_cheb_first)
    const bool baked = H.graph_exec != nullptr;                     // the captured V-cycle reads the buffers of its capture
    hipLaunchKernelGGL(k_restrict_sum, cols.per_column((H.ncg + 255) / 256), dim3(256), 0, st, H.ncg, H.tiles, (const double*)H.part, L0.b,
                       cols.nil, fuse ? (const double*)L0.dinv : (const double*)nullptr, 1.0 / Cheb::theta_of(L0), baked ? H.entry_r : L0.r,
                       baked ? H.entry_d0 : L0.d0, baked ? H.entry_x : L0.x);
    return restrict_tail(c, H, st);
}
