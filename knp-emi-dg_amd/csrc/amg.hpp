// CSR levels of the auxiliary-space AMG hierarchy (device pointers).
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>
#include <vector>

struct CsrDev {
    int64_t nrows = 0, ncols = 0, nnz = 0;
    int32_t* rowptr = nullptr;
    int32_t* col = nullptr;
    float* val = nullptr;          // fp32 storage (preconditioner data; symmetric entries round identically), fp64 arithmetic
};

struct AmgLevel {
    int64_t n = 0, ncoarse = 0;
    CsrDev A, P, R;
    double* dinv = nullptr;
    double rho = 1.0, cheb_lower = 0.1;
    int cheb_degree = 3;
    double *x = nullptr, *b = nullptr, *r = nullptr, *d0 = nullptr, *d1 = nullptr;
};

// The column count of a hierarchy as the launches need it: level vectors carry the columns INTERLEAVED in pairs when their number is
// even ([ncol / nil][n][nil]; amg_vcycle.hip: row_dot), and the row kernels then take grid.y = ncol / nil column groups.
struct AmgCols {
    int ncol, nil;                  // right-hand-side columns; interleave width (2 for an even count, else 1)
    unsigned groups;                // column groups = grid.y of the kernels that work on interleaved rows
    explicit AmgCols(int n) : ncol(n), nil(n % 2 == 0 ? 2 : 1), groups((unsigned)(n / (n % 2 == 0 ? 2 : 1))) {}
    dim3 per_column(int64_t nx) const { return dim3((unsigned)nx, (unsigned)ncol); }   // grid of the kernels that take one column each
};

// Chebyshev polynomial smoother of D^-1 A on [cheb_lower * rho, rho]: the interval's constants and the running rho of the three-term
// recurrence.  The first update is d = dinv r / theta; next() yields (c1, c2) of every further one, d <- c1 d + c2 dinv r.  (The
// DG-level two-step form of krylov.hip, bj_cheb2, is a closed form of its own.)
struct Cheb {
    double theta, delta, sigma, rho;
    // the centre of the interval alone: 1 / theta scales a level's first update (also where no recurrence follows)
    static double theta_of(const AmgLevel& L) { return 0.5 * (L.rho + L.cheb_lower * L.rho); }
    explicit Cheb(const AmgLevel& L) {
        const double lmax = L.rho, lmin = L.cheb_lower * L.rho;
        theta = theta_of(L);
        delta = 0.5 * (lmax - lmin);
        sigma = theta / delta;
        rho = 1.0 / sigma;
    }
    struct Step { double c1, c2; };
    Step next() {
        const double rho_new = 1.0 / (2.0 * sigma - rho);
        const Step s{rho_new * rho, 2.0 * rho_new / delta};
        rho = rho_new;
        return s;
    }
};

// Tables of the tile-wise restriction on the device (amg_tables.hpp builds them, amg_restrict.hip: k_restrict_tiles / k_restrict_sum and
// the fused kernels of krylov.hip read them; passed to kernels by value, like CsrDev): every tile of consecutive owned cells sums, per
// conforming dof it touches (a "slot"), the tile's DG values out of LDS; the slots of one conforming dof are then added in fixed order.
struct TileTables {
    int tile_cells = 0;
    int64_t ntiles = 0, nslots = 0;
    const int32_t* tile_off = nullptr;      // [ntiles + 1] first slot of every tile
    const int32_t* slot_ptr = nullptr;      // [nslots + 1] CSR over slot_idx
    const uint16_t* slot_idx = nullptr;     // [nc_owned * nd] tile-local DG dof index, grouped by slot
    const int32_t *part_ptr = nullptr, *part_idx = nullptr;   // CSR: conforming dof -> its slots
    // decided once, where the tables are built (amg_tables.hpp: tiles_usable): a tile's values fit the dynamic LDS of a workgroup
    bool usable() const { return ntiles > 0; }
};

struct AmgHierarchy {
    bool ready = false;
    int ncol = 1;                   // right-hand-side columns carried by one V-cycle (level vectors are [ncol / nil][n][nil])
    AmgCols cols() const { return AmgCols(ncol); }
    int64_t ncg = 0;
    int32_t* dg2cg = nullptr;       // [nc*nd] conforming dof of every DG dof
    int32_t *cg_ptr = nullptr, *cg_idx = nullptr;   // CSR list: conforming dof -> DG dofs (owned cells only)
    TileTables tiles;
    double* part = nullptr;         // [ncol][nslots] per-tile partial sums
    int part_cols = 0;
    std::vector<AmgLevel> levels;
    float* pinv = nullptr;          // dense pseudo-inverse of the coarsest level (fp32 storage)
    // Partitioned runs: level 0 holds THIS RANK'S rows only (the conforming dofs of its owned cells + of the membrane facets assigned to it,
    // local numbering), its matrix this rank's share of the global one (the shares add up to it, also as fp32 values: every entry is on
    // one rank -- amg.py: Dist0Space.split_matrix): products are per-rank partial sums, made consistent at the
    // shared dofs by interface_accumulate (comm.hip); levels >= 1 stay replicated behind one all-reduce of the level-1 residual
    bool dist0 = false;
    double* t0 = nullptr;           // [ncol][n_0] work vector of the distributed level
    hipGraphExec_t graph_exec = nullptr;   // one V-cycle (fixed kernel sequence on fixed buffers; dist0: levels >= 1)
    bool graph_tried = false;
    // Level 0's zero-guess first Chebyshev update comes with stage 2 of the tile-wise restriction (k_restrict_sum) instead of a launch
    // of its own: one process, tile tables, a smoothed level 0 with a coarser level below.  The V-cycle swaps level buffers while it runs
    // (and a captured graph keeps the pointers of its capture), so the restriction writes where THIS V-cycle will read: entry_* = the
    // level-0 buffers at the start of the captured V-cycle (eager V-cycles start from the current ones)
    bool fuse_first0 = false;
    double *entry_x = nullptr, *entry_r = nullptr, *entry_d0 = nullptr;
};

#ifdef __HIPCC__
// Stage 1 of the tile-wise restriction, behind the barrier that completes the tile's values in LDS (s_r): thread by thread, every slot of
// tile blockIdx.x (256 threads) sums its entries in the order of slot_idx.  Shared by amg_restrict.hip: k_restrict_tiles and the fused kernels of
// krylov.hip (k_cg_update_restrict, k_bj_cheb2_restrict).  The summation order is a CONTRACT between them: the fused paths are tested
// bit for bit against the unfused ones, so all three go through this one loop.
__device__ __forceinline__ void tile_slot_sums(const double* s_r, const int32_t* __restrict__ tile_off, const int32_t* __restrict__ slot_ptr,
                                               const uint16_t* __restrict__ slot_idx, double* __restrict__ part) {
    const int p1 = tile_off[blockIdx.x + 1];
    for (int p = tile_off[blockIdx.x] + threadIdx.x; p < p1; p += 256) {
        double acc = 0.0;
        const int e = slot_ptr[p + 1];
        for (int k = slot_ptr[p]; k < e; ++k) acc += s_r[slot_idx[k]];
        part[p] = acc;
    }
}
#endif

struct knp_ctx;
// amg_vcycle.hip
int amg_vcycle(knp_ctx* c, AmgHierarchy& H, hipStream_t on_stream = nullptr);
// y = A x on the columns of H, on stream st (the density-dispatched k_csr: the restriction's tail applies level 0's R with it)
void amg_csr_apply(const AmgHierarchy& H, const CsrDev& A, const double* x, double* y, hipStream_t st);
// amg_restrict.hip
// stage 1 of the tile-wise restriction may be done by a fused kernel of krylov.hip: buffer first, the remaining stages afterwards
int amg_restrict_tiles_prepare(knp_ctx* c, AmgHierarchy& H);
int amg_restrict_finish(knp_ctx* c, AmgHierarchy& H, hipStream_t on_stream = nullptr);
// restricts r_dg, or r_dg - ct * t_dg when t_dg is given
int amg_restrict_from_dg(knp_ctx* c, AmgHierarchy& H, const double* r_dg, hipStream_t on_stream = nullptr, int64_t r_stride = 0,
                         const double* t_dg = nullptr, double ct = 0.0);
// amg_upload.hip
void amg_free(AmgHierarchy& H);
