// The hierarchy of the auxiliary-space preconditioner on the device: uploads (knp_amg_begin: transfer tables, knp_amg_level: one CSR
// level, knp_amg_finish: the coarsest level's dense pseudo-inverse), their range checks, and the release of it all.  The setup itself
// is host work (knpemidg/amg.py); the transfer tables are built by amg_tables.hpp.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "amg.hpp"
#include "amg_tables.hpp"

namespace {

template <typename T> int up(knp_ctx* c, T** dst, const T* src, size_t n) {
    HIPCHK(c, hipMalloc((void**)dst, (n ? n : 1) * sizeof(T)));
    if (n) HIPCHK(c, host_memcpy(c, *dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

int up_csr(knp_ctx* c, CsrDev& M, int64_t nrows, int64_t ncols, const int32_t* rp, const int32_t* ci, const double* v) {
    M.nrows = nrows; M.ncols = ncols; M.nnz = rp[nrows];
    int rc = up(c, &M.rowptr, rp, (size_t)nrows + 1);
    rc |= up(c, &M.col, ci, (size_t)M.nnz);
    std::vector<float> v32((size_t)M.nnz);
    for (size_t i = 0; i < v32.size(); ++i) v32[i] = (float)v[i];
    rc |= up(c, &M.val, v32.data(), v32.size());
    return rc;
}

// (the tile tables are read-only on the device: their record holds const pointers)
template <typename T> int up_const(knp_ctx* c, const T** dst, const std::vector<T>& src) {
    T* p = nullptr;
    const int rc = up(c, &p, src.data(), src.size());
    *dst = p;
    return rc;
}
template <typename T> void free_const(const T* p) { hipFree(const_cast<T*>(p)); }

void free_csr(CsrDev& M) { hipFree(M.rowptr); hipFree(M.col); hipFree(M.val); M = CsrDev(); }

AmgHierarchy* amg_slot(knp_ctx* c, int which) {
    if (which < 0 || which >= (int)c->amg.size()) return nullptr;
    return &c->amg[which];
}

}  // namespace

void amg_free(AmgHierarchy& H) {
    for (auto& L : H.levels) {
        free_csr(L.A); free_csr(L.P); free_csr(L.R);
        hipFree(L.dinv); hipFree(L.x); hipFree(L.b); hipFree(L.r); hipFree(L.d0); hipFree(L.d1);
    }
    if (H.graph_exec) hipGraphExecDestroy(H.graph_exec);
    hipFree(H.pinv); hipFree(H.dg2cg); hipFree(H.cg_ptr); hipFree(H.cg_idx); hipFree(H.t0); hipFree(H.part);
    free_const(H.tiles.tile_off); free_const(H.tiles.slot_ptr); free_const(H.tiles.slot_idx);
    free_const(H.tiles.part_ptr); free_const(H.tiles.part_idx);
    H = AmgHierarchy();
}

extern "C" {

// cg_ptr / cg_idx = null: the inverse map (conforming dof -> the OWNED DG dofs that inject into it, ascending) is derived here
// (amg_tables.hpp: cg_inverse)
int knp_amg_begin(knp_ctx* c, int which, int64_t ncg, const int32_t* dg2cg, const int32_t* cg_ptr, const int32_t* cg_idx) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H) { c->err = "amg: bad slot"; return -1; }
    amg_free(*H);
    const int64_t ndof = c->m.nc * c->nd;                    // dg2cg: conforming dof of every DG dof (injection)
    for (int64_t i = 0; i < ndof; ++i)
        if (dg2cg[i] < 0 || dg2cg[i] >= ncg) { c->err = "amg: dg2cg out of range"; return -1; }
    CgInverse own;
    if (!cg_ptr || !cg_idx) {
        own = cg_inverse(dg2cg, c->m.nc_owned, c->nd, ncg);
        cg_ptr = own.ptr.data();
        cg_idx = own.idx.data();
    }
    if (cg_ptr[ncg] > ndof) { c->err = "amg: cg_ptr inconsistent"; return -1; }
    for (int64_t k = 0; k < cg_ptr[ncg]; ++k)
        if (cg_idx[k] < 0 || cg_idx[k] >= ndof) { c->err = "amg: cg_idx out of range"; return -1; }
    // tables of the tile-wise restriction over the owned cells; none where a tile does not fit (tiles_usable): the gather form runs
    static const int tile_env = env_int("KNP_RESTRICT_TILE", 0);
    const int tile_cells = tile_env > 0 ? tile_env : (c->nd <= 4 ? 512 : 256);   // 16 KB / 20 KB of LDS per workgroup (r=2: 512 -> 10.55, 1024 -> 10.71, 256 -> 10.69 ms/step)
    const TileTablesHost T = restrict_tile_tables(dg2cg, c->m.nc_owned, c->nd, ncg, tile_cells);
    H->ncg = ncg;
    int rc = up(c, &H->dg2cg, dg2cg, (size_t)ndof);
    rc |= up(c, &H->cg_ptr, cg_ptr, (size_t)ncg + 1);
    rc |= up(c, &H->cg_idx, cg_idx, (size_t)cg_ptr[ncg]);
    if (T.ntiles > 0) {
        TileTables& D = H->tiles;
        rc |= up_const(c, &D.tile_off, T.tile_off);
        rc |= up_const(c, &D.slot_ptr, T.slot_ptr);
        rc |= up_const(c, &D.slot_idx, T.slot_idx);
        rc |= up_const(c, &D.part_ptr, T.part_ptr);
        rc |= up_const(c, &D.part_idx, T.part_idx);
        D.tile_cells = T.tile_cells; D.ntiles = T.ntiles; D.nslots = T.nslots;
    }
    return rc;
}

int knp_amg_level(knp_ctx* c, int which, int64_t n, const int32_t* rpA, const int32_t* ciA, const double* vA, const double* dinv,
                  double rho, int cheb_degree, double cheb_lower, int64_t ncoarse, const int32_t* rpP, const int32_t* ciP,
                  const double* vP, const int32_t* rpR, const int32_t* ciR, const double* vR) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H) { c->err = "amg: bad slot"; return -1; }
    if (H->levels.empty() ? (n != H->ncg) : (n != H->levels.back().ncoarse)) { c->err = "amg: level size mismatch"; return -1; }
    for (int64_t k = 0; k < rpA[n]; ++k)
        if (ciA[k] < 0 || ciA[k] >= n) { c->err = "amg: A column out of range"; return -1; }
    AmgLevel L;
    L.n = n; L.ncoarse = ncoarse; L.rho = rho; L.cheb_degree = cheb_degree; L.cheb_lower = cheb_lower;
    int rc = up_csr(c, L.A, n, n, rpA, ciA, vA);
    rc |= up(c, &L.dinv, dinv, (size_t)n);
    if (ncoarse > 0) {
        for (int64_t k = 0; k < rpP[n]; ++k)
            if (ciP[k] < 0 || ciP[k] >= ncoarse) { c->err = "amg: P column out of range"; return -1; }
        for (int64_t k = 0; k < rpR[ncoarse]; ++k)
            if (ciR[k] < 0 || ciR[k] >= n) { c->err = "amg: R column out of range"; return -1; }
        rc |= up_csr(c, L.P, n, ncoarse, rpP, ciP, vP);
        rc |= up_csr(c, L.R, ncoarse, n, rpR, ciR, vR);
    }
    double** w[] = {&L.x, &L.b, &L.r, &L.d0, &L.d1};
    const size_t nbuf = (size_t)(n ? n : 1) * (size_t)H->ncol;          // [ncol / nil][n][nil], nil = 2 interleaved columns when ncol is even
    for (auto p : w) {
        if (hipMalloc((void**)p, nbuf * sizeof(double)) != hipSuccess) rc = -2;
        else hipMemset(*p, 0, nbuf * sizeof(double));
    }
    H->levels.push_back(L);
    return rc;
}

static int amg_finish_impl(knp_ctx* c, int which, int64_t n, const double* pinv64, const float* pinv32) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H || H->levels.empty() || H->levels.back().n != n || H->levels.back().ncoarse != 0) {
        c->err = "amg: finish does not match the last level"; return -1;
    }
    if (!pinv64 && !pinv32) { c->err = "amg: finish without a coarse inverse"; return -1; }
    int rc;
    if (pinv32) rc = up(c, &H->pinv, pinv32, (size_t)n * n);
    else {
        std::vector<float> p32((size_t)n * n);
        for (size_t i = 0; i < p32.size(); ++i) p32[i] = (float)pinv64[i];
        rc = up(c, &H->pinv, p32.data(), p32.size());
    }
    const bool fuse_env = env_flag("KNP_FUSE_FIRST0", true);   // read per upload: tests switch it
    H->fuse_first0 = fuse_env && !c->dist && H->tiles.usable() && H->levels.size() > 1 && H->levels[0].cheb_degree > 0;
    H->ready = (rc == 0);
    return rc;
}

int knp_amg_finish(knp_ctx* c, int which, int64_t n, const double* pinv) { return amg_finish_impl(c, which, n, pinv, nullptr); }
// the same with the inverse already rounded to fp32 (the device stores it in fp32 either way)
int knp_amg_finish_f32(knp_ctx* c, int which, int64_t n, const float* pinv) { return amg_finish_impl(c, which, n, nullptr, pinv); }

// Marks hierarchy `which` as carrying a ROW-DISTRIBUTED level 0 (between knp_amg_begin and the first knp_amg_level): ncg, dg2cg and the
// level-0 matrices are this rank's rows in local numbering, A this rank's share of the global matrix (knp_amg_interface first).
int knp_amg_dist0(knp_ctx* c, int which) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H || !H->levels.empty()) { c->err = "amg: dist0 must be set after begin and before the first level"; return -1; }
    if (!c->dist) { c->err = "amg: a distributed level 0 needs a communicator"; return -1; }
    H->dist0 = true;
    return 0;
}

int knp_amg_columns(knp_ctx* c, int which, int ncol) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H || !H->levels.empty()) { c->err = "amg: columns must be set after begin and before the first level"; return -1; }
    if (ncol < 1 || ncol > KNP_MAX_SYS || (which == 0 && ncol != 1)) { c->err = "amg: bad column count"; return -1; }
    H->ncol = ncol;
    return 0;
}

int knp_amg_clear(knp_ctx* c, int which) {
    if (!c) return -1;
    AmgHierarchy* H = amg_slot(c, which);
    if (!H) return -1;
    amg_free(*H);
    return 0;
}

}  // extern "C"
