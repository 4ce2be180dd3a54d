// Life of a context: knp_ctx_create / knp_ctx_destroy, the coefficient and geometry setters, the debug tables and the field transfers
// (see include/knpemi_hip.h for the contract and the reference interfaces each entry point replaces).
#include "knpemi_internal.hpp"
#include "context_tables.hpp"
#include "krylov.hpp"
#include <chrono>
#include <cstdio>
#include <cstring>

namespace {

thread_local std::string g_err;   // what knp_last_error(null) reports: why knp_ctx_create returned no context

// KNP_DMA_PAD zero bytes follow every table: the ring-staged applies (apply_ring.hip) read whole 256-cell blocks of the per-cell
// tables with 16-byte DMA granules, also where the last block runs past the end of the mesh
#define KNP_DMA_PAD 4096
template <typename T> int dev_alloc_copy(knp_ctx* c, T** dst, const T* src, size_t n) {
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    HIPCHK(c, hipMalloc((void**)dst, bytes + KNP_DMA_PAD));
    HIPCHK(c, hipMemset((char*)*dst + bytes, 0, KNP_DMA_PAD));
    if (src && n) HIPCHK(c, host_memcpy(c, *dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

template <typename T> int dev_zeros(knp_ctx* c, T** dst, size_t n) {
    HIPCHK(c, hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T)));
    HIPCHK(c, hipMemset(*dst, 0, std::max<size_t>(n, 1) * sizeof(T)));
    return 0;
}

}  // namespace

extern "C" {

const char* knp_last_error(knp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// knp_ctx_create gives up on a context that has its stream: everything built so far is released
static int create_failed(knp_ctx* c, int rc, std::string why) {
    g_err = std::move(why);                                                 // a copy: `why` may have been built from c->err
    knp_ctx_destroy(c);
    return rc;
}

static int upload_mesh(knp_ctx* c, const MeshIn& in, const FacetTables& T, const std::vector<double>& hcell) {
    MeshDev& m = c->m;
    std::vector<double> cpad;
    const double* csrc = in.coords;
    size_t cstride = in.dim;
    if (in.dim == 3) {
        cpad.resize(in.nv * 4, 0.0);
        for (int64_t v = 0; v < in.nv; ++v) for (int k = 0; k < 3; ++k) cpad[4 * v + k] = in.coords[3 * v + k];
        csrc = cpad.data();
        cstride = 4;
    }
    int rc = 0;
    rc |= dev_alloc_copy(c, &m.h, hcell.data(), hcell.size());
    rc |= dev_alloc_copy(c, &m.coords, csrc, (size_t)in.nv * cstride);
    rc |= dev_alloc_copy(c, &m.cells, in.cells, (size_t)in.nc * in.NV);
    rc |= dev_alloc_copy(c, &m.nbr, T.nbr.data(), T.nbr.size());
    rc |= dev_alloc_copy(c, &m.fflag, T.fflag.data(), T.fflag.size());
    rc |= dev_alloc_copy(c, &m.cfacet, T.cfacet.data(), T.cfacet.size());
    rc |= dev_alloc_copy(c, &m.mf, T.mf.data(), T.mf.size());
    return rc;
}

static int upload_halo_lists(knp_ctx* c, const FacetTables& T) {
    MeshDev& m = c->m;
    if (!(m.dim == 3 && c->degree == 1 && m.nc_owned > 0 && m.nc < (int64_t(1) << 29))) return 0;
    HaloLists H;
    halo_block_lists(m.nc_owned, T, H);
    if (!H.stride) return 0;
    int rc = 0;
    rc |= dev_alloc_copy(c, &m.hb_src, H.src.data(), H.src.size());
    rc |= dev_alloc_copy(c, &m.hb_loc, H.loc.data(), H.loc.size());
    rc |= dev_zeros(c, &c->halo_ctr, KNP_HALO_CTR_INTS);
    m.hb_stride = H.stride;
    m.hb_long0 = H.long0;
    return rc;
}

// the fields, the solver workspace and the status block
static int allocate_fields(knp_ctx* c, const std::vector<float>& ivol) {
    Fields* fl = &c->fields;
    const int64_t nc = c->m.nc, nf = c->m.nf, ndof = nc * c->nd, ns = c->p.n_sys, n_ions = c->p.n_ions;
    const int64_t sizes[KNP_F_COUNT] = {ndof, ns * ndof, ns * ndof, ndof, nf, n_ions * nf, n_ions * nf, ndof, ndof,
                                        ndof, ns * ndof, ns * ndof, ns * ndof, (int64_t)KNP_FACET_TMP_SLOTS * nf};
    int rc = 0;
    for (int i = 0; i < KNP_F_COUNT; ++i) {
        fl->n[i] = sizes[i];
        rc |= dev_zeros(c, &fl->f[i], sizes[i]);
    }
    rc |= dev_zeros(c, &fl->emi.binv, ndof * c->nd);
    rc |= dev_zeros(c, &fl->knp.binv, ns * ndof * c->nd);
    double** wk[] = {&fl->r, &fl->z, &fl->p, &fl->w, &fl->rhat, &fl->v, &fl->y};
    for (auto pp : wk) rc |= dev_zeros(c, pp, ns * ndof);
    rc |= dev_zeros(c, &c->D, (size_t)n_ions * nc);
    rc |= dev_zeros(c, &c->rho, nc);
    c->partial_blocks = grid_for(c->m.nc_owned) + 8;
    rc |= dev_zeros(c, &c->partial, (size_t)c->partial_blocks * KNP_MAX_SYS * KNP_MAX_RED);
    // the status block: status words | Krylov scalars, reduction results, GMRES state.  One allocation, so that a look is one copy
    char* blk = nullptr;
    rc |= dev_zeros(c, &blk, KNP_STATUS_BYTES + sizeof(double) * KNP_SCAL_DOUBLES);
    c->status = (int*)blk;
    c->scal = blk ? (double*)(blk + KNP_STATUS_BYTES) : nullptr;
    if (!rc && hipHostMalloc(&c->pinned, KNP_PINNED_BYTES) != hipSuccess) rc = -2;
    if (!rc) memset(c->pinned, 0, KNP_PINNED_BYTES);
    if (!rc) rc = dev_alloc_copy(c, &fl->ivol, ivol.data(), ivol.size());
    return rc;
}

int knp_ctx_create(knp_ctx** out, int device, int dim, int degree, int n_ions, int64_t nv, int64_t nc, int64_t nc_owned,
                   int64_t nf, const double* coords, const int32_t* cells, const uint32_t* cell_tags,
                   const int32_t* facet_cells, const int8_t* facet_local, const uint32_t* facet_tags, int n_membrane_tags,
                   const uint32_t* membrane_tags) {
    if (!out) return -1;
    *out = nullptr;
    if (dim != 2 && dim != 3) { g_err = "dim must be 2 or 3"; return -1; }
    if (degree != 1 && degree != 2) { g_err = "degree must be 1 or 2"; return -1; }
    if (n_ions < 2 || n_ions > KNP_MAX_IONS) { g_err = "n_ions out of range"; return -1; }
    if (nc_owned < 0 || nc_owned > nc) { g_err = "nc_owned out of range"; return -1; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { g_err = "no HIP device visible"; return -5; }
    if (device < 0 || device >= ndev) { g_err = "device index out of range"; return -5; }
    // KNP_DEBUG_SETUP=1: wall-clock stamps of the stages below on stderr (next to the host-side stamps of knpemidg/_abi.py)
    const bool stamps = env_int("KNP_DEBUG_SETUP", 0) == 1;
    auto t_last = std::chrono::steady_clock::now();
    auto stamp = [&](const char* what) {
        if (!stamps) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "[knp setup            +%6.3f] knp_ctx_create: %s\n", std::chrono::duration<double>(now - t_last).count(), what);
        t_last = now;
    };
    knp_ctx* c = new knp_ctx();
    c->device = device;
    c->degree = degree;
    c->p2_assembled = degree != 1 && env_int("KNP_P2_ASSEMBLED", 0) == 1;
    const int NV = dim + 1;
    c->nd = degree == 1 ? NV : NV * (NV + 1) / 2;             // P2: vertices, then edges (a,b), a<b, lexicographic
    c->p.n_ions = n_ions;
    c->p.n_sys = n_ions - 1;
    c->amg.resize(1 + (size_t)(n_ions - 1));
    if (hipSetDevice(device) != hipSuccess) { g_err = "hipSetDevice failed"; delete c; return -5; }
    if (hipStreamCreate(&c->stream) != hipSuccess) { g_err = "hipStreamCreate failed"; delete c; return -5; }
    hipEventCreate(&c->ev0);
    hipEventCreate(&c->ev1);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->ncu = prop.multiProcessorCount;
    stamp("HIP runtime, stream");

    const MeshIn in{dim, NV, nv, nc, nc_owned, nf, coords, cells, cell_tags, facet_cells, facet_local, facet_tags, n_membrane_tags, membrane_tags};
    FacetTables T;
    if (const char* why = facet_tables(in, T)) return create_failed(c, -1, why);
    stamp("facet flags, neighbours");
    c->h_fflag = T.fflag;
    c->h_ctag.assign(cell_tags, cell_tags + nc);
    c->h_mf_mask.assign((size_t)nf, 0);
    c->h_mf_row.assign((size_t)nf, -1);
    for (size_t i = 0; i < T.mf.size(); i += 6) {
        c->h_mf_mask[(size_t)T.mf[i + 4]] = 1;
        c->h_mf_row[(size_t)T.mf[i + 4]] = (int32_t)(i / 6);
    }
    MeshDev& m = c->m;
    m.dim = dim; m.nv = nv; m.nc = nc; m.nc_owned = nc_owned; m.nf = nf; m.nmf = (int64_t)T.mf.size() / 6;
    m.c_begin = 0; m.c_end = nc_owned; m.n_interior = nc_owned;
    std::vector<double> hcell;
    std::vector<float> ivol;
    cell_metrics(in, hcell, ivol);
    stamp("diameters, volumes");
    int rc = upload_mesh(c, in, T, hcell);
    stamp("mesh tables on the device");
    rc |= upload_halo_lists(c, T);
    if (rc) return create_failed(c, -2, c->err);
    stamp("halo lists");
    if (allocate_fields(c, ivol)) return create_failed(c, -2, "device allocation failed: " + c->err);
    *out = c;
    stamp("fields allocated");
    return 0;
}

void knp_ctx_destroy(knp_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (auto& H : c->amg) amg_free(H);
    for (auto st : c->aux_streams) hipStreamDestroy(st);
    for (auto ev : c->aux_events) hipEventDestroy(ev);
    if (c->fork_event) hipEventDestroy(c->fork_event);
    surf_destroy_all(c);            // before the ODE tables its state addresses point into
    fieldmesh_destroy_all(c);
    ode_destroy_all(c);
    source_destroy(c);
    rec_destroy(c);
    grid_destroy_all(c);
    state_destroy(c);
    tab_free(c);
    Fields& fl = c->fields;
    for (int i = 0; i < KNP_F_COUNT; ++i) hipFree(fl.f[i]);
    hipFree(fl.bj_idx); hipFree(fl.bj_tab); hipFree(fl.ivol);
    double* wk[] = {fl.r, fl.z, fl.p, fl.w, fl.rhat, fl.v, fl.y};
    for (auto p : wk) hipFree(p);
    for (PrecState* s : {&fl.emi, &fl.knp}) { hipFree(s->binv); hipFree(s->hist); hipFree(s->tmp); }
    ring_u_free(c);
    hipFree(c->m.hb_src); hipFree(c->m.hb_loc);
    hipFree(c->m.cls); hipFree(c->m.cls_table); hipFree(c->m.cls_ext); hipFree(c->m.coords); hipFree(c->m.h); hipFree(c->m.cells); hipFree(c->m.nbr); hipFree(c->m.fflag); hipFree(c->m.cfacet); hipFree(c->m.mf);
    hipFree(c->mat); hipFree(c->nmat4); hipFree(c->dtab); hipFree(c->halo_ctr);
    hipFree(c->D); hipFree(c->rho); hipFree(c->fsrc); hipFree(c->mms_C); hipFree(c->extra_emi); hipFree(c->extra_knp); hipFree(c->partial); hipFree(c->status); /* c->scal: same allocation */ hipFree(c->gm_V);
    hipFree(c->halo_send_idx); hipFree(c->halo_sendbuf);
    if (c->pinned) hipHostFree(c->pinned);
    if (c->ev0) hipEventDestroy(c->ev0);
    if (c->ev1) hipEventDestroy(c->ev1);

    for (int w = 0; w < 2; ++w)
        for (auto& pr : c->tev[w]) { hipEventDestroy(pr.first); hipEventDestroy(pr.second); }
    comm_destroy(c);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

int knp_set_params(knp_ctx* c, double C_M, double dt, double Fc, double R, double T, double C_phi, double tau_emi,
                   double tau_knp, const double* z, const double* D, const double* rho, const double* fsrc, int splitting) {
    if (!c || !z || !D) return -1;
    Params& p = c->p;
    p.C_M = C_M; p.dt = dt; p.F = Fc; p.R = R; p.T = T; p.C_phi = C_phi; p.psi = Fc / (R * T);
    p.tau_emi = tau_emi; p.tau_knp = tau_knp; p.splitting = splitting;
    if (splitting == 2 && !c->mms_C) { c->err = "MMS mode needs knp_set_mms first"; return -1; }
    c->fields.reset_lagged();                                                // new coefficients: rebuild the block-Jacobi inverses
    for (int i = 0; i < p.n_ions; ++i) {
        p.z[i] = z[i];
        if (z[i] == 0.0) { c->err = "ion valence z must be non-zero"; return -1; }
    }
    if (!(dt > 0.0)) { c->err = "dt must be positive"; return -1; }
    HIPCHK(c, host_memcpy(c, c->D, D, sizeof(double) * p.n_ions * c->m.nc, hipMemcpyHostToDevice));
    c->fields.bj_tab_state = 0;                                             // D / dt may have changed: rebuild the block-Jacobi table
    // distinct D tuples over the cells (any dimension / degree): one of the keys of the KNP block-Jacobi table (empty beyond 256)
    const int64_t nc = c->m.nc;
    const int ni = p.n_ions;
    std::vector<double> tuples;                                             // [id][ni]
    const int nm = scan_materials(nc, ni, D, 256, c->h_mat, tuples);
    c->nmat = 0;
    if (c->m.dim == 3 && c->degree == 1 && c->m.hb_stride && nm >= 0 && nm <= KNP_MAX_MAT) {
        // few enough for the halo- and ring-staged KNP applies: the same ids as bytes, the tuples as [ni][KNP_MAX_MAT]
        std::vector<uint8_t> mat(c->h_mat.begin(), c->h_mat.end());
        std::vector<double> tab((size_t)ni * KNP_MAX_MAT, 0.0);
        for (int q = 0; q < nm; ++q)
            for (int i = 0; i < ni; ++i) tab[(size_t)i * KNP_MAX_MAT + q] = tuples[(size_t)q * ni + i];
        if (!c->mat) { HIPCHK(c, hipMalloc((void**)&c->mat, (size_t)nc + KNP_DMA_PAD)); HIPCHK(c, hipMemset(c->mat, 0, (size_t)nc + KNP_DMA_PAD)); }
        if (!c->nmat4) { HIPCHK(c, hipMalloc((void**)&c->nmat4, (size_t)nc * 4 + KNP_DMA_PAD)); HIPCHK(c, hipMemset(c->nmat4, 0, (size_t)nc * 4 + KNP_DMA_PAD)); }
        if (!c->dtab) HIPCHK(c, hipMalloc((void**)&c->dtab, sizeof(double) * KNP_MAX_IONS * KNP_MAX_MAT));
        HIPCHK(c, host_memcpy(c, c->mat, mat.data(), (size_t)nc, hipMemcpyHostToDevice));
        HIPCHK(c, host_memcpy(c, c->dtab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
        c->nmat = nm;
        int rcm = launch_neighbour_materials(c);
        if (rcm) return rcm;
    }
    if (rho) HIPCHK(c, host_memcpy(c, c->rho, rho, sizeof(double) * c->m.nc, hipMemcpyHostToDevice));
    else HIPCHK(c, hipMemset(c->rho, 0, sizeof(double) * c->m.nc));
    if (fsrc) {
        if (!c->fsrc) HIPCHK(c, hipMalloc((void**)&c->fsrc, sizeof(double) * p.n_sys * c->m.nc));
        HIPCHK(c, host_memcpy(c, c->fsrc, fsrc, sizeof(double) * p.n_sys * c->m.nc, hipMemcpyHostToDevice));
    } else if (c->fsrc) {
        hipFree(c->fsrc);
        c->fsrc = nullptr;
    }
    return 0;
}

int knp_set_geometry_classes(knp_ctx* c, int ncls, const uint16_t* cls, const double* table) {
    if (!c) return -1;
    hipFree(c->m.cls); hipFree(c->m.cls_table); hipFree(c->m.cls_ext);
    c->m.cls = nullptr; c->m.cls_table = nullptr; c->m.cls_ext = nullptr; c->m.ncls = 0;
    c->h_cls.clear();
    c->fields.bj_tab_state = 0;
    if (ncls <= 0) return 0;
    if (ncls > 65535 || !cls || !table) { c->err = "geometry classes: bad arguments"; return -1; }
    for (int64_t k = 0; k < c->m.nc; ++k)
        if (cls[k] >= ncls) { c->err = "geometry class id out of range"; return -1; }
    HIPCHK(c, hipMalloc((void**)&c->m.cls, sizeof(uint16_t) * c->m.nc + KNP_DMA_PAD));
    HIPCHK(c, hipMemset(c->m.cls, 0, sizeof(uint16_t) * c->m.nc + KNP_DMA_PAD));
    HIPCHK(c, host_memcpy(c, c->m.cls, cls, sizeof(uint16_t) * c->m.nc, hipMemcpyHostToDevice));
    c->h_cls.assign(cls, cls + c->m.nc);
    c->fields.bj_tab_state = 0;
    HIPCHK(c, hipMalloc((void**)&c->m.cls_table, sizeof(double) * (size_t)ncls * KNP_CLS_STRIDE));
    HIPCHK(c, host_memcpy(c, c->m.cls_table, table, sizeof(double) * (size_t)ncls * KNP_CLS_STRIDE, hipMemcpyHostToDevice));
    // derived per-facet coefficients of the classed P1 applies, so that no lane recomputes what only depends on the class:
    //   [8 i + 0] gr = G_ii / L_i          [8 i + 1..3] G_{a_m i} - L_{a_m} gr  (neighbour's gradient through the own basis, cell_geom.hpp)
    //   [8 i + 4] (2 / (h + h')) sqrt(G_ii) D vol   [8 i + 5] -L_i D vol (the neighbour's D vol')   [8 i + 6] sqrt(G_ii) D vol   [8 i + 7] 0
    std::vector<double> ext((size_t)ncls * KNP_CLS_EXT, 0.0);
    for (int q = 0; q < ncls; ++q) {
        const double* rec = table + (size_t)q * KNP_CLS_STRIDE;
        double G[4][4];
        int k = 1;
        for (int a = 0; a < 4; ++a)
            for (int b = a; b < 4; ++b) { G[a][b] = rec[k]; G[b][a] = rec[k]; ++k; }
        const double DV = 3.0 * rec[0];
        for (int i = 0; i < 4; ++i) {
            const double* L = rec + 11 + 6 * i;
            const double sqG = L[4], hinv = L[5];
            double* e = ext.data() + (size_t)q * KNP_CLS_EXT + 8 * i;
            if (L[i] != 0.0) {
                const double gr = G[i][i] / L[i];
                e[0] = gr;
                for (int mm = 0; mm < 3; ++mm) { const int a = mm + (mm >= i); e[1 + mm] = G[a][i] - L[a] * gr; }
            }
            e[4] = hinv * sqG * DV;
            e[5] = -L[i] * DV;
            e[6] = sqG * DV;
        }
    }
    hipFree(c->m.cls_ext); c->m.cls_ext = nullptr;
    HIPCHK(c, hipMalloc((void**)&c->m.cls_ext, sizeof(double) * ext.size()));
    HIPCHK(c, host_memcpy(c, c->m.cls_ext, ext.data(), sizeof(double) * ext.size(), hipMemcpyHostToDevice));
    c->m.ncls = ncls;
    return 0;
}

// Host-integrated load vector of the ion sources, int f_k v dx(0) (solver.py:599), for sources that are not constants: added to
// L_knp by the right-hand-side kernels.  src[n_sys][nc*nd] in device cell order, or null to clear.  (The manufactured-solution
// mode owns the same buffer: knp_set_mms.)  Species with a device-evaluated source (knp_source_register, source.hip) write their rows
// of the same buffer after this call, on the same stream: while one is registered, null zeroes the buffer instead of freeing it.
int knp_set_source(knp_ctx* c, const double* src) {
    if (!c) return -1;
    if (c->p.splitting == 2) { c->err = "knp_set_source: the manufactured-solution mode sets its own data terms"; return -1; }
    const int64_t n = (int64_t)c->p.n_sys * c->m.nc * c->nd;
    if (!src && c->extra_knp && source_registered(c)) {
        HIPCHK(c, hipMemsetAsync(c->extra_knp, 0, sizeof(double) * n, c->stream));
        return 0;
    }
    if (!src) {
        hipFree(c->extra_knp);
        c->extra_knp = nullptr;
        return 0;
    }
    if (!c->extra_knp) HIPCHK(c, hipMalloc((void**)&c->extra_knp, sizeof(double) * n));
    HIPCHK(c, host_memcpy(c, c->extra_knp, src, sizeof(double) * n, hipMemcpyHostToDevice));
    return 0;
}

int knp_set_mms(knp_ctx* c, const double* C, const double* extra_emi, const double* extra_knp) {
    if (!c) return -1;
    // the MMS branch of the KNP right-hand side reads C for every membrane facet: in that mode the table cannot be taken away
    if (!C && c->p.splitting == 2) { c->err = "knp_set_mms: C must not be null in MMS mode (splitting == 2); the tables are unchanged"; return -1; }
    const int64_t ndof = c->m.nc * c->nd, ns = c->p.n_sys;
    hipFree(c->mms_C); hipFree(c->extra_emi); hipFree(c->extra_knp);
    c->mms_C = c->extra_emi = c->extra_knp = nullptr;
    if (C) {
        HIPCHK(c, hipMalloc((void**)&c->mms_C, sizeof(double) * ns * c->m.nc));
        HIPCHK(c, host_memcpy(c, c->mms_C, C, sizeof(double) * ns * c->m.nc, hipMemcpyHostToDevice));
    }
    if (extra_emi) {
        HIPCHK(c, hipMalloc((void**)&c->extra_emi, sizeof(double) * ndof));
        HIPCHK(c, host_memcpy(c, c->extra_emi, extra_emi, sizeof(double) * ndof, hipMemcpyHostToDevice));
    }
    if (extra_knp) {
        HIPCHK(c, hipMalloc((void**)&c->extra_knp, sizeof(double) * ns * ndof));
        HIPCHK(c, host_memcpy(c, c->extra_knp, extra_knp, sizeof(double) * ns * ndof, hipMemcpyHostToDevice));
    }
    return 0;
}

int64_t knp_field_size(knp_ctx* c, int field) { return chk_field(c, field) ? -1 : c->fields.n[field]; }

static int64_t debug_table_ptr(knp_ctx* c, int which, const void** p) {
    const MeshDev& m = c->m;
    const int64_t NV = m.dim + 1;
    const int64_t nblk = (m.nc_owned + KNP_HALO_BLK - 1) / KNP_HALO_BLK;
    switch (which) {
        case KNP_DT_CELLS: *p = m.cells; return m.nc * NV * 4;
        case KNP_DT_NBR: *p = m.nbr; return m.nc * NV * 4;
        case KNP_DT_FLAG: *p = m.fflag; return m.nc * 4;
        case KNP_DT_CFACET: *p = m.cfacet; return m.nc * NV * 4;
        case KNP_DT_MF: *p = m.mf; return m.nmf * 6 * 4;
        case KNP_DT_HB_SRC: *p = m.hb_src; return m.hb_src ? nblk * m.hb_stride * 4 : 0;
        case KNP_DT_HB_LOC: *p = m.hb_loc; return m.hb_loc ? m.nc_owned * 4 * 2 : 0;
        case KNP_DT_META: *p = nullptr; return 8 * 8;
        case KNP_DT_RU_META: case KNP_DT_RU_HB_SRC: case KNP_DT_RU_HB_LOC: case KNP_DT_RU_VB_SRC: case KNP_DT_RU_VLOC: case KNP_DT_RU_HINV4:
            return ring_u_debug_table(c, which, p, nullptr);
        default: return -1;
    }
}
int64_t knp_debug_table_size(knp_ctx* c, int which) {
    const void* p = nullptr;
    return c ? debug_table_ptr(c, which, &p) : -1;
}
int knp_debug_table(knp_ctx* c, int which, void* out, int64_t nbytes) {
    if (!c) return -1;
    const void* p = nullptr;
    const int64_t n = debug_table_ptr(c, which, &p);
    if (n < 0 || nbytes != n || (n && !out)) { c->err = "debug_table: unknown table or size mismatch"; return -1; }
    if (which == KNP_DT_META) {
        const int64_t meta[8] = {c->m.nc, c->m.nc_owned, c->m.nf, c->m.nmf, c->m.hb_stride, c->m.hb_long0, c->m.n_interior, c->m.dim};
        memcpy(out, meta, sizeof(meta));
        return 0;
    }
    if (which == KNP_DT_RU_META) {
        int64_t meta[4] = {0, 0, 0, 0};
        if (n) ring_u_debug_table(c, which, &p, meta);
        if (n) memcpy(out, meta, sizeof(meta));
        return 0;
    }
    if (n) HIPCHK(c, host_memcpy(c, out, p, (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

int knp_upload(knp_ctx* c, int field, const double* src, int64_t offset, int64_t count) {
    if (chk_field(c, field)) return -1;
    if (offset < 0 || count < 0 || offset + count > c->fields.n[field]) { c->err = "upload range out of bounds"; return -1; }
    HIPCHK(c, hipMemcpyAsync(c->fields.f[field] + offset, src, sizeof(double) * count, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    // a caller-supplied state may be far from the one the lagged block-Jacobi inverses were built for
    if (field == KNP_F_C || field == KNP_F_C_ELIM || field == KNP_F_PHI || field == KNP_F_KAPPA) c->fields.reset_lagged();
    if (field == KNP_F_PHI) { c->fields.emi.nh = 0; c->last_peclet = -1.0f; }   // a caller-supplied state is not a point of the solution history
    if (field == KNP_F_C) c->fields.knp.nh = 0;
    return 0;
}

int knp_download(knp_ctx* c, int field, double* dst, int64_t offset, int64_t count) {
    if (chk_field(c, field)) return -1;
    if (offset < 0 || count < 0 || offset + count > c->fields.n[field]) { c->err = "download range out of bounds"; return -1; }
    HIPCHK(c, hipMemcpyAsync(dst, c->fields.f[field] + offset, sizeof(double) * count, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    return 0;
}

int knp_copy_field(knp_ctx* c, int dst, int src) {
    if (chk_field(c, dst) || chk_field(c, src)) return -1;
    if (c->fields.n[dst] != c->fields.n[src]) { c->err = "copy_field: size mismatch"; return -1; }
    HIPCHK(c, hipMemcpyAsync(c->fields.f[dst], c->fields.f[src], sizeof(double) * c->fields.n[src], hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

/* Owned cells [0, n_interior) of the device order have no ghost neighbour: with a communicator their part of an operator apply is
 * launched while the halo exchange of the input vector is in flight, the remaining owned cells after it (comm.hip: dist_apply). */
int knp_set_interior(knp_ctx* c, int64_t n_interior) {
    if (!c) return -1;
    if (n_interior < 0 || n_interior > c->m.nc_owned) { c->err = "set_interior: out of range"; return -1; }
    // every owned cell below n_interior must really be interior (checked once on the host copy of the neighbour table)
    std::vector<int32_t> nbr((size_t)c->m.nc_owned * (c->m.dim + 1));
    HIPCHK(c, host_memcpy(c, nbr.data(), c->m.nbr, sizeof(int32_t) * nbr.size(), hipMemcpyDeviceToHost));
    for (int64_t k = 0; k < n_interior * (c->m.dim + 1); ++k)
        if (nbr[k] >= c->m.nc_owned) { c->err = "set_interior: a cell below n_interior has a ghost neighbour"; return -1; }
    c->m.n_interior = n_interior;
    return 0;
}

}  // extern "C"
