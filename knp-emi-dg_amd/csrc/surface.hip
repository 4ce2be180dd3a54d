// Membrane-surface snapshots: per selected membrane facet the facet fields (phi_M, the Nernst potentials E_k, the channel currents
// I_ch_k and their sum), the facet means of the one-sided traces of phi and the concentrations, and gating variables read from the ODE
// state tables.  A frame is [n_planes][n]: the field planes in the order given, then the state planes; knpemidg/surface.py holds the
// host statement (SurfaceSpec.sample_host), the geometry of the surface and the files.
//
// One kernel per frame:
//   k_surf_sample   one thread per selected facet, consecutive threads on consecutive selected facets (ascending facet id), so a wave
//                   writes consecutive elements of every plane.  The thread reads its row of the membrane-facet table once
//                   (cell_e, cell_i, their local facets, the facet id) and loops over the planes:
//                     gather       PHI_M[f], E[k nf + f], I_CH[k nf + f]: the bits of the facet arrays
//                     I_ch_total   I_CH[f] + I_CH[nf + f] + ..., added in ion order, every sum rounded on its own
//                     trace        the nd nodal values of cell_e (cell_i) are loaded once and the facet mean is formed with compile-time
//                                  weights over the dofs of the local facet (the vertex opposite to local facet j is vertex j):
//                                  P1 (sum of the D vertex values) / D;  P2 in 3D (sum of the three edge values) / 3;  P2 in 2D
//                                  (u_a + u_b + 4 u_ab) / 6 -- the exact mean of the quadratic (Simpson).  Dofs are taken in ascending
//                                  local order (vertices, then the edges (a, b), a < b: knp_set_tabulation)
//                     state        the value behind the address the host formed for this facet, NaN for a null address
//                   fp32 frames are the fp64 value rounded once at the store.  No atomics, no LDS, no scratch.
// Every index a thread uses was checked on the host by knp_surf_create: the rows come from the context's own facet table, the state
// addresses are formed from checked (handle, row, column) triples as knp_rec_add_states forms them.
//
// Frames go through frame_pipe.hpp (two pinned buffers, an event per frame, fetch waits for that event only), as the voxel grid's
// do.  A surface sampler holds no step-to-step state: it adds no checkpoint block.  The samplers of a context are its SurfState
// (knp_ctx::surf), created with the first one and freed by surf_destroy_all.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "frame_pipe.hpp"
#include <cmath>

#define KNP_SURF_MAX 4              // samplers per context
#define KNP_SURF_MAX_PLANES 48      // field and state planes of one sampler

bool ode_state_table(knp_ctx* c, int handle, const double** states, int64_t* n, int* ns);   // ode.hip

namespace {

enum { SP_GATHER = 0, SP_TOTAL = 1, SP_TRACE_E = 2, SP_TRACE_I = 3, SP_STATE = 4 };   // what the kernel does for a plane

struct SurfPlanes {                 // by value into the kernel, in the order of the frame
    int n, n_ions;
    int op[KNP_SURF_MAX_PLANES];
    const void* p[KNP_SURF_MAX_PLANES];   // gather / total: the facet array (row of the ion); trace: the nodal field; state: [n] addresses
};

struct Surf {
    int64_t n = 0;
    int n_fields = 0, n_states = 0;
    bool f32 = false;
    int kind[KNP_SURF_MAX_PLANES] = {0}, ion[KNP_SURF_MAX_PLANES] = {0};
    int32_t* row = nullptr;            // device [n]: row of the membrane-facet table of every selected facet
    const double** st_addr = nullptr;  // device [n_states][n]: address of the value in an ODE state table, or null
    FramePipe pipe;
    int planes() const { return n_fields + n_states; }
    size_t frame_bytes() const { return (size_t)planes() * (size_t)n * (f32 ? 4 : 8); }
};

}  // namespace

struct SurfState {
    Surf* s[KNP_SURF_MAX] = {nullptr};
};

namespace {

// facet mean of the trace of the nodal function u[ND] of one cell on its local facet lf (see the head of the file)
template <int D, int P> __device__ __forceinline__ double surf_facet_mean(const double* __restrict__ u, int lf) {
    constexpr int NV = D + 1, ND = P == 1 ? NV : NV * (NV + 1) / 2;
    double v[ND];
    if constexpr (D == 3 && P == 1) {
        const double2 a = *reinterpret_cast<const double2*>(u), b = *reinterpret_cast<const double2*>(u + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    } else {
#pragma unroll
        for (int a = 0; a < ND; ++a) v[a] = u[a];
    }
    double s = 0.0;
    if constexpr (P == 1 || D == 2) {
#pragma unroll
        for (int a = 0; a < NV; ++a) s = __dadd_rn(s, a != lf ? v[a] : 0.0);
    }
    if constexpr (P == 2) {
        int e = NV;
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
            for (int b = a + 1; b < NV; ++b) {
                const double ve = D == 2 ? __dmul_rn(4.0, v[e]) : v[e];
                s = __dadd_rn(s, (a != lf && b != lf) ? ve : 0.0);
                ++e;
            }
    }
    return __ddiv_rn(s, P == 1 ? (double)D : (D == 3 ? 3.0 : 6.0));
}

template <int D, int P, typename OUT>
__global__ __launch_bounds__(KNP_BLOCK) void k_surf_sample(int64_t n, int64_t nf, const int32_t* __restrict__ rows, const int32_t* __restrict__ mf,
                                                           SurfPlanes S, OUT* __restrict__ out) {
    constexpr int NV = D + 1, ND = P == 1 ? NV : NV * (NV + 1) / 2, STRIDE = (D == 3 && P == 1) ? 4 : ND;
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t* __restrict__ r = mf + 6 * (int64_t)rows[i];
    const int64_t ce = r[0], ci = r[1], f = r[4];
    const int le = r[2], li = r[3];
    for (int q = 0; q < S.n; ++q) {
        const int op = S.op[q];
        double v;
        if (op == SP_GATHER) {
            v = ((const double*)S.p[q])[f];
        } else if (op == SP_TOTAL) {
            const double* __restrict__ I = (const double*)S.p[q];
            v = I[f];
            for (int k = 1; k < S.n_ions; ++k) v = __dadd_rn(v, I[(int64_t)k * nf + f]);
        } else if (op == SP_TRACE_E) {
            v = surf_facet_mean<D, P>((const double*)S.p[q] + ce * STRIDE, le);
        } else if (op == SP_TRACE_I) {
            v = surf_facet_mean<D, P>((const double*)S.p[q] + ci * STRIDE, li);
        } else {
            const double* a = ((const double* const*)S.p[q])[i];
            v = a ? *a : __builtin_nan("");
        }
        out[(int64_t)q * n + i] = (OUT)v;
    }
}

template <int D, int P, typename OUT> void surf_launch(knp_ctx* c, const Surf& s, const SurfPlanes& S) {
    hipLaunchKernelGGL((k_surf_sample<D, P, OUT>), dim3((unsigned)grid_for(s.n)), dim3(KNP_BLOCK), 0, c->stream, s.n, c->m.nf, (const int32_t*)s.row,
                       (const int32_t*)c->m.mf, S, (OUT*)s.pipe.frame);
}
template <int D, int P> void surf_type(knp_ctx* c, const Surf& s, const SurfPlanes& S) {
    if (s.f32) surf_launch<D, P, float>(c, s, S);
    else surf_launch<D, P, double>(c, s, S);
}

void surf_free(Surf* s) {
    if (!s) return;
    hipFree(s->row); hipFree((void*)s->st_addr);
    s->pipe.release();
    delete s;
}

Surf* surf_find(knp_ctx* c, int handle, const char* who) {
    if (!c->surf || handle < 0 || handle >= KNP_SURF_MAX || !c->surf->s[handle]) {
        c->err = std::string(who) + ": no surface sampler with handle " + std::to_string(handle) + " (knp_surf_create)";
        return nullptr;
    }
    return c->surf->s[handle];
}

}  // namespace

void surf_destroy_all(knp_ctx* c) {
    if (!c->surf) return;
    host_stream_sync(c, c->stream);
    for (Surf* s : c->surf->s) surf_free(s);
    delete c->surf;
    c->surf = nullptr;
}

extern "C" {

int knp_surf_create(knp_ctx* c, int64_t n, const int32_t* facets, int n_fields, const int32_t* kind, const int32_t* ion, int n_states,
                    const int32_t* state_handle, const int64_t* state_row, const int32_t* state_col, int f32) {
    if (!c) return -1;
    const MeshDev& m = c->m;
    const int n_ions = c->p.n_ions;
    // ---- everything is validated before anything is allocated or uploaded ------------------------------------------------------
    if (c->dist || c->nranks > 1 || m.nc_owned != m.nc) {
        c->err = "knp_surf_create: not supported with several ranks (a partitioned context holds a part of the mesh)";
        return -7;
    }
    if (n < 1 || n >= (int64_t(1) << 31)) { c->err = "knp_surf_create: between 1 and 2^31 - 1 facets"; return -1; }
    if (n_fields < 0 || n_states < 0 || n_fields + n_states < 1 || n_fields + n_states > KNP_SURF_MAX_PLANES) {
        c->err = "knp_surf_create: between 1 and " + std::to_string(KNP_SURF_MAX_PLANES) + " field and state planes";
        return -1;
    }
    if (!facets || (n_fields && (!kind || !ion)) || (n_states && (!state_handle || !state_row || !state_col))) {
        c->err = "knp_surf_create: null argument";
        return -1;
    }
    if (c->h_mf_row.size() != (size_t)m.nf) { c->err = "knp_surf_create: the context holds no membrane-facet table"; return -1; }
    std::vector<int32_t> rows((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t f = facets[i];
        if (f < 0 || f >= m.nf || c->h_mf_row[(size_t)f] < 0) {
            c->err = "knp_surf_create: facet " + std::to_string(f) + " (entry " + std::to_string(i) + ") is not a membrane facet of the context";
            return -1;
        }
        if (i && facets[i - 1] >= facets[i]) { c->err = "knp_surf_create: the facets must be ascending (entry " + std::to_string(i) + ")"; return -1; }
        rows[(size_t)i] = c->h_mf_row[(size_t)f];
    }
    bool need_params = false;
    for (int q = 0; q < n_fields; ++q) {
        const int k = kind[q];
        if (k != KNP_SF_PHI_M && k != KNP_SF_E && k != KNP_SF_I_CH && k != KNP_SF_I_CH_TOTAL && k != KNP_SF_TRACE_E && k != KNP_SF_TRACE_I) {
            c->err = "knp_surf_create: unknown kind " + std::to_string(k);
            return -1;
        }
        const bool traced = k == KNP_SF_TRACE_E || k == KNP_SF_TRACE_I;
        if (((k == KNP_SF_E || k == KNP_SF_I_CH) && (ion[q] < 0 || ion[q] >= n_ions)) || (traced && (ion[q] < -1 || ion[q] >= n_ions))) {
            c->err = "knp_surf_create: ion " + std::to_string(ion[q]) + " outside " + (traced ? "-1" : "0") + " .. n_ions - 1";
            return -1;
        }
        need_params |= k == KNP_SF_E || k == KNP_SF_I_CH || k == KNP_SF_I_CH_TOTAL;
    }
    // dt > 0 is what knp_set_params insists on: it is 0 until the parameters have been set
    if (need_params && !(c->p.dt > 0.0)) { c->err = "knp_surf_create: the parameters were never set (knp_set_params)"; return -1; }
    if (need_params && (c->fields.n[KNP_F_E] < (int64_t)n_ions * m.nf || c->fields.n[KNP_F_I_CH] < (int64_t)n_ions * m.nf)) {
        c->err = "knp_surf_create: the facet fields hold fewer than n_ions rows";
        return -1;
    }
    std::vector<const double*> addr((size_t)n_states * (size_t)n, nullptr);
    for (int q = 0; q < n_states; ++q)
        for (int64_t i = 0; i < n; ++i) {
            const size_t e = (size_t)q * (size_t)n + (size_t)i;
            if (state_handle[e] == -1) continue;             // the facet's model has no such state: NaN
            const double* tab = nullptr;
            int64_t nrow = 0;
            int ns = 0;
            const std::string where = "knp_surf_create: state " + std::to_string(q) + ", facet entry " + std::to_string(i) + ": ";
            if (!ode_state_table(c, state_handle[e], &tab, &nrow, &ns)) { c->err = where + "unknown ODE handle " + std::to_string(state_handle[e]); return -1; }
            if (state_row[e] < 0 || state_row[e] >= nrow) {
                c->err = where + "row " + std::to_string(state_row[e]) + " outside the handle's " + std::to_string(nrow) + " rows";
                return -1;
            }
            if (state_col[e] < 0 || state_col[e] >= ns) {
                c->err = where + "column " + std::to_string(state_col[e]) + " outside the handle's " + std::to_string(ns) + " states";
                return -1;
            }
            addr[e] = tab + state_row[e] * ns + state_col[e];
        }
    int handle = -1;
    for (int s = 0; s < KNP_SURF_MAX && handle < 0; ++s)
        if (!c->surf || !c->surf->s[s]) handle = s;
    if (handle < 0) { c->err = "knp_surf_create: at most 4 surface samplers per context"; return -1; }

    HIPCHK(c, hipSetDevice(c->device));
    Surf* s = new Surf();
    s->n = n; s->n_fields = n_fields; s->n_states = n_states; s->f32 = f32 != 0;
    for (int q = 0; q < n_fields; ++q) { s->kind[q] = kind[q]; s->ion[q] = ion[q]; }
    bool ok = hipMalloc((void**)&s->row, 4 * (size_t)n) == hipSuccess &&
              (!n_states || hipMalloc((void**)&s->st_addr, sizeof(double*) * addr.size()) == hipSuccess);
    ok = ok && s->pipe.alloc(s->frame_bytes());
    if (!ok) {
        (void)hipGetLastError();
        surf_free(s);
        c->err = "knp_surf_create: allocation failed";
        return -2;
    }
    auto upload = [&]() -> int {
        HIPCHK(c, host_memcpy(c, s->row, rows.data(), 4 * (size_t)n, hipMemcpyHostToDevice));
        if (n_states) HIPCHK(c, host_memcpy(c, (void*)s->st_addr, addr.data(), sizeof(double*) * addr.size(), hipMemcpyHostToDevice));
        return 0;
    };
    if (int rc = upload()) {
        surf_free(s);
        return rc;
    }
    // ---- from here on the context changes ------------------------------------------------------------------------------------------
    if (!c->surf) c->surf = new SurfState();
    c->surf->s[handle] = s;
    return handle;
}

int knp_surf_sample(knp_ctx* c, int surf) {
    if (!c) return -1;
    Surf* sp = surf_find(c, surf, "knp_surf_sample");
    if (!sp) return -1;
    Surf& s = *sp;
    const int n_sys = c->p.n_sys;
    const int64_t ndof = c->m.nc * c->nd;
    SurfPlanes S;
    S.n = s.planes(); S.n_ions = c->p.n_ions;
    for (int q = 0; q < KNP_SURF_MAX_PLANES; ++q) { S.op[q] = SP_GATHER; S.p[q] = nullptr; }
    for (int q = 0; q < s.n_fields; ++q) {
        const int k = s.ion[q];
        switch (s.kind[q]) {
            case KNP_SF_PHI_M: S.p[q] = knp_field_ptr(c, KNP_F_PHI_M, nullptr); break;
            case KNP_SF_E: S.p[q] = knp_field_ptr(c, KNP_F_E, nullptr) + (int64_t)k * c->m.nf; break;
            case KNP_SF_I_CH: S.p[q] = knp_field_ptr(c, KNP_F_I_CH, nullptr) + (int64_t)k * c->m.nf; break;
            case KNP_SF_I_CH_TOTAL: S.op[q] = SP_TOTAL; S.p[q] = knp_field_ptr(c, KNP_F_I_CH, nullptr); break;
            default:
                S.op[q] = s.kind[q] == KNP_SF_TRACE_E ? SP_TRACE_E : SP_TRACE_I;
                S.p[q] = k < 0 ? knp_field_ptr(c, KNP_F_PHI, nullptr)
                               : (k < n_sys ? knp_field_ptr(c, KNP_F_C, nullptr) + (int64_t)k * ndof : knp_field_ptr(c, KNP_F_C_ELIM, nullptr));
        }
    }
    for (int q = 0; q < s.n_states; ++q) { S.op[s.n_fields + q] = SP_STATE; S.p[s.n_fields + q] = s.st_addr + (int64_t)q * s.n; }
    const int b = s.pipe.begin(c, "knp_surf_sample", "knp_surf_fetch");
    if (b < 0) return b;
    if (c->m.dim == 3) { if (c->degree == 1) surf_type<3, 1>(c, s, S); else surf_type<3, 2>(c, s, S); }
    else { if (c->degree == 1) surf_type<2, 1>(c, s, S); else surf_type<2, 2>(c, s, S); }
    HIPCHK(c, hipGetLastError());
    return s.pipe.end(c, b);
}

int knp_surf_fetch(knp_ctx* c, int surf, void* out, size_t bytes) {
    if (!c || !out) return -1;
    Surf* s = surf_find(c, surf, "knp_surf_fetch");
    if (!s) return -1;
    return s->pipe.fetch(c, "knp_surf_fetch", "knp_surf_sample", "n_planes x n values of the sampler's type", out, bytes);
}

int knp_surf_destroy(knp_ctx* c, int surf) {
    if (!c) return -1;
    Surf* s = surf_find(c, surf, "knp_surf_destroy");
    if (!s) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, host_stream_sync(c, c->stream));
    c->surf->s[surf] = nullptr;
    surf_free(s);
    return 0;
}

int knp_surf_timing(knp_ctx* c, int surf, float* sample_ms, float* copy_ms) {
    if (!c || !sample_ms || !copy_ms) return -1;
    Surf* s = surf_find(c, surf, "knp_surf_timing");
    if (!s) return -1;
    *sample_ms = s->pipe.sample_ms; *copy_ms = s->pipe.copy_ms;
    return 0;
}

}  // extern "C"
