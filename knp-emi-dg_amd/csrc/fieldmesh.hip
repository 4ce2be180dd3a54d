// Volume-field snapshots on the mesh: per output node the arithmetic mean of a list of nodal values of phi and of concentrations.
// A node is a pair (mesh entity, cell tag) -- or, for the exact DG values, one (cell, local dof) -- and its list holds the (cell,
// local dof) pairs that contribute; knpemidg/fieldmesh.py builds the nodes, the lists and the output mesh and holds the host
// statement (FieldMeshSpec.sample_host).  A frame is [n_fields][n_nodes] in the order the fields were given.
//
// One kernel per frame:
//   k_fieldmesh_sample   one thread per node, consecutive threads on consecutive nodes, so a wave stores consecutive elements of every
//                        plane.  The thread walks its list ONCE -- entries in the outer loop, planes in the inner one -- with one fp64
//                        accumulator per plane in registers (the plane loop is unrolled over KNP_FM_MAX_PLANES with a uniform guard,
//                        so the accumulators are never indexed at run time): the first value as it is, every further one added with
//                        __dadd_rn in list order, then ONE __ddiv_rn by the list's length; fp32 frames round that value once at the
//                        store.  A list of length one gives the nodal value's bits (v / 1.0).  An entry is the offset cell * nd + dof
//                        of the value in a nodal array, the same for every plane; offsets and list bounds are stored in 32 bits
//                        (knp_fieldmesh_create refuses contexts with 2^32 nodal values or more) and widened to 64 before any
//                        arithmetic.  No atomics, no LDS, no scratch.
// The lists are CSR: a wave's loads of one list position are as close in memory as the lists are long, and the values they point at
// are as close as the node order makes them (fieldmesh.py numbers the nodes along the device's cell order).
// Every index a thread uses was checked on the host by knp_fieldmesh_create: ptr starts at 0, strictly increases and ends at the
// entry count; every cell is an owned cell of the context, every dof below nd.
//
// Frames go through frame_pipe.hpp as the voxel grid's and the membrane surface's do.  A sampler holds no step-to-step state: it adds
// no checkpoint block.  The samplers of a context are its FieldMeshState (knp_ctx::fieldmesh), freed by fieldmesh_destroy_all.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "frame_pipe.hpp"

#define KNP_FM_MAX 4                               // samplers per context
#define KNP_FM_MAX_PLANES (KNP_MAX_IONS + 1)       // phi and every concentration

namespace {

struct FmPlanes {                   // by value into the kernel, in the order of the frame
    int n;
    const double* p[KNP_FM_MAX_PLANES];
};

struct FieldMesh {
    int64_t n = 0, nnz = 0;
    int n_fields = 0;
    bool f32 = false;
    int kind[KNP_FM_MAX_PLANES] = {0}, ion[KNP_FM_MAX_PLANES] = {0};
    uint32_t* ptr = nullptr;           // device [n + 1]
    uint32_t* off = nullptr;           // device [nnz]: cell * nd + dof
    FramePipe pipe;
    size_t frame_bytes() const { return (size_t)n_fields * (size_t)n * (f32 ? 4 : 8); }
};

}  // namespace

struct FieldMeshState {
    FieldMesh* s[KNP_FM_MAX] = {nullptr};
};

namespace {

template <typename OUT>
__global__ __launch_bounds__(KNP_BLOCK) void k_fieldmesh_sample(int64_t n, const uint32_t* __restrict__ ptr, const uint32_t* __restrict__ off,
                                                                FmPlanes S, OUT* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int64_t b = ptr[i], e = ptr[i + 1];
    double acc[KNP_FM_MAX_PLANES];
    {
        const int64_t o = off[b];
#pragma unroll
        for (int q = 0; q < KNP_FM_MAX_PLANES; ++q)
            if (q < S.n) acc[q] = S.p[q][o];
    }
    for (int64_t j = b + 1; j < e; ++j) {
        const int64_t o = off[j];
#pragma unroll
        for (int q = 0; q < KNP_FM_MAX_PLANES; ++q)
            if (q < S.n) acc[q] = __dadd_rn(acc[q], S.p[q][o]);
    }
    const double m = (double)(e - b);
#pragma unroll
    for (int q = 0; q < KNP_FM_MAX_PLANES; ++q)
        if (q < S.n) out[(int64_t)q * n + i] = (OUT)__ddiv_rn(acc[q], m);
}

template <typename OUT> void fm_launch(knp_ctx* c, const FieldMesh& s, const FmPlanes& S) {
    hipLaunchKernelGGL((k_fieldmesh_sample<OUT>), dim3((unsigned)grid_for(s.n)), dim3(KNP_BLOCK), 0, c->stream, s.n, (const uint32_t*)s.ptr,
                       (const uint32_t*)s.off, S, (OUT*)s.pipe.frame);
}

void fm_free(FieldMesh* s) {
    if (!s) return;
    hipFree(s->ptr); hipFree(s->off);
    s->pipe.release();
    delete s;
}

FieldMesh* fm_find(knp_ctx* c, int handle, const char* who) {
    if (!c->fieldmesh || handle < 0 || handle >= KNP_FM_MAX || !c->fieldmesh->s[handle]) {
        c->err = std::string(who) + ": no field-mesh sampler with handle " + std::to_string(handle) + " (knp_fieldmesh_create)";
        return nullptr;
    }
    return c->fieldmesh->s[handle];
}

}  // namespace

void fieldmesh_destroy_all(knp_ctx* c) {
    if (!c->fieldmesh) return;
    host_stream_sync(c, c->stream);
    for (FieldMesh* s : c->fieldmesh->s) fm_free(s);
    delete c->fieldmesh;
    c->fieldmesh = nullptr;
}

extern "C" {

int knp_fieldmesh_create(knp_ctx* c, int64_t n_nodes, const int64_t* ptr, const int32_t* entries, int n_fields, const int32_t* kind,
                         const int32_t* ion, int f32, int* handle_out) {
    if (!c) return -1;
    const MeshDev& m = c->m;
    const int n_ions = c->p.n_ions;
    const int64_t nd = c->nd;
    // ---- everything is validated before anything is allocated or uploaded ------------------------------------------------------
    if (c->dist || c->nranks > 1 || m.nc_owned != m.nc) {
        c->err = "knp_fieldmesh_create: not supported with several ranks (a partitioned context holds a part of the mesh)";
        return -7;
    }
    if (!ptr || !entries || !kind || !ion || !handle_out) { c->err = "knp_fieldmesh_create: null argument"; return -1; }
    if (n_nodes < 1 || n_nodes >= (int64_t(1) << 31)) { c->err = "knp_fieldmesh_create: between 1 and 2^31 - 1 nodes"; return -1; }
    if (n_fields < 1 || n_fields > KNP_FM_MAX_PLANES) {
        c->err = "knp_fieldmesh_create: between 1 and " + std::to_string(KNP_FM_MAX_PLANES) + " field planes";
        return -1;
    }
    if (m.nc_owned * nd >= (int64_t(1) << 32)) { c->err = "knp_fieldmesh_create: the context holds 2^32 nodal values or more"; return -1; }
    if (ptr[0] != 0) { c->err = "knp_fieldmesh_create: ptr must start at 0"; return -1; }
    for (int64_t i = 0; i < n_nodes; ++i)
        if (ptr[i + 1] <= ptr[i]) {
            c->err = "knp_fieldmesh_create: ptr must be strictly increasing: the list of node " + std::to_string(i) +
                     (ptr[i + 1] == ptr[i] ? " is empty" : " ends before it starts");
            return -1;
        }
    const int64_t nnz = ptr[n_nodes];
    if (nnz >= (int64_t(1) << 32)) { c->err = "knp_fieldmesh_create: fewer than 2^32 entries"; return -1; }
    std::vector<uint32_t> off((size_t)nnz);
    for (int64_t j = 0; j < nnz; ++j) {
        const int64_t cell = entries[2 * j], dof = entries[2 * j + 1];
        if (cell < 0 || cell >= m.nc_owned) {
            c->err = "knp_fieldmesh_create: cell " + std::to_string(cell) + " (entry " + std::to_string(j) + ") outside the context's " +
                     std::to_string(m.nc_owned) + " owned cells";
            return -1;
        }
        if (dof < 0 || dof >= nd) {
            c->err = "knp_fieldmesh_create: dof " + std::to_string(dof) + " (entry " + std::to_string(j) + ") outside 0 .. " + std::to_string(nd - 1);
            return -1;
        }
        off[(size_t)j] = (uint32_t)(cell * nd + dof);
    }
    for (int q = 0; q < n_fields; ++q) {
        if (kind[q] != KNP_FM_PHI && kind[q] != KNP_FM_C) { c->err = "knp_fieldmesh_create: unknown kind " + std::to_string(kind[q]); return -1; }
        if (kind[q] == KNP_FM_C && (ion[q] < 0 || ion[q] >= n_ions)) {
            c->err = "knp_fieldmesh_create: ion " + std::to_string(ion[q]) + " outside 0 .. n_ions - 1";
            return -1;
        }
    }
    const int64_t ndof = m.nc * nd;
    if (c->fields.n[KNP_F_PHI] < ndof || c->fields.n[KNP_F_C] < (int64_t)c->p.n_sys * ndof || c->fields.n[KNP_F_C_ELIM] < ndof) {
        c->err = "knp_fieldmesh_create: the nodal fields are shorter than the mesh";
        return -1;
    }
    int handle = -1;
    for (int s = 0; s < KNP_FM_MAX && handle < 0; ++s)
        if (!c->fieldmesh || !c->fieldmesh->s[s]) handle = s;
    if (handle < 0) { c->err = "knp_fieldmesh_create: at most 4 field-mesh samplers per context"; return -1; }
    std::vector<uint32_t> p32((size_t)n_nodes + 1);
    for (int64_t i = 0; i <= n_nodes; ++i) p32[(size_t)i] = (uint32_t)ptr[i];

    HIPCHK(c, hipSetDevice(c->device));
    FieldMesh* s = new FieldMesh();
    s->n = n_nodes; s->nnz = nnz; s->n_fields = n_fields; s->f32 = f32 != 0;
    for (int q = 0; q < n_fields; ++q) { s->kind[q] = kind[q]; s->ion[q] = kind[q] == KNP_FM_PHI ? -1 : ion[q]; }
    bool ok = hipMalloc((void**)&s->ptr, 4 * p32.size()) == hipSuccess && hipMalloc((void**)&s->off, 4 * off.size()) == hipSuccess;
    ok = ok && s->pipe.alloc(s->frame_bytes());
    if (!ok) {
        (void)hipGetLastError();
        fm_free(s);
        c->err = "knp_fieldmesh_create: allocation failed";
        return -2;
    }
    auto upload = [&]() -> int {
        HIPCHK(c, host_memcpy(c, s->ptr, p32.data(), 4 * p32.size(), hipMemcpyHostToDevice));
        HIPCHK(c, host_memcpy(c, s->off, off.data(), 4 * off.size(), hipMemcpyHostToDevice));
        return 0;
    };
    if (int rc = upload()) {
        fm_free(s);
        return rc;
    }
    // ---- from here on the context changes ------------------------------------------------------------------------------------------
    if (!c->fieldmesh) c->fieldmesh = new FieldMeshState();
    c->fieldmesh->s[handle] = s;
    *handle_out = handle;
    return 0;
}

int knp_fieldmesh_sample(knp_ctx* c, int fm) {
    if (!c) return -1;
    FieldMesh* sp = fm_find(c, fm, "knp_fieldmesh_sample");
    if (!sp) return -1;
    FieldMesh& s = *sp;
    const int n_sys = c->p.n_sys;
    const int64_t ndof = c->m.nc * c->nd;
    FmPlanes S;
    S.n = s.n_fields;
    for (int q = 0; q < KNP_FM_MAX_PLANES; ++q) S.p[q] = nullptr;
    for (int q = 0; q < s.n_fields; ++q) {
        const int k = s.ion[q];
        S.p[q] = k < 0 ? knp_field_ptr(c, KNP_F_PHI, nullptr)
                       : (k < n_sys ? knp_field_ptr(c, KNP_F_C, nullptr) + (int64_t)k * ndof : knp_field_ptr(c, KNP_F_C_ELIM, nullptr));
    }
    const int b = s.pipe.begin(c, "knp_fieldmesh_sample", "knp_fieldmesh_fetch");
    if (b < 0) return b;
    if (s.f32) fm_launch<float>(c, s, S);
    else fm_launch<double>(c, s, S);
    HIPCHK(c, hipGetLastError());
    return s.pipe.end(c, b);
}

int knp_fieldmesh_fetch(knp_ctx* c, int fm, void* out, size_t bytes) {
    if (!c || !out) return -1;
    FieldMesh* s = fm_find(c, fm, "knp_fieldmesh_fetch");
    if (!s) return -1;
    return s->pipe.fetch(c, "knp_fieldmesh_fetch", "knp_fieldmesh_sample", "n_fields x n_nodes values of the sampler's type", out, bytes);
}

int knp_fieldmesh_destroy(knp_ctx* c, int fm) {
    if (!c) return -1;
    FieldMesh* s = fm_find(c, fm, "knp_fieldmesh_destroy");
    if (!s) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, host_stream_sync(c, c->stream));
    c->fieldmesh->s[fm] = nullptr;
    fm_free(s);
    return 0;
}

int knp_fieldmesh_timing(knp_ctx* c, int fm, float* sample_ms, float* copy_ms) {
    if (!c || !sample_ms || !copy_ms) return -1;
    FieldMesh* s = fm_find(c, fm, "knp_fieldmesh_timing");
    if (!s) return -1;
    *sample_ms = s->pipe.sample_ms; *copy_ms = s->pipe.copy_ms;
    return 0;
}

}  // extern "C"
