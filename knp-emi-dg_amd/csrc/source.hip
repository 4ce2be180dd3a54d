// Device-evaluated ion sources (knpemidg.Expression): the runtime-compiled kernels of knpemidg/expression.py -- csrc/source_rtc.hpp
// around the user's expression -- registered per species and launched before every KNP solve.  An evaluation writes the load vector
// int f v dx(0) of the context's ECS cells (tag 0, owned and ghost) into the species' row of knp_ctx::extra_knp, the buffer the
// right-hand-side kernels already add to L_knp: one launch on the context's stream, the parameters by value, no copy and no wait.
// A knpemidg.FieldExpression (knp_source_register_fields) is the same with two additions: the kernel carries its own cell list (the
// cells whose tag is one of the registered subdomains) and reads phi and level-n concentrations through pointers that are looked
// up at every evaluation and passed by value as well.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "source_rtc.hpp"
#include <cstring>

struct SourceKernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    int n_params = 0;
    // knp_source_register_fields only: the kernel's own cell list and the fields it reads
    int n_fields = -1;             // -1: a plain source over the shared ECS list below
    int field_ids[KNP_SOURCE_MAX_FIELDS] = {0};      // 0: phi, 1 + i: ion i of the ion list (the eliminated one last)
    int32_t* sel = nullptr;        // [nsel] cells whose tag is one of the registered ones, device order
    int64_t nsel = 0;
};

// knp_ctx::src: owned by the context, so two contexts driven from two host threads share nothing here
struct SourceState {
    int32_t* sel = nullptr;        // [nsel] ECS cells in device order
    int64_t nsel = -1;             // -1: not built yet
    int nq = 0;                    // quadrature rule + basis values (knp_source_set_rule); one allocation: bary | w | B
    double* rule = nullptr;
    const double *bary = nullptr, *w = nullptr, *B = nullptr;
    SourceKernel k[KNP_MAX_SYS];
    int registered() const {
        int n = 0;
        for (const SourceKernel& s : k) n += s.fn != nullptr;
        return n;
    }
};

namespace {

SourceState* state_of(knp_ctx* c) { return c->src; }
SourceState& state_make(knp_ctx* c) {
    if (!c->src) c->src = new SourceState();
    return *c->src;
}

int64_t row_len(const knp_ctx* c) { return c->m.nc * c->nd; }

// drop one species' kernel; the stream is drained first: no launch of it may still be in flight when its module goes
void drop_kernel(knp_ctx* c, SourceKernel& K) {
    if (!K.mod) return;
    host_stream_sync(c, c->stream);
    hipModuleUnload(K.mod);
    hipFree(K.sel);
    K = SourceKernel();
}

// a registration over an existing source of the species: the old kernel may have written cells the new one never visits (other
// subdomains), so its row is zeroed on the stream first; then the kernel goes
int replace_kernel(knp_ctx* c, SourceKernel& K, int species) {
    if (!K.fn) return 0;
    if (c->extra_knp && c->p.splitting != 2)
        HIPCHK(c, hipMemsetAsync(c->extra_knp + (size_t)species * (size_t)row_len(c), 0, sizeof(double) * (size_t)row_len(c), c->stream));
    drop_kernel(c, K);
    return 0;
}

int ensure_buffer(knp_ctx* c) {
    if (c->extra_knp) return 0;
    const size_t bytes = sizeof(double) * (size_t)c->p.n_sys * (size_t)row_len(c);
    HIPCHK(c, hipMalloc((void**)&c->extra_knp, std::max<size_t>(bytes, 8)));
    HIPCHK(c, hipMemset(c->extra_knp, 0, std::max<size_t>(bytes, 8)));
    return 0;
}

// device copy of a host cell list (at least one element allocated, so that an empty list still owns a pointer)
int upload_cells(knp_ctx* c, const std::vector<int32_t>& sel, int32_t** out) {
    HIPCHK(c, hipMalloc((void**)out, std::max<size_t>(sel.size(), 1) * sizeof(int32_t)));
    if (!sel.empty()) HIPCHK(c, host_memcpy(c, *out, sel.data(), sel.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

}  // namespace

bool source_registered(knp_ctx* c) {
    const SourceState* S = state_of(c);
    return S && S->registered() > 0;
}

void source_destroy(knp_ctx* c) {
    SourceState* S = state_of(c);
    if (!S) return;
    for (SourceKernel& K : S->k) drop_kernel(c, K);
    hipFree(S->sel);
    hipFree(S->rule);
    delete S;
    c->src = nullptr;
}

extern "C" {

int knp_source_set_rule(knp_ctx* c, int nq, const double* bary, const double* w, const double* B) {
    if (!c) return -1;
    if (nq < 1 || nq > 4096 || !bary || !w || !B) { c->err = "source_set_rule: 1..4096 points with their weights and basis values"; return -1; }
    SourceState& S = state_make(c);
    const size_t NV = (size_t)c->m.dim + 1, nd = (size_t)c->nd;
    const size_t n = (size_t)nq * (NV + 1 + nd);
    HIPCHK(c, host_stream_sync(c, c->stream));           // an evaluation in flight still reads the old tables
    hipFree(S.rule);
    S.rule = nullptr; S.nq = 0;
    HIPCHK(c, hipMalloc((void**)&S.rule, n * sizeof(double)));
    HIPCHK(c, host_memcpy(c, S.rule, bary, (size_t)nq * NV * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, host_memcpy(c, S.rule + (size_t)nq * NV, w, (size_t)nq * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(c, host_memcpy(c, S.rule + (size_t)nq * (NV + 1), B, (size_t)nq * nd * sizeof(double), hipMemcpyHostToDevice));
    S.bary = S.rule; S.w = S.rule + (size_t)nq * NV; S.B = S.rule + (size_t)nq * (NV + 1);
    S.nq = nq;
    return 0;
}

int knp_source_register(knp_ctx* c, int species, const void* code, size_t size, const char* kernel_name, int n_params) {
    if (!c) return -1;
    if (c->p.splitting == 2) { c->err = "source_register: the manufactured-solution mode sets its own data terms"; return -1; }
    if (species < 0 || species >= c->p.n_sys) { c->err = "source_register: species outside [0, n_sys)"; return -1; }
    if (n_params < 0 || n_params > KNP_SOURCE_MAX_PARAMS) { c->err = "source_register: 0..32 parameters"; return -1; }
    if (!code || !size || !kernel_name) { c->err = "source_register: no code object / kernel name"; return -1; }
    SourceState& S = state_make(c);
    if (!S.nq) { c->err = "source_register: no quadrature rule yet (knp_source_set_rule)"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    if (S.nsel < 0) {
        // the host path's `subdomains == 0`: every cell of the context with tag 0, ghosts included, ascending device order
        std::vector<int32_t> sel;
        for (int64_t k = 0; k < c->m.nc; ++k)
            if (c->h_ctag[(size_t)k] == 0u) sel.push_back((int32_t)k);
        if (int rc = upload_cells(c, sel, &S.sel)) return rc;
        S.nsel = (int64_t)sel.size();
    }
    if (int rc = ensure_buffer(c)) return rc;
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (int rc = rtc_load_kernel(c, "source_register", code, kernel_name, &mod, &fn)) return rc;
    if (int rc = replace_kernel(c, S.k[species], species)) { hipModuleUnload(mod); return rc; }
    S.k[species].mod = mod;
    S.k[species].fn = fn;
    S.k[species].n_params = n_params;
    return 0;
}

int knp_source_register_fields(knp_ctx* c, int species, const void* code, size_t size, const char* kernel_name, int n_params, int n_fields,
                               const int* field_ids, int n_tags, const int* tags) {
    if (!c) return -1;
    if (c->p.splitting == 2) { c->err = "source_register_fields: the manufactured-solution mode sets its own data terms"; return -1; }
    if (species < 0 || species >= c->p.n_sys) { c->err = "source_register_fields: species outside [0, n_sys)"; return -1; }
    if (n_params < 0 || n_params > KNP_SOURCE_MAX_PARAMS) { c->err = "source_register_fields: 0..32 parameters"; return -1; }
    if (!code || !size || !kernel_name) { c->err = "source_register_fields: no code object / kernel name"; return -1; }
    static_assert(KNP_SOURCE_MAX_FIELDS == KNP_MAX_IONS + 1, "phi and every ion");
    if (n_fields < 0 || n_fields > KNP_SOURCE_MAX_FIELDS || (n_fields > 0 && !field_ids)) { c->err = "source_register_fields: 0..9 fields (phi and at most 8 ions)"; return -1; }
    for (int i = 0; i < n_fields; ++i) {
        if (field_ids[i] < 0 || field_ids[i] > c->p.n_ions) { c->err = "source_register_fields: field id outside [0, n_ions] (0: phi, 1 + i: ion i)"; return -1; }
        for (int j = 0; j < i; ++j)
            if (field_ids[j] == field_ids[i]) { c->err = "source_register_fields: a field id is listed twice"; return -1; }
    }
    if (n_tags < 1 || !tags) { c->err = "source_register_fields: at least one subdomain tag"; return -1; }
    SourceState& S = state_make(c);
    if (!S.nq) { c->err = "source_register_fields: no quadrature rule yet (knp_source_set_rule)"; return -1; }
    HIPCHK(c, hipSetDevice(c->device));
    // every cell of the context, owned and ghost, whose tag is one of `tags`: ascending device order
    std::vector<int32_t> sel;
    for (int64_t k = 0; k < c->m.nc; ++k)
        for (int t = 0; t < n_tags; ++t)
            if (tags[t] >= 0 && c->h_ctag[(size_t)k] == (uint32_t)tags[t]) { sel.push_back((int32_t)k); break; }
    if (int rc = ensure_buffer(c)) return rc;
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (int rc = rtc_load_kernel(c, "source_register_fields", code, kernel_name, &mod, &fn)) return rc;
    int32_t* dsel = nullptr;
    if (int rc = upload_cells(c, sel, &dsel)) { hipModuleUnload(mod); hipFree(dsel); return rc; }
    if (int rc = replace_kernel(c, S.k[species], species)) { hipModuleUnload(mod); hipFree(dsel); return rc; }
    SourceKernel& K = S.k[species];
    K.mod = mod;
    K.fn = fn;
    K.n_params = n_params;
    K.n_fields = n_fields;
    for (int i = 0; i < n_fields; ++i) K.field_ids[i] = field_ids[i];
    K.sel = dsel;
    K.nsel = (int64_t)sel.size();
    return 0;
}

int knp_source_eval(knp_ctx* c, int species, const double* params, int n_params) {
    if (!c) return -1;
    SourceState* S = state_of(c);
    if (species < 0 || species >= c->p.n_sys || !S || !S->k[species].fn) { c->err = "source_eval: no source registered for this species"; return -1; }
    if (c->p.splitting == 2) { c->err = "source_eval: the manufactured-solution mode sets its own data terms"; return -1; }
    if (n_params != S->k[species].n_params || (n_params > 0 && !params)) { c->err = "source_eval: parameter count differs from the registered kernel's"; return -1; }
    if (!c->extra_knp) { c->err = "source_eval: the source buffer is gone (knp_set_mms)"; return -1; }
    const SourceKernel& K = S->k[species];
    const bool with_fields = K.n_fields >= 0;
    int64_t n = with_fields ? K.nsel : S->nsel;
    if (!n) return 0;                                    // no cell in the list: nothing to launch, the row stays zero
    SourceParams p;
    memset(&p, 0, sizeof(p));
    for (int i = 0; i < n_params; ++i) p.v[i] = params[i];
    const int32_t* sel = with_fields ? K.sel : S->sel;
    const double* coords = c->m.coords;
    const int32_t* cells = c->m.cells;
    int nq = S->nq;
    const double *bary = S->bary, *w = S->w, *B = S->B;
    double* out = c->extra_knp + (size_t)species * (size_t)row_len(c);
    const unsigned grid = (unsigned)((n + KNP_SOURCE_BLOCK - 1) / KNP_SOURCE_BLOCK);
    if (with_fields) {
        // the field pointers as they are now (never cached across steps): phi of this step's EMI solve, level-n concentrations
        SourceFields fld;
        memset(&fld, 0, sizeof(fld));
        for (int i = 0; i < K.n_fields; ++i) {
            const int id = K.field_ids[i];
            const bool solved = id >= 1 && id <= c->p.n_sys;
            const double* f = knp_field_ptr(c, id == 0 ? KNP_F_PHI : solved ? KNP_F_C_PREV : KNP_F_C_ELIM, nullptr);
            if (!f) { c->err = "source_eval: a field the source reads is not allocated"; return -1; }
            if (solved) f += (int64_t)(id - 1) * row_len(c);
            if (c->nd % 2 == 0 && ((uintptr_t)f & 15u)) { c->err = "source_eval: a field the source reads is not 16-byte aligned"; return -1; }
            fld.v[i] = f;
        }
        void* args[] = {&n, &sel, &coords, &cells, &nq, &bary, &w, &B, &fld, &p, &out};
        HIPCHK(c, hipModuleLaunchKernel(K.fn, grid, 1, 1, KNP_SOURCE_BLOCK, 1, 1, 0, c->stream, args, nullptr));
        return 0;
    }
    void* args[] = {&n, &sel, &coords, &cells, &nq, &bary, &w, &B, &p, &out};
    HIPCHK(c, hipModuleLaunchKernel(K.fn, grid, 1, 1, KNP_SOURCE_BLOCK, 1, 1, 0, c->stream, args, nullptr));
    return 0;
}

int knp_source_clear(knp_ctx* c, int species) {
    if (!c) return -1;
    if (species < 0 || species >= c->p.n_sys) { c->err = "source_clear: species outside [0, n_sys)"; return -1; }
    SourceState* S = state_of(c);
    if (!S || !S->k[species].fn) return 0;
    if (c->extra_knp && c->p.splitting != 2)
        HIPCHK(c, hipMemsetAsync(c->extra_knp + (size_t)species * (size_t)row_len(c), 0, sizeof(double) * (size_t)row_len(c), c->stream));
    drop_kernel(c, S->k[species]);
    return 0;
}

int64_t knp_source_cells(knp_ctx* c) {
    const SourceState* S = c ? state_of(c) : nullptr;
    return S ? S->nsel : -1;
}

int knp_source_download(knp_ctx* c, double* out) {
    if (!c || !out) return -1;
    if (!c->extra_knp) return 1;
    HIPCHK(c, host_stream_sync(c, c->stream));
    HIPCHK(c, host_memcpy(c, out, c->extra_knp, sizeof(double) * (size_t)c->p.n_sys * (size_t)row_len(c), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
