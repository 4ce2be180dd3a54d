// Checkpoint of the step-to-step state: knp_state_describe / knp_state_save / knp_state_load (include/knpemi_hip.h).
//
// solve.hip, ode.hip and record.hip each list the state they own as blocks [ncomp][count][width] (knpemi_internal.hpp: StateBlk).  A
// save packs every device block into one staging buffer -- per-cell blocks through the cell permutation, so that the snapshot is in
// the caller's numbering whatever order the device keeps --, copies the staging buffer to pinned host memory in one transfer and
// puts the prologue, the block table and the few host-side counters around it.  A load checks the table against the context's own
// first, then runs the same path backwards.  The solvers' upload path (knp_upload) is not involved: nothing is invalidated.
//
// The pack kernels are plain streams: one element per thread, consecutive threads on consecutive elements of the caller-ordered
// side (8 bytes per lane for the fp64 blocks), 64-bit indices, a guarded tail.  The permuted side is read or written in runs of one
// cell's `width` values (32 to 400 bytes), so it moves whole cache lines too once the neighbouring lanes are counted.
//
// The cell permutation, the staging buffers and the timing events of a context are its CkptState (knp_ctx::ckpt), freed by state_destroy.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include <cstring>

// knp_ctx::ckpt: created by the first knp_state_cell_order / knp_state_save / knp_state_load, freed by state_destroy
struct CkptState {
    int32_t* rank = nullptr;          // device [nc]: caller's cell id -> device cell (null: identity)
    void* staging = nullptr;          // device
    void* pinned = nullptr;           // host
    size_t cap = 0;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    float pack_ms = 0.f, copy_ms = 0.f;
};

namespace {

CkptState& ckpt_make(knp_ctx* c) {
    if (!c->ckpt) c->ckpt = new CkptState();
    return *c->ckpt;
}

const unsigned char MAGIC[8] = {'K', 'N', 'P', 'S', 'T', 'A', 'T', 'E'};
const int32_t VERSION = 1;

size_t type_size(int type) { return type == KNP_ST_F64 || type == KNP_ST_I64 ? 8 : 4; }
size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

// staging[comp][i][a] = dev[comp][rank[i]][a]  (rank null: a copy).  n = ncomp * count * width elements.
template <typename T>
__global__ __launch_bounds__(KNP_BLOCK) void k_state_gather(int64_t n, int64_t count, int64_t width, const int32_t* __restrict__ rank,
                                                            const T* __restrict__ dev, T* __restrict__ staging) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n) return;
    int64_t src = i;
    if (rank) {
        const int64_t per = count * width, comp = i / per, rem = i - comp * per, cell = rem / width, a = rem - cell * width;
        src = comp * per + (int64_t)rank[cell] * width + a;
    }
    staging[i] = dev[src];
}

// dev[comp][rank[i]][a] = staging[comp][i][a]
template <typename T>
__global__ __launch_bounds__(KNP_BLOCK) void k_state_scatter(int64_t n, int64_t count, int64_t width, const int32_t* __restrict__ rank,
                                                             const T* __restrict__ staging, T* __restrict__ dev) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n) return;
    int64_t dst = i;
    if (rank) {
        const int64_t per = count * width, comp = i / per, rem = i - comp * per, cell = rem / width, a = rem - cell * width;
        dst = comp * per + (int64_t)rank[cell] * width + a;
    }
    dev[dst] = staging[i];
}

template <typename T> void launch_pack(knp_ctx* c, const StateBlk& b, const int32_t* rank, void* staging, bool save) {
    const int64_t n = (int64_t)b.ncomp * b.count * b.width;
    if (n <= 0) return;
    const dim3 g((unsigned)grid_for(n)), blk(KNP_BLOCK);
    const int32_t* r = b.kind == KNP_SK_CELL_DOF ? rank : nullptr;
    if (save) hipLaunchKernelGGL(k_state_gather<T>, g, blk, 0, c->stream, n, b.count, b.width, r, (const T*)b.dev, (T*)staging);
    else hipLaunchKernelGGL(k_state_scatter<T>, g, blk, 0, c->stream, n, b.count, b.width, r, (const T*)staging, (T*)b.dev);
}

struct Layout {
    std::vector<StateBlk> blocks;
    std::vector<knp_state_block> table;
    size_t header = 0, dev_bytes = 0, total = 0;      // payload of the device blocks first (one copy), host values behind it
};

int build_layout(knp_ctx* c, Layout& L) {
    int rc;
    if ((rc = fields_state_blocks(c, L.blocks))) return rc;
    if ((rc = ode_state_blocks(c, L.blocks))) return rc;
    if ((rc = rec_state_blocks(c, L.blocks))) return rc;
    L.header = align256(KNP_STATE_PROLOGUE + sizeof(knp_state_block) * L.blocks.size());
    L.table.resize(L.blocks.size());
    size_t off = L.header;
    for (int pass = 0; pass < 2; ++pass) {
        for (size_t i = 0; i < L.blocks.size(); ++i) {
            const StateBlk& b = L.blocks[i];
            if ((b.dev != nullptr) != (pass == 0)) continue;
            knp_state_block& t = L.table[i];
            t.id = b.id; t.kind = b.kind; t.type = b.type; t.ncomp = b.ncomp; t.count = b.count; t.width = b.width;
            t.offset = (int64_t)off;
            off += align256(type_size(b.type) * (size_t)b.ncomp * (size_t)b.count * (size_t)b.width);
        }
        if (pass == 0) L.dev_bytes = off - L.header;
    }
    L.total = off;
    return 0;
}

int refuse_ranks(knp_ctx* c, const char* who) {
    if (c->dist || c->nranks > 1 || c->m.nc_owned != c->m.nc) {
        c->err = std::string(who) + ": not supported with several ranks (a partitioned context holds ghost cells and shares its solves)";
        return -7;
    }
    return 0;
}

int ensure_buffers(knp_ctx* c, CkptState& S, size_t bytes) {
    for (auto& e : S.ev)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (bytes <= S.cap) return 0;
    if (S.staging) hipFree(S.staging);
    if (S.pinned) hipHostFree(S.pinned);
    S.staging = S.pinned = nullptr;
    S.cap = 0;
    HIPCHK(c, hipMalloc(&S.staging, bytes));
    HIPCHK(c, hipHostMalloc(&S.pinned, bytes));
    S.cap = bytes;
    return 0;
}

void pack_all(knp_ctx* c, const Layout& L, CkptState& S, bool save) {
    for (size_t i = 0; i < L.blocks.size(); ++i) {
        const StateBlk& b = L.blocks[i];
        if (!b.dev) continue;
        void* st = (char*)S.staging + ((size_t)L.table[i].offset - L.header);
        if (b.type == KNP_ST_F64 || b.type == KNP_ST_I64) launch_pack<double>(c, b, S.rank, st, save);
        else launch_pack<float>(c, b, S.rank, st, save);          // 4-byte elements are moved as bits
    }
}

}  // namespace

void state_destroy(knp_ctx* c) {
    if (!c->ckpt) return;
    CkptState& S = *c->ckpt;
    hipFree(S.rank);
    hipFree(S.staging);
    if (S.pinned) hipHostFree(S.pinned);
    for (auto e : S.ev)
        if (e) hipEventDestroy(e);
    delete c->ckpt;
    c->ckpt = nullptr;
}

const int32_t* state_cell_rank(knp_ctx* c) {
    return c->ckpt ? c->ckpt->rank : nullptr;
}

extern "C" {

int knp_state_cell_order(knp_ctx* c, const int64_t* order) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    CkptState& S = ckpt_make(c);
    HIPCHK(c, host_stream_sync(c, c->stream));
    hipFree(S.rank);
    S.rank = nullptr;
    if (!order) return 0;
    const int64_t nc = c->m.nc;
    std::vector<int32_t> rank((size_t)nc, -1);
    for (int64_t d = 0; d < nc; ++d) {
        if (order[d] < 0 || order[d] >= nc || rank[(size_t)order[d]] >= 0) { c->err = "knp_state_cell_order: not a permutation of the cells"; return -1; }
        rank[(size_t)order[d]] = (int32_t)d;
    }
    HIPCHK(c, hipMalloc((void**)&S.rank, sizeof(int32_t) * (size_t)(nc ? nc : 1)));
    if (nc) HIPCHK(c, host_memcpy(c, S.rank, rank.data(), sizeof(int32_t) * (size_t)nc, hipMemcpyHostToDevice));
    return 0;
}

int64_t knp_state_describe(knp_ctx* c, knp_state_block* out, int64_t cap, int64_t* bytes) {
    if (!c) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    Layout L;
    int rc = build_layout(c, L);
    if (rc) return rc;
    if (bytes) *bytes = (int64_t)L.total;
    if (out)
        for (int64_t i = 0; i < cap && i < (int64_t)L.table.size(); ++i) out[i] = L.table[(size_t)i];
    return (int64_t)L.table.size();
}

int knp_state_save(knp_ctx* c, void* host_buf, size_t bytes) {
    if (!c || !host_buf) return -1;
    int rc = refuse_ranks(c, "knp_state_save");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    Layout L;
    if ((rc = build_layout(c, L))) return rc;
    if (bytes != L.total) { c->err = "knp_state_save: the buffer must hold exactly the bytes knp_state_describe reports"; return -1; }
    CkptState& S = ckpt_make(c);
    if ((rc = ensure_buffers(c, S, L.dev_bytes ? L.dev_bytes : 256))) return rc;
    HIPCHK(c, hipMemsetAsync(S.staging, 0, L.dev_bytes, c->stream));          // the padding between blocks: same bytes in every snapshot
    HIPCHK(c, hipEventRecord(S.ev[0], c->stream));
    pack_all(c, L, S, true);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(S.ev[1], c->stream));
    HIPCHK(c, hipMemcpyAsync(S.pinned, S.staging, L.dev_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipEventRecord(S.ev[2], c->stream));
    { const int rc_ = sync_check_ode(c); if (rc_) return rc_; }
    HIPCHK(c, hipEventElapsedTime(&S.pack_ms, S.ev[0], S.ev[1]));
    HIPCHK(c, hipEventElapsedTime(&S.copy_ms, S.ev[1], S.ev[2]));
    char* out = (char*)host_buf;
    memset(out, 0, L.header);
    memcpy(out, MAGIC, 8);
    const int32_t nblk = (int32_t)L.table.size();
    const int64_t total = (int64_t)L.total;
    memcpy(out + 8, &VERSION, 4);
    memcpy(out + 12, &nblk, 4);
    memcpy(out + 16, &total, 8);
    memcpy(out + KNP_STATE_PROLOGUE, L.table.data(), sizeof(knp_state_block) * L.table.size());
    memcpy(out + L.header, S.pinned, L.dev_bytes);
    memset(out + L.header + L.dev_bytes, 0, L.total - L.header - L.dev_bytes);
    for (size_t i = 0; i < L.blocks.size(); ++i)
        if (!L.blocks[i].dev) memcpy(out + L.table[i].offset, L.blocks[i].host.data(), L.blocks[i].host.size());
    return 0;
}

int knp_state_load(knp_ctx* c, const void* host_buf, size_t bytes) {
    if (!c || !host_buf) return -1;
    int rc = refuse_ranks(c, "knp_state_load");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const char* in = (const char*)host_buf;
    int32_t ver = 0, nblk = 0;
    int64_t total = 0;
    if (bytes < KNP_STATE_PROLOGUE || memcmp(in, MAGIC, 8) != 0) { c->err = "knp_state_load: not a state snapshot"; return -8; }
    memcpy(&ver, in + 8, 4); memcpy(&nblk, in + 12, 4); memcpy(&total, in + 16, 8);
    if (ver != VERSION) { c->err = "knp_state_load: snapshot version " + std::to_string(ver) + ", this library reads " + std::to_string(VERSION); return -8; }
    Layout L;
    if ((rc = build_layout(c, L))) return rc;
    if (nblk != (int32_t)L.table.size() || (size_t)total != L.total || bytes != L.total) {
        c->err = "knp_state_load: the snapshot holds " + std::to_string(nblk) + " blocks in " + std::to_string((long long)total) + " bytes, this context " +
                 std::to_string(L.table.size()) + " in " + std::to_string(L.total);
        return -8;
    }
    std::vector<knp_state_block> theirs(L.table.size());
    memcpy(theirs.data(), in + KNP_STATE_PROLOGUE, sizeof(knp_state_block) * theirs.size());
    for (size_t i = 0; i < theirs.size(); ++i) {
        const knp_state_block &a = theirs[i], &b = L.table[i];
        if (a.id != b.id || a.kind != b.kind || a.type != b.type || a.ncomp != b.ncomp || a.count != b.count || a.width != b.width || a.offset != b.offset) {
            c->err = "knp_state_load: block " + std::to_string(b.id) + " differs: the snapshot has [" + std::to_string(a.ncomp) + "][" +
                     std::to_string((long long)a.count) + "][" + std::to_string((long long)a.width) + "] (id " + std::to_string(a.id) + "), this context [" +
                     std::to_string(b.ncomp) + "][" + std::to_string((long long)b.count) + "][" + std::to_string((long long)b.width) + "]";
            return -8;
        }
    }
    // ---- from here on the context changes ------------------------------------------------------------------------------------------
    CkptState& S = ckpt_make(c);
    if ((rc = ensure_buffers(c, S, L.dev_bytes ? L.dev_bytes : 256))) return rc;
    if ((rc = fields_state_prepare_load(c))) return rc;
    memcpy(S.pinned, in + L.header, L.dev_bytes);
    HIPCHK(c, hipEventRecord(S.ev[0], c->stream));
    HIPCHK(c, hipMemcpyAsync(S.staging, S.pinned, L.dev_bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipEventRecord(S.ev[1], c->stream));
    pack_all(c, L, S, false);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(S.ev[2], c->stream));
    HIPCHK(c, host_stream_sync(c, c->stream));
    HIPCHK(c, hipEventElapsedTime(&S.copy_ms, S.ev[0], S.ev[1]));
    HIPCHK(c, hipEventElapsedTime(&S.pack_ms, S.ev[1], S.ev[2]));
    for (size_t i = 0; i < L.blocks.size(); ++i)
        if (!L.blocks[i].dev && L.blocks[i].apply) L.blocks[i].apply(c, L.blocks[i].id, in + L.table[i].offset);
    return knp_update_kappa(c);                       // derived from the restored concentrations, as the next solve would find it
}

int knp_state_timing(knp_ctx* c, float* pack_ms, float* copy_ms) {
    if (!c || !pack_ms || !copy_ms) return -1;
    *pack_ms = c->ckpt ? c->ckpt->pack_ms : 0.f;
    *copy_ms = c->ckpt ? c->ckpt->copy_ms : 0.f;
    return 0;
}

}  // extern "C"
