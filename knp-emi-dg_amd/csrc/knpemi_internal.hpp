// Internal declarations of libknpemi_hip.so (gfx950 only).  The public C ABI is
// include/knpemi_hip.h; nothing here is visible to callers.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include <map>
#include "../../include/knpemi_hip.h"
#include "amg.hpp"

// block-Jacobi inverses are preconditioner data: stored in fp32 (half the bytes of the largest stream of the fused Krylov
// vector kernels), applied in fp64 arithmetic; the EMI blocks are symmetrised before rounding so that PCG keeps an exactly
// symmetric preconditioner
typedef float bjreal;

#define KNP_MAX_IONS 8          // total species incl. the eliminated one
#define KNP_MAX_SYS 7           // solved species (batched KNP systems)
#define KNP_BLOCK 256
#define KNP_MAX_RED 8           // partial sums per block per system in one reduction pass
#define KNP_ODE_FAIL_SLOT (2 * KNP_MAX_SYS)   // word of knp_ctx::status raised by k_ode_step (read back with the solver status)
#define KNP_PECLET_SLOT (2 * KNP_MAX_SYS + 1)     // bits of a float: max over the owned cells of psi max|z| (max - min nodal phi), set by knp_update_dnphi
#define KNP_STATUS_WORDS (2 * KNP_MAX_SYS + 2)
#define KNP_STATUS_BYTES (sizeof(int) * KNP_STATUS_WORDS)   // knp_ctx::scal starts this far into the status block (context.hip)
#define KNP_PINNED_BYTES 4096

// facet kinds stored in bits 2..3 of the per-(cell, local facet) flag byte
enum : uint32_t { FK_SIPG = 0u, FK_MEMBRANE = 1u, FK_EXTERIOR = 2u, FK_INACTIVE = 3u };
// bits 0..1: local facet index of this facet in the neighbour cell
// bit 4    : this cell is the `plus` (ECS-like, lower tag) side of the oriented normal n_g

struct MeshDev {
    int dim = 0;
    int64_t nv = 0, nc = 0, nc_owned = 0, nf = 0, nmf = 0;
    int64_t c_begin = 0, c_end = 0;   // cell range of the operator-apply launches: [0, nc_owned), or the interior / boundary part of it
    int64_t n_interior = 0;           // owned cells [0, n_interior) have no ghost neighbour (device order: interior first)
    double* coords = nullptr;      // [nv][4] in 3D (padded), [nv][2] in 2D
    int32_t* cells = nullptr;      // [nc][dim+1]
    double* h = nullptr;           // [nc] cell diameters (UFL CellDiameter: longest edge)
    int32_t* nbr = nullptr;        // [nc][dim+1]
    uint32_t* fflag = nullptr;     // [nc] packed 4 x u8 flag bytes
    int32_t* cfacet = nullptr;     // [nc][dim+1] global facet ids
    int32_t* mf = nullptr;         // [nmf][6]: cell_e, cell_i, lf_e, lf_i, facet, owner flag
    uint16_t* cls = nullptr;       // [nc] geometry class of every cell (structured meshes), or null
    double* cls_table = nullptr;   // [ncls][KNP_CLS_STRIDE]
    double* cls_ext = nullptr;     // [ncls][KNP_CLS_EXT]: per facet 8 derived coefficients (context.hip: knp_set_geometry_classes), read by the halo-staged KNP apply
    int ncls = 0;
    // per-256-cell-block neighbour tables of the halo-staged applies (3D P1; blocks are aligned at multiples of 256 from cell 0)
    int32_t* hb_src = nullptr;     // [nblk][hb_stride]: 4 * neighbour cell + its local facet, one entry per coupled facet whose neighbour lies
                                   // outside the block; -1 behind the block's last entry
    uint16_t* hb_loc = nullptr;    // [nc_owned][4] LDS entry of the neighbour behind facet i: < 256 in-block cell, else 256 + position in the list
    int hb_stride = 0;             // longest list of the blocks [0, hb_long0), rounded up to 8 (0: no tables)
    int64_t hb_long0 = 0;          // first block whose list is longer than one entry per thread (cut cells of a partition), else the block count
};
#define KNP_CLS_STRIDE 36
#define KNP_CLS_EXT 32
#define KNP_HALO_BLK 256
#define KNP_MAX_MAT 16
#define CLS_MAX_LDS 32          // most geometry classes whose records the LDS-staged and ring-staged applies keep in LDS
#define KNP_HALO_CTR_INTS (2 * 2 * 64 * 32)   // knp_ctx::halo_ctr: [2 operators][2 sets][64 queues], one 128-byte line per counter (apply_p1_halo.hpp)

struct Params {
    int n_ions = 0;                // total species, last one eliminated
    int n_sys = 0;                 // n_ions - 1
    double C_M = 0, dt = 0, F = 0, R = 0, T = 0, C_phi = 0, psi = 0;
    double tau_emi = 0, tau_knp = 0;
    double z[KNP_MAX_IONS] = {0};
    double f_source[KNP_MAX_IONS] = {0};
    int splitting = 1;
};

// one quadrature rule with the reference basis tabulated at its points (DG-p path, tab_rhs.hip / tab_assembled.hip); device pointers
struct TabRule {
    int nq = 0;
    const double* w = nullptr;     // [nq], sums to 1
    const double* B = nullptr;     // [nloc][nq][nd]        nloc = 1 (cell rule) or dim+1 (one per local facet)
    const double* dB = nullptr;    // [nloc][nq][nd][dim+1] derivatives with respect to the barycentric coordinates
};
#define KNP_TAB_COUNT 11

struct KernelArgsIons {            // small by-value structs for kernels
    int n;
    double z[KNP_MAX_IONS];
};

// What one linear system (EMI or KNP) keeps from solve to solve (solve.hip).  The inverses and the spectral bound lag behind the
// coefficients; the history feeds the extrapolated initial guess.
struct PrecState {
    bjreal* binv = nullptr;        // per-cell block-Jacobi inverses, rebuilt every KNP_BJ_LAG-th solve (like the AMG hierarchy)
    double* hist = nullptr;        // [2][n] previous converged solutions: x0 = 2 x_{k-1} - x_{k-2}; allocated by the first solve
    int nh = 0;                    // valid history entries
    int age = 0;                   // solves since the inverses were rebuilt
    double* tmp = nullptr;         // scratch of the Chebyshev block-Jacobi smoother
    double lmax = 0.0;             // lambda_max(Binv A) estimate (power iteration; redone after every reset of the lagged inverses,
    int lmax_age = 0;              // every 64 solves, and when the iteration count jumps by > 1.5x)
    int it_ref = 0;                // iteration count right after the last estimate
};

// the fields of the public ABI (knp_field) and the solver state of a context
struct Fields {
    double* f[KNP_F_COUNT] = {nullptr};
    int64_t n[KNP_F_COUNT] = {0};
    double *r = nullptr, *z = nullptr, *p = nullptr, *w = nullptr, *rhat = nullptr, *v = nullptr, *y = nullptr;   // Krylov work vectors
    PrecState emi, knp;
    int bj_used_tab = -1;          // block set of the last KNP solve (1: drift-free class table, 0: per-cell inverses); a flip redoes the estimate
    // KNP block-Jacobi table (structured meshes): 0 = not built yet, 1 = ready, -1 = unavailable for this context
    int bj_tab_state = 0;
    uint16_t* bj_idx = nullptr;    // [nc_owned]
    bjreal* bj_tab = nullptr;      // [entries][n_sys][nd*nd]
    int bj_entries = 0;
    float* ivol = nullptr;         // [nc] 1 / cell volume: weights of the residual norms of the stopping tests (krylov.hip)
    double emi_r_abs = 0.0;        // knp_emi_residual_target: > 0 -> PCG stops on ||b - A phi||_w <= this
    // everything that is lagged behind the coefficients: the block-Jacobi inverses AND the spectral bound of the Chebyshev
    // block-Jacobi smoother built on them (a stale / too small lambda_max makes the polynomial amplify the top modes)
    void reset_lagged() {
        emi.age = knp.age = 0;
        emi.lmax = knp.lmax = 0.0;
    }
};

// Per-context state of the subsystems, each defined in the file that owns it.  The owner creates its struct at the first call that
// needs it and frees it (and nulls the pointer) in its destroy function below: the library keeps no per-context state outside the context.
struct SourceState;                // source.hip: the context's device-evaluated ion sources
struct OdeState;                   // ode.hip: membrane-model sets and runtime-compiled models
struct RecState;                   // record.hip: the time-series recorder
struct GridState;                  // grid.hip: voxel grids and the uploaded tag table
struct SurfState;                  // surface.hip: membrane-surface samplers
struct FieldMeshState;             // fieldmesh.hip: volume-field samplers on the mesh
struct CkptState;                  // state.hip: cell permutation, checkpoint staging, events
struct RingUState;                 // apply_ring_u.hip: per-block tables of the unstructured ring

struct knp_ctx {
    int device = 0;
    int degree = 1;
    bool p2_assembled = false;     // KNP_P2_ASSEMBLED=1 when the context was created: fixed for the context's life (its blocks exist or not)
    int nd = 0;                    // dofs per cell
    hipStream_t stream = nullptr;
    MeshDev m;
    Params p;
    double* D = nullptr;           // [n_ions][nc]
    // D is piecewise constant by subdomain in every reference configuration (make_global of D_sub, solver.py:88-112): when the cells
    // carry <= KNP_MAX_MAT distinct coefficient tuples the halo-staged KNP apply reads a 1-byte material id per cell and per facet
    // neighbour instead of n_sys doubles (set by knp_set_params; nmat = 0 -> general per-cell D, the kernels read c->D)
    uint8_t* mat = nullptr;        // [nc] material id of the cell
    uint8_t* nmat4 = nullptr;      // [nc][4] material id of the neighbour behind every facet (3D)
    double* dtab = nullptr;        // [n_ions][KNP_MAX_MAT]
    int nmat = 0;
    // host copies of what decides a cell's KNP block-Jacobi block on a structured mesh (solve.hip: build_bj_table): geometry class,
    // material (distinct D tuple, any count up to 65535; empty = too many), flag bytes (facet kinds)
    std::vector<uint16_t> h_cls, h_mat;
    std::vector<uint32_t> h_fflag;
    std::vector<uint32_t> h_ctag;    // [nc] subdomain tag of every cell, device order: the table the grid sampler's tag filter and tag volume read (grid.hip)
    std::vector<uint8_t> h_mf_mask;  // [nf] 1 on membrane facets: what knp_rec_create checks the caller's facet sets against
    std::vector<int32_t> h_mf_row;   // [nf] row of the membrane-facet table (MeshDev::mf), -1 off the membrane: what knp_surf_create selects by
    int* halo_ctr = nullptr;       // [KNP_HALO_CTR_INTS] block counters of the persistent halo-staged applies (apply_p1_halo.hpp)
    int halo_flip[2] = {0, 0};
    double* rho = nullptr;         // [nc]
    double* fsrc = nullptr;        // [n_sys][nc] DG0 source on ECS cells, or null
    // manufactured-solution mode (splitting == 2): constant coupling coefficients + host-integrated data terms
    double* mms_C = nullptr;       // [n_sys][nc]
    double* extra_emi = nullptr;   // [nc*nd]
    double* extra_knp = nullptr;   // [n_sys][nc*nd]
    SourceState* src = nullptr;    // device-evaluated ion sources writing rows of extra_knp (source.hip; created by the first call that needs it)
    OdeState* ode = nullptr;       // ode.hip (knp_ode_create / knp_ode_register)
    RecState* rec = nullptr;       // record.hip (knp_rec_create)
    GridState* grid = nullptr;     // grid.hip (knp_grid_create)
    SurfState* surf = nullptr;     // surface.hip (knp_surf_create)
    FieldMeshState* fieldmesh = nullptr;   // fieldmesh.hip (knp_fieldmesh_create)
    CkptState* ckpt = nullptr;     // state.hip (knp_state_cell_order / knp_state_save / knp_state_load)
    RingUState* ring_u = nullptr;  // apply_ring_u.hip (ring_u_cells)
    // launch caches of the persistent applies: what the context's device answered, asked once per context
    int ncu = 256;                 // compute units of the device (knp_ctx_create; 256 when the query fails)
    std::map<const void*, size_t> lds_granted;                        // kernel -> dynamic LDS granted to it (ring_common.hpp: grant_lds)
    std::map<std::pair<const void*, size_t>, int> halo_wg_per_cu;     // (kernel, LDS bytes) -> occupancy answer (apply_p1_halo.hpp: halo_grid)
    // DG-p (p >= 2) path: tabulated rules + assembled cell blocks [nc][dim+2][nd][nd] (tab_rhs.hip, tab_assembled.hip)
    TabRule tab[KNP_TAB_COUNT];
    double* tab_mem[KNP_TAB_COUNT] = {nullptr};
    double* blk_emi = nullptr;
    double* blk_knp = nullptr;     // [n_sys] x the same
    std::map<int, double*> vecs;   // handle -> device pointer
    std::map<int, int64_t> vlen;
    int next_handle = 1;
    // Krylov workspace
    double* partial = nullptr;     // [grid][KNP_MAX_SYS][KNP_MAX_RED]
    int64_t partial_blocks = 0;
    // status and scal are views into ONE device allocation (the status block: status words | Krylov scalars ...), so that a look
    // fetches the status words and the systems' scalar rows with one copy (krylov.hip: status_look)
    double* scal = nullptr;        // device scalars
    int* status = nullptr;         // device: per system {converged flag, iterations}, then the ODE failure flag and the Peclet word
    void* pinned = nullptr;        // host pinned mirror of the head of the status block: status words | scalar rows
    long long host_round_trips = 0;   // blocking waits of the host on the device made through this context (knp_host_round_trips)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    int emi_dg_cheb = -1;          // DG-level Chebyshev step of the EMI preconditioner: -1 default (on for degree 1), 0 / 1 (knp_set_emi_dg_smoother)
    int knp_krylov = 0;            // KNP Krylov method: 0 BiCGStab (default), 1 restarted GMRES (knp_set_knp_krylov)
    int gm_restart = 30;
    double* gm_V = nullptr;        // GMRES basis, allocated at the first GMRES solve
    int gm_alloc = 0;              // basis vectors allocated
    int last_it_emi = 0, last_it_knp = 0;   // iteration counts of the previous solves (chunking of the status polls)
    double knp_early = 0.0;                 // knp_knp_early_stop: a residual this factor under the tolerance ends a BiCGStab solve before min_it
    float last_peclet = -1.0f;              // cell Peclet number of the drift seen by the last status poll (< 0: not read yet)
    // auxiliary-space AMG hierarchies: [0] EMI, [1 + k] KNP species k
    std::vector<AmgHierarchy> amg;
    std::vector<hipStream_t> aux_streams;   // one per extra KNP species: their V-cycles run concurrently
    std::vector<hipEvent_t> aux_events;
    hipEvent_t fork_event = nullptr;
    // distributed
    void* comm = nullptr;          // ncclComm_t: reductions + serial halo exchanges, on the context's stream
    void* comm_halo = nullptr;     // ncclComm_t of the overlapped halo exchanges, on halo_stream
    void* shm = nullptr;           // host-staged shared-memory communicator (comm.hip: knp_comm_init_shm), instead of RCCL
    hipStream_t halo_stream = nullptr;
    hipEvent_t halo_ready = nullptr, halo_done = nullptr;
    int rank = 0, nranks = 1;
    bool dist = false;             // communicator active: halo exchanges + all-reduced reductions
    std::vector<int> halo_peer;
    std::vector<int64_t> halo_send_off, halo_send_cnt, halo_recv_off, halo_recv_cnt;
    int32_t* halo_send_idx = nullptr;   // device: owned cell ids to pack, grouped by peer
    double* halo_sendbuf = nullptr;
    int64_t halo_send_total = 0;
    // row-distributed finest conforming level (amg_vcycle.hip: dist0; knp_amg_interface): the conforming dofs this rank shares with peers.
    // The list of one peer is the same on both sides (ascending global dof), so message p is sent and received with one layout
    std::vector<int> if_peer;
    std::vector<int64_t> if_off, if_cnt;
    int64_t if_total = 0, if_nuniq = 0;
    int32_t* if_idx = nullptr;      // device [if_total]: local conforming dof of every message position, grouped by peer
    int32_t* if_uvtx = nullptr;     // device [if_nuniq]: the distinct shared dofs
    int32_t* if_aptr = nullptr;     // device [if_nuniq + 1]: CSR over if_asrc
    int32_t* if_asrc = nullptr;     // device: message positions of the dof's other owners in ascending rank order, -1 = this rank's own value
    double *if_send = nullptr, *if_recv = nullptr;   // device [if_total * KNP_MAX_SYS]
    // optional in-solver timing of the operator applies (knp_apply_timing): event pairs recorded around every launch
    bool time_applies = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> tev[2];   // [0] EMI, [1] KNP
    size_t tev_used[2] = {0, 0};
    std::string err;
    Fields fields;
};

#define HIPCHK(ctx, call)                                                        \
    do {                                                                         \
        hipError_t e_ = (call);                                                  \
        if (e_ != hipSuccess) {                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);      \
            return -2;                                                           \
        }                                                                        \
    } while (0)

// scalars of the KNP operator, by value into the apply kernels
struct KnpArgs {
    int ns;
    double inv_dt, psi, tau;
    double z[KNP_MAX_SYS];
};
// closed-form P1 facet integrals: mass / triple-product entries of a (D-1)-simplex
template <int D> struct FacetConst;
template <> struct FacetConst<3> { static constexpr double mass = 1.0 / 12.0, trip = 1.0 / 60.0; };
template <> struct FacetConst<2> { static constexpr double mass = 1.0 / 6.0, trip = 1.0 / 24.0; };

// integer / on-off environment knobs.  Both read the environment on every call (tests switch some knobs inside one process); a site
// that wants its value fixed for the process keeps it in a static of its own
inline int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}
inline bool env_flag(const char* name, bool dflt) { return env_int(name, dflt ? 1 : 0) != 0; }

// every blocking wait of the host goes through one of these three, which count it (knp_ctx::host_round_trips)
inline hipError_t host_stream_sync(knp_ctx* c, hipStream_t s) { ++c->host_round_trips; return hipStreamSynchronize(s); }
inline hipError_t host_event_sync(knp_ctx* c, hipEvent_t e) { ++c->host_round_trips; return hipEventSynchronize(e); }
inline hipError_t host_memcpy(knp_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
    ++c->host_round_trips;
    return hipMemcpy(dst, src, bytes, kind);
}

inline int chk_field(knp_ctx* c, int field) {
    if (!c) return -1;
    if (field < 0 || field >= KNP_F_COUNT) { c->err = "unknown field id"; return -1; }
    return 0;
}
// device array and length of a field of the public ABI, or null for an unknown id
inline double* knp_field_ptr(knp_ctx* c, int field, int64_t* n) {
    if (!c || field < 0 || field >= KNP_F_COUNT) return nullptr;
    if (n) *n = c->fields.n[field];
    return c->fields.f[field];
}

// A runtime-compiled code object onto the context's current device: its module and the named kernel, or -2 with the module unloaded
// again (ode.hip: membrane models, source.hip: ion sources; `who` names the caller in the error text)
inline int rtc_load_kernel(knp_ctx* c, const char* who, const void* code, const char* kernel_name, hipModule_t* mod_out, hipFunction_t* fn_out) {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    HIPCHK(c, hipModuleLoadData(&mod, code));            // reads the ELF's own size
    const hipError_t e = hipModuleGetFunction(&fn, mod, kernel_name);
    if (e != hipSuccess) {
        hipModuleUnload(mod);
        c->err = std::string(who) + ": kernel " + kernel_name + " not in the code object: " + hipGetErrorString(e);
        return -2;
    }
    *mod_out = mod;
    *fn_out = fn;
    return 0;
}

inline int64_t grid_for(int64_t n) { return (n + KNP_BLOCK - 1) / KNP_BLOCK; }

// KERN<3> or KERN<2> by the mesh dimension, KNP_BLOCK threads per block
#define DISPATCH_DIM(c, KERN, grid, ...)                                                         \
    do {                                                                                         \
        if ((c)->m.dim == 3) hipLaunchKernelGGL(KERN<3>, grid, dim3(KNP_BLOCK), 0, (c)->stream, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERN<2>, grid, dim3(KNP_BLOCK), 0, (c)->stream, __VA_ARGS__);    \
        HIPCHK(c, hipGetLastError());                                                            \
    } while (0)

// f(std::integral_constant<int, NS>) for NS = n_sys in 1..MAXNS, the kernel instances the caller has; -1 for any other count
template <int MAXNS, typename F> int dispatch_nsys(int n_sys, F&& f) {
    static_assert(MAXNS >= 1 && MAXNS <= 4, "instances exist for at most four solved species");
    if (n_sys == 1) return f(std::integral_constant<int, 1>());
    if constexpr (MAXNS >= 2) if (n_sys == 2) return f(std::integral_constant<int, 2>());
    if constexpr (MAXNS >= 3) if (n_sys == 3) return f(std::integral_constant<int, 3>());
    if constexpr (MAXNS >= 4) if (n_sys == 4) return f(std::integral_constant<int, 4>());
    return -1;
}

// ---- launchers implemented in the .hip files --------------------------------------------
int launch_emi_apply(knp_ctx* c, const double* x, const double* kappa, double* y);
int launch_knp_apply(knp_ctx* c, const double* x, const double* dnphi, double* y);
int launch_emi_blockjacobi(knp_ctx* c, const double* kappa, bjreal* binv);
int launch_knp_blockjacobi(knp_ctx* c, const double* dnphi, bjreal* binv);
int launch_dnphi(knp_ctx* c, const double* phi, double* dnphi);
int launch_neighbour_materials(knp_ctx* c);
int apply_variant(knp_ctx* c, int which);
int launch_kappa(knp_ctx* c, const double* cc, const double* celim, double* kappa);
int launch_emi_rhs(knp_ctx* c, const double* cc, const double* celim, const double* phiM,
                   const double* Ich, double* b);
int launch_knp_rhs(knp_ctx* c, const double* cc, const double* cprev, const double* celim,
                   const double* phi, const double* phiM, const double* Ich, double* b);
int launch_step_updates(knp_ctx* c, const double* cc, double* celim, const double* phi,
                        double* phiM, double* E);
int launch_facet_trace(knp_ctx* c, const double* nodal, int side, double* out);

// DG-p path, p >= 2: what every step needs (tab_rhs.hip: nodal coefficient fields, right-hand sides, membrane-facet updates over the
// tabulated rules of knp_set_tabulation) ...
int tab_kappa(knp_ctx* c, const double* cc, const double* celim, double* kappa);
int tab_emi_rhs(knp_ctx* c, const double* cc, const double* celim, const double* phiM, const double* Ich, double* b);
int tab_knp_rhs(knp_ctx* c, const double* cc, const double* cprev, const double* celim, const double* phi, const double* phiM,
                const double* Ich, double* b);
int tab_step_updates(knp_ctx* c, const double* cc, double* celim, const double* phi, double* phiM, double* E, bool do_celim);
int tab_facet_trace(knp_ctx* c, const double* nodal, int side, double* out);
void tab_free(knp_ctx* c);                              // the rules, and the blocks below
// ... and the assembled operator blocks of KNP_P2_ASSEMBLED=1 (tab_assembled.hip: A/B runs against the matrix-free applies only)
inline bool p2_assembled(const knp_ctx* c) { return c->p2_assembled; }   // KNP_P2_ASSEMBLED=1: round-1 path (quadrature-assembled cell blocks) instead of the matrix-free applies
int tab_assemble_emi(knp_ctx* c, const double* kappa);
int tab_assemble_knp(knp_ctx* c, const double* phi);
int tab_apply(knp_ctx* c, int which, const double* x, double* y);
int tab_block_inverse(knp_ctx* c, int which, bjreal* binv);
void tab_free_blocks(knp_ctx* c);

// what a P2 KNP operator kernel, matrix-free or assembling, takes from the parameters: one record, one filler
struct KnpOpArgs { double inv_dt, psi, tau; double z[KNP_MAX_SYS]; };
inline KnpOpArgs knp_op_args(const knp_ctx* c) {
    KnpOpArgs ka;
    ka.inv_dt = 1.0 / c->p.dt; ka.psi = c->p.psi; ka.tau = c->p.tau_knp;
    for (int k = 0; k < KNP_MAX_SYS; ++k) ka.z[k] = k < c->p.n_sys ? c->p.z[k] : 0.0;
    return ka;
}

// ring-staged P1 applies on structured 3D meshes (apply_ring.hip): loader wave + LDS-DMA ring + consumer waves
bool ring_usable(const knp_ctx* c, int which);       // which: 0 EMI, 1 KNP
// apply_ring_u.hip: the ring-staged applies for 3D P1 meshes WITHOUT geometry classes (geometry from staged vertex coordinates)
int64_t ring_u_cells(knp_ctx* c, int which);         // leading owned cells the unstructured ring covers (0: not usable); builds its tables once
void ring_u_free(knp_ctx* c);
int64_t ring_u_debug_table(knp_ctx* c, int which, const void** p, int64_t meta[4]);   // KNP_DT_RU_*: bytes (0: no usable ring), device pointer or meta
int ring_u_emi_apply(knp_ctx* c, const MeshDev& m, const double* x, const double* kappa, double* y, int reserve_cus);
int ring_u_knp_apply(knp_ctx* c, const MeshDev& m, const double* x, const double* gphi, double* y, const KnpArgs& ka, int reserve_cus);
int ring_emi_apply(knp_ctx* c, const MeshDev& m, const double* x, const double* kappa, double* y, int reserve_cus);
int ring_knp_apply(knp_ctx* c, const MeshDev& m, const double* x, const double* gphi, double* y, const KnpArgs& ka, int reserve_cus);

// matrix-free DG-P2 applies and their cell-diagonal block inverses (apply_p2.hip; its device pieces: p2_frame.hpp)
int p2_emi_apply(knp_ctx* c, const double* x, const double* kappa, double* y);
int p2_knp_apply(knp_ctx* c, const double* x, const double* phi, double* y);
int p2_block_inverse(knp_ctx* c, int which, const double* coef, bjreal* binv);

int halo_exchange(knp_ctx* c, double* v, int nfields);
// y = A x on the owned cells with the halo exchange of x folded in (which: 0 = EMI, 1 = KNP): without a communicator a plain
// launch; with one, interior cells are computed while the exchange is in flight on the halo stream / communicator (comm.hip)
int dist_apply(knp_ctx* c, int which, double* x, const double* coef, double* y);

int launch_nernst_only(knp_ctx* c, const double* cc, const double* celim, double* E);
void comm_destroy(knp_ctx* c);
int allreduce_red(knp_ctx* c, double* red, int count);
int allreduce_max(knp_ctx* c, double* host_value);
int allreduce_max_word(knp_ctx* c, int* dev_word);                 // max of a float-bits status word over the ranks, on the solver's stream
int allreduce_sum_host(knp_ctx* c, double* host_values, int n);    // sum of n <= 56 host values over the ranks (synchronous)
int allreduce_array(knp_ctx* c, double* dev, int64_t n);           // in-place sum of a device array of any length over the ranks (stream S)
// v [ncol / nil][n][nil] holds per-rank partial sums at the shared conforming dofs: afterwards every owner holds the full sum
// (same bits on every owner: added in rank order).  On the context's stream; 2 messages per peer (comm.hip)
int interface_accumulate(knp_ctx* c, double* v, int64_t n, int ncol);
int max_abs_diff(knp_ctx* c, const double* a, const double* b, int nsys, double* out);
// ---- checkpoint (state.hip): every source file lists the step-to-step state it owns as blocks [ncomp][count][width]
struct StateBlk {
    int id = 0, kind = 0, type = 0, ncomp = 1;    // knp_state_kind / knp_state_type (include/knpemi_hip.h)
    int64_t count = 0, width = 1;
    void* dev = nullptr;                           // device array, or null: host values
    std::vector<char> host;                        // host values as they are now (what a save writes)
    void (*apply)(knp_ctx*, int id, const char* data) = nullptr;   // host values: takes a loaded block
};
int fields_state_blocks(knp_ctx* c, std::vector<StateBlk>& out);   // solve.hip: fields, solution histories, lagged inverses, counters
int fields_state_prepare_load(knp_ctx* c);                         // solve.hip: builds what a first solve would build over restored arrays
int ode_state_blocks(knp_ctx* c, std::vector<StateBlk>& out);      // ode.hip: state / parameter tables and step sizes of every model
int rec_state_blocks(knp_ctx* c, std::vector<StateBlk>& out);      // record.hip: ring, row counter, map accumulators
void state_destroy(knp_ctx* c);                                    // state.hip: staging buffers of the context
const int32_t* state_cell_rank(knp_ctx* c);                        // state.hip: device [nc] caller's cell id -> device cell, or null = identity
template <typename T> inline void state_push_host(StateBlk& b, const T* v, int64_t n) {
    b.count = n;
    b.host.assign((const char*)v, (const char*)v + sizeof(T) * (size_t)n);
}

void ode_destroy_all(knp_ctx* c);   // ode.hip: frees the context's membrane models and runtime-compiled kernels
void rec_destroy(knp_ctx* c);       // record.hip: frees the context's time-series recorder, if any
void grid_destroy_all(knp_ctx* c);  // grid.hip: frees the context's voxel-grid samplers, if any
void surf_destroy_all(knp_ctx* c);  // surface.hip: frees the context's membrane-surface samplers, if any
void fieldmesh_destroy_all(knp_ctx* c);   // fieldmesh.hip: frees the context's volume-field samplers on the mesh, if any
void source_destroy(knp_ctx* c);    // source.hip: unloads the context's device-evaluated ion sources, frees their cell list and rule
bool source_registered(knp_ctx* c); // source.hip: some species has a device-evaluated source (knp_source_register)
int ode_check_failed(knp_ctx* c);   // ode.hip: reads and clears the ODE failure flag (stream idle); sets c->err
int status_look(knp_ctx* c);        // krylov.hip: head of the status block -> c->pinned, one copy and one stream wait
int sync_check_ode(knp_ctx* c);     // ode.hip: waits for the stream and checks the ODE failure flag (0, -2 HIP error, -4 ODE failure)
