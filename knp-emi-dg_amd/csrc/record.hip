// Time-series recorder: point probes, membrane-set means and region integrals sampled on the device right after step III, so that
// a run without field output still yields the traces the reference's figure scripts read back from results.h5
// (examples/idealized-geometries/make_figures_3D.py:28-168).  One sample = one row of n_ch doubles + its time in a small device
// buffer; the row counter lives on the device, so a sample is four launches on the solver's stream (one more each for state
// channels and a membrane map) and no host synchronisation.
//
// Row layout:  [probe][phi, c_0 .. c_{n_sys-1}, c_elim]  |  [set][phi_M, E_0 .. E_{n_ions-1}, I_ch_0 .. I_ch_{n_ions-1}]  |
//              [region][int c_0 dx .. int c_{n_ions-1} dx, volume mean of phi]
//              | [set][state_0 .. state_{n_names-1}]   (only after knp_rec_add_states: area-weighted means of ODE state columns,
//              e.g. the gating variables n, m, h; behind the region block, so that every other offset stays where it is)
// Every sum runs in a fixed order (thread-strided partial sums -> wave shuffle -> LDS -> one value; no floating-point atomics), so
// two runs with the same inputs give the same bits.
//
// Timing of the state channels: the solver steps the membrane ODEs of step k before the PDE solves of step k, so the row sampled at
// the end of step k sees the states AFTER ODE step k -- the pairing the reference's saved fields have.
//
// Per-facet membrane map (knp_rec_add_map): persistent per selected facet -- previous phi_M, activation time (first upward crossing
// of the threshold, linearly interpolated between two samples), repolarisation time (first downward crossing after it), peak and
// its time, number of upward crossings.  One more launch per sample, a pure stream without reductions; read back on request only
// (knp_rec_map_read).
//
// Partition mode (knp_rec_create_part / knp_rec_add_states_part / knp_rec_add_map_part): every rank of a partitioned run holds the
// tables of what it OWNS -- a probe whose cell another rank owns has cell -1, a set or a state channel may be empty, the weights are the
// global ones and so sum to <= 1 per rank, inv_rvol comes from the caller (1 / GLOBAL region volume) -- and writes its partial row with
// the same kernels.  Nothing is communicated per sample.  knp_rec_read sums the waiting rows over the ranks in place (allreduce_array,
// comm.hip: one all-reduce of rows x n_ch doubles on the solver's stream); knp_rec_map_read spreads the rank's map arrays to their
// global positions in a staging buffer (k_rec_map_spread: exact zeros elsewhere, so an owner's NaN survives), sums that and copies it
// out once.  Still no floating-point atomics: the shm transport adds in rank order, so every rank reads the same bits.
//
// The recorder of a context is its RecState (knp_ctx::rec): created by knp_rec_create, freed by rec_destroy, shared with no other context.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>

bool ode_state_table(knp_ctx* c, int handle, const double** states, int64_t* n, int* ns);   // ode.hip

#define KNP_REC_MAX_REGIONS 16
#define KNP_REC_FINISH_BLOCK 1024

// knp_ctx::rec: the context's one recorder, created by knp_rec_create / knp_rec_create_part, freed by rec_destroy
struct RecState {
    int64_t capacity = 0, n_ch = 0, n_points = 0, n_sets = 0, n_blk = 0;
    int n_regions = 0;
    int64_t rows_host = 0;          // samples enqueued since the last read (the device counter reaches the same number)
    int32_t* point_cell = nullptr;  // [n_points]
    double* point_w = nullptr;      // [n_points][nd]
    int64_t* set_ptr = nullptr;     // [n_sets + 1]
    int32_t* set_facet = nullptr;
    double* set_w = nullptr;
    uint8_t* region = nullptr;      // [nc_owned], 255 = not counted
    double* vol = nullptr;          // [nc_owned]
    double* inv_rvol = nullptr;     // [n_regions] 1 / region volume
    double* partials = nullptr;     // [n_blk][n_regions][n_ions + 1]
    double* buf = nullptr;          // rows [capacity][n_ch], then t [capacity]
    int* count = nullptr;           // rows written since the last read
    std::vector<double> host;       // staging of one read
    // state channels (knp_rec_add_states), optional
    int64_t n_base = 0;             // channels of knp_rec_create; the state channels follow them in the row
    int64_t n_sch = 0;
    int64_t* st_ptr = nullptr;      // [n_sch + 1]
    const double** st_src = nullptr;   // per entry the address of its value in an ODE state table
    double* st_w = nullptr;
    // per-facet map (knp_rec_add_map), optional
    int64_t n_map = 0, map_k = 0;   // map_k: samples since arming; its parity names the slot of t_hist with the previous sample's time
    bool map_armed = false;
    double thr = 0.0, thr_r = 0.0;
    int32_t* map_facet = nullptr;   // [n_map]
    double* map_prev = nullptr;     // [n_map] phi_M at the previous sample
    double* map_out = nullptr;      // t_act, t_repol, peak, t_peak [4][n_map], then n_up int32 [n_map]: one block, one transfer
    double* t_hist = nullptr;       // [2] times of the last two samples, next to the row counter: sampling never synchronises
    std::vector<double> map_host;
    // partition mode
    bool part = false;
    int64_t n_map_glob = 0;         // entries of knp_rec_map_read's outputs (= n_map outside partition mode); non-zero = there is a map
    int32_t* map_src = nullptr;     // [n_map_glob] position in this rank's map arrays, -1 = another rank's facet
    double* map_stage = nullptr;    // [5][n_map_glob] t_act, t_repol, peak, t_peak, n_up as doubles
};

namespace {

struct RecFields {                  // nodal fields in row order: phi, c_0 .. c_{n_sys-1}, c_elim
    const double* f[KNP_MAX_IONS + 1];
};

__device__ __forceinline__ double rec_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

// sum over the block, valid in thread 0; lds holds blockDim.x / 64 doubles and may be reused after the call
__device__ __forceinline__ double rec_block_sum(double v, double* lds) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nw = blockDim.x >> 6;
    v = rec_wave_sum(v);
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double s = 0.0;
    if (threadIdx.x == 0) {
        s = lds[0];
        for (int w = 1; w < nw; ++w) s += lds[w];
    }
    __syncthreads();
    return s;
}

// one thread per (probe, field): value = sum_a w_a u[cell nd + a]
__global__ __launch_bounds__(64) void k_rec_points(int64_t n_points, int nfld, int nd, RecFields F, const int32_t* __restrict__ cell,
                                                   const double* __restrict__ w, const int* __restrict__ count, int64_t capacity,
                                                   int64_t n_ch, double* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = *count;
    if (i >= n_points * nfld || row >= capacity) return;
    const int64_t p = i / nfld;
    const int q = (int)(i - p * nfld);
    const int64_t cp = cell[p];
    double s = 0.0;
    if (cp >= 0) {                                     // -1 (partition mode): another rank's probe, an exact zero here
        const double* u = F.f[q] + cp * nd;
        const double* wp = w + p * nd;
        for (int a = 0; a < nd; ++a) s += wp[a] * u[a];
    }
    rows[row * n_ch + i] = s;
}

// one workgroup per membrane set: weighted means of PHI_M, E[k], I_CH[k]; the workgroup strides over the set's facets in list order
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_sets(int n_ions, int64_t nf, const double* __restrict__ phiM, const double* __restrict__ E,
                                                        const double* __restrict__ Ich, const int64_t* __restrict__ set_ptr,
                                                        const int32_t* __restrict__ facet, const double* __restrict__ w,
                                                        const int* __restrict__ count, int64_t capacity, int64_t n_ch, int64_t ch0,
                                                        double* __restrict__ rows) {
    __shared__ double lds[KNP_BLOCK / 64];
    const int64_t row = *count;
    if (row >= capacity) return;
    const int s = blockIdx.x, nq = 1 + 2 * n_ions;
    const int64_t lo = set_ptr[s], hi = set_ptr[s + 1];
    for (int q = 0; q < nq; ++q) {
        const double* fld = q == 0 ? phiM : (q <= n_ions ? E + (int64_t)(q - 1) * nf : Ich + (int64_t)(q - 1 - n_ions) * nf);
        double acc = 0.0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += KNP_BLOCK) acc += w[i] * fld[facet[i]];
        const double v = rec_block_sum(acc, lds);
        if (threadIdx.x == 0) rows[row * n_ch + ch0 + (int64_t)s * nq + q] = v;
    }
}

// nodal weights of the exact cell integral: P1 1/(d+1); P2 triangle 0 (vertices) and 1/3 (edges); P2 tetrahedron -1/20 and 1/5
template <int ND> __device__ __forceinline__ double rec_cell_mean(const double* __restrict__ u, int64_t c) {
    constexpr int NV = ND == 3 || ND == 6 ? 3 : 4;
    double v[ND];
    if constexpr (ND % 2 == 0) {
        const double2* q = reinterpret_cast<const double2*>(u + (int64_t)ND * c);
#pragma unroll
        for (int k = 0; k < ND / 2; ++k) { const double2 t = q[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
    } else {
#pragma unroll
        for (int k = 0; k < ND; ++k) v[k] = u[(int64_t)ND * c + k];
    }
    double sv = 0.0, se = 0.0;
#pragma unroll
    for (int k = 0; k < NV; ++k) sv += v[k];
#pragma unroll
    for (int k = NV; k < ND; ++k) se += v[k];
    if constexpr (ND == NV) return sv * (1.0 / NV);
    else if constexpr (ND == 6) return se * (1.0 / 3.0);
    else return se * 0.2 - sv * 0.05;
}

// stage 1 of the region integrals: per 256-cell block the sums of vol * cell mean per (region, quantity) -> partials[blk][region][q],
// q in the order of RecFields (phi, then the n_ions concentrations, eliminated ion last).  A wave that holds no cell of a region
// contributes an exact zero without the shuffles.
template <int ND>
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_regions(int64_t nc_owned, int n_regions, int nq, RecFields F, const uint8_t* __restrict__ region,
                                                           const double* __restrict__ vol, double* __restrict__ partials) {
    __shared__ double lds[KNP_BLOCK / 64][KNP_REC_MAX_REGIONS][KNP_MAX_IONS + 1];
    const int64_t c = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int r = 255;
    double val[KNP_MAX_IONS + 1];
#pragma unroll
    for (int q = 0; q <= KNP_MAX_IONS; ++q) val[q] = 0.0;
    if (c < nc_owned) {
        r = region[c];
        if (r != 255) {
            const double vc = vol[c];
#pragma unroll
            for (int q = 0; q <= KNP_MAX_IONS; ++q)
                if (q < nq) val[q] = vc * rec_cell_mean<ND>(F.f[q], c);
        }
    }
    for (int rr = 0; rr < n_regions; ++rr) {
        const bool mine = r == rr;
        const bool any = __ballot(mine) != 0ull;
#pragma unroll
        for (int q = 0; q <= KNP_MAX_IONS; ++q)
            if (q < nq) {
                double s = 0.0;
                if (any) s = rec_wave_sum(mine ? val[q] : 0.0);
                if (lane == 0) lds[wv][rr][q] = s;
            }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < n_regions * nq; j += KNP_BLOCK) {
        const int rr = j / nq, q = j - rr * nq;
        double s = lds[0][rr][q];
#pragma unroll
        for (int w = 1; w < KNP_BLOCK / 64; ++w) s += lds[w][rr][q];
        partials[(int64_t)blockIdx.x * n_regions * nq + j] = s;
    }
}

// stage 2 (one workgroup): every (region, quantity) partial column is summed in the fixed order of k_reduce (krylov.hip) -- thread t
// takes blocks t, t + 1024, ... in ascending order, then wave shuffle, then the waves in ascending order --, the row and its time are
// written and the row counter advances.  Runs for every sample, also without regions.
__global__ __launch_bounds__(KNP_REC_FINISH_BLOCK) void k_rec_finish(int64_t n_blk, int n_regions, int nq, const double* __restrict__ partials,
                                                                     const double* __restrict__ inv_rvol, double t, int* __restrict__ count,
                                                                     int64_t capacity, int64_t n_ch, int64_t ch0, double* __restrict__ rows,
                                                                     double* __restrict__ times) {
    __shared__ double lds[KNP_REC_FINISH_BLOCK / 64];
    const int64_t row = *count;
    if (row >= capacity) return;
    const int nout = n_regions * nq;
    for (int j = 0; j < nout; ++j) {
        double acc = 0.0;
        for (int64_t b0 = threadIdx.x; b0 < n_blk; b0 += 4 * KNP_REC_FINISH_BLOCK) {
            double v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int64_t b = b0 + (int64_t)u * KNP_REC_FINISH_BLOCK;
                v[u] = b < n_blk ? partials[b * nout + j] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += v[u];
        }
        const double s = rec_block_sum(acc, lds);
        if (threadIdx.x == 0) {
            // partial columns are in field order (phi first); the row holds the integrals of the ions, then the volume mean of phi
            const int rr = j / nq, q = j - rr * nq;
            rows[row * n_ch + ch0 + (int64_t)rr * nq + (q == 0 ? nq - 1 : q - 1)] = q == 0 ? s * inv_rvol[rr] : s;
        }
    }
    if (threadIdx.x == 0) {
        times[row] = t;
        *count = (int)row + 1;
    }
}

// one workgroup per state channel: sum_i w_i * (state value of entry i), the workgroup strides over the entries in list order
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_states(const int64_t* __restrict__ ptr, const double* const* __restrict__ src,
                                                          const double* __restrict__ w, const int* __restrict__ count, int64_t capacity,
                                                          int64_t n_ch, int64_t ch0, double* __restrict__ rows) {
    __shared__ double lds[KNP_BLOCK / 64];
    const int64_t row = *count;
    if (row >= capacity) return;
    const int s = blockIdx.x;
    const int64_t lo = ptr[s], hi = ptr[s + 1];
    double acc = 0.0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += KNP_BLOCK) acc += w[i] * *src[i];
    const double v = rec_block_sum(acc, lds);
    if (threadIdx.x == 0) rows[row * n_ch + ch0 + s] = v;
}

// arming of the map: prev = peak = phi_M now, t_peak = t0, no crossing seen yet
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_map_arm(int64_t n, const int32_t* __restrict__ facet, const double* __restrict__ phiM, double t0,
                                                           double* __restrict__ t_hist, double* __restrict__ prev, double* __restrict__ out,
                                                           int32_t* __restrict__ n_up) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double v = phiM[facet[i]], nan = __builtin_nan("");
    prev[i] = v;
    out[i] = nan; out[n + i] = nan; out[2 * n + i] = v; out[3 * n + i] = t0;
    n_up[i] = 0;
    if (i == 0) { t_hist[0] = t0; t_hist[1] = t0; }
}

// one thread per selected facet: crossings between the previous sample (v0 at t0) and this one (v1 at t1), peak, prev <- v1.
// t0 is read from t_hist[slot] and t1 goes to the other slot, which the next sample reads: no thread reads what another writes.
// A refused sample (buffer full) leaves everything as it is, prev included.
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_map(int64_t n, const int32_t* __restrict__ facet, const double* __restrict__ phiM, double thr,
                                                       double thr_r, double t1, double* __restrict__ t_hist, int slot,
                                                       const int* __restrict__ count, int64_t capacity, double* __restrict__ prev,
                                                       double* __restrict__ out, int32_t* __restrict__ n_up) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= n || *count >= capacity) return;
    const double t0 = t_hist[slot];
    if (i == 0) t_hist[slot ^ 1] = t1;
    const double v0 = prev[i], v1 = phiM[facet[i]];
    double ta = out[i];
    if (v0 < thr && v1 >= thr) {
        n_up[i] += 1;
        if (isnan(ta)) {
            ta = t0 + (thr - v0) / (v1 - v0) * (t1 - t0);
            out[i] = ta;
        }
    }
    if (!isnan(ta) && isnan(out[n + i]) && v0 >= thr_r && v1 < thr_r) out[n + i] = t0 + (thr_r - v0) / (v1 - v0) * (t1 - t0);
    if (v1 > out[2 * n + i]) { out[2 * n + i] = v1; out[3 * n + i] = t1; }
    prev[i] = v1;
}

// partition mode, at a read: one thread per GLOBAL map entry.  The rank's four double arrays and n_up (as a double) go to the global
// positions of the facets it owns, an exact 0.0 everywhere else; the sum over the ranks is then every owner's value, NaN included.
__global__ __launch_bounds__(KNP_BLOCK) void k_rec_map_spread(int64_t n_glob, int64_t n_loc, const int32_t* __restrict__ src,
                                                              const double* __restrict__ out, const int32_t* __restrict__ n_up,
                                                              double* __restrict__ stage) {
    const int64_t g = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (g >= n_glob) return;
    const int64_t j = src[g];
#pragma unroll
    for (int q = 0; q < 4; ++q) stage[q * n_glob + g] = j >= 0 ? out[q * n_loc + j] : 0.0;
    stage[4 * n_glob + g] = j >= 0 ? (double)n_up[j] : 0.0;
}

template <typename T> int rec_upload(knp_ctx* c, T** dst, const T* src, size_t n) {
    HIPCHK(c, hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) HIPCHK(c, host_memcpy(c, *dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

void rec_free(RecState& R) {
    hipFree(R.point_cell); hipFree(R.point_w); hipFree(R.set_ptr); hipFree(R.set_facet); hipFree(R.set_w); hipFree(R.region);
    hipFree(R.vol); hipFree(R.inv_rvol); hipFree(R.partials); hipFree(R.buf); hipFree(R.count);
    hipFree(R.st_ptr); hipFree(R.st_src); hipFree(R.st_w);
    hipFree(R.map_facet); hipFree(R.map_prev); hipFree(R.map_out); hipFree(R.t_hist);
    hipFree(R.map_src); hipFree(R.map_stage);
}

RecState* rec_find(knp_ctx* c, const char* who) {
    if (!c->rec) c->err = std::string(who) + ": no recorder (knp_rec_create)";
    return c->rec;
}

}  // namespace

// checkpoint (state.hip): the row buffer with its times, the device row counter, the map accumulators and the host-side counters.  The
// sizes carry the configuration (capacity, channels, map facets): a snapshot of another recorder does not load.  Block ids 2000 + q.
static void rec_apply_host(knp_ctx* c, int, const char* data) {
    if (!c->rec) return;
    int64_t v[3];
    memcpy(v, data, sizeof(v));
    c->rec->rows_host = v[0]; c->rec->map_k = v[1]; c->rec->map_armed = v[2] != 0;
}

int rec_state_blocks(knp_ctx* c, std::vector<StateBlk>& out) {
    if (!c->rec) return 0;
    RecState& R = *c->rec;
    auto push = [&](int id, int kind, int type, int ncomp, int64_t count, int64_t width, void* dev) {
        StateBlk b; b.id = id; b.kind = kind; b.type = type; b.ncomp = ncomp; b.count = count; b.width = width; b.dev = dev;
        out.push_back(b);
    };
    push(2000, KNP_SK_OPAQUE, KNP_ST_F64, 1, R.capacity, R.n_ch + 1, R.buf);       // [capacity][n_ch] rows, then [capacity] times
    push(2001, KNP_SK_OPAQUE, KNP_ST_I32, 1, 1, 1, R.count);
    if (R.n_map) {
        push(2002, KNP_SK_MEMBRANE_FACET, KNP_ST_F64, 1, R.n_map, 1, R.map_prev);
        push(2003, KNP_SK_MEMBRANE_FACET, KNP_ST_F64, 4, R.n_map, 1, R.map_out);
        push(2004, KNP_SK_MEMBRANE_FACET, KNP_ST_I32, 1, R.n_map, 1, R.map_out + 4 * R.n_map);
        push(2005, KNP_SK_OPAQUE, KNP_ST_F64, 1, 2, 1, R.t_hist);
    }
    const int64_t v[3] = {R.rows_host, R.map_k, R.map_armed ? 1 : 0};
    StateBlk b; b.id = 2006; b.kind = KNP_SK_OPAQUE; b.type = KNP_ST_I64; b.apply = rec_apply_host;
    state_push_host(b, v, 3);
    out.push_back(b);
    return 0;
}

void rec_destroy(knp_ctx* c) {
    if (!c->rec) return;
    host_stream_sync(c, c->stream);
    rec_free(*c->rec);
    delete c->rec;
    c->rec = nullptr;
}

// knp_rec_create (part = false: validation, uploads and launches as they always were) and knp_rec_create_part
static int rec_create(knp_ctx* c, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w, int64_t n_sets,
                      const int64_t* set_ptr, const int32_t* set_facet, const double* set_w, int n_regions, const uint8_t* region,
                      const double* vol, const double* inv_rvol, bool part) {
    if (!c) return -1;
    const MeshDev& m = c->m;
    const int nd = c->nd, n_ions = c->p.n_ions;
    // ---- validation: nothing below may ever index outside a field ----------------------------------------------------------
    if (capacity < 1 || capacity > (int64_t(1) << 24)) { c->err = "knp_rec_create: capacity out of range"; return -1; }
    if (n_points < 0 || n_sets < 0 || n_regions < 0) { c->err = "knp_rec_create: negative count"; return -1; }
    if (n_regions > KNP_REC_MAX_REGIONS) { c->err = "knp_rec_create: at most 16 regions"; return -1; }
    const bool sets_listed = n_sets && (!part || (set_ptr && set_ptr[n_sets] > 0));      // partition mode: every set may be empty here
    if ((n_points && (!point_cell || !point_w)) || (n_sets && !set_ptr) || (sets_listed && (!set_facet || !set_w)) ||
        (n_regions && (!region || !vol || (part && !inv_rvol)))) {
        c->err = "knp_rec_create: null table";
        return -1;
    }
    for (int64_t p = 0; p < n_points; ++p)
        if ((point_cell[p] < 0 && !(part && point_cell[p] == -1)) || point_cell[p] >= m.nc_owned) {
            c->err = "knp_rec_create: probe " + std::to_string(p) + " sits in cell " + std::to_string(point_cell[p]) + ", not an owned cell";
            return -1;
        }
    int64_t n_sf = 0;
    if (n_sets) {
        if (set_ptr[0] != 0) { c->err = "knp_rec_create: set_ptr must start at 0"; return -1; }
        for (int64_t s = 0; s < n_sets; ++s)
            if (part ? set_ptr[s + 1] < set_ptr[s] : set_ptr[s + 1] <= set_ptr[s]) {
                c->err = "knp_rec_create: membrane set " + std::to_string(s) + (part ? " has a negative length" : " is empty");
                return -1;
            }
        n_sf = set_ptr[n_sets];
        for (int64_t i = 0; i < n_sf; ++i)
            if (set_facet[i] < 0 || set_facet[i] >= m.nf || !c->h_mf_mask[(size_t)set_facet[i]]) {
                c->err = "knp_rec_create: facet " + std::to_string(set_facet[i]) + " is not a membrane facet";
                return -1;
            }
    }
    std::vector<double> rvol((size_t)n_regions, 0.0);
    if (n_regions) {
        for (int64_t k = 0; k < m.nc; ++k)
            if (region[k] != 255 && region[k] >= n_regions) {
                c->err = "knp_rec_create: cell " + std::to_string(k) + " has region id " + std::to_string((int)region[k]) + " >= n_regions";
                return -1;
            }
        if (part) {                                    // 1 / GLOBAL region volume: the ranks' partial means add up
            for (int r = 0; r < n_regions; ++r) {
                if (!(inv_rvol[r] >= 0.0) || !std::isfinite(inv_rvol[r])) {
                    c->err = "knp_rec_create: inv_rvol of region " + std::to_string(r) + " must be finite and not negative";
                    return -1;
                }
                rvol[(size_t)r] = inv_rvol[r];
            }
        } else {
            for (int64_t k = 0; k < m.nc_owned; ++k)
                if (region[k] != 255) rvol[region[k]] += vol[k];
            for (int r = 0; r < n_regions; ++r) rvol[(size_t)r] = rvol[(size_t)r] > 0.0 ? 1.0 / rvol[(size_t)r] : 0.0;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    rec_destroy(c);                                    // one recorder per context: a second create replaces the first

    RecState R;
    R.capacity = capacity; R.n_points = n_points; R.n_sets = n_sets; R.n_regions = n_regions; R.part = part;
    R.n_ch = n_points * (n_ions + 1) + n_sets * (1 + 2 * n_ions) + (int64_t)n_regions * (n_ions + 1);
    R.n_base = R.n_ch;
    R.n_blk = n_regions ? (m.nc_owned + KNP_BLOCK - 1) / KNP_BLOCK : 0;
    int rc = 0;
    rc |= rec_upload(c, &R.point_cell, point_cell, (size_t)n_points);
    rc |= rec_upload(c, &R.point_w, point_w, (size_t)n_points * nd);
    rc |= rec_upload(c, &R.set_ptr, set_ptr, n_sets ? (size_t)n_sets + 1 : 0);
    rc |= rec_upload(c, &R.set_facet, set_facet, (size_t)n_sf);
    rc |= rec_upload(c, &R.set_w, set_w, (size_t)n_sf);
    rc |= rec_upload(c, &R.region, region, n_regions ? (size_t)m.nc_owned : 0);
    rc |= rec_upload(c, &R.vol, vol, n_regions ? (size_t)m.nc_owned : 0);
    rc |= rec_upload(c, &R.inv_rvol, rvol.data(), (size_t)n_regions);
    if (!rc && hipMalloc((void**)&R.partials, sizeof(double) * std::max<size_t>((size_t)R.n_blk * n_regions * (n_ions + 1), 1)) != hipSuccess) rc = -2;
    const size_t nbuf = (size_t)capacity * (size_t)(R.n_ch + 1);
    if (!rc && hipMalloc((void**)&R.buf, sizeof(double) * nbuf) != hipSuccess) rc = -2;
    if (!rc && hipMalloc((void**)&R.count, sizeof(int)) != hipSuccess) rc = -2;
    if (!rc && (hipMemset(R.buf, 0, sizeof(double) * nbuf) != hipSuccess || hipMemset(R.count, 0, sizeof(int)) != hipSuccess)) rc = -2;
    if (rc) {
        rec_free(R);
        if (c->err.empty()) c->err = "knp_rec_create: device allocation failed";
        return -2;
    }
    R.host.resize(nbuf);
    c->rec = new RecState(R);
    return 0;
}

static int rec_add_states(knp_ctx* c, int64_t n_channels, const int64_t* chan_ptr, const int32_t* entry_handle, const int64_t* entry_row,
                          const int32_t* entry_col, const double* entry_w, bool part) {
    if (!c) return -1;
    RecState* Rp = rec_find(c, "knp_rec_add_states");
    if (!Rp) return -1;
    RecState& R = *Rp;
    if (part != R.part) { c->err = "knp_rec_add_states: the recorder was created in the other mode (knp_rec_create / knp_rec_create_part)"; return -1; }
    // ---- validation, all of it before the first upload: no entry may address anything outside its state table ------------------
    if (R.rows_host) { c->err = "knp_rec_add_states: samples are waiting (call it right after knp_rec_create)"; return -1; }
    if (n_channels < 1 || n_channels > (int64_t(1) << 20)) { c->err = "knp_rec_add_states: channel count out of range"; return -1; }
    if (!chan_ptr) { c->err = "knp_rec_add_states: null table"; return -1; }
    if (chan_ptr[0] != 0) { c->err = "knp_rec_add_states: chan_ptr must start at 0"; return -1; }
    for (int64_t s = 0; s < n_channels; ++s)
        if (part ? chan_ptr[s + 1] < chan_ptr[s] : chan_ptr[s + 1] <= chan_ptr[s]) {
            c->err = "knp_rec_add_states: channel " + std::to_string(s) + (part ? " has a negative length" : " is empty");
            return -1;
        }
    const int64_t ne = chan_ptr[n_channels];
    if ((ne || !part) && (!entry_handle || !entry_row || !entry_col || !entry_w)) { c->err = "knp_rec_add_states: null table"; return -1; }
    std::vector<const double*> src((size_t)ne);
    for (int64_t s = 0; s < n_channels; ++s) {
        double wsum = 0.0;
        for (int64_t i = chan_ptr[s]; i < chan_ptr[s + 1]; ++i) {
            const double* tab = nullptr;
            int64_t n = 0;
            int ns = 0;
            const std::string where = "knp_rec_add_states: channel " + std::to_string(s) + ", entry " + std::to_string(i - chan_ptr[s]) + ": ";
            if (!ode_state_table(c, entry_handle[i], &tab, &n, &ns)) { c->err = where + "unknown ODE handle " + std::to_string(entry_handle[i]); return -1; }
            if (entry_row[i] < 0 || entry_row[i] >= n) {
                c->err = where + "row " + std::to_string(entry_row[i]) + " outside the handle's " + std::to_string(n) + " rows";
                return -1;
            }
            if (entry_col[i] < 0 || entry_col[i] >= ns) {
                c->err = where + "column " + std::to_string(entry_col[i]) + " outside the handle's " + std::to_string(ns) + " states";
                return -1;
            }
            src[(size_t)i] = tab + entry_row[i] * ns + entry_col[i];
            wsum += entry_w[i];
            if (part && !(entry_w[i] >= 0.0)) { c->err = where + "negative weight"; return -1; }
        }
        // partition mode: the weights are those of the global channel, of which this rank holds a part
        if (part && !(wsum <= 1.0 + 1e-12)) { c->err = "knp_rec_add_states: the weights of channel " + std::to_string(s) + " sum to more than 1"; return -1; }
        if (!part && !(std::fabs(wsum - 1.0) <= 1e-12)) { c->err = "knp_rec_add_states: the weights of channel " + std::to_string(s) + " do not sum to 1"; return -1; }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, host_stream_sync(c, c->stream));        // nothing may still write into the row buffer that is replaced below
    int64_t* d_ptr = nullptr;
    const double** d_src = nullptr;
    double *d_w = nullptr, *d_buf = nullptr;
    const int64_t n_ch = R.n_base + n_channels;
    const size_t nbuf = (size_t)R.capacity * (size_t)(n_ch + 1);
    int rc = 0;
    rc |= rec_upload(c, &d_ptr, chan_ptr, (size_t)n_channels + 1);
    rc |= rec_upload(c, &d_src, src.data(), (size_t)ne);
    rc |= rec_upload(c, &d_w, entry_w, (size_t)ne);
    if (!rc && (hipMalloc((void**)&d_buf, sizeof(double) * nbuf) != hipSuccess || hipMemset(d_buf, 0, sizeof(double) * nbuf) != hipSuccess)) rc = -2;
    if (rc) {
        hipFree(d_ptr); hipFree(d_src); hipFree(d_w); hipFree(d_buf);
        if (c->err.empty()) c->err = "knp_rec_add_states: device allocation failed";
        return -2;
    }
    hipFree(R.st_ptr); hipFree(R.st_src); hipFree(R.st_w); hipFree(R.buf);        // a second call replaces the first
    R.st_ptr = d_ptr; R.st_src = d_src; R.st_w = d_w; R.buf = d_buf;
    R.n_sch = n_channels;
    R.n_ch = n_ch;
    R.host.assign(nbuf, 0.0);
    return 0;
}

// knp_rec_add_map (part = false, n_glob = n) and knp_rec_add_map_part: n facets of this rank, facet i at position pos[i] of the
// n_glob entries that knp_rec_map_read returns
static int rec_add_map(knp_ctx* c, int64_t n_glob, int64_t n, const int32_t* facets, const int64_t* pos, double threshold, double repolarisation,
                       bool part) {
    if (!c) return -1;
    RecState* Rp = rec_find(c, "knp_rec_add_map");
    if (!Rp) return -1;
    RecState& R = *Rp;
    if (part != R.part) { c->err = "knp_rec_add_map: the recorder was created in the other mode (knp_rec_create / knp_rec_create_part)"; return -1; }
    if (part ? (n_glob < 1 || n < 0 || n > n_glob || (n && (!facets || !pos))) : (n < 1 || !facets)) { c->err = "knp_rec_add_map: empty facet selection"; return -1; }
    if (n_glob > (int64_t(1) << 30)) { c->err = "knp_rec_add_map: too many facets"; return -1; }
    if (!std::isfinite(threshold) || !std::isfinite(repolarisation)) { c->err = "knp_rec_add_map: thresholds must be finite"; return -1; }
    for (int64_t i = 0; i < n; ++i)
        if (facets[i] < 0 || facets[i] >= c->m.nf || !c->h_mf_mask[(size_t)facets[i]]) {
            c->err = "knp_rec_add_map: facet " + std::to_string(facets[i]) + " is not a membrane facet";
            return -1;
        }
    std::vector<int32_t> src;
    if (part) {
        src.assign((size_t)n_glob, -1);
        for (int64_t i = 0; i < n; ++i) {
            if (pos[i] < 0 || pos[i] >= n_glob || src[(size_t)pos[i]] >= 0) {
                c->err = "knp_rec_add_map: position " + std::to_string(pos[i]) + " of facet " + std::to_string(facets[i]) + " is outside the map or taken twice";
                return -1;
            }
            src[(size_t)pos[i]] = (int32_t)i;
        }
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, host_stream_sync(c, c->stream));
    const size_t na = (size_t)std::max<int64_t>(n, 1);     // a rank may own no facet of the map
    int32_t *d_facet = nullptr, *d_src = nullptr;
    double *d_prev = nullptr, *d_out = nullptr, *d_t = nullptr, *d_stage = nullptr;
    int rc = rec_upload(c, &d_facet, facets, (size_t)n);
    if (!rc && (hipMalloc((void**)&d_prev, sizeof(double) * na) != hipSuccess ||
                hipMalloc((void**)&d_out, (4 * sizeof(double) + sizeof(int32_t)) * na) != hipSuccess ||
                hipMalloc((void**)&d_t, 2 * sizeof(double)) != hipSuccess)) rc = -2;
    if (!rc && part) {
        rc = rec_upload(c, &d_src, src.data(), (size_t)n_glob);
        if (!rc && hipMalloc((void**)&d_stage, 5 * sizeof(double) * (size_t)n_glob) != hipSuccess) rc = -2;
    }
    if (rc) {
        hipFree(d_facet); hipFree(d_prev); hipFree(d_out); hipFree(d_t); hipFree(d_src); hipFree(d_stage);
        if (c->err.empty()) c->err = "knp_rec_add_map: device allocation failed";
        return -2;
    }
    hipFree(R.map_facet); hipFree(R.map_prev); hipFree(R.map_out); hipFree(R.t_hist); hipFree(R.map_src); hipFree(R.map_stage);
    R.map_facet = d_facet; R.map_prev = d_prev; R.map_out = d_out; R.t_hist = d_t; R.map_src = d_src; R.map_stage = d_stage;
    R.n_map = n; R.n_map_glob = n_glob; R.map_k = 0; R.map_armed = false;
    R.thr = threshold; R.thr_r = repolarisation;
    R.map_host.assign(part ? (size_t)(5 * n_glob) : (size_t)(4 * n + (n + 1) / 2), 0.0);
    return 0;
}

extern "C" {

int knp_rec_create(knp_ctx* c, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w, int64_t n_sets,
                   const int64_t* set_ptr, const int32_t* set_facet, const double* set_w, int n_regions, const uint8_t* region,
                   const double* vol) {
    return rec_create(c, capacity, n_points, point_cell, point_w, n_sets, set_ptr, set_facet, set_w, n_regions, region, vol, nullptr, false);
}

int knp_rec_create_part(knp_ctx* c, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w, int64_t n_sets,
                        const int64_t* set_ptr, const int32_t* set_facet, const double* set_w, int n_regions, const uint8_t* region,
                        const double* vol, const double* inv_rvol) {
    return rec_create(c, capacity, n_points, point_cell, point_w, n_sets, set_ptr, set_facet, set_w, n_regions, region, vol, inv_rvol, true);
}

int knp_rec_add_states(knp_ctx* c, int64_t n_channels, const int64_t* chan_ptr, const int32_t* entry_handle, const int64_t* entry_row,
                       const int32_t* entry_col, const double* entry_w) {
    return rec_add_states(c, n_channels, chan_ptr, entry_handle, entry_row, entry_col, entry_w, false);
}

int knp_rec_add_states_part(knp_ctx* c, int64_t n_channels, const int64_t* chan_ptr, const int32_t* entry_handle, const int64_t* entry_row,
                            const int32_t* entry_col, const double* entry_w) {
    return rec_add_states(c, n_channels, chan_ptr, entry_handle, entry_row, entry_col, entry_w, true);
}

int knp_rec_add_map(knp_ctx* c, int64_t n, const int32_t* facets, double threshold, double repolarisation) {
    return rec_add_map(c, n, n, facets, nullptr, threshold, repolarisation, false);
}

int knp_rec_add_map_part(knp_ctx* c, int64_t n_global, int64_t n, const int32_t* facets, const int64_t* positions, double threshold,
                         double repolarisation) {
    return rec_add_map(c, n_global, n, facets, positions, threshold, repolarisation, true);
}

int knp_rec_map_arm(knp_ctx* c, double t0) {
    if (!c) return -1;
    RecState* Rp = rec_find(c, "knp_rec_map_arm");
    if (!Rp) return -1;
    RecState& R = *Rp;
    if (!R.n_map_glob) { c->err = "knp_rec_map_arm: no map (knp_rec_add_map)"; return -1; }
    if (!std::isfinite(t0)) { c->err = "knp_rec_map_arm: the time must be finite"; return -1; }
    if (R.n_map)                                       // (partition mode: a rank may own no facet of the map)
        hipLaunchKernelGGL(k_rec_map_arm, dim3((unsigned)((R.n_map + KNP_BLOCK - 1) / KNP_BLOCK)), dim3(KNP_BLOCK), 0, c->stream, R.n_map, R.map_facet,
                           knp_field_ptr(c, KNP_F_PHI_M, nullptr), t0, R.t_hist, R.map_prev, R.map_out, reinterpret_cast<int32_t*>(R.map_out + 4 * R.n_map));
    HIPCHK(c, hipGetLastError());
    R.map_k = 0;
    R.map_armed = true;
    return 0;
}

int knp_rec_map_read(knp_ctx* c, int64_t n, double* t_act, double* t_repol, double* peak, double* t_peak, int32_t* n_up) {
    if (!c) return -1;
    RecState* Rp = rec_find(c, "knp_rec_map_read");
    if (!Rp) return -1;
    RecState& R = *Rp;
    if (!R.n_map_glob) { c->err = "knp_rec_map_read: no map (knp_rec_add_map)"; return -1; }
    if (!R.map_armed) { c->err = "knp_rec_map_read: the map is not armed (knp_rec_map_arm)"; return -1; }
    if (n != R.n_map_glob || !t_act || !t_repol || !peak || !t_peak || !n_up) { c->err = "knp_rec_map_read: outputs must hold one entry per map facet"; return -1; }
    const size_t nn = (size_t)n;
    if (R.part) {
        // every rank's arrays at their global positions, zeros elsewhere; summed over the ranks; one copy.  Collective.
        hipLaunchKernelGGL(k_rec_map_spread, dim3((unsigned)((n + KNP_BLOCK - 1) / KNP_BLOCK)), dim3(KNP_BLOCK), 0, c->stream, n, R.n_map,
                           R.map_src, R.map_out, reinterpret_cast<const int32_t*>(R.map_out + 4 * R.n_map), R.map_stage);
        HIPCHK(c, hipGetLastError());
        int rc = allreduce_array(c, R.map_stage, 5 * n);
        if (rc) return rc;
        HIPCHK(c, host_stream_sync(c, c->stream));
        HIPCHK(c, host_memcpy(c, R.map_host.data(), R.map_stage, 5 * sizeof(double) * nn, hipMemcpyDeviceToHost));
        const double* h = R.map_host.data();
        std::memcpy(t_act, h, sizeof(double) * nn);
        std::memcpy(t_repol, h + nn, sizeof(double) * nn);
        std::memcpy(peak, h + 2 * nn, sizeof(double) * nn);
        std::memcpy(t_peak, h + 3 * nn, sizeof(double) * nn);
        for (size_t i = 0; i < nn; ++i) n_up[i] = (int32_t)h[4 * nn + i];      // small whole numbers: exact
        return 0;
    }
    HIPCHK(c, host_stream_sync(c, c->stream));
    HIPCHK(c, host_memcpy(c, R.map_host.data(), R.map_out, (4 * sizeof(double) + sizeof(int32_t)) * nn, hipMemcpyDeviceToHost));
    const double* h = R.map_host.data();
    std::memcpy(t_act, h, sizeof(double) * nn);
    std::memcpy(t_repol, h + nn, sizeof(double) * nn);
    std::memcpy(peak, h + 2 * nn, sizeof(double) * nn);
    std::memcpy(t_peak, h + 3 * nn, sizeof(double) * nn);
    std::memcpy(n_up, h + 4 * nn, sizeof(int32_t) * nn);
    return 0;
}

int knp_rec_sample(knp_ctx* c, double t) {
    if (!c) return -1;
    RecState* Rp = rec_find(c, "knp_rec_sample");
    if (!Rp) return -1;
    RecState& R = *Rp;
    if (R.rows_host >= R.capacity) { c->err = "knp_rec_sample: buffer full (knp_rec_read empties it)"; return -5; }
    if (R.n_map_glob && !R.map_armed) { c->err = "knp_rec_sample: the membrane map is not armed (knp_rec_map_arm)"; return -1; }
    const MeshDev& m = c->m;
    const int n_ions = c->p.n_ions, n_sys = c->p.n_sys, nfld = n_ions + 1, nd = c->nd;
    const int64_t ndof = m.nc * nd;
    RecFields F;
    for (int q = 0; q <= KNP_MAX_IONS; ++q) F.f[q] = nullptr;
    const double* cc = knp_field_ptr(c, KNP_F_C, nullptr);
    F.f[0] = knp_field_ptr(c, KNP_F_PHI, nullptr);
    for (int k = 0; k < n_sys; ++k) F.f[1 + k] = cc + (int64_t)k * ndof;
    F.f[n_ions] = knp_field_ptr(c, KNP_F_C_ELIM, nullptr);
    double* rows = R.buf;
    double* times = R.buf + R.capacity * R.n_ch;
    if (R.n_points) {
        const int64_t n = R.n_points * nfld;
        hipLaunchKernelGGL(k_rec_points, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c->stream, R.n_points, nfld, nd, F, R.point_cell, R.point_w,
                           R.count, R.capacity, R.n_ch, rows);
    }
    const int64_t ch_sets = R.n_points * nfld, ch_reg = ch_sets + R.n_sets * (1 + 2 * n_ions);
    if (R.n_sets)
        hipLaunchKernelGGL(k_rec_sets, dim3((unsigned)R.n_sets), dim3(KNP_BLOCK), 0, c->stream, n_ions, m.nf, knp_field_ptr(c, KNP_F_PHI_M, nullptr),
                           knp_field_ptr(c, KNP_F_E, nullptr), knp_field_ptr(c, KNP_F_I_CH, nullptr), R.set_ptr, R.set_facet, R.set_w, R.count,
                           R.capacity, R.n_ch, ch_sets, rows);
    if (R.n_regions) {
        const dim3 g((unsigned)R.n_blk), b(KNP_BLOCK);
#define REC_REGIONS(ND_) hipLaunchKernelGGL(k_rec_regions<ND_>, g, b, 0, c->stream, m.nc_owned, R.n_regions, nfld, F, R.region, R.vol, R.partials)
        if (nd == 3) REC_REGIONS(3);
        else if (nd == 4) REC_REGIONS(4);
        else if (nd == 6) REC_REGIONS(6);
        else REC_REGIONS(10);
#undef REC_REGIONS
    }
    if (R.n_sch)
        hipLaunchKernelGGL(k_rec_states, dim3((unsigned)R.n_sch), dim3(KNP_BLOCK), 0, c->stream, R.st_ptr, R.st_src, R.st_w, R.count, R.capacity, R.n_ch,
                           R.n_base, rows);
    if (R.n_map_glob) {
        if (R.n_map)
            hipLaunchKernelGGL(k_rec_map, dim3((unsigned)((R.n_map + KNP_BLOCK - 1) / KNP_BLOCK)), dim3(KNP_BLOCK), 0, c->stream, R.n_map, R.map_facet,
                               knp_field_ptr(c, KNP_F_PHI_M, nullptr), R.thr, R.thr_r, t, R.t_hist, (int)(R.map_k & 1), R.count, R.capacity, R.map_prev,
                               R.map_out, reinterpret_cast<int32_t*>(R.map_out + 4 * R.n_map));
        ++R.map_k;
    }
    hipLaunchKernelGGL(k_rec_finish, dim3(1), dim3(KNP_REC_FINISH_BLOCK), 0, c->stream, R.n_blk, R.n_regions, nfld, R.partials, R.inv_rvol, t, R.count,
                       R.capacity, R.n_ch, ch_reg, rows, times);
    HIPCHK(c, hipGetLastError());
    ++R.rows_host;
    return 0;
}

int knp_rec_read(knp_ctx* c, int64_t* n_rows, double* t_out, double* rows_out) {
    if (!c || !n_rows) return -1;
    RecState* Rp = rec_find(c, "knp_rec_read");
    if (!Rp) return -1;
    RecState& R = *Rp;
    *n_rows = 0;
    if (R.rows_host > 0 && (!t_out || !rows_out)) { c->err = "knp_rec_read: null output"; return -1; }
    HIPCHK(c, host_stream_sync(c, c->stream));
    if (R.rows_host == 0) return 0;
    if (R.part && c->dist) {
        // partition mode: the waiting partial rows are summed over the ranks in place; every rank has taken the same number of samples,
        // so every rank reaches this call with the same length.  The times are the same everywhere and are not reduced.
        int rc = allreduce_array(c, R.buf, R.rows_host * R.n_ch);
        if (rc) return rc;
        HIPCHK(c, host_stream_sync(c, c->stream));
    }
    // one device-to-host copy: the rows and, behind them, their times
    HIPCHK(c, host_memcpy(c, R.host.data(), R.buf, sizeof(double) * R.host.size(), hipMemcpyDeviceToHost));
    const int64_t n = R.rows_host;
    std::memcpy(rows_out, R.host.data(), sizeof(double) * (size_t)(n * R.n_ch));
    std::memcpy(t_out, R.host.data() + R.capacity * R.n_ch, sizeof(double) * (size_t)n);
    HIPCHK(c, hipMemsetAsync(R.count, 0, sizeof(int), c->stream));
    R.rows_host = 0;
    *n_rows = n;
    return 0;
}

int64_t knp_rec_channels(knp_ctx* c) {
    if (!c) return -1;
    return c->rec ? c->rec->n_ch : -1;
}

int knp_rec_destroy(knp_ctx* c) {
    if (!c) return -1;
    hipSetDevice(c->device);
    rec_destroy(c);
    return 0;
}

}  // extern "C"
