// Time-series recorder: point probes, membrane-set means and region integrals sampled on the device right after step III, so that
// a run without field output still yields the traces the reference's figure scripts read back from results.h5
// (examples/idealized-geometries/make_figures_3D.py:28-168).  One sample = one row of n_ch doubles + its time in a small device
// buffer; the row counter lives on the device, so a sample is four launches on the solver's stream and no host synchronisation.
//
// Row layout:  [probe][phi, c_0 .. c_{n_sys-1}, c_elim]  |  [set][phi_M, E_0 .. E_{n_ions-1}, I_ch_0 .. I_ch_{n_ions-1}]  |
//              [region][int c_0 dx .. int c_{n_ions-1} dx, volume mean of phi]
// Every sum runs in a fixed order (thread-strided partial sums -> wave shuffle -> LDS -> one value; no floating-point atomics), so
// two runs with the same inputs give the same bits.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include <algorithm>
#include <cstring>

double* knp_field_ptr(knp_ctx* c, int field, int64_t* n);   // abi.hip

#define KNP_REC_MAX_REGIONS 16
#define KNP_REC_FINISH_BLOCK 1024

namespace {

struct Recorder {
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
};

std::map<knp_ctx*, Recorder> g_rec;

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
    const double* u = F.f[q] + (int64_t)cell[p] * nd;
    const double* wp = w + p * nd;
    double s = 0.0;
    for (int a = 0; a < nd; ++a) s += wp[a] * u[a];
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

template <typename T> int rec_upload(knp_ctx* c, T** dst, const T* src, size_t n) {
    HIPCHK(c, hipMalloc((void**)dst, std::max<size_t>(n, 1) * sizeof(T)));
    if (n) HIPCHK(c, hipMemcpy(*dst, src, n * sizeof(T), hipMemcpyHostToDevice));
    return 0;
}

void rec_free(Recorder& R) {
    hipFree(R.point_cell); hipFree(R.point_w); hipFree(R.set_ptr); hipFree(R.set_facet); hipFree(R.set_w); hipFree(R.region);
    hipFree(R.vol); hipFree(R.inv_rvol); hipFree(R.partials); hipFree(R.buf); hipFree(R.count);
}

}  // namespace

void rec_destroy(knp_ctx* c) {
    auto it = g_rec.find(c);
    if (it == g_rec.end()) return;
    hipStreamSynchronize(c->stream);
    rec_free(it->second);
    g_rec.erase(it);
}

extern "C" {

int knp_rec_create(knp_ctx* c, int64_t capacity, int64_t n_points, const int32_t* point_cell, const double* point_w, int64_t n_sets,
                   const int64_t* set_ptr, const int32_t* set_facet, const double* set_w, int n_regions, const uint8_t* region,
                   const double* vol) {
    if (!c) return -1;
    const MeshDev& m = c->m;
    const int nd = c->nd, n_ions = c->p.n_ions;
    // ---- validation: nothing below may ever index outside a field ----------------------------------------------------------
    if (capacity < 1 || capacity > (int64_t(1) << 24)) { c->err = "knp_rec_create: capacity out of range"; return -1; }
    if (n_points < 0 || n_sets < 0 || n_regions < 0) { c->err = "knp_rec_create: negative count"; return -1; }
    if (n_regions > KNP_REC_MAX_REGIONS) { c->err = "knp_rec_create: at most 16 regions"; return -1; }
    if ((n_points && (!point_cell || !point_w)) || (n_sets && (!set_ptr || !set_facet || !set_w)) || (n_regions && (!region || !vol))) {
        c->err = "knp_rec_create: null table";
        return -1;
    }
    for (int64_t p = 0; p < n_points; ++p)
        if (point_cell[p] < 0 || point_cell[p] >= m.nc_owned) {
            c->err = "knp_rec_create: probe " + std::to_string(p) + " sits in cell " + std::to_string(point_cell[p]) + ", not an owned cell";
            return -1;
        }
    int64_t n_sf = 0;
    if (n_sets) {
        if (set_ptr[0] != 0) { c->err = "knp_rec_create: set_ptr must start at 0"; return -1; }
        for (int64_t s = 0; s < n_sets; ++s)
            if (set_ptr[s + 1] <= set_ptr[s]) { c->err = "knp_rec_create: membrane set " + std::to_string(s) + " is empty"; return -1; }
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
        for (int64_t k = 0; k < m.nc_owned; ++k)
            if (region[k] != 255) rvol[region[k]] += vol[k];
        for (int r = 0; r < n_regions; ++r) rvol[(size_t)r] = rvol[(size_t)r] > 0.0 ? 1.0 / rvol[(size_t)r] : 0.0;
    }
    HIPCHK(c, hipSetDevice(c->device));
    rec_destroy(c);                                    // one recorder per context: a second create replaces the first

    Recorder R;
    R.capacity = capacity; R.n_points = n_points; R.n_sets = n_sets; R.n_regions = n_regions;
    R.n_ch = n_points * (n_ions + 1) + n_sets * (1 + 2 * n_ions) + (int64_t)n_regions * (n_ions + 1);
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
    g_rec[c] = R;
    return 0;
}

int knp_rec_sample(knp_ctx* c, double t) {
    if (!c) return -1;
    auto it = g_rec.find(c);
    if (it == g_rec.end()) { c->err = "knp_rec_sample: no recorder (knp_rec_create)"; return -1; }
    Recorder& R = it->second;
    if (R.rows_host >= R.capacity) { c->err = "knp_rec_sample: buffer full (knp_rec_read empties it)"; return -5; }
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
    hipLaunchKernelGGL(k_rec_finish, dim3(1), dim3(KNP_REC_FINISH_BLOCK), 0, c->stream, R.n_blk, R.n_regions, nfld, R.partials, R.inv_rvol, t, R.count,
                       R.capacity, R.n_ch, ch_reg, rows, times);
    HIPCHK(c, hipGetLastError());
    ++R.rows_host;
    return 0;
}

int knp_rec_read(knp_ctx* c, int64_t* n_rows, double* t_out, double* rows_out) {
    if (!c || !n_rows) return -1;
    auto it = g_rec.find(c);
    if (it == g_rec.end()) { c->err = "knp_rec_read: no recorder (knp_rec_create)"; return -1; }
    Recorder& R = it->second;
    *n_rows = 0;
    if (R.rows_host > 0 && (!t_out || !rows_out)) { c->err = "knp_rec_read: null output"; return -1; }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (R.rows_host == 0) return 0;
    // one device-to-host copy: the rows and, behind them, their times
    HIPCHK(c, hipMemcpy(R.host.data(), R.buf, sizeof(double) * R.host.size(), hipMemcpyDeviceToHost));
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
    auto it = g_rec.find(c);
    return it == g_rec.end() ? -1 : it->second.n_ch;
}

int knp_rec_destroy(knp_ctx* c) {
    if (!c) return -1;
    hipSetDevice(c->device);
    rec_destroy(c);
    return 0;
}

}  // extern "C"
