// Fields sampled on a regular voxel grid: the view between the recorder's handful of probes (record.hip) and the download of every
// DoF on the unstructured mesh.  A grid is lo[d], h[d], shape[d]; point i along axis k is lo[k] + i h[k] (one rounding for the
// product, one for the sum: what numpy computes for the host path, knpemidg/grid.py).  A frame is [n_fields][nz][ny][nx].
//
// Two one-time kernels and one (two with derived quantities) per frame:
//   k_grid_locate   one thread per cell, in the CALLER's numbering (the device cell follows from the permutation of
//                   knp_state_cell_order): the grid indices inside the cell's bounding box, padded as recorder.locate_points pads it,
//                   are tested with the barycentric coordinates in fp64; where min lambda >= -tol the thread does an integer
//                   atomicMin of its caller's id into owner[point].  The minimum of integers does not depend on the order of
//                   arrival: of several cells that contain a point the lowest caller's id wins, whatever order the device keeps.
//                   A grid finer than the mesh makes the per-thread loops uneven; accepted for a pass that runs once.
//   k_grid_weights  one thread per point: the owner's device cell (-1 outside), its subdomain tag and the d+1 barycentric
//                   coordinates, recomputed with the arithmetic of the locate pass.
//   k_grid_sample   one thread per point, consecutive threads on consecutive x: cell and lambda are read once (4 + 8 (d+1) bytes),
//                   the basis weights are formed in registers (P1: lambda; P2: vertices lambda_a (2 lambda_a - 1), edges (a, b), a < b,
//                   4 lambda_a lambda_b, the local dof order of knp_set_tabulation) and the loop over the selected fields runs
//                   inside the thread: nd gathered doubles in, 8 (or 4) bytes out per field and point; NaN where no cell owns the point.
//   k_grid_sample_derived   only for a grid with derived quantities, after k_grid_sample: -grad phi, the ion fluxes and the current
//                   density in the owner cell, d component planes per quantity behind the nodal planes (see the kernel).
// The barycentric arithmetic of the first two uses explicitly rounded products and sums (no contraction into FMAs), so the host
// path reproduces owners and lambda bit for bit.
//
// Frames land in one of two pinned host buffers: kernel, asynchronous copy and an event on the context's stream;
// knp_grid_fetch waits for that event only (frame_pipe.hpp, shared with surface.hip).  The grid holds no step-to-step state: it
// adds no checkpoint block.
// The grids of a context and its uploaded tag table are its GridState (knp_ctx::grid): created with the first grid, freed by
// grid_destroy_all, shared with no other context.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "frame_pipe.hpp"
#include <cmath>
#include <cstring>

#define KNP_GRID_MAX 8              // grids per context
#define KNP_GRID_MAX_TAGS 8         // subdomain tags of one filter
#define KNP_GRID_NONE 0x7f7f7f7f    // owner[] before the locate pass (what a byte-wise memset can write); above every cell id

namespace {

struct GridGeom {                   // by value into the kernels
    double lo[3], h[3];
    int64_t n[3];
};
struct GridTags {
    int n;
    uint32_t t[KNP_GRID_MAX_TAGS];
};
struct GridFields {                 // the selected nodal fields, in the order of the frame
    int n;
    const double* f[KNP_MAX_IONS + 1];
};

#define KNP_GD_MAX (2 * KNP_MAX_IONS + 2)   // derived quantities of one grid: efield, current, a flux and a diffusive flux per ion
struct GridDerived {                // the selected derived quantities, in the order of the frame; by value into k_grid_sample_derived
    int n, n_ions;
    unsigned ions;                  // bit k: ion k's value, gradient and D are needed (every ion when `current` is selected)
    int kind[KNP_GD_MAX], ion[KNP_GD_MAX];
    const double* phi;
    const double* conc[KNP_MAX_IONS];   // nodal concentrations, the eliminated ion last
    const double* D;                // [n_ions][nc]
    int64_t nc;
    double z[KNP_MAX_IONS], psi, F;
};

struct Grid {
    int dim = 0, n_fields = 0, n_derived = 0;
    bool f32 = false;
    int64_t npts = 0;
    GridGeom G;
    int field[KNP_MAX_IONS + 1] = {0};
    int kind[KNP_GD_MAX] = {0}, ion[KNP_GD_MAX] = {0};
    int32_t* owner = nullptr;       // [npts] caller's cell id, -1 outside
    int32_t* cell = nullptr;        // [npts] device cell, -1 outside
    int32_t* tag = nullptr;         // [npts] subdomain tag of the owner, -1 outside
    double* lam = nullptr;          // [dim + 1][npts]
    FramePipe pipe;                 // frame [planes()][npts]: the nodal planes, then dim component planes (x first) per derived quantity
    float locate_ms = 0.f, weights_ms = 0.f;
    int planes() const { return n_fields + dim * n_derived; }
    size_t frame_bytes() const { return (size_t)planes() * (size_t)npts * (f32 ? 4 : 8); }
};

}  // namespace

// knp_ctx::grid: created by the first knp_grid_create that passes validation and allocation, freed by grid_destroy_all
struct GridState {
    Grid* g[KNP_GRID_MAX] = {nullptr};
    uint32_t* ctag = nullptr;       // device [nc]: the context's subdomain table, uploaded with the first grid
};

namespace {

// ---- arithmetic shared by the locate and the weights pass: every product and sum rounded on its own -------------------------------
__device__ __forceinline__ double g_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double g_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double g_sub(double a, double b) { return __dsub_rn(a, b); }
__device__ __forceinline__ double grid_coord(const GridGeom& G, int k, int64_t i) { return g_add(G.lo[k], g_mul((double)i, G.h[k])); }

// x0 and the rows c_j of the adjugate of the edge matrix: lambda_j = ((p - x0) . c_j) / det, j = 1 .. D; lambda_0 = 1 - sum
template <int D> struct CellGeo {
    double x0[D], c[D][D], det;
    double lo[D], hi[D];            // padded bounding box
};

// the vertices of device cell dc
template <int D>
__device__ __forceinline__ void grid_cell_vertices(const double* __restrict__ coords, const int32_t* __restrict__ cells, int64_t dc, double (&x)[D + 1][D]) {
    constexpr int CS = D == 3 ? 4 : 2;
#pragma unroll
    for (int a = 0; a <= D; ++a) {
        const double* xv = coords + (int64_t)cells[dc * (D + 1) + a] * CS;
#pragma unroll
        for (int k = 0; k < D; ++k) x[a][k] = xv[k];
    }
}

// the adjugate rows c_j of the edge matrix e_j = x_j - x_0 and its determinant: the one statement of them that the locate pass, the
// weights pass and the derived quantities (grad lambda_j = c_j / det) share
template <int D>
__device__ __forceinline__ void grid_adjugate(const double (&x)[D + 1][D], double (&c)[D][D], double& det) {
    double e[D][D];
#pragma unroll
    for (int j = 0; j < D; ++j)
#pragma unroll
        for (int k = 0; k < D; ++k) e[j][k] = g_sub(x[j + 1][k], x[0][k]);
    if constexpr (D == 2) {
        c[0][0] = e[1][1]; c[0][1] = -e[1][0];
        c[1][0] = -e[0][1]; c[1][1] = e[0][0];
        det = g_add(g_mul(e[0][0], c[0][0]), g_mul(e[0][1], c[0][1]));
    } else {
        // c_1 = e_2 x e_3, c_2 = e_3 x e_1, c_3 = e_1 x e_2
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const double* a = e[(j + 1) % 3];
            const double* b = e[(j + 2) % 3];
            c[j][0] = g_sub(g_mul(a[1], b[2]), g_mul(a[2], b[1]));
            c[j][1] = g_sub(g_mul(a[2], b[0]), g_mul(a[0], b[2]));
            c[j][2] = g_sub(g_mul(a[0], b[1]), g_mul(a[1], b[0]));
        }
        det = g_add(g_add(g_mul(e[0][0], c[0][0]), g_mul(e[0][1], c[0][1])), g_mul(e[0][2], c[0][2]));
    }
}

template <int D>
__device__ __forceinline__ void grid_cell_geo(const double* __restrict__ coords, const int32_t* __restrict__ cells, int64_t dc, CellGeo<D>& K) {
    double x[D + 1][D];
    grid_cell_vertices<D>(coords, cells, dc, x);
    grid_adjugate<D>(x, K.c, K.det);
    double ext = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        double lo = x[0][k], hi = x[0][k];
#pragma unroll
        for (int a = 1; a <= D; ++a) { lo = fmin(lo, x[a][k]); hi = fmax(hi, x[a][k]); }
        K.x0[k] = x[0][k]; K.lo[k] = lo; K.hi[k] = hi;
        ext = fmax(ext, g_sub(hi, lo));
    }
    const double pad = g_mul(1.0e-9, ext);             // prefilter only; the barycentric test decides
#pragma unroll
    for (int k = 0; k < D; ++k) { K.lo[k] = g_sub(K.lo[k], pad); K.hi[k] = g_add(K.hi[k], pad); }
}

// lam[0 .. D] of point p; returns the smallest
template <int D> __device__ __forceinline__ double grid_bary(const CellGeo<D>& K, const double* p, double* lam) {
    double r[D];
#pragma unroll
    for (int k = 0; k < D; ++k) r[k] = g_sub(p[k], K.x0[k]);
    double sum = 0.0, mn;
#pragma unroll
    for (int j = 0; j < D; ++j) {
        double s = g_mul(r[0], K.c[j][0]);
#pragma unroll
        for (int k = 1; k < D; ++k) s = g_add(s, g_mul(r[k], K.c[j][k]));
        lam[j + 1] = __ddiv_rn(s, K.det);
        sum = j == 0 ? lam[1] : g_add(sum, lam[j + 1]);
    }
    lam[0] = g_sub(1.0, sum);
    mn = lam[0];
#pragma unroll
    for (int j = 1; j <= D; ++j) mn = fmin(mn, lam[j]);
    return mn;
}

__device__ __forceinline__ bool grid_tag_ok(const GridTags& T, uint32_t t) {
    if (!T.n) return true;
    bool ok = false;
    for (int q = 0; q < T.n; ++q) ok |= T.t[q] == t;
    return ok;
}

// [i0, i1] of the grid indices along axis k that can lie in [lo, hi]: one index of slack on both sides, the exact test follows per point
__device__ __forceinline__ bool grid_range(const GridGeom& G, int k, double lo, double hi, int64_t& i0, int64_t& i1) {
    const int64_t n = G.n[k];
    if (n == 1) { i0 = i1 = 0; return true; }
    const double a = floor((lo - G.lo[k]) / G.h[k]) - 1.0, b = ceil((hi - G.lo[k]) / G.h[k]) + 1.0;
    if (!(a <= (double)(n - 1)) || !(b >= 0.0)) return false;
    i0 = a > 0.0 ? (int64_t)a : 0;
    i1 = b < (double)(n - 1) ? (int64_t)b : n - 1;
    return i0 <= i1;
}

template <int D>
__global__ __launch_bounds__(KNP_BLOCK) void k_grid_locate(int64_t nc, const double* __restrict__ coords, const int32_t* __restrict__ cells,
                                                           const int32_t* __restrict__ rank, const uint32_t* __restrict__ ctag, GridTags T,
                                                           GridGeom G, double tol, int32_t* __restrict__ owner) {
    const int64_t id = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;      // caller's cell id
    if (id >= nc) return;
    const int64_t dc = rank ? (int64_t)rank[id] : id;
    if (!grid_tag_ok(T, ctag[dc])) return;
    CellGeo<D> K;
    grid_cell_geo<D>(coords, cells, dc, K);
    int64_t i0[3] = {0, 0, 0}, i1[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < D; ++k)
        if (!grid_range(G, k, K.lo[k], K.hi[k], i0[k], i1[k])) return;
    double p[3], lam[D + 1];
    for (int64_t iz = i0[2]; iz <= i1[2]; ++iz) {
        if constexpr (D == 3) {
            p[2] = grid_coord(G, 2, iz);
            if (!(p[2] >= K.lo[2] && p[2] <= K.hi[2])) continue;
        }
        for (int64_t iy = i0[1]; iy <= i1[1]; ++iy) {
            p[1] = grid_coord(G, 1, iy);
            if (!(p[1] >= K.lo[1] && p[1] <= K.hi[1])) continue;
            const int64_t row = D == 3 ? (iz * G.n[1] + iy) * G.n[0] : iy * G.n[0];
            for (int64_t ix = i0[0]; ix <= i1[0]; ++ix) {
                p[0] = grid_coord(G, 0, ix);
                if (!(p[0] >= K.lo[0] && p[0] <= K.hi[0])) continue;
                if (grid_bary<D>(K, p, lam) >= -tol) atomicMin(&owner[row + ix], (int32_t)id);
            }
        }
    }
}

template <int D>
__global__ __launch_bounds__(KNP_BLOCK) void k_grid_weights(int64_t npts, const double* __restrict__ coords, const int32_t* __restrict__ cells,
                                                            const int32_t* __restrict__ rank, const uint32_t* __restrict__ ctag, GridGeom G,
                                                            int32_t* __restrict__ owner, int32_t* __restrict__ cell, int32_t* __restrict__ tag,
                                                            double* __restrict__ lam_out) {
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= npts) return;
    const int32_t id = owner[i];
    if (id == KNP_GRID_NONE) {
        owner[i] = -1; cell[i] = -1; tag[i] = -1;
#pragma unroll
        for (int a = 0; a <= D; ++a) lam_out[(int64_t)a * npts + i] = 0.0;
        return;
    }
    const int64_t dc = rank ? (int64_t)rank[id] : (int64_t)id;
    CellGeo<D> K;
    grid_cell_geo<D>(coords, cells, dc, K);
    double p[D], lam[D + 1];
    int64_t rem = i;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        const int64_t q = rem / G.n[k];
        p[k] = grid_coord(G, k, rem - q * G.n[k]);
        rem = q;
    }
    grid_bary<D>(K, p, lam);
    cell[i] = (int32_t)dc;
    tag[i] = (int32_t)ctag[dc];
#pragma unroll
    for (int a = 0; a <= D; ++a) lam_out[(int64_t)a * npts + i] = lam[a];
}

template <int D, int P, typename OUT>
__global__ __launch_bounds__(KNP_BLOCK) void k_grid_sample(int64_t npts, const int32_t* __restrict__ cell, const double* __restrict__ lam,
                                                           GridFields F, OUT* __restrict__ out) {
    constexpr int NV = D + 1, ND = P == 1 ? NV : NV * (NV + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= npts) return;
    const int64_t c = cell[i];
    if (c < 0) {
        for (int q = 0; q < F.n; ++q) out[(int64_t)q * npts + i] = (OUT)__builtin_nan("");
        return;
    }
    double l[NV], w[ND];
#pragma unroll
    for (int a = 0; a < NV; ++a) l[a] = lam[(int64_t)a * npts + i];
    if constexpr (P == 1) {
#pragma unroll
        for (int a = 0; a < NV; ++a) w[a] = l[a];
    } else {
        int e = NV;
#pragma unroll
        for (int a = 0; a < NV; ++a) w[a] = l[a] * (2.0 * l[a] - 1.0);
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
            for (int b = a + 1; b < NV; ++b) w[e++] = 4.0 * l[a] * l[b];
    }
    for (int q = 0; q < F.n; ++q) {
        const double* __restrict__ u = F.f[q] + c * ND;
        double s = 0.0;
#pragma unroll
        for (int a = 0; a < ND; ++a) s += w[a] * u[a];
        out[(int64_t)q * npts + i] = (OUT)s;
    }
}

template <int D, int P, typename OUT> void sample_launch(knp_ctx* c, const Grid& g, const GridFields& F) {
    hipLaunchKernelGGL((k_grid_sample<D, P, OUT>), dim3((unsigned)grid_for(g.npts)), dim3(KNP_BLOCK), 0, c->stream, g.npts, g.cell, g.lam, F,
                       (OUT*)g.pipe.frame);
}
template <int D, int P> void sample_type(knp_ctx* c, const Grid& g, const GridFields& F) {
    if (g.f32) sample_launch<D, P, float>(c, g, F);
    else sample_launch<D, P, double>(c, g, F);
}

// value (when VALUE) and gradient of the nodal function u[ND] at the point: sum_a u_a w_a and sum_a u_a grad w_a
template <int D, int ND, bool VALUE>
__device__ __forceinline__ double grid_value_grad(const double* __restrict__ u, const double (&w)[ND], const double (&dw)[ND][D], double (&g)[D]) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) g[k] = 0.0;
#pragma unroll
    for (int a = 0; a < ND; ++a) {
        const double ua = u[a];
        if constexpr (VALUE) s += w[a] * ua;
#pragma unroll
        for (int k = 0; k < D; ++k) g[k] += ua * dw[a][k];
    }
    return s;
}

template <int D, typename OUT>
__device__ __forceinline__ void grid_store_vector(OUT* __restrict__ out, int64_t npts, int64_t i, int q, const double (&v)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) out[((int64_t)q * D + k) * npts + i] = (OUT)v[k];
}

// Electric field, ion fluxes and current density in the owner cell, one thread per point, consecutive threads on consecutive x.
// cell and lambda are read once; the adjugate rows and det are rebuilt from the owner's vertices (grid_adjugate: 4 gathers that
// neighbouring points share, against 8 d d more table bytes per point and frame); grad lambda_j = c_j / det, grad lambda_0 = -sum;
// the basis values w and gradients dw (P1: grad lambda_a; P2: vertices (4 lambda_a - 1) grad lambda_a, edges (a, b)
// 4 (lambda_b grad lambda_a + lambda_a grad lambda_b)) are formed once in registers, then grad phi, then the loop over the ions
// the selected quantities need: value, gradient, D of the owner, J_k = -D_k grad c_k - z_k D_k psi c_k grad phi; `current`
// accumulates F z_k J_k in the same loop.  out: the planes behind the grid's nodal planes, [quantity][component][npts].
template <int D, int P, typename OUT>
__global__ __launch_bounds__(KNP_BLOCK) void k_grid_sample_derived(int64_t npts, const int32_t* __restrict__ cell, const double* __restrict__ lam,
                                                                   const double* __restrict__ coords, const int32_t* __restrict__ cells,
                                                                   GridDerived Q, OUT* __restrict__ out) {
    constexpr int NV = D + 1, ND = P == 1 ? NV : NV * (NV + 1) / 2;
    const int64_t i = (int64_t)blockIdx.x * KNP_BLOCK + threadIdx.x;
    if (i >= npts) return;
    const int64_t c = cell[i];
    if (c < 0) {
        for (int q = 0; q < Q.n * D; ++q) out[(int64_t)q * npts + i] = (OUT)__builtin_nan("");
        return;
    }
    double l[NV], gl[NV][D], w[ND], dw[ND][D];
#pragma unroll
    for (int a = 0; a < NV; ++a) l[a] = lam[(int64_t)a * npts + i];
    {
        double x[NV][D], adj[D][D], det;
        grid_cell_vertices<D>(coords, cells, c, x);
        grid_adjugate<D>(x, adj, det);
        const double inv = 1.0 / det;
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < D; ++j) { gl[j + 1][k] = adj[j][k] * inv; s += gl[j + 1][k]; }
            gl[0][k] = -s;
        }
    }
    if constexpr (P == 1) {
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            w[a] = l[a];
#pragma unroll
            for (int k = 0; k < D; ++k) dw[a][k] = gl[a][k];
        }
    } else {
        int e = NV;
#pragma unroll
        for (int a = 0; a < NV; ++a) {
            w[a] = l[a] * (2.0 * l[a] - 1.0);
#pragma unroll
            for (int k = 0; k < D; ++k) dw[a][k] = (4.0 * l[a] - 1.0) * gl[a][k];
        }
#pragma unroll
        for (int a = 0; a < NV; ++a)
#pragma unroll
            for (int b = a + 1; b < NV; ++b) {
                w[e] = 4.0 * l[a] * l[b];
#pragma unroll
                for (int k = 0; k < D; ++k) dw[e][k] = 4.0 * (l[b] * gl[a][k] + l[a] * gl[b][k]);
                ++e;
            }
    }
    double gphi[D], cur[D], v[D];
    grid_value_grad<D, ND, false>(Q.phi + c * ND, w, dw, gphi);
#pragma unroll
    for (int k = 0; k < D; ++k) { cur[k] = 0.0; v[k] = -gphi[k]; }
    for (int q = 0; q < Q.n; ++q)
        if (Q.kind[q] == KNP_GD_EFIELD) grid_store_vector<D>(out, npts, i, q, v);
    for (int s = 0; s < Q.n_ions; ++s) {
        if (!(Q.ions >> s & 1u)) continue;
        double gc[D], diff[D], flux[D];
        const double cs = grid_value_grad<D, ND, true>(Q.conc[s] + c * ND, w, dw, gc);
        const double Ds = Q.D[(int64_t)s * Q.nc + c], drift = Q.z[s] * Ds * Q.psi * cs, fz = Q.F * Q.z[s];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            diff[k] = -Ds * gc[k];
            flux[k] = diff[k] - drift * gphi[k];
            cur[k] += fz * flux[k];
        }
        for (int q = 0; q < Q.n; ++q) {
            if (Q.ion[q] != s) continue;
            if (Q.kind[q] == KNP_GD_FLUX) grid_store_vector<D>(out, npts, i, q, flux);
            else if (Q.kind[q] == KNP_GD_FLUX_DIFFUSIVE) grid_store_vector<D>(out, npts, i, q, diff);
        }
    }
    for (int q = 0; q < Q.n; ++q)
        if (Q.kind[q] == KNP_GD_CURRENT) grid_store_vector<D>(out, npts, i, q, cur);
}

template <int D, int P, typename OUT> void derived_launch(knp_ctx* c, const Grid& g, const GridDerived& Q) {
    hipLaunchKernelGGL((k_grid_sample_derived<D, P, OUT>), dim3((unsigned)grid_for(g.npts)), dim3(KNP_BLOCK), 0, c->stream, g.npts, g.cell, g.lam,
                       c->m.coords, c->m.cells, Q, (OUT*)g.pipe.frame + (int64_t)g.n_fields * g.npts);
}
template <int D, int P> void derived_type(knp_ctx* c, const Grid& g, const GridDerived& Q) {
    if (g.f32) derived_launch<D, P, float>(c, g, Q);
    else derived_launch<D, P, double>(c, g, Q);
}

void grid_free(Grid* g) {
    if (!g) return;
    hipFree(g->owner); hipFree(g->cell); hipFree(g->tag); hipFree(g->lam);
    g->pipe.release();
    delete g;
}

Grid* grid_find(knp_ctx* c, int handle, const char* who) {
    if (!c->grid || handle < 0 || handle >= KNP_GRID_MAX || !c->grid->g[handle]) {
        c->err = std::string(who) + ": no grid with handle " + std::to_string(handle) + " (knp_grid_create)";
        return nullptr;
    }
    return c->grid->g[handle];
}

}  // namespace

void grid_destroy_all(knp_ctx* c) {
    if (!c->grid) return;
    host_stream_sync(c, c->stream);
    for (Grid* g : c->grid->g) grid_free(g);
    hipFree(c->grid->ctag);
    delete c->grid;
    c->grid = nullptr;
}

extern "C" {

int knp_grid_create(knp_ctx* c, const double* lo, const double* h, const int64_t* shape, double tol, int n_tags, const uint32_t* tags,
                    int n_fields, const int32_t* fields, int f32) {
    return knp_grid_create_derived(c, lo, h, shape, tol, n_tags, tags, n_fields, fields, 0, nullptr, nullptr, f32);
}

int knp_grid_create_derived(knp_ctx* c, const double* lo, const double* h, const int64_t* shape, double tol, int n_tags, const uint32_t* tags,
                            int n_fields, const int32_t* fields, int n_derived, const int32_t* kind, const int32_t* ion, int f32) {
    if (!c) return -1;
    const MeshDev& m = c->m;
    const int d = m.dim, n_ions = c->p.n_ions;
    // ---- everything is validated before anything is allocated or uploaded ------------------------------------------------------
    if (c->dist || c->nranks > 1 || m.nc_owned != m.nc) {
        c->err = "knp_grid_create: not supported with several ranks (a partitioned context holds a part of the mesh)";
        return -7;
    }
    if (!lo || !h || !shape || (n_tags && !tags) || (n_fields > 0 && !fields) || (n_derived > 0 && (!kind || !ion))) {
        c->err = "knp_grid_create: null argument";
        return -1;
    }
    double npts = 1.0;
    for (int k = 0; k < d; ++k) {
        if (!std::isfinite(lo[k]) || !std::isfinite(h[k])) { c->err = "knp_grid_create: the bounds of axis " + std::to_string(k) + " are not finite"; return -1; }
        if (shape[k] < 1) { c->err = "knp_grid_create: shape[" + std::to_string(k) + "] must be at least 1"; return -1; }
        if (shape[k] > 1 && !(h[k] > 0.0)) { c->err = "knp_grid_create: the spacing of axis " + std::to_string(k) + " must be positive"; return -1; }
        if (!std::isfinite(lo[k] + (double)(shape[k] - 1) * h[k])) { c->err = "knp_grid_create: the bounds of axis " + std::to_string(k) + " are not finite"; return -1; }
        npts *= (double)shape[k];
    }
    if (!(npts < 2147483648.0)) { c->err = "knp_grid_create: the grid must hold fewer than 2^31 points"; return -1; }
    if (!(tol >= 0.0) || !std::isfinite(tol)) { c->err = "knp_grid_create: tol must be finite and not negative"; return -1; }
    if (n_tags < 0 || n_tags > KNP_GRID_MAX_TAGS) { c->err = "knp_grid_create: at most 8 subdomain tags"; return -1; }
    if (n_derived < 0) { c->err = "knp_grid_create_derived: n_derived must not be negative"; return -1; }
    if (n_derived == 0 && (n_fields < 1 || n_fields > n_ions + 1)) { c->err = "knp_grid_create: between 1 and n_ions + 1 fields"; return -1; }
    if (n_fields < 0 || n_fields > n_ions + 1) { c->err = "knp_grid_create_derived: between 0 and n_ions + 1 nodal fields"; return -1; }
    for (int q = 0; q < n_fields; ++q)
        if (fields[q] < 0 || fields[q] > n_ions) { c->err = "knp_grid_create: unknown field id " + std::to_string(fields[q]); return -1; }
    if (n_derived > 2 * n_ions + 2) { c->err = "knp_grid_create_derived: at most 2 n_ions + 2 derived quantities"; return -1; }
    for (int q = 0; q < n_derived; ++q) {
        if (kind[q] != KNP_GD_EFIELD && kind[q] != KNP_GD_FLUX && kind[q] != KNP_GD_FLUX_DIFFUSIVE && kind[q] != KNP_GD_CURRENT) {
            c->err = "knp_grid_create_derived: unknown kind " + std::to_string(kind[q]);
            return -1;
        }
        if ((kind[q] == KNP_GD_FLUX || kind[q] == KNP_GD_FLUX_DIFFUSIVE) && (ion[q] < 0 || ion[q] >= n_ions)) {
            c->err = "knp_grid_create_derived: ion " + std::to_string(ion[q]) + " outside 0 .. n_ions - 1";
            return -1;
        }
    }
    // dt > 0 is what knp_set_params insists on: it is 0 until the parameters (z, D, psi, F) have been set
    if (n_derived && !(c->p.dt > 0.0)) { c->err = "knp_grid_create_derived: the parameters were never set (knp_set_params)"; return -1; }
    if (m.nc >= (int64_t)KNP_GRID_NONE) { c->err = "knp_grid_create: too many cells"; return -1; }
    if (c->h_ctag.size() != (size_t)m.nc) { c->err = "knp_grid_create: the context holds no subdomain table"; return -1; }
    int handle = -1;
    for (int s = 0; s < KNP_GRID_MAX && handle < 0; ++s)
        if (!c->grid || !c->grid->g[s]) handle = s;
    if (handle < 0) { c->err = "knp_grid_create: at most 8 grids per context"; return -1; }

    HIPCHK(c, hipSetDevice(c->device));
    Grid* g = new Grid();
    g->dim = d; g->n_fields = n_fields; g->n_derived = n_derived; g->f32 = f32 != 0; g->npts = (int64_t)npts;
    for (int k = 0; k < 3; ++k) { g->G.lo[k] = k < d ? lo[k] : 0.0; g->G.h[k] = k < d && shape[k] > 1 ? h[k] : 0.0; g->G.n[k] = k < d ? shape[k] : 1; }
    for (int q = 0; q < n_fields; ++q) g->field[q] = fields[q];
    for (int q = 0; q < n_derived; ++q) { g->kind[q] = kind[q]; g->ion[q] = kind[q] == KNP_GD_FLUX || kind[q] == KNP_GD_FLUX_DIFFUSIVE ? ion[q] : -1; }
    GridTags T;
    T.n = n_tags;
    for (int q = 0; q < KNP_GRID_MAX_TAGS; ++q) T.t[q] = q < n_tags ? tags[q] : 0u;
    const size_t np = (size_t)g->npts;
    uint32_t* ctag = c->grid ? c->grid->ctag : nullptr;
    const bool own_ctag = ctag == nullptr;
    bool ok = hipMalloc((void**)&g->owner, 4 * np) == hipSuccess && hipMalloc((void**)&g->cell, 4 * np) == hipSuccess &&
              hipMalloc((void**)&g->tag, 4 * np) == hipSuccess && hipMalloc((void**)&g->lam, 8 * np * (size_t)(d + 1)) == hipSuccess;
    ok = ok && g->pipe.alloc(g->frame_bytes());
    if (ok && own_ctag) ok = hipMalloc((void**)&ctag, 4 * (size_t)std::max<int64_t>(m.nc, 1)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        grid_free(g);
        if (own_ctag) hipFree(ctag);
        c->err = "knp_grid_create: allocation failed";
        return -2;
    }
    // ---- from here on the context changes ------------------------------------------------------------------------------------------
    if (!c->grid) c->grid = new GridState();
    GridState& X = *c->grid;
    X.ctag = ctag;
    X.g[handle] = g;
    int rc = 0;
    auto run = [&]() -> int {
        if (own_ctag && m.nc) HIPCHK(c, host_memcpy(c, ctag, c->h_ctag.data(), 4 * (size_t)m.nc, hipMemcpyHostToDevice));
        const int32_t* rank = state_cell_rank(c);
        HIPCHK(c, hipMemsetAsync(g->owner, 0x7f, 4 * np, c->stream));
        HIPCHK(c, hipEventRecord(g->pipe.ev[0][0], c->stream));
        if (m.nc) DISPATCH_DIM(c, k_grid_locate, dim3((unsigned)grid_for(m.nc)), m.nc, m.coords, m.cells, rank, ctag, T, g->G, tol, g->owner);
        HIPCHK(c, hipEventRecord(g->pipe.ev[0][1], c->stream));
        DISPATCH_DIM(c, k_grid_weights, dim3((unsigned)grid_for(g->npts)), g->npts, m.coords, m.cells, rank, ctag, g->G, g->owner, g->cell, g->tag, g->lam);
        HIPCHK(c, hipEventRecord(g->pipe.ev[0][2], c->stream));
        HIPCHK(c, host_stream_sync(c, c->stream));
        HIPCHK(c, hipEventElapsedTime(&g->locate_ms, g->pipe.ev[0][0], g->pipe.ev[0][1]));
        HIPCHK(c, hipEventElapsedTime(&g->weights_ms, g->pipe.ev[0][1], g->pipe.ev[0][2]));
        return 0;
    };
    if ((rc = run())) {
        X.g[handle] = nullptr;
        grid_free(g);
        return rc;
    }
    return handle;
}

int knp_grid_points(knp_ctx* c, int grid, int32_t* owner, int32_t* tag) {
    if (!c) return -1;
    Grid* g = grid_find(c, grid, "knp_grid_points");
    if (!g) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    if (owner) HIPCHK(c, host_memcpy(c, owner, g->owner, 4 * (size_t)g->npts, hipMemcpyDeviceToHost));
    if (tag) HIPCHK(c, host_memcpy(c, tag, g->tag, 4 * (size_t)g->npts, hipMemcpyDeviceToHost));
    return 0;
}

int knp_grid_sample(knp_ctx* c, int grid) {
    if (!c) return -1;
    Grid* gp = grid_find(c, grid, "knp_grid_sample");
    if (!gp) return -1;
    Grid& g = *gp;
    const int n_sys = c->p.n_sys;
    const int64_t ndof = c->m.nc * c->nd;
    const double* cc = knp_field_ptr(c, KNP_F_C, nullptr);
    GridFields F;
    F.n = g.n_fields;
    for (int q = 0; q <= KNP_MAX_IONS; ++q) F.f[q] = nullptr;
    for (int q = 0; q < g.n_fields; ++q) {
        const int id = g.field[q];
        F.f[q] = id == 0 ? knp_field_ptr(c, KNP_F_PHI, nullptr) : (id <= n_sys ? cc + (int64_t)(id - 1) * ndof : knp_field_ptr(c, KNP_F_C_ELIM, nullptr));
    }
    const int b = g.pipe.begin(c, "knp_grid_sample", "knp_grid_fetch");
    if (b < 0) return b;
    if (g.n_fields) {
        if (g.dim == 3) { if (c->degree == 1) sample_type<3, 1>(c, g, F); else sample_type<3, 2>(c, g, F); }
        else { if (c->degree == 1) sample_type<2, 1>(c, g, F); else sample_type<2, 2>(c, g, F); }
        HIPCHK(c, hipGetLastError());
    }
    if (g.n_derived) {
        const int n_ions = c->p.n_ions;
        GridDerived Q;
        memset(&Q, 0, sizeof(Q));
        Q.n = g.n_derived; Q.n_ions = n_ions;
        for (int q = 0; q < g.n_derived; ++q) {
            Q.kind[q] = g.kind[q]; Q.ion[q] = g.ion[q];
            Q.ions |= g.kind[q] == KNP_GD_CURRENT ? (1u << n_ions) - 1u : (g.ion[q] >= 0 ? 1u << g.ion[q] : 0u);
        }
        Q.phi = knp_field_ptr(c, KNP_F_PHI, nullptr);
        for (int s = 0; s < n_ions; ++s) {
            Q.conc[s] = s < n_sys ? cc + (int64_t)s * ndof : knp_field_ptr(c, KNP_F_C_ELIM, nullptr);
            Q.z[s] = c->p.z[s];
        }
        Q.D = c->D; Q.nc = c->m.nc; Q.psi = c->p.psi; Q.F = c->p.F;
        if (g.dim == 3) { if (c->degree == 1) derived_type<3, 1>(c, g, Q); else derived_type<3, 2>(c, g, Q); }
        else { if (c->degree == 1) derived_type<2, 1>(c, g, Q); else derived_type<2, 2>(c, g, Q); }
        HIPCHK(c, hipGetLastError());
    }
    return g.pipe.end(c, b);
}

int knp_grid_fetch(knp_ctx* c, int grid, void* out, size_t bytes) {
    if (!c || !out) return -1;
    Grid* gp = grid_find(c, grid, "knp_grid_fetch");
    if (!gp) return -1;
    return gp->pipe.fetch(c, "knp_grid_fetch", "knp_grid_sample", "n_fields x points values of the grid's type", out, bytes);
}

int knp_grid_destroy(knp_ctx* c, int grid) {
    if (!c) return -1;
    Grid* g = grid_find(c, grid, "knp_grid_destroy");
    if (!g) return -1;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, host_stream_sync(c, c->stream));
    c->grid->g[grid] = nullptr;
    grid_free(g);
    return 0;
}

int knp_grid_timing(knp_ctx* c, int grid, float* locate_ms, float* weights_ms, float* sample_ms, float* copy_ms) {
    if (!c || !locate_ms || !weights_ms || !sample_ms || !copy_ms) return -1;
    Grid* g = grid_find(c, grid, "knp_grid_timing");
    if (!g) return -1;
    *locate_ms = g->locate_ms; *weights_ms = g->weights_ms; *sample_ms = g->pipe.sample_ms; *copy_ms = g->pipe.copy_ms;
    return 0;
}

}  // extern "C"
