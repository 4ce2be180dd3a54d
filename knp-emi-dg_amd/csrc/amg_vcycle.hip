// The V-cycle of the auxiliary-space preconditioner  M^-1 = B^-1 + P Ac^+ P^T  (setup: knpemidg/amg.py) over a smoothed-aggregation
// hierarchy stored as CSR levels: Chebyshev-Jacobi polynomial smoothing (fused SpMV + recurrence kernels, no sequential sweeps), CSR
// restriction / prolongation, dense pseudo-inverse on the coarsest level; its capture into a graph; the row-distributed level 0 of
// partitioned runs.  The DG <-> conforming transfers around it are amg_restrict.hip and the k_prolong_* kernels of krylov.hip; the
// hierarchy comes from amg_upload.hip.  Stands in for hypre BoomerAMG (reference: src/knpemidg/solver.py:433, 505, 688, 767).
#include "knpemi_internal.hpp"
#include "amg.hpp"
#include <cstdlib>
#include <cstdio>
#include <type_traits>
#include <utility>

namespace {

// Level vectors carry NC right-hand-side columns INTERLEAVED ([n][NC]; further column groups behind each other): a gather of entry
// `col` fetches both species' values from one 16-byte location.  With the columns stored one behind the other every gather pulled
// its own 64-byte sector out of L2 for 8 useful bytes, and the two-column kernels were bound by exactly that: k_csr-type kernels
// cost 24 bytes of useful data per entry but ran at the L2's sector rate (a 28-entry-per-row product took 1.9x the time of a
// 15-entry one -- linear in the entries, not in the launches; profiles/README.md, round 2).
// Partial dot products of CSR row `row` with the NC interleaved columns of x over this lane's entries (lane, lane+G, ...); the loop
// is unrolled so that U (col, val) pairs are in flight per lane.
template <int G, int NC>
__device__ __forceinline__ void row_dot(const CsrDev& A, int64_t row, int lane, const double* __restrict__ x, double* out) {
    constexpr int U = NC == 1 ? 4 : 2;                    // (col, val) pairs in flight per lane
    double s[U][NC];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int j = 0; j < NC; ++j) s[u][j] = 0.0;
    if (row < A.nrows) {
        const int e = A.rowptr[row + 1];
        int k = A.rowptr[row] + lane;
        for (; k + (U - 1) * G < e; k += U * G) {
            int cc[U];
            double vv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) { cc[u] = A.col[k + u * G]; vv[u] = A.val[k + u * G]; }      // float -> double
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < NC; ++j) s[u][j] = fma(vv[u], x[(int64_t)cc[u] * NC + j], s[u][j]);
        }
#pragma unroll
        for (int u = 0; u < U - 1; ++u) {
            if (k < e) {
                const int c0 = A.col[k];
                const double v0 = A.val[k];
#pragma unroll
                for (int j = 0; j < NC; ++j) s[u][j] = fma(v0, x[(int64_t)c0 * NC + j], s[u][j]);
                k += G;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        double t = U == 4 ? (s[0][j] + s[1][j]) + (s[2 % U][j] + s[3 % U][j]) : s[0][j] + s[1][j];
#pragma unroll
        for (int off = G / 2; off > 0; off >>= 1) t += __shfl_down(t, off, G);
        out[j] = t;
    }
}

// y = A x (MODE 0) | y = b - A x (MODE 1) | y += A x (MODE 2); G lanes cooperate on one row; NC columns per thread, the rest of the
// right-hand-side columns along grid.y
template <int MODE, int G, int NC>
__global__ __launch_bounds__(256) void k_csr(CsrDev A, const double* __restrict__ x, const double* __restrict__ b,
                                             double* __restrict__ y) {
    x += (int64_t)blockIdx.y * NC * A.ncols;
    y += (int64_t)blockIdx.y * NC * A.nrows;
    if (MODE == 1) b += (int64_t)blockIdx.y * NC * A.nrows;
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    double s[NC];
    row_dot<G, NC>(A, row, lane, x, s);
    if (row < A.nrows && lane == 0) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int64_t o = row * NC + j;
            if (MODE == 0) y[o] = s[j];
            else if (MODE == 1) y[o] = b[o] - s[j];
            else y[o] += s[j];
        }
    }
}

// b_c = R r together with the first (zero-guess) Chebyshev update of the level that receives it:  rc = b_c ; d = dinv b_c / theta ;
// x = d  -- the separate k_cheb_first launch (5 us, three vector writes of a vector this kernel has in registers) goes away
template <int G, int NC>
__global__ __launch_bounds__(256) void k_csr_first(CsrDev R, const double* __restrict__ rfine, const double* __restrict__ dinv, double inv_theta,
                                                   double* __restrict__ bc, double* __restrict__ rc, double* __restrict__ d,
                                                   double* __restrict__ x) {
    rfine += (int64_t)blockIdx.y * NC * R.ncols;
    const int64_t o = (int64_t)blockIdx.y * NC * R.nrows;
    bc += o; rc += o; d += o; x += o;
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    double s[NC];
    row_dot<G, NC>(R, row, lane, rfine, s);
    if (row < R.nrows && lane == 0) {
        const double w = dinv[row] * inv_theta;
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int64_t q = row * NC + j;
            const double v = w * s[j];
            bc[q] = s[j];
            rc[q] = s[j];
            d[q] = v;
            x[q] = v;
        }
    }
}

// first Chebyshev update:  d = dinv r / theta ;  x = d (zero guess) or x += d
__global__ void k_cheb_first(int64_t n, int nil, const double* __restrict__ dinv, const double* __restrict__ b, double inv_theta,
                             double* __restrict__ r, double* __restrict__ d, double* __restrict__ x) {
    // zero initial guess: r = b ; d = dinv r / theta ; x = d.   grid.y = column group, nil interleaved columns per row
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * nil) return;
    const int64_t o = (int64_t)blockIdx.y * n * nil;
    b += o; r += o; d += o; x += o;
    const double bi = b[i];
    const double v = dinv[i / nil] * bi * inv_theta;
    r[i] = bi;
    d[i] = v;
    x[i] = v;
}

// non-zero guess, fused:  r = b - A x ;  d = dinv r / theta ;  xout = x + d     (xout != x: neighbours still read x)
template <int G, int NC>
__global__ __launch_bounds__(256) void k_cheb_first_res(CsrDev A, const double* __restrict__ dinv, const double* __restrict__ b,
                                                        const double* __restrict__ x, double inv_theta, double* __restrict__ r,
                                                        double* __restrict__ d, double* __restrict__ xout) {
    const int64_t o = (int64_t)blockIdx.y * NC * A.nrows;
    b += o; x += o; r += o; d += o; xout += o;
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    double s[NC];
    row_dot<G, NC>(A, row, lane, x, s);
    if (row < A.nrows && lane == 0) {
        const double di = dinv[row];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int64_t q = row * NC + j;
            const double rn = b[q] - s[j];
            const double v = di * rn * inv_theta;
            r[q] = rn;
            d[q] = v;
            xout[q] = x[q] + v;
        }
    }
}

// fused step:  r -= A d_in ;  d_out = c1 d_in + c2 dinv r ;  x += d_out        (G lanes per row)
template <int G, int NC>
__global__ __launch_bounds__(256) void k_cheb_step(CsrDev A, const double* __restrict__ dinv, const double* __restrict__ din,
                                                   double c1, double c2, double* __restrict__ r, double* __restrict__ dout,
                                                   double* __restrict__ x) {
    const int64_t o = (int64_t)blockIdx.y * NC * A.nrows;
    din += o; r += o; dout += o; x += o;
    const int64_t row = ((int64_t)blockIdx.x * 256 + threadIdx.x) / G;
    const int lane = threadIdx.x % G;
    double s[NC];
    row_dot<G, NC>(A, row, lane, din, s);
    if (row < A.nrows && lane == 0) {
        const double di = dinv[row];
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const int64_t q = row * NC + j;
            const double rn = r[q] - s[j];
            const double dn = fma(c1, din[q], c2 * di * rn);
            r[q] = rn;
            dout[q] = dn;
            x[q] += dn;
        }
    }
}

// dense y = M b on the coarsest level (n up to a few thousand): one workgroup per row, 4 independent loads in flight per
// lane; M is the pseudo-inverse stored in fp32 (preconditioner data: half the bytes, still an exactly symmetric
// operator because symmetric entries round identically), accumulation in fp64, fixed reduction tree.
constexpr int DENSE_ROWS = 2;
template <int NC>
__global__ __launch_bounds__(256) void k_dense_mv(int n, const float* __restrict__ M, const double* __restrict__ b,
                                                  double* __restrict__ y) {
    // DENSE_ROWS rows per workgroup (they share the loads of b: with one row per workgroup every workgroup pulls the whole of b through
    // its L1 -- 151 MB for two columns against 38 MB of matrix at n = 3 089), 4 independent row segments in flight per lane and row;
    // lanes read consecutive entries (a 16-byte-per-lane layout touches four times the cache lines per load of b and is slower);
    // NC right-hand-side columns share the pass over the fp32 rows (further columns along grid.y)
    __shared__ double part[4][DENSE_ROWS][NC];
    const int row0 = blockIdx.x * DENSE_ROWS;
    b += (int64_t)blockIdx.y * NC * n;
    y += (int64_t)blockIdx.y * NC * n;
    const float* __restrict__ Mr[DENSE_ROWS];
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; ++r) Mr[r] = M + (int64_t)(row0 + r < n ? row0 + r : n - 1) * n;      // (a duplicate row is not stored)
    double s[DENSE_ROWS][4][NC];
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; ++r)
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NC; ++j) s[r][u][j] = 0.0;
    int k = threadIdx.x;
    for (; k + 768 < n; k += 1024) {
        float m[DENSE_ROWS][4];
#pragma unroll
        for (int r = 0; r < DENSE_ROWS; ++r)
#pragma unroll
            for (int u = 0; u < 4; ++u) m[r][u] = Mr[r][k + 256 * u];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int j = 0; j < NC; ++j) {
                const double bv = b[(int64_t)(k + 256 * u) * NC + j];
#pragma unroll
                for (int r = 0; r < DENSE_ROWS; ++r) s[r][u][j] = fma((double)m[r][u], bv, s[r][u][j]);
            }
    }
    for (; k < n; k += 256) {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double bv = b[(int64_t)k * NC + j];
#pragma unroll
            for (int r = 0; r < DENSE_ROWS; ++r) s[r][0][j] = fma((double)Mr[r][k], bv, s[r][0][j]);
        }
    }
#pragma unroll
    for (int r = 0; r < DENSE_ROWS; ++r)
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            double v = (s[r][0][j] + s[r][1][j]) + (s[r][2][j] + s[r][3][j]);
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
            if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][r][j] = v;
        }
    __syncthreads();
    if ((int)threadIdx.x < DENSE_ROWS * NC) {
        const int r = threadIdx.x / NC, j = threadIdx.x % NC;
        if (row0 + r < n) y[(int64_t)(row0 + r) * NC + j] = (part[0][r][j] + part[1][r][j]) + (part[2][r][j] + part[3][r][j]);
    }
}

// ---- the one density dispatch ---------------------------------------------------------------------------------------------------------
// rows with up to this many entries on average get 4 lanes (KNP_AMG_G4; 12 = never; 40: -1.3 % per step at r=2 P1, -1 % for P2 at r=1)
static double g4_limit() {
    static const double v = getenv("KNP_AMG_G4") ? atof(getenv("KNP_AMG_G4")) : 40.0;
    return v;
}

template <int N> using int_c = std::integral_constant<int, N>;

// kern<<<grid, 256, 0, st>>>(args...), every argument converted to the kernel's own parameter type
template <typename... P, typename... Args> void launch256(void (*kern)(P...), dim3 grid, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, static_cast<P>(args)...);
}

// Picks the lanes per row G by the average row length of A (four bands: G = 1 / 4 / 8 / 64), the columns per thread NC (2 when the
// hierarchy's columns are interleaved in pairs) and the grid, and launches kernel(int_c<G>, int_c<NC>) with args on stream st.  Every
// row kernel of the V-cycle is launched through here (tests/amg_ref.py mirrors the rule: BANDS).
template <typename K, typename... Args> void by_density(const CsrDev& A, const AmgCols& cols, hipStream_t st, K kernel, const Args&... args) {
    const double avg = A.nrows ? (double)A.nnz / (double)A.nrows : 0.0;
    auto with_lanes = [&](auto g) {
        const dim3 grid((unsigned)((A.nrows * decltype(g)::value + 255) / 256), cols.groups);
        if (cols.nil == 2) launch256(kernel(g, int_c<2>()), grid, st, args...);
        else launch256(kernel(g, int_c<1>()), grid, st, args...);
    };
    if (avg <= 12.0) with_lanes(int_c<1>());
    else if (avg <= g4_limit()) with_lanes(int_c<4>());
    else if (avg <= 96.0) with_lanes(int_c<8>());
    else with_lanes(int_c<64>());
}

// y = A x (MODE 0) | y = b - A x (MODE 1) | y += A x (MODE 2)
template <int MODE> void launch_csr(const CsrDev& A, const AmgCols& cols, hipStream_t st, const double* x, const double* b, double* y) {
    by_density(A, cols, st, [](auto g, auto nc) { return k_csr<MODE, decltype(g)::value, decltype(nc)::value>; }, A, x, b, y);
}

// first_done: the zero-guess first update was written by the kernel that produced L.b (k_csr_first, k_restrict_sum)
void smooth(knp_ctx* c, const AmgCols& cols, AmgLevel& L, bool zero_guess, bool first_done = false) {
    Cheb ch(L);
    if (zero_guess && first_done) {
    } else if (zero_guess) {
        hipLaunchKernelGGL(k_cheb_first, dim3((unsigned)((L.n * cols.nil + 255) / 256), cols.groups), dim3(256), 0, c->stream, L.n, cols.nil,
                           L.dinv, L.b, 1.0 / ch.theta, L.r, L.d0, L.x);
    } else {
        // x lives in L.x; the fused kernel writes the updated iterate to L.d1 (free at this point), then swap
        by_density(L.A, cols, c->stream, [](auto g, auto nc) { return k_cheb_first_res<decltype(g)::value, decltype(nc)::value>; },
                   L.A, L.dinv, L.b, L.x, 1.0 / ch.theta, L.r, L.d0, L.d1);
        std::swap(L.x, L.d1);
    }
    double* din = L.d0;
    double* dout = L.d1;
    for (int k = 1; k < L.cheb_degree; ++k) {
        const Cheb::Step st = ch.next();
        by_density(L.A, cols, c->stream, [](auto g, auto nc) { return k_cheb_step<decltype(g)::value, decltype(nc)::value>; },
                   L.A, L.dinv, din, st.c1, st.c2, L.r, dout, L.x);
        std::swap(din, dout);
    }
}

// x_0 = V(b_0) from level l0 down; level vectors b/x of level l0 are filled / read by the caller
int amg_vcycle_eager(knp_ctx* c, AmgHierarchy& H, int l0 = 0) {
    const int nl = (int)H.levels.size();
    const AmgCols cols = H.cols();
    hipStream_t st = c->stream;
    bool first_done = l0 == 0 && H.fuse_first0;                     // level 0's first update came with the restriction (k_restrict_sum)
    for (int l = l0; l < nl - 1; ++l) {
        AmgLevel& L = H.levels[l];
        if (L.cheb_degree == 0) {                                    // transfer-only level: x = 0, r = b
            // level 0: amg_restrict_from_dg already went down to level 1 (outside the captured graph, see there)
            if (l > 0) launch_csr<0>(L.R, cols, st, L.b, nullptr, H.levels[l + 1].b);
            first_done = false;
            continue;
        }
        smooth(c, cols, L, true, first_done);
        launch_csr<1>(L.A, cols, st, L.x, L.b, L.r);                 // r = b - A x
        AmgLevel& N = H.levels[l + 1];
        first_done = l + 1 < nl - 1 && N.cheb_degree > 0;
        if (first_done)                                              // b_{l+1} = R r and the next level's first update at once
            by_density(L.R, cols, st, [](auto g, auto nc) { return k_csr_first<decltype(g)::value, decltype(nc)::value>; },
                       L.R, L.r, N.dinv, 1.0 / Cheb::theta_of(N), N.b, N.r, N.d0, N.x);
        else
            launch_csr<0>(L.R, cols, st, L.r, nullptr, N.b);         // b_{l+1} = R r
    }
    AmgLevel& C = H.levels[nl - 1];
    const dim3 gdense((unsigned)((C.n + DENSE_ROWS - 1) / DENSE_ROWS), cols.groups);
    if (cols.nil == 2) hipLaunchKernelGGL(k_dense_mv<2>, gdense, dim3(256), 0, st, (int)C.n, (const float*)H.pinv, C.b, C.x);
    else hipLaunchKernelGGL(k_dense_mv<1>, gdense, dim3(256), 0, st, (int)C.n, (const float*)H.pinv, C.b, C.x);
    for (int l = nl - 2; l >= l0; --l) {
        AmgLevel& L = H.levels[l];
        if (L.cheb_degree == 0) {
            launch_csr<0>(L.P, cols, st, H.levels[l + 1].x, nullptr, L.x);   // x = P x_{l+1}
            continue;
        }
        launch_csr<2>(L.P, cols, st, H.levels[l + 1].x, nullptr, L.x);       // x += P x_{l+1}
        smooth(c, cols, L, false);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

// The V-cycle is ~40 tiny launch-bound kernels on fixed buffers: capture it once into a hipGraph and replay it
// (kernel boundaries ~1.5 us instead of ~5 us of eager launch latency each).
int amg_vcycle_levels(knp_ctx* c, AmgHierarchy& H, int l0, hipStream_t on_stream) {
    static const bool use_graph = !env_flag("KNP_NO_GRAPH", false);
    if (use_graph && !H.graph_tried) {
        H.graph_tried = true;
        hipGraph_t graph = nullptr;
        hipGraphExec_t exec = nullptr;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            H.entry_x = H.levels[0].x; H.entry_r = H.levels[0].r; H.entry_d0 = H.levels[0].d0;
            std::vector<std::pair<double*, double*>> keep;           // the smoother swaps (x, d1) of a level as it goes
            for (auto& L : H.levels) keep.emplace_back(L.x, L.d1);
            const int rc = amg_vcycle_eager(c, H, l0);
            const hipError_t e = hipStreamEndCapture(c->stream, &graph);
            if (rc == 0 && e == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) == hipSuccess)
                H.graph_exec = exec;
            else                                                     // nothing ran: the eager V-cycle below starts from the buffers the
                for (size_t l = 0; l < H.levels.size(); ++l) { H.levels[l].x = keep[l].first; H.levels[l].d1 = keep[l].second; }   // restriction wrote
            if (graph) hipGraphDestroy(graph);
            if (getenv("KNP_DEBUG")) fprintf(stderr, "[knp] V-cycle graph capture: rc=%d end=%d exec=%p\n", rc, (int)e, (void*)H.graph_exec);
        } else if (getenv("KNP_DEBUG")) {
            fprintf(stderr, "[knp] hipStreamBeginCapture failed\n");
        }
        (void)hipGetLastError();
    }
    if (H.graph_exec) {
        HIPCHK(c, hipGraphLaunch(H.graph_exec, on_stream ? on_stream : c->stream));
        return 0;
    }
    return amg_vcycle_eager(c, H, l0);  // eager fallback always runs on the context's stream
}

}  // namespace

// ---- row-distributed level 0 (partitioned runs) ---------------------------------------------------------------------------------------
// Vectors on level 0 come in two kinds (the usual bookkeeping of non-overlapping domain decomposition): ACCUMULATED -- every rank that
// has a shared dof holds its full value (x, the smoother's d, the accumulated residual) -- and DISTRIBUTED -- every rank holds the
// part its own cells / facets contributed (the restricted DG residual b, and every product with the rank's share of the matrix).  A product
// needs no communication; turning its result into an accumulated vector is one interface exchange (interface_accumulate); the
// restriction to the replicated level 1 is a per-rank partial sum behind one all-reduce of n_1 values (29 k at r=2, 6.5x fewer than the
// level-0 vector the replicated design all-reduced).  Arithmetic per dof is that of smooth() / amg_vcycle_eager on the global level.
__global__ void k_l0_first_nz(int64_t n, int nil, const double* __restrict__ dinv, const double* __restrict__ r, double inv_theta,
                              double* __restrict__ d, double* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * nil) return;
    const int64_t o = (int64_t)blockIdx.y * n * nil;
    const double v = dinv[i / nil] * r[o + i] * inv_theta;
    d[o + i] = v;
    x[o + i] += v;
}

// r -= t (t = accumulated A d) ;  d = c1 d + c2 dinv r ;  x += d
__global__ void k_l0_step(int64_t n, int nil, const double* __restrict__ dinv, const double* __restrict__ t, double c1, double c2,
                          double* __restrict__ r, double* __restrict__ d, double* __restrict__ x) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * nil) return;
    const int64_t o = (int64_t)blockIdx.y * n * nil;
    const double rn = r[o + i] - t[o + i];
    const double dn = fma(c1, d[o + i], c2 * dinv[i / nil] * rn);
    r[o + i] = rn;
    d[o + i] = dn;
    x[o + i] += dn;
}

static int dist0_smooth(knp_ctx* c, AmgHierarchy& H, bool zero_guess) {
    AmgLevel& L = H.levels[0];
    const AmgCols cols = H.cols();
    const dim3 g((unsigned)((L.n * cols.nil + 255) / 256), cols.groups);
    Cheb ch(L);
    int rc;
    if (zero_guess) {                                                // r = acc(b) ; d = x = dinv r / theta
        HIPCHK(c, hipMemcpyAsync(H.t0, L.b, sizeof(double) * (size_t)L.n * cols.ncol, hipMemcpyDeviceToDevice, c->stream));
        if ((rc = interface_accumulate(c, H.t0, L.n, cols.ncol))) return rc;
        hipLaunchKernelGGL(k_cheb_first, g, dim3(256), 0, c->stream, L.n, cols.nil, L.dinv, (const double*)H.t0, 1.0 / ch.theta, L.r, L.d0, L.x);
    } else {                                                         // r = acc(b - A x) ; d = dinv r / theta ; x += d
        launch_csr<1>(L.A, cols, c->stream, L.x, L.b, L.r);
        if ((rc = interface_accumulate(c, L.r, L.n, cols.ncol))) return rc;
        hipLaunchKernelGGL(k_l0_first_nz, g, dim3(256), 0, c->stream, L.n, cols.nil, L.dinv, (const double*)L.r, 1.0 / ch.theta, L.d0, L.x);
    }
    for (int k = 1; k < L.cheb_degree; ++k) {
        const Cheb::Step st = ch.next();
        launch_csr<0>(L.A, cols, c->stream, L.d0, nullptr, H.t0);
        if ((rc = interface_accumulate(c, H.t0, L.n, cols.ncol))) return rc;
        hipLaunchKernelGGL(k_l0_step, g, dim3(256), 0, c->stream, L.n, cols.nil, L.dinv, (const double*)H.t0, st.c1, st.c2, L.r, L.d0, L.x);
    }
    HIPCHK(c, hipGetLastError());
    return 0;
}

static int amg_vcycle_dist0(knp_ctx* c, AmgHierarchy& H) {
    if (H.levels.size() < 2) { c->err = "amg: a distributed level 0 needs a coarser level"; return -1; }
    const AmgCols cols = H.cols();
    AmgLevel& L = H.levels[0];
    AmgLevel& N = H.levels[1];
    if (!H.t0) HIPCHK(c, hipMalloc((void**)&H.t0, sizeof(double) * (size_t)(L.n ? L.n : 1) * (size_t)H.ncol));
    int rc;
    if (L.cheb_degree > 0) {
        if ((rc = dist0_smooth(c, H, true))) return rc;
        launch_csr<1>(L.A, cols, c->stream, L.x, L.b, L.r);          // distributed residual b - A x
        launch_csr<0>(L.R, cols, c->stream, L.r, nullptr, N.b);      // this rank's part of the level-1 right-hand side
        if ((rc = allreduce_red(c, N.b, (int)(N.n * H.ncol)))) return rc;
    }                                                                // (transfer-only: the restriction's tail went down to level 1 already)
    if ((rc = amg_vcycle_levels(c, H, 1, nullptr))) return rc;
    if (L.cheb_degree == 0) {
        launch_csr<0>(L.P, cols, c->stream, N.x, nullptr, L.x);
        HIPCHK(c, hipGetLastError());
        return 0;
    }
    launch_csr<2>(L.P, cols, c->stream, N.x, nullptr, L.x);
    return dist0_smooth(c, H, false);
}

int amg_vcycle(knp_ctx* c, AmgHierarchy& H, hipStream_t on_stream) {
    if (!H.dist0) return amg_vcycle_levels(c, H, 0, on_stream);
    if (on_stream && on_stream != c->stream) { c->err = "amg: the distributed level 0 runs on the context's stream"; return -1; }
    return amg_vcycle_dist0(c, H);
}

void amg_csr_apply(const AmgHierarchy& H, const CsrDev& A, const double* x, double* y, hipStream_t st) {
    launch_csr<0>(A, H.cols(), st, x, nullptr, y);
}
