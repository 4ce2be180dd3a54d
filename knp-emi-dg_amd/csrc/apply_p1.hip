// Matrix-free P1 SIPG operator applies (EMI potential operator, batched KNP species operator),
// cell-based gather: one thread owns one cell, computes the cell's volume integral and the
// contribution of each of its D+1 facets to ITS OWN test functions, reading the neighbour's
// DoFs / coefficients / apex vertex.  No atomics, bitwise reproducible.
//
// Replaces: dolfin.assemble(a_emi) + PETSc MatMult        (reference: src/knpemidg/solver.py:325-328,346,477,509)
//           dolfin.assemble(A_knp) + PETSc MatMult        (reference: src/knpemidg/solver.py:586-594,730,771)
// P1 facet integrals are closed forms (mass / triple-product matrices of a (D-1)-simplex); the
// geometry enters only through the own cell's Gram matrix and the neighbour apex's barycentric
// coordinates (cell_geom.hpp).
//
// One translation unit; the kernels live in one header per family, the selection in apply_plan.hpp:
//   apply_p1_direct.hpp  coordinate-path applies, block-Jacobi inverses, gphi, neighbour materials
//   apply_p1_cls.hpp     geometry-class + LDS-staged applies
//   apply_p1_halo.hpp    halo-staged persistent KNP apply with its counters, grid and launch
// (the ring-staged families are translation units of their own: apply_ring.hip, apply_ring_u.hip)
#include "apply_p1_direct.hpp"
#include "apply_p1_cls.hpp"
#include "apply_p1_halo.hpp"
#include "apply_plan.hpp"

static_assert(APPLY_PLAN_BLK == KNP_HALO_BLK, "the plan counts head cells in blocks of the halo tables");

// ------------------------------------------------------------------------------------------
// launchers
// ------------------------------------------------------------------------------------------
static inline int64_t grid8(int64_t n) { return ((grid_for(n) + 7) / 8) * 8; }

// event pair around one apply launch while knp_apply_timing is on (the in-solver figure next to knp_bench_apply's)
struct ApplyTimerScope {
    knp_ctx* c; int which; bool on;
    ApplyTimerScope(knp_ctx* ctx, int w) : c(ctx), which(w), on(ctx->time_applies) {
        if (!on) return;
        auto& pool = c->tev[which];
        if (c->tev_used[which] == pool.size()) {
            hipEvent_t a, b;
            if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) { on = false; return; }
            pool.push_back({a, b});
        }
        hipEventRecord(pool[c->tev_used[which]].first, c->stream);
    }
    ~ApplyTimerScope() {
        if (!on) return;
        hipEventRecord(c->tev[which][c->tev_used[which]].second, c->stream);
        ++c->tev_used[which];
    }
};

// CUs a persistent head kernel leaves free: with an active communicator the interior launch runs next to the halo exchange (halo_grid)
static int halo_reserve_cus(const knp_ctx* c) { return (c->dist && c->halo_stream) ? env_int("KNP_HALO_RESERVE_CU", 8) : 0; }

// The plan's inputs of a P1 context.  The ring families are asked in the plan's order and only until one says yes: ring_u_cells builds
// and uploads its tables at its first call, so it is asked only after ring_usable said no (with classes present it returns 0 at once).
// halo_lds (KNP launcher): the LDS footprint knp_halo_usable computed.
static ApplyInputs apply_inputs(knp_ctx* c, int which, size_t* halo_lds = nullptr) {
    ApplyInputs in;
    in.degree = c->degree; in.dim = c->m.dim;
    if (c->degree != 1) { in.p2_assembled = p2_assembled(c); return in; }
    in.cls = c->m.cls != nullptr; in.ncls = c->m.ncls; in.ncls_max = CLS_MAX_LDS;
    in.n_sys = c->p.n_sys; in.hb_long0 = c->m.hb_long0;
    in.ring = ring_usable(c, which);
    if (!in.ring) in.ring_u_cells = ring_u_cells(c, which);
    if (!in.ring && in.ring_u_cells <= 0 && which == 1) in.halo = knp_halo_usable(c, halo_lds, &in.halo_mat);
    return in;
}

// which kernel an operator apply runs (bench.py / tests name the kernel they measured): the head family of the plan, see ApplyFamily
int apply_variant(knp_ctx* c, int which) { return plan_apply(apply_inputs(c, which), which).head; }

static KnpArgs make_knp_args(knp_ctx* c) {
    KnpArgs ka;
    ka.ns = c->p.n_sys;
    ka.inv_dt = 1.0 / c->p.dt;
    ka.psi = c->p.psi;
    ka.tau = c->p.tau_knp;
    for (int k = 0; k < KNP_MAX_SYS; ++k) ka.z[k] = (k < c->p.n_sys) ? c->p.z[k] : 0.0;
    return ka;
}

int launch_emi_apply(knp_ctx* c, const double* x, const double* kappa, double* y) {
    ApplyTimerScope t(c, 0);
    if (c->degree != 1) return p2_assembled(c) ? tab_apply(c, 0, x, y) : p2_emi_apply(c, x, kappa, y);
    if (c->m.c_end - c->m.c_begin <= 0) return 0;
    ApplySegment seg[2];
    const int nseg = apply_segments(plan_apply(apply_inputs(c, 0), 0), c->m.c_begin, c->m.c_end, seg);
    for (int i = 0; i < nseg; ++i) {
        MeshDev m = c->m;                          // the cell range of this launch
        m.c_begin = seg[i].begin; m.c_end = seg[i].end;
        const dim3 g((unsigned)grid8(m.c_end - m.c_begin));
        int rc = 0;
        switch (seg[i].family) {
            case AF_RING_EMI: rc = ring_emi_apply(c, m, x, kappa, y, halo_reserve_cus(c)); break;
            case AF_RING_U: rc = ring_u_emi_apply(c, m, x, kappa, y, halo_reserve_cus(c)); break;
            case AF_CLS:
                hipLaunchKernelGGL((k_emi_apply_cls_staged<3, 256>), g, dim3(KNP_BLOCK), 0, c->stream, m, x, kappa, y, c->p.C_phi, c->p.tau_emi);
                HIPCHK(c, hipGetLastError());
                break;
            default: DISPATCH_DIM(c, k_emi_apply, g, m, x, kappa, y, c->p.C_phi, c->p.tau_emi);
        }
        if (rc) return rc;
    }
    return 0;
}

int launch_knp_apply(knp_ctx* c, const double* x, const double* gphi, double* y) {
    ApplyTimerScope t(c, 1);
    if (c->degree != 1) return p2_assembled(c) ? tab_apply(c, 1, x, y) : p2_knp_apply(c, x, gphi, y);     // P2: gphi holds phi (launch_dnphi)
    if (c->m.c_end - c->m.c_begin <= 0) return 0;
    const KnpArgs ka = make_knp_args(c);
    size_t halo_lds = 0;
    const ApplyInputs in = apply_inputs(c, 1, &halo_lds);
    ApplySegment seg[2];
    const int nseg = apply_segments(plan_apply(in, 1), c->m.c_begin, c->m.c_end, seg);
    for (int i = 0; i < nseg; ++i) {
        MeshDev m = c->m;                          // the cell range of this launch
        m.c_begin = seg[i].begin; m.c_end = seg[i].end;
        const dim3 g((unsigned)grid8(m.c_end - m.c_begin)), b(KNP_BLOCK);
        int rc = 0;
        switch (seg[i].family) {
            case AF_RING_KNP: rc = ring_knp_apply(c, m, x, gphi, y, ka, halo_reserve_cus(c)); break;
            case AF_RING_U: rc = ring_u_knp_apply(c, m, x, gphi, y, ka, halo_reserve_cus(c)); break;
            case AF_HALO:
            case AF_HALO_MAT: rc = knp_halo_launch(c, m, x, gphi, y, ka, halo_lds, in.halo_mat, halo_reserve_cus(c)); break;
            case AF_CLS:                           // the plan admits at most three solved species
                dispatch_nsys<3>(c->p.n_sys, [&](auto ns) {
                    hipLaunchKernelGGL((k_knp_apply_cls_staged<3, decltype(ns)::value, 256>), g, b, 0, c->stream, m, x, gphi, c->D, y, ka);
                    return 0;
                });
                HIPCHK(c, hipGetLastError());
                break;
            default:
                rc = dispatch_nsys<4>(c->p.n_sys, [&](auto ns) {
                    constexpr int NS = decltype(ns)::value;
                    if (c->m.dim == 3) hipLaunchKernelGGL((k_knp_apply<3, NS>), g, b, 0, c->stream, m, x, gphi, c->D, y, ka);
                    else hipLaunchKernelGGL((k_knp_apply<2, NS>), g, b, 0, c->stream, m, x, gphi, c->D, y, ka);
                    return 0;
                });
                if (rc) { c->err = "knp_apply supports 1..4 solved species"; return -1; }
                HIPCHK(c, hipGetLastError());
        }
        if (rc) return rc;
    }
    return 0;
}

int launch_emi_blockjacobi(knp_ctx* c, const double* kappa, bjreal* binv) {
    if (c->degree != 1) return p2_assembled(c) ? tab_block_inverse(c, 0, binv) : p2_block_inverse(c, 0, kappa, binv);
    const double shift = 0.0;
    DISPATCH_DIM(c, k_emi_blockjacobi, dim3((unsigned)grid_for(c->m.nc_owned)), c->m, kappa, binv, c->p.C_phi, c->p.tau_emi, shift);
    return 0;
}

int launch_knp_blockjacobi(knp_ctx* c, const double* gphi, bjreal* binv) {
    if (c->degree != 1) return p2_assembled(c) ? tab_block_inverse(c, 1, binv) : p2_block_inverse(c, 1, gphi, binv);
    const dim3 g((unsigned)grid_for(c->m.nc_owned), (unsigned)c->p.n_sys);
    DISPATCH_DIM(c, k_knp_blockjacobi, g, c->m, gphi, c->D, binv, make_knp_args(c));
    return 0;
}

int launch_neighbour_materials(knp_ctx* c) {
    const int64_t n = c->m.nc * 4;
    hipLaunchKernelGGL(k_neighbour_materials, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->m.nc, c->m.nbr, c->mat, c->nmat4);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, host_stream_sync(c, c->stream));
    return 0;
}

int launch_dnphi(knp_ctx* c, const double* phi, double* gphi) {
    if (c->degree != 1) {
        // P2: the matrix-free apply evaluates the drift from phi itself; the "derived" field keeps the potential the KNP
        // solve is frozen at (the assembled variant integrates it into the cell blocks instead)
        if (p2_assembled(c)) return tab_assemble_knp(c, phi);
        HIPCHK(c, hipMemcpyAsync(gphi, phi, sizeof(double) * c->m.nc * c->nd, hipMemcpyDeviceToDevice, c->stream));
        return 0;
    }
    DISPATCH_DIM(c, k_gphi, dim3((unsigned)grid_for(c->m.nc)), c->m, phi, gphi);
    return 0;
}
