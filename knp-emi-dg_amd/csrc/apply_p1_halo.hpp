// Halo-staged persistent KNP kernel of the matrix-free P1 applies (apply_p1.hip) with the host code that belongs to it: block
// counters, the occupancy-sized grid, the LDS footprint test and the launch.
#pragma once
#include "cell_geom.hpp"
#include <algorithm>

// ---- halo-staged persistent variants (3D P1, structured meshes) -------------------------------------------------------
// Measured on the staged kernels above (tools/pmc_apply.sh, profiles/r02_pmc_apply_halo.md): 60 % of the wave cycles are
// spent parked, and a probe with the facet arithmetic removed still takes 85 % of the time -- the kernels are bound by their
// memory phase, which is a CHAIN of dependent round trips (topology -> neighbour rows, inside the facet loop for the 17 %
// of the facets whose neighbour lies outside the workgroup's 256 cells).  For the KNP operator (the EMI twin of this kernel
// measured equal to k_emi_apply_cls_staged, 34.1 vs 33.9 us at r=2 and 277 vs 280 us at r=3, and was removed)
//   * the out-of-block neighbours of every 256-cell block are known in advance (MeshDev::hb_src / hb_loc, built once from
//     the topology): own records and halo records are loaded before the single barrier and the facet loop reads LDS only
//     (one uniform path, the facet-vertex permutation folded into the per-lane LDS address, no register selects);
//   * a workgroup walks several blocks of its XCD's chunk and fetches the NEXT block's halo list while it works on the
//     current one, so that a block's loads -- own and halo -- are one round trip;
//   * LDS is component-major ([component][entry]: consecutive cells on consecutive banks; the row-major layout of the
//     staged kernels spends 70 % of its LDS cycles in bank conflicts), the class table has an odd stride;
//   * D is read through a material table when the cells carry few distinct coefficient tuples (knp_set_params).
// LDS entries [0,256) = the block's cells, [256, 256+nh) = halo entries (one per out-of-block coupled facet).
#define HALO_FT KNP_CLS_EXT   // per-class facet record kept in LDS: 4 x 8 derived coefficients (MeshDev::cls_ext)
#define HALO_FTS 33      // its LDS stride (odd: lanes of different classes land on different banks)

// vol + Gram matrix of the cell's class, straight from the (L1/L2-resident) table into registers
__device__ __forceinline__ void load_class_gram(const double* __restrict__ table, unsigned cls, CellGeom<3>& K) {
    class_gram<3>(table + (size_t)cls * KNP_CLS_STRIDE, K);
}

// The blocks of one workgroup.  The block range is cut into nq contiguous chunks, nq/8 per XCD (XCD = blockIdx.x & 7,
// round-robin dispatch; an XCD's chunks are adjacent, so facet neighbours stay in its L2); workgroup w serves chunk queue w % nq
// with the other `members` workgroups of that queue.  Full rounds are strided (block = first + member + round * members); the
// remainder (< members blocks) goes to whichever workgroups get there first, through the queue's counter.  A workgroup knows
// its next block one iteration ahead, because that block's halo list is fetched while the current block is worked on.
// counters[2][HALO_NQ] (one 128-byte line each): this launch draws from set `flip` (zero on entry) and zeroes the other one --
// the previous launch's, which the next launch will draw from (launches of one context are ordered on its stream).
#define HALO_NQ 64            // counters per set (upper bound of the queue count nq, a multiple of 8)
#define HALO_CPAD 32          // ints between two counters: atomics on ONE line retire at ~13 ns chip-wide (measured with a draw per
                              // block: 31 104 draws on one line = 392 us, more than the whole kernel)
struct HaloWalk {
    int64_t b_lo, first, last, members, member, dyn0, cur, nxt;
    int n, rounds;
    int* ctr;
    __device__ __forceinline__ int64_t strided(int k) const { return first + member + (int64_t)k * members; }
    __device__ __forceinline__ HaloWalk(const MeshDev& m, int* counters, int flip_nq) {
        const int flip = flip_nq & 1;
        const unsigned nq = (unsigned)flip_nq >> 2;
        b_lo = m.c_begin / KNP_HALO_BLK;
        const int64_t nblk = (m.c_end - 1) / KNP_HALO_BLK - b_lo + 1;
        const int64_t chunk = (nblk + nq - 1) / nq;
        const unsigned q = blockIdx.x % nq;
        first = (int64_t)((q & 7u) * (nq >> 3) + (q >> 3)) * chunk;
        last = first + chunk < nblk ? first + chunk : nblk;
        members = gridDim.x / nq;
        member = blockIdx.x / nq;
        rounds = last > first ? (int)((last - first) / members) : 0;
        if (rounds < 2) rounds = 1 << 30;                                    // short chunks: strided throughout, no draws
        else if (flip_nq & 2) rounds = 2;                                    // default (KNP_HALO_DYN=0 turns it off): every block after the first two is drawn
        dyn0 = first + (int64_t)rounds * members;
        n = 0;
        cur = strided(0);
        nxt = strided(1);
        ctr = counters + (HALO_NQ * flip + q) * HALO_CPAD;
        if (blockIdx.x == 0 && threadIdx.x < HALO_NQ) counters[(HALO_NQ * (1 - flip) + threadIdx.x) * HALO_CPAD] = 0;
    }
    // thread 0, at the top of iteration n: the block after next
    __device__ __forceinline__ int64_t after_next() const { return n + 2 < rounds ? strided(n + 2) : dyn0 + atomicAdd(ctr, 1); }
    // every thread, after the iteration's second barrier
    __device__ __forceinline__ void advance(int64_t nn) { cur = nxt; nxt = nn; ++n; }
};

// s_D: MAT ? [NS][KNP_MAX_MAT] coefficient table indexed by the neighbour's material id dsel : [NS][ent] staged values
template <int NS, bool MAT, int I>
__device__ __forceinline__ void knp_facet_halo(const CellGeom<3>& K, uint32_t flags, unsigned loc, unsigned dsel, const double (*xv)[4],
                                               const double* gp, const double* Dk, const KnpArgs& ka, const lds_double* s_x,
                                               const lds_double* s_g, const lds_double* s_D, const lds_double* ft, unsigned ent,
                                               double (*y)[4]) {
    constexpr int D = 3, NV = 4;
    const uint32_t fb = (flags >> (8 * I)) & 0xffu;
    if (((fb >> 2) & 3u) != FK_SIPG) return;
    const unsigned j = fb & 3u;
    // class-level coefficients (cls_ext): nothing geometric is recomputed per lane
    const double gr = ft[8 * I], pen_geo = ft[8 * I + 4], nLI_DV = ft[8 * I + 5];
    double cf[D];
#pragma unroll
    for (int mm = 0; mm < D; ++mm) cf[mm] = ft[8 * I + 1 + mm];
    const double gp_nb = s_g[loc < KNP_HALO_BLK ? j * KNP_HALO_BLK + loc : loc + (KNP_HALO_BLK * NV - KNP_HALO_BLK)];
    const double DV = (double)D * K.vol;
    const double up_own = fmax(-gp[I], 0.0) * DV;
    const double up_nb = fmax(-gp_nb, 0.0) * nLI_DV;
    const double penA = ka.tau * pen_geo;
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        const lds_double* xl = s_x + (unsigned)k * NV * ent + loc;                  // component-major: [k][a][entry]
        const double xap = xl[j * ent];
        double xf[D];
#pragma unroll
        for (int mm = 0; mm < D; ++mm) xf[mm] = xl[(mm + (mm >= (int)j ? 1 : 0)) * ent];
        const double Dn = MAT ? s_D[(unsigned)k * KNP_MAX_MAT + dsel] : s_D[(unsigned)k * ent + loc];
        double s_own = 0.0;
#pragma unroll
        for (int a = 0; a < NV; ++a) s_own = fma(xv[k][a], K.G[a][I], s_own);
        double s_nb = xap * gr;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) s_nb = fma(xf[mm], cf[mm], s_nb);
        const double zp = ka.z[k] * ka.psi;
        const double c_own = penA * Dk[k] - zp * Dk[k] * up_own;
        const double c_nb = penA * Dn - zp * Dn * up_nb;
        double sdu = 0.0, w[D], sw = 0.0;
#pragma unroll
        for (int mm = 0; mm < D; ++mm) {
            const double xo = xv[k][mm + (mm >= I)];
            sdu += xo - xf[mm];
            w[mm] = fma(c_own, xo, -c_nb * xf[mm]);
            sw += w[mm];
        }
        const double t1 = 0.5 * K.vol * fma(Dk[k], s_own, Dn * s_nb);
        const double t2 = 0.5 * Dk[k] * K.vol * sdu;
#pragma unroll
        for (int a = 0; a < NV; ++a) y[k][a] = fma(K.G[a][I], t2, y[k][a]);
#pragma unroll
        for (int mm = 0; mm < D; ++mm)
            y[k][mm + (mm >= I)] += t1 + FacetConst<D>::mass * (sw + w[mm]);
    }
}

template <int NS, bool MAT>
__global__ __launch_bounds__(KNP_HALO_BLK) void k_knp_apply_halo(MeshDev m, const double* __restrict__ x,
                                                                 const double* __restrict__ gphi,
                                                                 const double* __restrict__ Dall, double* __restrict__ yout,
                                                                 KnpArgs ka, unsigned ent, const uint8_t* __restrict__ mat,
                                                                 const uint8_t* __restrict__ nmat4, const double* __restrict__ dtab,
                                                                 int* __restrict__ counters, int flip_nq) {
    constexpr int NV = 4, BLK = KNP_HALO_BLK;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double* s_x = smem;                                   // [NS][4][ent]
    double* s_g = s_x + NS * ent * NV;                    // [4][256] own gphi, then [ent - 256] the halo's one component
    double* s_D = s_g + BLK * NV + (ent - BLK);           // MAT: [NS][KNP_MAX_MAT] coefficient table ; else [NS][ent]
    double* s_ft = s_D + (MAT ? NS * KNP_MAX_MAT : NS * ent);   // [ncls][25]
    int* s_draw = reinterpret_cast<int*>(s_ft + m.ncls * HALO_FTS);
    const unsigned t = threadIdx.x;
    HaloWalk w(m, counters, flip_nq);
    if (w.cur >= w.last) return;
    for (int i = t; i < m.ncls * HALO_FT; i += BLK) s_ft[(i / HALO_FT) * HALO_FTS + (i % HALO_FT)] = m.cls_ext[i];
    if (MAT && t < NS * KNP_MAX_MAT) s_D[t] = dtab[t];
    const bool hl = (int)t < m.hb_stride;
    int src = hl ? m.hb_src[(w.b_lo + w.cur) * m.hb_stride + t] : -1;
    while (w.cur < w.last) {
        const int64_t c = (w.b_lo + w.cur) * BLK + t;
        const bool valid = c >= m.c_begin && c < m.c_end;
        const bool stage = c < m.nc;
        double xv[NS][NV], y[NS][NV], gp[NV], Dk[NS];
        if (stage) {
            load_nodal<3>(gphi, c, gp);
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                load_nodal<3>(x + (int64_t)k * m.nc * NV, c, xv[k]);
                if (!MAT) Dk[k] = Dall[(int64_t)k * m.nc + c];
            }
        }
        // this thread's halo entry: the list was fetched while the previous block was being worked on
        double2 hq[NS][2];
        double hg = 0.0, hD[NS];
        if (src >= 0) {
            const int64_t Kp = src >> 2;
            hg = gphi[Kp * NV + (src & 3)];
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                const double2* px = reinterpret_cast<const double2*>(x + (int64_t)k * m.nc * NV + Kp * NV);
                hq[k][0] = px[0];
                hq[k][1] = px[1];
                if (!MAT) hD[k] = Dall[(int64_t)k * m.nc + Kp];
            }
        }
        const int src_next = (hl && w.nxt < w.last) ? m.hb_src[(w.b_lo + w.nxt) * m.hb_stride + t] : -1;
        uint32_t flags = 0, nm = 0;
        unsigned cls = 0, mymat = 0;
        uint2 lw = make_uint2(0u, 0u);
        CellGeom<3> K;
        if (valid) {
            flags = m.fflag[c];
            cls = m.cls[c];
            lw = *reinterpret_cast<const uint2*>(m.hb_loc + c * NV);
            if (MAT) {
                mymat = mat[c];
                nm = *reinterpret_cast<const uint32_t*>(nmat4 + c * NV);
            }
            load_class_gram(m.cls_table, cls, K);
        }
        int64_t drawn = 0;
        if (t == 0) drawn = w.after_next();          // behind the iteration's loads: its return does not gate them (in-order counter)
        if (stage) {
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                if (!MAT) s_D[(unsigned)k * ent + t] = Dk[k];
#pragma unroll
                for (int a = 0; a < NV; ++a) s_x[((unsigned)k * NV + a) * ent + t] = xv[k][a];
            }
#pragma unroll
            for (int a = 0; a < NV; ++a) s_g[a * BLK + t] = gp[a];
        }
        if (src >= 0) {
            s_g[BLK * NV + t] = hg;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                double* dst = s_x + (unsigned)k * NV * ent + BLK + t;
                dst[0] = hq[k][0].x; dst[ent] = hq[k][0].y; dst[2 * ent] = hq[k][1].x; dst[3 * ent] = hq[k][1].y;
                if (!MAT) s_D[(unsigned)k * ent + BLK + t] = hD[k];
            }
        }
        __syncthreads();
        if (valid) {
            if (MAT) {
#pragma unroll
                for (int k = 0; k < NS; ++k) Dk[k] = TO_LDS(s_D)[k * KNP_MAX_MAT + mymat];
            }
            const lds_double* ft = TO_LDS(s_ft) + cls * HALO_FTS;
            const double mw = ka.inv_dt * K.vol / 20.0;
#pragma unroll
            for (int k = 0; k < NS; ++k) {
                double sx = 0.0;
#pragma unroll
                for (int a = 0; a < NV; ++a) sx += xv[k][a];
                const double drift = ka.z[k] * ka.psi * Dk[k] * K.vol * sx / (double)NV;
                const double dv = Dk[k] * K.vol;
#pragma unroll
                for (int a = 0; a < NV; ++a) {
                    double s = 0.0;
#pragma unroll
                    for (int bb = 0; bb < NV; ++bb) s = fma(K.G[a][bb], xv[k][bb], s);
                    y[k][a] = fma(mw, sx + xv[k][a], fma(dv, s, drift * gp[a]));
                }
            }
            knp_facet_halo<NS, MAT, 0>(K, flags, lw.x & 0xffffu, nm & 0xffu, xv, gp, Dk, ka, TO_LDS(s_x), TO_LDS(s_g), TO_LDS(s_D), ft, ent, y);
            knp_facet_halo<NS, MAT, 1>(K, flags, lw.x >> 16, (nm >> 8) & 0xffu, xv, gp, Dk, ka, TO_LDS(s_x), TO_LDS(s_g), TO_LDS(s_D), ft, ent, y);
            knp_facet_halo<NS, MAT, 2>(K, flags, lw.y & 0xffffu, (nm >> 16) & 0xffu, xv, gp, Dk, ka, TO_LDS(s_x), TO_LDS(s_g), TO_LDS(s_D), ft, ent, y);
            knp_facet_halo<NS, MAT, 3>(K, flags, lw.y >> 16, nm >> 24, xv, gp, Dk, ka, TO_LDS(s_x), TO_LDS(s_g), TO_LDS(s_D), ft, ent, y);
#pragma unroll
            for (int k = 0; k < NS; ++k) store_nodal<3>(yout + (int64_t)k * m.nc * NV, c, y[k]);
        }
        if (t == 0) *s_draw = (int)drawn;
        __syncthreads();                   // the next block overwrites the staging
        src = src_next;
        w.advance(*s_draw);
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------------
static_assert(KNP_HALO_CTR_INTS == 2 * 2 * HALO_NQ * HALO_CPAD, "knp_ctx::halo_ctr: [2 operators][2 sets][HALO_NQ] counters, HALO_CPAD ints apart");

// KNP_APPLY_HALO=0 selects the previous staged kernels (A/B runs)
static bool halo_enabled() { return env_int("KNP_APPLY_HALO", 1) != 0; }
static unsigned halo_entries(const knp_ctx* c) { return (unsigned)(KNP_HALO_BLK + c->m.hb_stride); }
// block counters of the persistent kernels: per operator two sets of 8 that swap roles at every launch (the kernel zeroes the
// set of the launch before it; launches of one context are ordered on its stream)
static int halo_queues() {
    const int v = (env_int("KNP_HALO_NQ", 8) / 8) * 8;
    return v < 8 ? 8 : (v > HALO_NQ ? HALO_NQ : v);
}
static int* halo_counters(knp_ctx* c, int which, int* flip_nq) {
    c->halo_flip[which] ^= 1;
    const int dyn = env_int("KNP_HALO_DYN", 1) ? 2 : 0;          // default: drawn (measured: -3..7 % at 8 M cells)
    *flip_nq = c->halo_flip[which] | dyn | (halo_queues() << 2);
    return c->halo_ctr + which * 2 * HALO_NQ * HALO_CPAD;
}
// persistent grid: as many workgroups as fit on the chip at once (a multiple of the 64 chunk queues), at most one per block;
// KNP_HALO_WG_PER_CU overrides the occupancy query (tuning)
// reserve_cus: with an active communicator the interior launch runs next to the halo exchange (pack kernel + RCCL's send / receive
// kernels on the high-priority halo stream, comm.hip): a persistent grid that occupies every CU would leave them nothing to run on
// until its first workgroups retire, so it is sized for (CUs - reserve_cus).
template <typename KernelT> static dim3 halo_grid(knp_ctx* c, const MeshDev& m, KernelT kernel, size_t lds, int reserve_cus) {
    const int64_t nb = (m.c_end - 1) / KNP_HALO_BLK - m.c_begin / KNP_HALO_BLK + 1;
    const int ncu = c->ncu;
    int per_cu = env_int("KNP_HALO_WG_PER_CU", 0);
    if (per_cu <= 0) {
        auto& cache = c->halo_wg_per_cu;                                       // one occupancy query per context, kernel instance and LDS size
        const auto key = std::make_pair((const void*)kernel, lds);
        auto it = cache.find(key);
        if (it == cache.end()) {
            int n = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kernel, KNP_HALO_BLK, lds) != hipSuccess || n < 1) n = 2;
            it = cache.emplace(key, n).first;
        }
        per_cu = it->second;
    }
    if (per_cu < 1) per_cu = 1;
    const int64_t nq = halo_queues();
    const int cus = std::max(ncu - std::max(reserve_cus, 0), ncu / 2);
    int64_t g = std::min<int64_t>(((nb + nq - 1) / nq) * nq, (int64_t)per_cu * cus);
    g = std::max<int64_t>(nq, (g / nq) * nq);
    return dim3((unsigned)g);
}

// the halo-staged persistent KNP kernel is usable when the class and halo tables exist, at most two species are solved and
// the block's LDS footprint stays below 64 KB
static bool knp_halo_usable(const knp_ctx* c, size_t* lds_bytes, bool* with_materials) {
    if (c->degree != 1 || c->m.dim != 3 || !c->m.cls || !c->m.hb_stride || !c->halo_ctr || c->p.n_sys > 2 || !halo_enabled()) return false;
    const bool matp = env_int("KNP_APPLY_MAT", 1) != 0 && c->nmat > 0;
    const size_t ns = (size_t)c->p.n_sys, ent = halo_entries(c);
    const size_t lds = sizeof(double) * (ns * ent * 4 + KNP_HALO_BLK * 4 + (ent - KNP_HALO_BLK) + (matp ? ns * KNP_MAX_MAT : ns * ent) +
                                         (size_t)c->m.ncls * HALO_FTS + 1);
    if (lds_bytes) *lds_bytes = lds;
    if (with_materials) *with_materials = matp;
    return lds <= 65536;
}

// one launch on the cell range of m (inside [0, hb_long0 * 256)); lds and matp are knp_halo_usable's answers.  Swaps the counter sets.
static int knp_halo_launch(knp_ctx* c, const MeshDev& m, const double* x, const double* gphi, double* y, const KnpArgs& ka, size_t lds,
                           bool matp, int reserve_cus) {
    const unsigned ent = halo_entries(c);
    int flip_nq = 0;
    int* ctr = halo_counters(c, 1, &flip_nq);
    auto launch = [&](auto ns, auto mat) {
        const auto kernel = k_knp_apply_halo<decltype(ns)::value, decltype(mat)::value>;
        hipLaunchKernelGGL(kernel, halo_grid(c, m, kernel, lds, reserve_cus), dim3(KNP_HALO_BLK), lds, c->stream, m, x, gphi, c->D, y, ka,
                           ent, (const uint8_t*)c->mat, (const uint8_t*)c->nmat4, (const double*)c->dtab, ctr, flip_nq);
        return 0;
    };
    dispatch_nsys<2>(c->p.n_sys, [&](auto ns) { return matp ? launch(ns, std::true_type()) : launch(ns, std::false_type()); });
    HIPCHK(c, hipGetLastError());
    return 0;
}
