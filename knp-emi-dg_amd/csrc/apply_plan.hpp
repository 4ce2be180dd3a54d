// Which kernel family an operator apply runs, and on which cells: the one definition that the launchers of apply_p1.hip walk and that
// apply_variant reports (knp_apply_variant in include/knpemi_hip.h; bench.py and the tests name the kernel they measured by it).
// Plain host C++ without HIP headers or the context: tools/apply_plan_check.cpp compiles it alone and checks the selection on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>

// the values are the variant codes of the ABI
enum ApplyFamily : int {
    AF_COORD = 0,         // coordinate path, any mesh (apply_p1_direct.hpp)
    AF_CLS = 1,           // geometry classes + LDS staging (apply_p1_cls.hpp)
    AF_HALO = 2,          // halo-staged persistent KNP kernel, D per cell (apply_p1_halo.hpp)
    AF_RING_EMI = 3,      // ring-staged EMI (apply_ring.hip)
    AF_HALO_MAT = 6,      // halo-staged, D from the material table
    AF_RING_KNP = 7,      // ring-staged KNP, material table (apply_ring.hip)
    AF_P2 = 8,            // matrix-free P2 (apply_p2.hip)
    AF_P2_ASSEMBLED = 9,  // assembled P2 blocks (tab_assembled.hip)
    AF_RING_U = 10        // ring-staged without geometry classes (apply_ring_u.hip)
};

constexpr int64_t APPLY_PLAN_BLK = 256;             // cells per block of the halo tables (KNP_HALO_BLK)
constexpr int64_t APPLY_ALL_CELLS = INT64_MAX;

// What the selection depends on, as plain values.  ring / ring_u_cells / halo are what the families' owners answered for the operator
// the plan is asked for (ring_usable, ring_u_cells, knp_halo_usable): the LDS limits behind those answers stay with the slot layouts.
struct ApplyInputs {
    int degree = 1, dim = 3;
    bool p2_assembled = false;
    bool cls = false;             // geometry classes present
    int ncls = 0, ncls_max = 0;   // their count, and the most the LDS-staged kernels hold (CLS_MAX_LDS)
    int n_sys = 1;                // solved species
    int64_t hb_long0 = 0;         // blocks [0, hb_long0) have halo lists that fit one entry per thread
    bool ring = false;
    int64_t ring_u_cells = 0;     // leading cells the unstructured ring covers
    bool halo = false, halo_mat = false;
};

// The head family takes the cells below head_cells, the tail family (a thread-per-cell kernel) the cut cells behind them.
// Without a staged head, head == tail and head_cells is APPLY_ALL_CELLS.
struct ApplyPlan { ApplyFamily head; int64_t head_cells; ApplyFamily tail; };

// which: 0 EMI, 1 KNP.  EMI: ring, unstructured ring, classes, coordinates.  KNP: ring, unstructured ring, halo, classes, coordinates.
// head_cells may be 0 (a usable ring on a mesh with hb_long0 == 0): then, and for any range that starts at or behind head_cells, only
// the tail kernel runs, while the head -- what apply_variant reports, which knows no range -- still names the ring family.
inline ApplyPlan plan_apply(const ApplyInputs& in, int which) {
    if (in.degree != 1) {
        const ApplyFamily f = in.p2_assembled ? AF_P2_ASSEMBLED : AF_P2;
        return {f, APPLY_ALL_CELLS, f};
    }
    const bool classed = in.dim == 3 && in.cls && in.ncls <= in.ncls_max && (which == 0 || in.n_sys <= 3);
    const ApplyFamily tail = classed ? AF_CLS : AF_COORD;
    const int64_t short_list_cells = in.hb_long0 * APPLY_PLAN_BLK;
    if (in.ring) return {which == 1 ? AF_RING_KNP : AF_RING_EMI, short_list_cells, tail};
    if (in.ring_u_cells > 0) return {AF_RING_U, in.ring_u_cells, tail};
    if (which == 1 && in.halo) return {in.halo_mat ? AF_HALO_MAT : AF_HALO, short_list_cells, tail};
    return {tail, APPLY_ALL_CELLS, tail};
}

struct ApplySegment { ApplyFamily family; int64_t begin, end; };

// the launches of the cell range [begin, end): none for an empty range, else the head's part and / or the tail's.  Returns their count.
inline int apply_segments(const ApplyPlan& p, int64_t begin, int64_t end, ApplySegment seg[2]) {
    int n = 0;
    if (begin < end && begin < p.head_cells) {
        seg[n++] = {p.head, begin, std::min(end, p.head_cells)};
        begin = seg[0].end;
    }
    if (begin < end) seg[n++] = {p.tail, begin, end};
    return n;
}
