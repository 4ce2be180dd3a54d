// Host-side tables of the DG -> conforming restriction (amg_upload.hip: knp_amg_begin uploads them; amg_restrict.hip and the fused kernels
// of krylov.hip read them).  Plain C++ on host memory, no HIP include, so that a stand-alone program can build and check them too
// (tools/check_amg_tables.cpp).  Everything here is a function of dg2cg (conforming dof of every DG dof, owned cells first), the number
// of owned cells, the dofs per cell nd, the number of conforming dofs ncg and the tile size.
#pragma once
#include <algorithm>
#include <cstdint>
#include <thread>
#include <utility>
#include <vector>

// CSR list conforming dof -> the OWNED DG dofs that inject into it, ascending: a stable counting sort of dg2cg over the owned dofs
// (instead of the caller's argsort of nc nd keys).  The gather restriction k_dg_restrict sums in this order.
struct CgInverse {
    std::vector<int32_t> ptr, idx;      // [ncg + 1], [n_owned_cells * nd]
};

inline CgInverse cg_inverse(const int32_t* dg2cg, int64_t n_owned_cells, int nd, int64_t ncg) {
    const int64_t nown = n_owned_cells * nd;
    CgInverse inv;
    inv.ptr.assign((size_t)ncg + 1, 0);
    for (int64_t i = 0; i < nown; ++i) ++inv.ptr[(size_t)dg2cg[i] + 1];
    for (int64_t v = 0; v < ncg; ++v) inv.ptr[(size_t)v + 1] += inv.ptr[(size_t)v];
    inv.idx.resize((size_t)nown);
    std::vector<int32_t> fill(inv.ptr.begin(), inv.ptr.end() - 1);
    for (int64_t i = 0; i < nown; ++i) inv.idx[(size_t)fill[(size_t)dg2cg[i]]++] = (int32_t)i;
    return inv;
}

// Tile-wise restriction: every tile of tile_cells consecutive owned cells (device order = Morton: a tile is a compact patch) sums, per
// conforming dof it touches (a "slot"), the tile's DG values out of LDS; the slots of one conforming dof are then added in ascending
// slot order.  Both orders are fixed HERE and are a bit-for-bit contract with every kernel that goes through tile_slot_sums (amg.hpp).
struct TileTablesHost {
    int tile_cells = 0;
    int64_t ntiles = 0, nslots = 0;     // ntiles = 0: no tables (tiles not usable, or no owned cell): the gather restriction runs
    std::vector<int32_t> tile_off;      // [ntiles + 1] first slot of every tile
    std::vector<int32_t> slot_ptr;      // [nslots + 1] CSR over slot_idx
    std::vector<uint16_t> slot_idx;     // [n_owned_cells * nd] tile-local DG dof index, grouped by slot, ascending within a slot
    std::vector<int32_t> part_ptr, part_idx;   // CSR: conforming dof -> its slots, ascending
};

// THE condition under which the tile kernels may run: a tile's values fit the 64 KB of dynamic LDS a workgroup can ask for (which also
// keeps a tile-local index inside uint16_t), and their count is even (k_restrict_tiles loads an aligned column in pairs).
inline bool tiles_usable(int64_t tile_cells, int nd) {
    return tile_cells > 0 && tile_cells * nd * (int64_t)sizeof(double) <= 65536 && (tile_cells * nd) % 2 == 0;
}

inline TileTablesHost restrict_tile_tables(const int32_t* dg2cg, int64_t n_owned_cells, int nd, int64_t ncg, int tile_cells) {
    TileTablesHost T;
    if (n_owned_cells <= 0 || !tiles_usable(tile_cells, nd)) return T;
    const int64_t n_own = n_owned_cells, ntiles = (n_own + tile_cells - 1) / tile_cells;
    // the per-tile sorts (2 048 keys each, ~2 000 tiles at 10^6 cells) run on a few host threads; the lists are stitched in tile order
    std::vector<std::vector<std::pair<int32_t, uint16_t>>> sorted((size_t)ntiles);
    {
        const int nthreads = (int)std::max<int64_t>(1, std::min<int64_t>(8, ntiles / 64));
        std::vector<std::thread> pool;
        for (int w = 0; w < nthreads; ++w)
            pool.emplace_back([&, w]() {
                for (int64_t t = w; t < ntiles; t += nthreads) {
                    const int64_t c0 = t * tile_cells, c1 = std::min<int64_t>(n_own, c0 + tile_cells);
                    auto& v = sorted[(size_t)t];
                    v.reserve((size_t)(c1 - c0) * nd);
                    for (int64_t i = c0 * nd; i < c1 * nd; ++i) v.emplace_back(dg2cg[i], (uint16_t)(i - c0 * nd));
                    std::sort(v.begin(), v.end());
                }
            });
        for (auto& th : pool) th.join();
    }
    std::vector<int32_t> slot_cg;       // conforming dof of every slot
    T.tile_off.assign((size_t)ntiles + 1, 0);
    T.slot_ptr.assign(1, 0);
    T.slot_idx.reserve((size_t)n_own * nd);
    for (int64_t t = 0; t < ntiles; ++t) {
        const auto& tmp = sorted[(size_t)t];
        for (size_t k = 0; k < tmp.size(); ++k) {
            if (k == 0 || tmp[k].first != tmp[k - 1].first) {
                if (k) T.slot_ptr.push_back((int32_t)T.slot_idx.size());
                slot_cg.push_back(tmp[k].first);
            }
            T.slot_idx.push_back(tmp[k].second);
        }
        if (!tmp.empty()) T.slot_ptr.push_back((int32_t)T.slot_idx.size());
        T.tile_off[(size_t)t + 1] = (int32_t)slot_cg.size();
    }
    const int64_t nslots = (int64_t)slot_cg.size();
    T.part_ptr.assign((size_t)ncg + 1, 0);
    T.part_idx.resize((size_t)nslots);
    for (int64_t p = 0; p < nslots; ++p) ++T.part_ptr[(size_t)slot_cg[(size_t)p] + 1];
    for (int64_t v = 0; v < ncg; ++v) T.part_ptr[(size_t)v + 1] += T.part_ptr[(size_t)v];
    std::vector<int32_t> fill(T.part_ptr.begin(), T.part_ptr.end() - 1);
    for (int64_t p = 0; p < nslots; ++p) T.part_idx[(size_t)fill[(size_t)slot_cg[(size_t)p]]++] = (int32_t)p;
    T.tile_cells = tile_cells; T.ntiles = ntiles; T.nslots = nslots;
    return T;
}
