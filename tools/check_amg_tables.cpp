// CPU check of the host tables of the DG -> conforming restriction (knp-emi-dg_amd/csrc/amg_tables.hpp): the inverse of dg2cg and the
// tile / slot / part tables whose summation order k_restrict_tiles / k_restrict_sum and the two fused kernels of krylov.hip follow bit
// for bit.  Runs on the mesh dumped by tools/dump_context_mesh.py (its P1 map: the cell's vertices); no GPU call and no HIP header;
// meant to be built with the host sanitizers:
//   python tools/dump_context_mesh.py /tmp/small_3d.bin
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -pthread -I knp-emi-dg_amd/csrc \
//       tools/check_amg_tables.cpp -o /tmp/check_amg_tables && /tmp/check_amg_tables /tmp/small_3d.bin
// Exit status 0 and "amg tables ok" = every check holds (and the sanitizers had nothing to report).
#include "amg_tables.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <numeric>

static int failures = 0;
#define EXPECT(cond, what)                                                                   \
    do {                                                                                     \
        if (!(cond)) { if (++failures <= 20) std::printf("FAIL %s: %s\n", tag, what); }      \
    } while (0)

static void check_inverse(const char* tag, const std::vector<int32_t>& dg2cg, int64_t n_own, int nd, int64_t ncg) {
    const CgInverse inv = cg_inverse(dg2cg.data(), n_own, nd, ncg);
    const int64_t nown = n_own * nd;
    std::vector<int32_t> order((size_t)nown);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return dg2cg[a] < dg2cg[b]; });
    EXPECT(inv.idx == order, "the inverse map is a stable sort of dg2cg over the owned dofs");
    EXPECT((int64_t)inv.ptr.size() == ncg + 1 && inv.ptr[0] == 0 && inv.ptr[(size_t)ncg] == nown, "inverse row pointers");
    for (int64_t v = 0; v < ncg; ++v)
        for (int32_t k = inv.ptr[v]; k < inv.ptr[v + 1]; ++k) EXPECT(dg2cg[inv.idx[k]] == v, "inverse entry maps to its row");
}

static void check_tiles(const char* tag, const std::vector<int32_t>& dg2cg, int64_t n_own, int nd, int64_t ncg, int tile_cells) {
    const TileTablesHost T = restrict_tile_tables(dg2cg.data(), n_own, nd, ncg, tile_cells);
    const int64_t nown = n_own * nd, tile_dofs = (int64_t)tile_cells * nd;
    EXPECT(T.tile_cells == tile_cells && T.ntiles == (n_own + tile_cells - 1) / tile_cells, "tile count");
    EXPECT((int64_t)T.tile_off.size() == T.ntiles + 1 && T.tile_off[0] == 0 && T.tile_off.back() == T.nslots, "tile offsets");
    EXPECT((int64_t)T.slot_ptr.size() == T.nslots + 1 && T.slot_ptr[0] == 0 && T.slot_ptr.back() == nown, "slot pointers");
    EXPECT((int64_t)T.slot_idx.size() == nown, "one slot entry per owned DG dof");
    if (failures) return;
    std::vector<int32_t> slot_cg((size_t)T.nslots, -1);
    std::vector<int> seen((size_t)nown, 0);
    for (int64_t t = 0; t < T.ntiles; ++t) {
        const int64_t d0 = t * tile_dofs, n = std::min(nown - d0, tile_dofs);
        for (int32_t p = T.tile_off[t]; p < T.tile_off[t + 1]; ++p) {
            EXPECT(T.slot_ptr[p] < T.slot_ptr[p + 1], "no empty slot");
            for (int32_t k = T.slot_ptr[p]; k < T.slot_ptr[p + 1]; ++k) {
                const int64_t loc = T.slot_idx[k];
                EXPECT(loc < n, "slot entry inside its own tile");
                if (loc >= n) continue;
                ++seen[(size_t)(d0 + loc)];
                if (k == T.slot_ptr[p]) slot_cg[p] = dg2cg[d0 + loc];
                else {
                    EXPECT(dg2cg[d0 + loc] == slot_cg[p], "entries of one slot map to one conforming dof");
                    EXPECT(T.slot_idx[k - 1] < loc, "entries of a slot in ascending tile-local order");
                }
            }
            if (p > T.tile_off[t]) EXPECT(slot_cg[p - 1] < slot_cg[p], "slots of a tile in ascending conforming-dof order");
        }
    }
    for (int64_t i = 0; i < nown; ++i) EXPECT(seen[(size_t)i] == 1, "every owned DG dof occurs exactly once");
    EXPECT((int64_t)T.part_ptr.size() == ncg + 1 && T.part_ptr[0] == 0 && T.part_ptr.back() == T.nslots, "part pointers");
    EXPECT((int64_t)T.part_idx.size() == T.nslots, "one part entry per slot");
    if (failures) return;
    std::vector<int> hit((size_t)T.nslots, 0);
    for (int64_t v = 0; v < ncg; ++v)
        for (int32_t k = T.part_ptr[v]; k < T.part_ptr[v + 1]; ++k) {
            const int32_t p = T.part_idx[k];
            EXPECT(p >= 0 && p < T.nslots, "part entry names a slot");
            if (p < 0 || p >= T.nslots) continue;
            ++hit[p];
            EXPECT(slot_cg[p] == v, "part entries grouped by conforming dof");
            if (k > T.part_ptr[v]) EXPECT(T.part_idx[k - 1] < p, "slots of a conforming dof in ascending order");
        }
    for (int64_t p = 0; p < T.nslots; ++p) EXPECT(hit[(size_t)p] == 1, "part_idx is a permutation of the slots");
    // the two-stage sum of an integer-valued vector (exact in any order) against the direct sum per conforming dof
    std::vector<double> r((size_t)nown), direct((size_t)ncg, 0.0), part((size_t)T.nslots), rc((size_t)ncg);
    for (int64_t i = 0; i < nown; ++i) { r[i] = (double)(((uint64_t)i * 2654435761u) % 2001) - 1000.0; direct[dg2cg[i]] += r[i]; }
    for (int64_t t = 0; t < T.ntiles; ++t)
        for (int32_t p = T.tile_off[t]; p < T.tile_off[t + 1]; ++p) {
            double acc = 0.0;
            for (int32_t k = T.slot_ptr[p]; k < T.slot_ptr[p + 1]; ++k) acc += r[(size_t)(t * tile_dofs + T.slot_idx[k])];
            part[p] = acc;
        }
    for (int64_t v = 0; v < ncg; ++v) {
        double s = 0.0;
        for (int32_t k = T.part_ptr[v]; k < T.part_ptr[v + 1]; ++k) s += part[T.part_idx[k]];
        rc[v] = s;
    }
    EXPECT(rc == direct, "two-stage sum equals the direct sum");
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: %s MESH.bin\n", argv[0]); return 2; }
    std::ifstream fs(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(fs)), std::istreambuf_iterator<char>());
    if (raw.size() < 64) { std::printf("cannot read %s\n", argv[1]); return 2; }
    // the header and layout of tools/dump_context_mesh.py; only nv (= ncg of the P1 space) and the dg2cg block at the end are used
    int64_t hd[8];
    memcpy(hd, raw.data(), sizeof(hd));
    const int nd = (int)hd[0] + 1;
    const int64_t nc = hd[2], ncg = hd[7];
    const size_t bytes = sizeof(int32_t) * (size_t)nc * nd;
    if (ncg <= 0 || ncg != hd[1] || raw.size() < 64 + bytes) { std::printf("%s: no dg2cg block\n", argv[1]); return 2; }
    std::vector<int32_t> dg2cg((size_t)nc * nd);           // an allocation of its own: an overrun is the sanitizer's to see
    memcpy(dg2cg.data(), raw.data() + raw.size() - (bytes + 7) / 8 * 8, bytes);
    for (int32_t v : dg2cg)
        if (v < 0 || v >= ncg) { std::printf("%s: dg2cg out of range\n", argv[1]); return 2; }

    const int builtin = nd <= 4 ? 512 : 256;               // knp_amg_begin's tile size
    int ntables = 0;
    for (int64_t n_own : {nc, nc - nc / 3}) {              // all cells owned; a third of them ghosts
        char tag[96];
        std::snprintf(tag, sizeof tag, "%lld owned cells", (long long)n_own);
        check_inverse(tag, dg2cg, n_own, nd, ncg);
        for (int tile_cells : {builtin, 1, 3, (int)nc + 5}) {
            if (!tiles_usable(tile_cells, nd)) continue;   // (an odd number of values per tile: 2D P1 with 1 or 3 cells)
            std::snprintf(tag, sizeof tag, "%lld owned cells, tiles of %d", (long long)n_own, tile_cells);
            check_tiles(tag, dg2cg, n_own, nd, ncg, tile_cells);
            ++ntables;
        }
    }
    {   // where the tile kernels cannot run there are no tables: more than 64 KB of values, an odd number of them, no owned cell
        const char* tag = "unusable tiles";
        EXPECT(!tiles_usable(65536 / 8 / nd + 1, nd) && restrict_tile_tables(dg2cg.data(), nc, nd, ncg, 65536 / 8 / nd + 1).ntiles == 0, "beyond 64 KB");
        EXPECT(tiles_usable(65536 / 8 / nd, nd) == ((65536 / 8 / nd * nd) % 2 == 0), "64 KB exactly");
        EXPECT(!tiles_usable(1, 3) && !tiles_usable(3, 3) && tiles_usable(2, 3), "odd tile sizes");
        EXPECT(restrict_tile_tables(dg2cg.data(), 0, nd, ncg, builtin).ntiles == 0, "no owned cell");
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("amg tables ok: %lld cells, %lld conforming dofs, %d table sets\n", (long long)nc, (long long)ncg, ntables);
    return 0;
}
