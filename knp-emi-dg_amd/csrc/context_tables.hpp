// Host-side steps of knp_ctx_create and knp_set_params (context.hip): the tables derived from the caller's raw mesh and coefficient
// arrays.  Plain C++ on host memory, no HIP call, so that a stand-alone program can run them too (tools/check_context_tables.cpp).
#pragma once
#include "knpemi_internal.hpp"
#include <algorithm>
#include <cmath>
#include <thread>

// contiguous chunks of [0, n) on a few host threads (the O(cells) table loops of knp_ctx_create: 0.6 s in one thread at 8 x 10^6 tets)
template <typename F> static void host_chunks(int64_t n, F f) {
    int nt = (int)std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char* ev = getenv("KNP_SETUP_THREADS")) nt = std::max(1, atoi(ev));
    nt = std::min(nt, 64);                                             // callers keep per-thread results in 64 slots
    if (n < (int64_t(1) << 16) || nt == 1) { f(0, n, 0); return; }
    std::vector<std::thread> pool;
    const int64_t chunk = (n + nt - 1) / nt;
    for (int t = 0; t < nt; ++t) {
        const int64_t lo = t * chunk, hi = std::min(n, lo + chunk);
        if (lo >= hi) break;
        pool.emplace_back([=]() { f(lo, hi, t); });
    }
    for (auto& th : pool) th.join();
}

// the caller's mesh as knp_ctx_create receives it (NV = dim + 1 vertices / facets per cell)
struct MeshIn {
    int dim, NV;
    int64_t nv, nc, nc_owned, nf;
    const double* coords;
    const int32_t* cells;
    const uint32_t* cell_tags;
    const int32_t* facet_cells;
    const int8_t* facet_local;
    const uint32_t* facet_tags;
    int n_membrane_tags;
    const uint32_t* membrane_tags;
};

struct FacetTables {
    std::vector<int32_t> nbr, cfacet;   // [nc][NV] neighbour cell / global facet behind every local facet, -1: none
    std::vector<uint8_t> fb;            // [nc][NV] flag bytes (knpemi_internal.hpp: FK_*)
    std::vector<uint32_t> fflag;        // [nc] the cell's flag bytes packed
    std::vector<int32_t> mf;            // [nmf][6] membrane facets in facet order: cell_e, cell_i, lf_e, lf_i, facet, owner flag
};

// Validates the cell and facet tables and derives the per-(cell, local facet) tables.  Null, or what is wrong with the input.
// NOTE: the facet matching relies on both cells of a facet listing the shared vertices in the same
// relative order (ascending ids in the caller's numbering); the ids themselves may be relabelled for
// storage locality, so they are not required to be ascending here.
static const char* facet_tables(const MeshIn& in, FacetTables& T) {
    const int NV = in.NV;
    const int64_t nc = in.nc, nc_owned = in.nc_owned;
    {
        int bad[64] = {0};
        host_chunks(nc * NV, [&](int64_t lo, int64_t hi, int t) {
            for (int64_t i = lo; i < hi; ++i)
                if (in.cells[i] < 0 || in.cells[i] >= in.nv) bad[t & 63] = 1;
        });
        for (int b : bad)
            if (b) return "cell vertex index out of range";
    }
    T.nbr.assign(nc * NV, -1);
    T.cfacet.assign(nc * NV, -1);
    T.fflag.assign(nc, 0);
    T.fb.assign(nc * NV, (uint8_t)(FK_EXTERIOR << 2));
    T.mf.clear();
    auto is_mem = [&](uint32_t t) {
        for (int i = 0; i < in.n_membrane_tags; ++i) if (in.membrane_tags[i] == t) return true;
        return false;
    };
    // facets in contiguous chunks: a (cell, local facet) entry belongs to exactly one facet, so the chunks write disjoint entries; the
    // membrane facets of a chunk are collected per chunk and appended in chunk order = facet order
    std::vector<std::vector<int32_t>> mf_part(64);
    int bad[64] = {0};
    host_chunks(in.nf, [&](int64_t flo, int64_t fhi, int tid) {
        auto& mine = mf_part[(size_t)(tid & 63)];
        for (int64_t f = flo; f < fhi; ++f) {
            const int64_t c0 = in.facet_cells[2 * f], c1 = in.facet_cells[2 * f + 1];
            const int l0 = in.facet_local[2 * f], l1 = in.facet_local[2 * f + 1];
            if (c0 < 0 || c0 >= nc || l0 < 0 || l0 >= NV || c1 >= nc || (c1 >= 0 && (l1 < 0 || l1 >= NV))) { bad[tid & 63] = 1; continue; }
            T.cfacet[c0 * NV + l0] = (int32_t)f;
            if (c1 < 0) continue;
            T.cfacet[c1 * NV + l1] = (int32_t)f;
            const uint32_t t = in.facet_tags[f];
            const uint32_t kind = (t == 0) ? FK_SIPG : (is_mem(t) ? FK_MEMBRANE : FK_INACTIVE);
            // plus (normal-leaving, lower tag) side; on equal tags the reference takes n('-'), i.e. side 1
            const int e_side = (in.cell_tags[c0] >= in.cell_tags[c1]) ? 1 : 0;
            T.nbr[c0 * NV + l0] = (int32_t)c1;
            T.nbr[c1 * NV + l1] = (int32_t)c0;
            T.fb[c0 * NV + l0] = (uint8_t)((l1 & 3) | (kind << 2) | ((e_side == 0 ? 1u : 0u) << 4));
            T.fb[c1 * NV + l1] = (uint8_t)((l0 & 3) | (kind << 2) | ((e_side == 1 ? 1u : 0u) << 4));
            if (kind == FK_MEMBRANE) {
                const int64_t ce = e_side == 0 ? c0 : c1, ci = e_side == 0 ? c1 : c0;
                const int le = e_side == 0 ? l0 : l1, li = e_side == 0 ? l1 : l0;
                const int active = (ce < nc_owned || ci < nc_owned) ? 1 : 0;
                mine.insert(mine.end(), {(int32_t)ce, (int32_t)ci, le, li, (int32_t)f, active});
            }
        }
    });
    for (int b : bad)
        if (b) return "facet table entry out of range";
    for (auto& part : mf_part) T.mf.insert(T.mf.end(), part.begin(), part.end());
    int missing[64] = {0};
    host_chunks(nc, [&](int64_t lo, int64_t hi, int tid) {
        for (int64_t k = lo; k < hi; ++k) {
            uint32_t w = 0;
            for (int a = 0; a < NV; ++a) {
                w |= (uint32_t)T.fb[k * NV + a] << (8 * a);
                if (k < nc_owned && T.cfacet[k * NV + a] < 0) missing[tid & 63] = 1;     // owned cells must have every neighbour present (one ghost layer)
            }
            T.fflag[k] = w;
        }
    });
    for (int b : missing)
        if (b) return "owned cell with a facet missing from the facet table";
    return nullptr;
}

// cell diameters (UFL CellDiameter: longest edge) and 1 / cell volume (weights of the residual norms)
static void cell_metrics(const MeshIn& in, std::vector<double>& hcell, std::vector<float>& ivol) {
    const int dim = in.dim, NV = in.NV;
    const double* coords = in.coords;
    const int32_t* cells = in.cells;
    hcell.assign(in.nc, 0.0);
    ivol.assign((size_t)in.nc, 1.0f);
    host_chunks(in.nc, [&](int64_t klo, int64_t khi, int) {
        for (int64_t k = klo; k < khi; ++k) {
            double h2 = 0.0;
            for (int a = 0; a < NV; ++a)
                for (int b = a + 1; b < NV; ++b) {
                    double d2 = 0.0;
                    for (int q = 0; q < dim; ++q) {
                        const double d = coords[(int64_t)cells[k * NV + a] * dim + q] - coords[(int64_t)cells[k * NV + b] * dim + q];
                        d2 += d * d;
                    }
                    h2 = std::max(h2, d2);
                }
            hcell[k] = std::sqrt(h2);
            double e[3][3] = {{0.0}};
            for (int a = 0; a < dim; ++a)
                for (int q = 0; q < dim; ++q)
                    e[a][q] = coords[(int64_t)cells[k * NV + a + 1] * dim + q] - coords[(int64_t)cells[k * NV] * dim + q];
            const double det = dim == 2 ? e[0][0] * e[1][1] - e[0][1] * e[1][0]
                                        : e[0][0] * (e[1][1] * e[2][2] - e[1][2] * e[2][1]) - e[0][1] * (e[1][0] * e[2][2] - e[1][2] * e[2][0]) +
                                          e[0][2] * (e[1][0] * e[2][1] - e[1][1] * e[2][0]);
            const double vol = std::fabs(det) / (dim == 2 ? 2.0 : 6.0);
            ivol[(size_t)k] = vol > 0.0 ? (float)(1.0 / vol) : 0.0f;
        }
    });
}

struct HaloLists {
    std::vector<int32_t> src;    // MeshDev::hb_src
    std::vector<uint16_t> loc;   // MeshDev::hb_loc
    int stride = 0;              // 0: no lists (no block has a coupled neighbour outside it, or the first block's list is too long)
    int64_t long0 = 0;
};

// halo- / ring-staged applies (3D): per block of 256 consecutive cells, the coupled (SIPG or membrane: a_emi couples both) neighbours
// outside the block
static void halo_block_lists(int64_t nc_owned, const FacetTables& T, HaloLists& H) {
    const int64_t B = KNP_HALO_BLK, nblk = (nc_owned + B - 1) / B;
    std::vector<std::vector<int32_t>> lists((size_t)nblk);
    H.loc.assign((size_t)nc_owned * 4, 0);
    for (int64_t b = 0; b < nblk; ++b) {
        auto& L = lists[(size_t)b];
        for (int64_t k = b * B; k < std::min(nc_owned, (b + 1) * B); ++k)
            for (int a = 0; a < 4; ++a) {
                const uint32_t kind = (T.fb[k * 4 + a] >> 2) & 3u;
                const int64_t nbk = T.nbr[k * 4 + a];
                if ((kind != FK_SIPG && kind != FK_MEMBRANE) || nbk < 0) continue;
                if (nbk / B == b) { H.loc[k * 4 + a] = (uint16_t)(nbk - b * B); continue; }
                H.loc[k * 4 + a] = (uint16_t)(B + L.size());
                L.push_back((int32_t)(nbk * 4 + (T.fb[k * 4 + a] & 3u)));
            }
    }
    // a partition's cells on the cut come last and sit in a plane: nearly all their neighbours are outside their block.  Blocks
    // whose list does not fit one entry per thread are left to the LDS-staged kernel: the halo-staged one covers [0, hb_long0 * 256)
    int64_t long0 = nblk;
    for (int64_t b = 0; b < nblk; ++b)
        if ((int64_t)lists[(size_t)b].size() > B) { long0 = b; break; }
    int hmax = 0;
    for (int64_t b = 0; b < long0; ++b) hmax = std::max(hmax, (int)lists[(size_t)b].size());
    const int hs = ((hmax + 7) / 8) * 8;
    if (hs == 0 || long0 == 0) return;
    H.src.assign((size_t)nblk * hs, -1);
    for (int64_t b = 0; b < long0; ++b) std::copy(lists[(size_t)b].begin(), lists[(size_t)b].end(), H.src.begin() + b * hs);
    H.stride = hs;
    H.long0 = long0;
}

// Material ids: the distinct coefficient tuples (D_0 .. D_{ni-1}) over the cells, numbered in order of first appearance.  D is
// [ni][nc]; id gets [nc] and tuples [count][ni].  Returns the count, or -1 (id and tuples cleared) beyond `cap` distinct tuples.
static int scan_materials(int64_t nc, int ni, const double* D, int cap, std::vector<uint16_t>& id, std::vector<double>& tuples) {
    id.assign((size_t)nc, 0);
    tuples.clear();
    int nm = 0;
    for (int64_t k = 0; k < nc; ++k) {
        int q = nm - 1;                                            // neighbours in the cell order mostly share the material: newest first
        for (; q >= 0; --q) {
            bool same = true;
            for (int i = 0; i < ni && same; ++i) same = tuples[(size_t)q * ni + i] == D[(int64_t)i * nc + k];
            if (same) break;
        }
        if (q < 0) {
            if (nm == cap) { id.clear(); tuples.clear(); return -1; }
            for (int i = 0; i < ni; ++i) tuples.push_back(D[(int64_t)i * nc + k]);
            q = nm++;
        }
        id[(size_t)k] = (uint16_t)q;
    }
    return nm;
}
