// CPU check of the host steps of knp_ctx_create and knp_set_params (knp-emi-dg_amd/csrc/context_tables.hpp): facet / neighbour tables,
// cell metrics, halo block lists and the material scan, on a mesh dumped by tools/dump_context_mesh.py.  No GPU call is made; meant
// to be built with the host sanitizers:
//   python tools/dump_context_mesh.py /tmp/small_3d.bin
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-omit-frame-pointer -pthread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -I knp-emi-dg_amd/csrc tools/check_context_tables.cpp -o /tmp/check_context_tables && /tmp/check_context_tables /tmp/small_3d.bin
// Exit status 0 and "context tables ok" = every check holds (and the sanitizers had nothing to report).
#include "context_tables.hpp"
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

static int failures = 0;
#define EXPECT(cond, what)                                  \
    do {                                                    \
        if (!(cond)) { std::printf("FAIL %s\n", what); ++failures; } \
    } while (0)

// ids must number the distinct tuples by first appearance
static void check_scan(const char* name, int64_t nc, int ni, const std::vector<double>& D, int cap, int want) {
    std::vector<uint16_t> id;
    std::vector<double> tuples;
    const int nm = scan_materials(nc, ni, D.data(), cap, id, tuples);
    if (nm != want) { std::printf("FAIL %s: %d materials, expected %d\n", name, nm, want); ++failures; return; }
    if (nm < 0) { EXPECT(id.empty() && tuples.empty(), "scan beyond the cap leaves nothing"); return; }
    EXPECT((int64_t)id.size() == nc && (int)tuples.size() == nm * ni, "scan sizes");
    int next = 0;
    for (int64_t k = 0; k < nc; ++k) {
        int64_t first = k;
        for (int64_t j = 0; j < k && first == k; ++j) {
            bool same = true;
            for (int i = 0; i < ni && same; ++i) same = D[(size_t)i * nc + j] == D[(size_t)i * nc + k];
            if (same) first = j;
        }
        const bool ok = first == k ? id[k] == next++ : id[k] == id[first];
        if (!ok) { std::printf("FAIL %s: id of cell %lld\n", name, (long long)k); ++failures; return; }
        for (int i = 0; i < ni; ++i) EXPECT(tuples[(size_t)id[k] * ni + i] == D[(size_t)i * nc + k], "tuple of the id");
    }
    EXPECT(next == nm, "count of first appearances");
}

int main(int argc, char** argv) {
    if (argc != 2) { std::printf("usage: %s MESH.bin\n", argv[0]); return 2; }
    std::ifstream fs(argv[1], std::ios::binary);
    std::vector<char> raw((std::istreambuf_iterator<char>(fs)), std::istreambuf_iterator<char>());
    if (raw.size() < 64) { std::printf("cannot read %s\n", argv[1]); return 2; }
    // int64 dim, nv, nc, nc_owned, nf, n_membrane_tags, n_ions, ncg; then the arrays below, each padded to 8 bytes (ncg > 0: behind them
    // dg2cg [nc][NV], which tools/check_amg_tables.cpp reads)
    int64_t hd[8];
    memcpy(hd, raw.data(), sizeof(hd));
    const int dim = (int)hd[0], NV = dim + 1, nmt = (int)hd[5], ni = (int)hd[6];
    const int64_t nv = hd[1], nc = hd[2], nc_owned = hd[3], nf = hd[4];
    size_t off = 64;
    auto take = [&](size_t bytes) {
        std::vector<char> v(raw.begin() + off, raw.begin() + off + bytes);     // own allocations: an overrun is the sanitizer's to see
        off += (bytes + 7) / 8 * 8;
        return v;
    };
    auto coords = take(sizeof(double) * nv * dim), cells = take(4 * nc * NV), ctags = take(4 * nc), fcells = take(4 * 2 * nf);
    auto flocal = take(2 * nf), ftags = take(4 * nf), mtags = take(4 * nmt), Draw = take(sizeof(double) * ni * nc);
    if (hd[7] > 0) take(4 * nc * NV);
    if (off != raw.size()) { std::printf("%s: unexpected size\n", argv[1]); return 2; }
    MeshIn in{dim, NV, nv, nc, nc_owned, nf, (const double*)coords.data(), (const int32_t*)cells.data(), (const uint32_t*)ctags.data(),
              (const int32_t*)fcells.data(), (const int8_t*)flocal.data(), (const uint32_t*)ftags.data(), nmt, (const uint32_t*)mtags.data()};

    FacetTables T;
    const char* why = facet_tables(in, T);
    EXPECT(why == nullptr, why ? why : "");
    if (why) return 1;
    int64_t n_mem = 0;
    for (int64_t f = 0; f < nf; ++f)
        for (int i = 0; i < nmt; ++i) n_mem += in.facet_cells[2 * f + 1] >= 0 && in.facet_tags[f] == in.membrane_tags[i];
    EXPECT((int64_t)T.mf.size() == 6 * n_mem && n_mem > 0, "one membrane record per interior facet with a membrane tag");
    for (int64_t k = 0; k < nc; ++k)
        for (int a = 0; a < NV; ++a) {
            const int64_t nb = T.nbr[k * NV + a];
            const uint8_t b = T.fb[k * NV + a];
            EXPECT(((T.fflag[k] >> (8 * a)) & 255u) == b, "packed flag bytes");
            if (nb < 0) { EXPECT(((b >> 2) & 3u) == FK_EXTERIOR, "no neighbour = exterior"); continue; }
            EXPECT(nb < nc && T.nbr[nb * NV + (b & 3)] == k && T.cfacet[nb * NV + (b & 3)] == T.cfacet[k * NV + a], "neighbour tables are mutual");
            EXPECT(((T.fb[nb * NV + (b & 3)] ^ b) >> 4 & 1u) == 1u, "exactly one plus side");
        }

    std::vector<double> hcell;
    std::vector<float> ivol;
    cell_metrics(in, hcell, ivol);
    for (int64_t k = 0; k < nc; ++k) EXPECT(hcell[k] > 0.0 && ivol[k] > 0.0f && std::isfinite(ivol[k]), "cell diameter and volume");

    if (dim == 3) {
        HaloLists H;
        halo_block_lists(nc_owned, T, H);
        const int64_t nblk = (nc_owned + KNP_HALO_BLK - 1) / KNP_HALO_BLK;
        EXPECT(H.stride > 0 && H.stride % 8 == 0 && H.long0 == nblk && (int64_t)H.src.size() == nblk * H.stride, "halo list layout");
        for (int64_t k = 0; k < nc_owned; ++k)
            for (int a = 0; a < 4; ++a) {
                const uint32_t kind = (T.fb[k * 4 + a] >> 2) & 3u;
                if ((kind != FK_SIPG && kind != FK_MEMBRANE) || T.nbr[k * 4 + a] < 0) continue;
                const int loc = H.loc[k * 4 + a];
                const int64_t b = k / KNP_HALO_BLK;
                const int64_t cell = loc < KNP_HALO_BLK ? b * KNP_HALO_BLK + loc : H.src[b * H.stride + (loc - KNP_HALO_BLK)] / 4;
                EXPECT(loc < KNP_HALO_BLK + H.stride && cell == T.nbr[k * 4 + a], "halo entry names the neighbour");
            }
    }

    // the mesh's own coefficients, then 17 and 257 distinct tuples over the same cells (the two caps of knp_set_params: KNP_MAX_MAT
    // materials for the device tables, 256 for the block-Jacobi table keys)
    std::vector<double> D((const double*)Draw.data(), (const double*)Draw.data() + (size_t)ni * nc);
    std::vector<uint16_t> id;
    std::vector<double> tuples;
    const int nm = scan_materials(nc, ni, D.data(), 256, id, tuples);
    EXPECT(nm >= 1 && nm <= KNP_MAX_MAT, "the dumped mesh has a few materials");
    check_scan("mesh coefficients", nc, ni, D, 256, nm);
    for (int distinct : {17, 256, 257}) {
        if (nc < distinct) { std::printf("FAIL mesh too small for %d tuples\n", distinct); ++failures; continue; }
        std::vector<double> Dn((size_t)ni * nc);
        for (int64_t k = 0; k < nc; ++k)
            for (int i = 0; i < ni; ++i) Dn[(size_t)i * nc + k] = 1.0 + i + (i == ni - 1 ? (double)((k * 7) % distinct) : 0.0);
        check_scan("many tuples, cap 256", nc, ni, Dn, 256, distinct <= 256 ? distinct : -1);
        check_scan("many tuples, cap KNP_MAX_MAT", nc, ni, Dn, KNP_MAX_MAT, -1);
    }

    // a facet entry out of range is reported, not followed
    {
        std::vector<char> bad = fcells;
        ((int32_t*)bad.data())[0] = (int32_t)nc;
        MeshIn in2 = in;
        in2.facet_cells = (const int32_t*)bad.data();
        FacetTables T2;
        const char* w = facet_tables(in2, T2);
        EXPECT(w && std::string(w) == "facet table entry out of range", "bad facet entry");
        std::vector<char> badc = cells;
        ((int32_t*)badc.data())[nc * NV - 1] = (int32_t)nv;
        in2 = in;
        in2.cells = (const int32_t*)badc.data();
        w = facet_tables(in2, T2);
        EXPECT(w && std::string(w) == "cell vertex index out of range", "bad cell vertex");
    }
    if (failures) return 1;
    std::printf("context tables ok: %lld cells, %lld membrane facets, %d materials\n", (long long)nc, (long long)n_mem, nm);
    return 0;
}
