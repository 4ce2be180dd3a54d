// CPU check of the apply plan (knp-emi-dg_amd/csrc/apply_plan.hpp): the head family of every configuration the GPU tests assert a
// variant code for, and the head / tail segments of a cell range.  Build: g++ -std=c++17 -I knp-emi-dg_amd/csrc tools/apply_plan_check.cpp
// (tests/test_host.py::test_apply_plan_selects_the_asserted_kernel_families runs it).  Exit status 0 = every row holds.
#include "apply_plan.hpp"
#include <cstdio>

static int failures = 0;

static void expect_head(const char* name, const ApplyInputs& in, int emi, int knp) {
    const int got[2] = {plan_apply(in, 0).head, plan_apply(in, 1).head};
    const int want[2] = {emi, knp};
    for (int which = 0; which < 2; ++which)
        if (want[which] >= 0 && got[which] != want[which]) {
            std::printf("FAIL %s: %s head %d, expected %d\n", name, which ? "KNP" : "EMI", got[which], want[which]);
            ++failures;
        }
}

static void expect_segments(const char* name, const ApplyPlan& p, int64_t begin, int64_t end, int n, ApplySegment s0 = {}, ApplySegment s1 = {}) {
    ApplySegment seg[2] = {};
    const ApplySegment want[2] = {s0, s1};
    bool ok = apply_segments(p, begin, end, seg) == n;
    for (int i = 0; ok && i < n; ++i) ok = seg[i].family == want[i].family && seg[i].begin == want[i].begin && seg[i].end == want[i].end;
    if (!ok) {
        std::printf("FAIL segments: %s\n", name);
        ++failures;
    }
}

int main() {
    // What the owners answer on a structured 3D P1 mesh with classes, material table and two species.  The launchers ask them in the
    // plan's order and stop at the first yes; a table row sets every answer the owner WOULD give (the operator-specific ones in
    // ring[] / halo), so one row serves both operators.
    struct Row {
        const char* name;
        ApplyInputs in;
        bool ring[2];          // ring_usable(c, 0 / 1)
        int emi, knp;          // expected codes, -1 = not asserted
    };
    ApplyInputs s;             // the structured mesh
    s.degree = 1; s.dim = 3; s.cls = true; s.ncls = 12; s.ncls_max = 32; s.n_sys = 2; s.hb_long0 = 61;
    s.halo = true; s.halo_mat = true;
    auto with = [](ApplyInputs in, auto&& change) { change(in); return in; };
    const Row rows[] = {
        {"defaults", s, {true, true}, 3, 7},
        {"KNP_APPLY_RING=0", s, {false, false}, 1, 6},
        {"KNP_APPLY_MAT=0", with(s, [](ApplyInputs& i) { i.halo_mat = false; }), {true, false}, -1, 2},
        {"KNP_APPLY_HALO=0", with(s, [](ApplyInputs& i) { i.halo = false; }), {true, false}, 3, 1},
        {"KNP_EMI_RING=0", s, {false, true}, 1, -1},
        {"cell-wise D", with(s, [](ApplyInputs& i) { i.halo_mat = false; }), {true, false}, -1, 2},
        {"three solved species", with(s, [](ApplyInputs& i) { i.n_sys = 3; i.halo = false; }), {true, false}, -1, 1},
        {"four solved species", with(s, [](ApplyInputs& i) { i.n_sys = 4; i.halo = false; }), {true, false}, -1, 0},
        {"33 classes, KNP_APPLY_HALO=0", with(s, [](ApplyInputs& i) { i.ncls = 33; i.halo = false; }), {false, false}, 0, 0},
    };
    for (const Row& r : rows)
        for (int which = 0; which < 2; ++which) {
            ApplyInputs in = r.in;
            in.ring = r.ring[which];
            if (which == 0) in.halo = in.halo_mat = false;            // knp_halo_usable is asked for KNP only
            expect_head(r.name, in, which == 0 ? r.emi : -1, which == 1 ? r.knp : -1);
        }

    ApplyInputs o;             // other meshes and degrees
    o.degree = 1; o.dim = 2; o.n_sys = 2; o.ncls_max = 32;
    expect_head("2D", o, 0, 0);
    o.dim = 3;
    expect_head("3D without classes, KNP_APPLY_RING_U=0", o, 0, 0);
    o.ring_u_cells = 15104;
    expect_head("3D without classes, unstructured ring", o, 10, 10);
    ApplyInputs p2 = s;
    p2.degree = 2;
    expect_head("degree 2", p2, 8, 8);
    p2.p2_assembled = true;
    expect_head("degree 2, assembled", p2, 9, 9);

    // segments: head limit L = 2 blocks
    const int64_t L = 2 * APPLY_PLAN_BLK, n = 1000;
    ApplyInputs g = s;
    g.ring = true; g.hb_long0 = 2;
    const ApplyPlan ring = plan_apply(g, 1);
    expect_segments("[0, n) with L < n: head and tail", ring, 0, n, 2, {AF_RING_KNP, 0, L}, {AF_CLS, L, n});
    expect_segments("L >= n: head only", ring, 0, L, 1, {AF_RING_KNP, 0, L});
    expect_segments("L > n: head only", ring, 100, 300, 1, {AF_RING_KNP, 100, 300});
    expect_segments("range starting at L: tail only", ring, L, n, 1, {AF_CLS, L, n});
    expect_segments("range starting behind L: tail only", ring, L + 7, n, 1, {AF_CLS, L + 7, n});
    expect_segments("empty range", ring, 300, 300, 0);
    expect_segments("reversed range", ring, 300, 200, 0);
    g.hb_long0 = 0;
    const ApplyPlan ring0 = plan_apply(g, 0);
    if (ring0.head != AF_RING_EMI) {
        std::printf("FAIL hb_long0 == 0: the head still names the ring family, got %d\n", (int)ring0.head);
        ++failures;
    }
    expect_segments("hb_long0 == 0: tail only", ring0, 0, n, 1, {AF_CLS, 0, n});
    const ApplyPlan unstructured = plan_apply(o, 0);
    expect_segments("unstructured ring: head and coordinate tail", unstructured, 0, 15552, 2, {AF_RING_U, 0, 15104}, {AF_COORD, 15104, 15552});
    const ApplyPlan flat = plan_apply(with(s, [](ApplyInputs& i) { i.halo = false; }), 1);
    expect_segments("no staged head: one launch", flat, 5, n, 1, {AF_CLS, 5, n});

    if (failures) return 1;
    std::printf("apply plan ok\n");
    return 0;
}
