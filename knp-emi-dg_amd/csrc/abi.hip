// C ABI of libknpemi_hip.so (see include/knpemi_hip.h for the contract and the reference
// interfaces each entry point replaces): the entry points that only pass on to a launcher, and the timing / bench helpers.
// The context's life and setters are in context.hip, the two solves and their state in solve.hip.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "krylov.hpp"

extern "C" {

int knp_update_kappa(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    return launch_kappa(c, f->f[KNP_F_C], f->f[KNP_F_C_ELIM], f->f[KNP_F_KAPPA]);
}

int knp_allreduce_sum(knp_ctx* c, double* values, int n) {
    if (!c || !values) return -1;
    return allreduce_sum_host(c, values, n);
}

static int chk_vec(knp_ctx* c, int fx, int fy, int64_t need) {
    if (chk_field(c, fx) || chk_field(c, fy)) return -1;
    if (fx == fy) { c->err = "apply: input and output fields must differ"; return -1; }
    if (c->fields.n[fx] < need || c->fields.n[fy] < need) { c->err = "apply: field too small for this operator"; return -1; }
    return 0;
}

int knp_emi_apply(knp_ctx* c, int fx, int fy) {
    if (!c) return -1;
    if (chk_vec(c, fx, fy, c->m.nc * c->nd)) return -1;
    Fields* f = &c->fields;
    return dist_apply(c, 0, f->f[fx], f->f[KNP_F_KAPPA], f->f[fy]);
}

int knp_knp_apply(knp_ctx* c, int fx, int fy) {
    if (!c) return -1;
    if (chk_vec(c, fx, fy, (int64_t)c->p.n_sys * c->m.nc * c->nd)) return -1;
    Fields* f = &c->fields;
    return dist_apply(c, 1, f->f[fx], f->f[KNP_F_DNPHI], f->f[fy]);
}

int knp_emi_rhs(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    return launch_emi_rhs(c, f->f[KNP_F_C], f->f[KNP_F_C_ELIM], f->f[KNP_F_PHI_M], f->f[KNP_F_I_CH], f->f[KNP_F_B_EMI]);
}

int knp_knp_rhs(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    return launch_knp_rhs(c, f->f[KNP_F_C], f->f[KNP_F_C_PREV], f->f[KNP_F_C_ELIM], f->f[KNP_F_PHI], f->f[KNP_F_PHI_M],
                          f->f[KNP_F_I_CH], f->f[KNP_F_B_KNP]);
}

int knp_step_updates(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    HIPCHK(c, hipMemcpyAsync(f->f[KNP_F_C_PREV], f->f[KNP_F_C], sizeof(double) * f->n[KNP_F_C], hipMemcpyDeviceToDevice, c->stream));
    return launch_step_updates(c, f->f[KNP_F_C], f->f[KNP_F_C_ELIM], f->f[KNP_F_PHI], f->f[KNP_F_PHI_M], f->f[KNP_F_E]);
}

// Picard level update (solver.py:882-910): C_ELIM and E from the current C; phi_M and C_PREV are left alone
int knp_picard_updates(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    return launch_step_updates(c, f->f[KNP_F_C], f->f[KNP_F_C_ELIM], nullptr, nullptr, f->f[KNP_F_E]);
}

int knp_max_abs_diff(knp_ctx* c, int fa, int fb, double* out) {
    if (chk_field(c, fa) || chk_field(c, fb) || !out) return -1;
    const int64_t ndof = c->m.nc * c->nd;
    if (c->fields.n[fa] != c->fields.n[fb] || c->fields.n[fa] % ndof) { c->err = "max_abs_diff: nodal fields of equal size expected"; return -1; }
    return max_abs_diff(c, c->fields.f[fa], c->fields.f[fb], (int)(c->fields.n[fa] / ndof), out);
}

int knp_nernst(knp_ctx* c) {
    if (!c) return -1;
    Fields* f = &c->fields;
    return launch_nernst_only(c, f->f[KNP_F_C], f->f[KNP_F_C_ELIM], f->f[KNP_F_E]);
}

int knp_facet_trace(knp_ctx* c, int field, int species, int side, int slot) {
    if (chk_field(c, field)) return -1;
    if (side != 0 && side != 1) { c->err = "side must be 0 (plus) or 1 (minus)"; return -1; }
    if (slot < 0 || slot >= KNP_FACET_TMP_SLOTS) { c->err = "facet_trace: scratch slot out of range"; return -1; }
    const int64_t ndof = c->m.nc * c->nd;
    if (species < 0 || (int64_t)(species + 1) * ndof > c->fields.n[field]) { c->err = "facet_trace: species out of range"; return -1; }
    return launch_facet_trace(c, c->fields.f[field] + (int64_t)species * ndof, side, c->fields.f[KNP_F_FACET_TMP] + (int64_t)slot * c->m.nf);
}

int knp_sync(knp_ctx* c) {
    if (!c) return -1;
    return sync_check_ode(c);
}

long long knp_host_round_trips(knp_ctx* c) { return c ? c->host_round_trips : -1; }

int knp_timer_begin(knp_ctx* c) {
    if (!c) return -1;
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    return 0;
}

int knp_timer_end(knp_ctx* c, float* ms) {
    if (!c || !ms) return -1;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, host_event_sync(c, c->ev1));
    HIPCHK(c, hipEventElapsedTime(ms, c->ev0, c->ev1));
    return 0;
}

int knp_bench_apply(knp_ctx* c, int which, int reps, float* avg_ms) {
    if (!c || !avg_ms || reps < 1) return -1;
    Fields* f = &c->fields;
    int rc = 0;
    // three input / output pairs in rotation (X -> Y, r -> z, p -> w: 3 x the vectors of one apply), so that back-to-back
    // launches cannot be served from the 256 MiB Infinity Cache once the working set of ONE apply approaches it
    const int64_t n = (which == 0 ? 1 : c->p.n_sys) * c->m.nc * c->nd;
    double* in[3] = {f->f[KNP_F_X], f->r, f->p};
    double* out[3] = {f->f[KNP_F_Y], f->z, f->w};
    for (int k = 1; k < 3; ++k) HIPCHK(c, hipMemcpyAsync(in[k], in[0], sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    const double* coef = which == 0 ? f->f[KNP_F_KAPPA] : f->f[KNP_F_DNPHI];
    const bool was_timing = c->time_applies;
    c->time_applies = false;
    auto one = [&](int k) { return which == 0 ? launch_emi_apply(c, in[k % 3], coef, out[k % 3]) : launch_knp_apply(c, in[k % 3], coef, out[k % 3]); };
    // untimed launches first: code object load, LDS grant, and the clock ramp of a chip that idled during the host-side preparation
    // (as many as are timed: with one or twenty of them the first of two measured kernels read 5-20 % slow, 36 us against 30 us for
    // the EMI apply at r=2)
    for (int i = 0; i < reps && !rc; ++i) rc = one(i);
    if (!rc) {
        HIPCHK(c, hipEventRecord(c->ev0, c->stream));
        for (int i = 0; i < reps && !rc; ++i) rc = one(i + 1);
    }
    c->time_applies = was_timing;
    if (rc) return rc;
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    HIPCHK(c, host_event_sync(c, c->ev1));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    *avg_ms = ms / (float)reps;
    return 0;
}

int knp_apply_timing(knp_ctx* c, int enable) {
    if (!c) return -1;
    c->time_applies = enable != 0;
    return 0;
}

int knp_apply_variant(knp_ctx* c, int which) {
    if (!c || (which != 0 && which != 1)) return -1;
    return apply_variant(c, which);
}

int knp_apply_timing_read(knp_ctx* c, int which, float* avg_ms, int* count) {
    if (!c || (which != 0 && which != 1) || !avg_ms || !count) return -1;
    HIPCHK(c, host_stream_sync(c, c->stream));
    double sum = 0.0;
    for (size_t i = 0; i < c->tev_used[which]; ++i) {
        float ms = 0.f;
        HIPCHK(c, hipEventElapsedTime(&ms, c->tev[which][i].first, c->tev[which][i].second));
        sum += ms;
    }
    *count = (int)c->tev_used[which];
    *avg_ms = *count ? (float)(sum / *count) : 0.f;
    c->tev_used[which] = 0;
    return 0;
}

int knp_halo_exchange(knp_ctx* c, int field) {
    if (chk_field(c, field)) return -1;
    const int64_t ndof = c->m.nc * c->nd;
    if (c->fields.n[field] % ndof) { c->err = "halo_exchange: not a nodal field"; return -1; }
    if (!c->dist) return 0;
    return halo_exchange(c, c->fields.f[field], (int)(c->fields.n[field] / ndof));
}

}  // extern "C"
