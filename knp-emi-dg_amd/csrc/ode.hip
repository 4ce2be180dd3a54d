// Batched membrane ODE integrator: one thread per membrane facet, per-thread adaptive Dormand-Prince 5(4)
// (same pair, step controller and tolerances as knpemidg/membrane.py:integrate_batch, which it replaces on
// the device).  Every row carries its own time and step, so a facet's result does not depend on which other
// facets share the launch (ranks that both hold a cut facet compute bitwise identical outputs).
// Stands in for the per-facet numbalsoda.lsoda loop (reference: src/knpemidg/membrane.py:84-119) for the
// membrane models of the idealized examples (reference: examples/idealized-geometries/mm_hh.py:118-161).
// A set may be switched to a second integrator for stiff models (knp_ode_set_method: ode_stiff.hpp, extrapolated linearly implicit
// Euler); it shares the tables, the stimulus, the step-size carry-over and the failure flag, and adds four step / call counters.
// The sets and the runtime-compiled models of a context are its OdeState (knp_ctx::ode): nothing here is shared between contexts.
#include "../../include/knpemi_hip.h"
#include "knpemi_internal.hpp"
#include "ode_dp5.hpp"
#include "ode_stiff.hpp"
#include <hip/hiprtc.h>
#include <cstdlib>
#include <cstring>

#define ODE_MAX_STATES 11
#define ODE_MAX_PARAMS 20
#define ODE_MAX_OPS 12
#define ODE_RTC_ID0 1000        // model ids of runtime-compiled right-hand sides (knp_ode_register): 1000, 1001, ... per context

struct OdeSet {
    int model = 0;              // 1 = HH with synaptic stimulus, 2 = HH without, 3 = EMIx HH (cm/ms/mV), 4 = glial, 5 = passive leak, 6 = EMIx calibration system, >= 1000 = a registered HIP_RHS kernel
    int ns = 0, np = 0;
    int64_t n = 0;
    int32_t* facet = nullptr;   // [n] facet id of every node
    double* states = nullptr;   // [n][ns]
    double* params = nullptr;   // [n][np]
    double* h = nullptr;        // [n] last accepted step size
    int* fail = nullptr;        // device flag: the context's status word KNP_ODE_FAIL_SLOT (read back with the next status poll)
    uint8_t* stim_mask = nullptr;   // [n] rows on which the stimulus parameters are re-imposed every step (membrane.py:98-104)
    int method = 0;             // integrator of knp_ode_step: 0 = Dormand-Prince 5(4) (ode_dp5.hpp), 1 = stiff (ode_stiff.hpp)
    unsigned long long* stats = nullptr;   // [4] accepted, rejected, right-hand-side calls, Jacobians: added up by the stiff kernel
    int n_stim = 0;
    int stim_col[ODE_MAX_STIM] = {0};
    double stim_val[ODE_MAX_STIM] = {0};
};

// a model module's HIP_RHS compiled by hipRTC (knpemidg/ode_rtc.py) and loaded on one context's device
#define ODE_N_METHODS 2
struct RtcModel {
    hipModule_t mod[ODE_N_METHODS] = {nullptr, nullptr};     // one code object and kernel per method; either may be absent
    hipFunction_t fn[ODE_N_METHODS] = {nullptr, nullptr};
    int ns = 0, np = 0;
};

// knp_ctx::ode: created by the first knp_ode_create / knp_ode_register, freed by ode_destroy_all.  A handle is an index into `sets`, a
// registered model id is ODE_RTC_ID0 + an index into `rtc`; neither vector ever shrinks while the context lives.
struct OdeState {
    std::vector<OdeSet> sets;
    std::vector<RtcModel> rtc;
};

static OdeState& ode_make(knp_ctx* c) {
    if (!c->ode) c->ode = new OdeState();
    return *c->ode;
}

static const RtcModel* rtc_model(knp_ctx* c, int model) {
    if (!c->ode || model < ODE_RTC_ID0 || model - ODE_RTC_ID0 >= (int)c->ode->rtc.size()) return nullptr;
    return &c->ode->rtc[model - ODE_RTC_ID0];
}

// Hodgkin-Huxley squid axon + leak + Na/K pump (+ decaying synaptic conductance), SI units.
// parameter layout (mm_hh.py:56-64): 0 g_Na_bar 1 g_K_bar 2 g_leak_Na 3 g_leak_K 4 E_Na 5 E_K 6 Cm 7 stim_amplitude
//  8 I_ch_Na 9 I_ch_K 10 I_ch_Cl 11 K_e 12 Na_i 13 m_K 14 m_Na 15 I_max 16 E_Cl ; states: m h n V
template <bool STIM> __device__ __forceinline__ void hh_rhs(double t, const double* y, double* p, double* dy) {
    const double m = y[0], h = y[1], n = y[2], V = y[3];
    const double u = 1.0e3 * (V + 65.0e-3);
    const double alpha_m = 0.1e3 * (25.0 - u) / (exp((25.0 - u) / 10.0) - 1.0);
    const double beta_m = 4.0e3 * exp(-u / 18.0);
    dy[0] = (1 - m) * alpha_m - m * beta_m;
    const double alpha_h = 0.07e3 * exp(-u / 20.0);
    const double beta_h = 1.0e3 / (exp((30.0 - u) / 10.0) + 1.0);
    dy[1] = (1 - h) * alpha_h - h * beta_h;
    const double alpha_n = 0.01e3 * (10.0 - u) / (exp((10.0 - u) / 10.0) - 1.0);
    const double beta_n = 0.125e3 * exp(-u / 80.0);
    dy[2] = (1 - n) * alpha_n - n * beta_n;
    const double a = 1 + p[13] / p[11], b = 1 + p[14] / p[12];
    const double i_pump = p[15] / (a * a * b * b * b);
    double g_stim = 0.0;
    if (STIM) g_stim = (t < 125e-3) ? p[7] * exp(-fmod(t, 0.03) / 0.002) : 0.0;
    const double i_Na = (p[2] + p[0] * h * m * m * m + g_stim) * (V - p[4]) + 3 * i_pump;
    const double n2 = n * n;
    const double i_K = (p[3] + p[1] * n2 * n2) * (V - p[5]) - 2 * i_pump;
    p[8] = i_Na;
    p[9] = i_K;
    p[10] = 0.0;
    dy[3] = (-i_K - i_Na) / p[6];
}

// EMIx neuron membrane: the same HH kinetics in cm / ms / mV units with a periodically re-triggered synaptic
// conductance (reference: examples/emix-simulations/mm_hh.py:118-161); same parameter layout as above.
__device__ __forceinline__ void hh_emix_rhs(double t, const double* y, double* p, double* dy) {
    const double m = y[0], h = y[1], n = y[2], V = y[3];
    const double alpha_m = 0.1 * (V + 40.0) / (1.0 - exp(-(V + 40.0) / 10.0));
    const double beta_m = 4.0 * exp(-(V + 65.0) / 18.0);
    const double alpha_h = 0.07 * exp(-(V + 65.0) / 20.0);
    const double beta_h = 1.0 / (1.0 + exp(-(V + 35.0) / 10.0));
    const double alpha_n = 0.01 * (V + 55.0) / (1.0 - exp(-(V + 55.0) / 10.0));
    const double beta_n = 0.125 * exp(-(V + 65.0) / 80.0);
    dy[0] = (1 - m) * alpha_m - m * beta_m;
    dy[1] = (1 - h) * alpha_h - h * beta_h;
    dy[2] = (1 - n) * alpha_n - n * beta_n;
    const double g_stim = p[7] * exp(-fmod(t, 20.0) / 2.0);
    const double a = 1 + p[13] / p[11], b = 1 + p[14] / p[12];
    const double i_pump = p[15] / (a * a * b * b * b);
    const double i_Na = (p[2] + p[0] * h * m * m * m + g_stim) * (V - p[4]) + 3 * i_pump;
    const double n2 = n * n;
    const double i_K = (p[3] + p[1] * n2 * n2) * (V - p[5]) - 2 * i_pump;
    p[8] = i_Na;
    p[9] = i_K;
    p[10] = 0.0;
    dy[3] = (-i_K - i_Na) / p[6];
}

// Glial membrane: Kir 4.1 + Na leak + Na/K pump, one state (reference: examples/emix-simulations/mm_glial.py:117-170).
// parameters 0..15 as above, 16 K_e_init, 17 K_i_init, 18 E_Cl
__device__ __forceinline__ void glial_rhs(double t, const double* y, double* p, double* dy) {
    const double V = y[0];
    const double a = 1 + p[13] / p[11], b = 1 + p[14] / p[12];
    const double i_pump = p[15] / (a * a * b * b * b);
    const double E_K_init = 8.314e3 * 300e3 / 96485e3 * log(p[16] / p[17]);
    const double dphi = V - p[5];
    const double A = 1 + exp(18.4 / 42.4);
    const double B = 1 + exp(-(0.1186e3 + E_K_init) / 0.0441e3);
    const double C = 1 + exp((dphi + 0.0185e3) / 0.0425e3);
    const double D = 1 + exp(-(0.1186e3 + V) / 0.0441e3);
    const double g_Kir = sqrt(p[11] / p[16]) * (A * B) / (C * D);
    const double i_Kir = p[3] * g_Kir * (V - p[5]);
    const double i_Na = p[2] * (V - p[4]) + 3 * i_pump;
    const double i_K = i_Kir - 2 * i_pump;
    p[8] = i_Na;
    p[9] = i_K;
    p[10] = 0.0;
    dy[0] = (-i_K - i_Na) / p[6];
}

// Passive membrane: Na / K leak + Na/K pump + decaying synaptic conductance on the Na leak, one state, SI units
// (reference: examples/rat-neuron/mm_leak.py:107-133).  parameters (mm_leak.py:44-50): 0 g_leak_Na 1 g_leak_K 2 E_Na 3 E_K 4 Cm
//  5 stim_amplitude 6 I_ch_Na 7 I_ch_K 8 I_ch_Cl 9 K_e 10 Na_i 11 m_K 12 m_Na 13 I_max 14 E_Cl
__device__ __forceinline__ void leak_rhs(double t, const double* y, double* p, double* dy) {
    const double V = y[0];
    const double g_stim = p[5] * exp(-fmod(t, 0.03) / 0.002);
    const double a = 1 + p[11] / p[9], b = 1 + p[12] / p[10];
    const double i_pump = p[13] / (a * a * b * b * b);
    const double i_Na = (p[0] + g_stim) * (V - p[2]) + 3 * i_pump;
    const double i_K = p[1] * (V - p[3]) - 2 * i_pump;
    p[6] = i_Na;
    p[7] = i_K;
    p[8] = 0.0;
    dy[0] = (-i_K - i_Na) / p[4];
}

// EMIx calibration system: the neuronal HH membrane and the glial membrane above coupled through the ECS / neuron / glia compartment
// concentrations their currents change; integrated alone until stationary it yields the initial state of the full run
// (reference: examples/emix-simulations/mm_calibration.py:143-255, run_calibration.py:13-90).
// states: m h n V_n V_g K_e K_n K_g Na_e Na_n Na_g ; parameters: 0 g_Na_bar 1 g_K_bar 2 g_leak_Na_n 3 g_leak_K_n 4 g_leak_Na_g
//  5 g_leak_K_g 6 Cm 7 stim_amplitude 8 m_K 9 m_Na 10 I_max_n 11 I_max_g
__device__ __forceinline__ void calibration_rhs(double t, const double* y, double* p, double* dy) {
    const double m = y[0], h = y[1], n = y[2], Vn = y[3], Vg = y[4];
    const double K_e = y[5], K_n = y[6], K_g = y[7], Na_e = y[8], Na_n = y[9], Na_g = y[10];
    const double c = 8.314e3 * 300e3 / 96485e3;
    const double ICS_vol = 3.42e-11 / 2.0, ECS_vol = 7.08e-11, surface = 2.29e-6, F = 96485e3;
    const double K_g_init = 102.74050220804774, K_e_init = 3.32597273958481;
    const double E_Na_n = c * log(Na_e / Na_n), E_K_n = c * log(K_e / K_n);
    const double E_Na_g = c * log(Na_e / Na_g), E_K_g = c * log(K_e / K_g);
    const double E_K_init = c * log(K_e_init / K_g_init);
    const double alpha_m = 0.1 * (Vn + 40.0) / (1.0 - exp(-(Vn + 40.0) / 10.0));
    const double beta_m = 4.0 * exp(-(Vn + 65.0) / 18.0);
    const double alpha_h = 0.07 * exp(-(Vn + 65.0) / 20.0);
    const double beta_h = 1.0 / (1.0 + exp(-(Vn + 35.0) / 10.0));
    const double alpha_n = 0.01 * (Vn + 55.0) / (1.0 - exp(-(Vn + 55.0) / 10.0));
    const double beta_n = 0.125 * exp(-(Vn + 65.0) / 80.0);
    dy[0] = (1 - m) * alpha_m - m * beta_m;
    dy[1] = (1 - h) * alpha_h - h * beta_h;
    dy[2] = (1 - n) * alpha_n - n * beta_n;
    const double g_stim = p[7] * exp(-fmod(t, 20.0) / 2.0);
    const double a = 1 + p[8] / K_e, bn = 1 + p[9] / Na_n, bg = 1 + p[9] / Na_g;
    const double i_pump_n = p[10] / (a * a * bn * bn * bn);
    const double i_pump_g = p[11] / (a * a * bg * bg * bg);
    const double A = 1 + exp(18.4 / 42.4);
    const double B = 1 + exp(-(0.1186e3 + E_K_init) / 0.0441e3);
    const double C = 1 + exp((Vg - E_K_g + 0.0185e3) / 0.0425e3);
    const double D = 1 + exp(-(0.1186e3 + Vg) / 0.0441e3);
    const double i_Kir = p[5] * sqrt(K_e / K_e_init) * (A * B) / (C * D) * (Vg - E_K_g);
    const double i_Na_n = (p[2] + p[0] * h * m * m * m + g_stim) * (Vn - E_Na_n) + 3 * i_pump_n;
    const double n2 = n * n;
    const double i_K_n = (p[3] + p[1] * n2 * n2) * (Vn - E_K_n) - 2 * i_pump_n;
    const double i_Na_g = p[4] * (Vg - E_Na_g) + 3 * i_pump_g;
    const double i_K_g = i_Kir - 2 * i_pump_g;
    dy[3] = (-i_K_n - i_Na_n) / p[6];
    dy[4] = (-i_K_g - i_Na_g) / p[6];
    const double ke = surface / (F * ECS_vol), ki = surface / (F * ICS_vol);
    dy[5] = (i_K_n + i_K_g) * ke;
    dy[6] = -i_K_n * ki;
    dy[7] = -i_K_g * ki;
    dy[8] = (i_Na_n + i_Na_g) * ke;
    dy[9] = -i_Na_n * ki;
    dy[10] = -i_Na_g * ki;
}

template <int MODEL> __device__ __forceinline__ void model_rhs(double t, const double* y, double* p, double* dy) {
    if (MODEL == 1) hh_rhs<true>(t, y, p, dy);
    else if (MODEL == 2) hh_rhs<false>(t, y, p, dy);
    else if (MODEL == 3) hh_emix_rhs(t, y, p, dy);
    else if (MODEL == 4) glial_rhs(t, y, p, dy);
    else if (MODEL == 5) leak_rhs(t, y, p, dy);
    else calibration_rhs(t, y, p, dy);
}

template <int MODEL> struct BuiltinRhs {
    __device__ __forceinline__ void operator()(double t, const double* y, double* p, double* dy) const { model_rhs<MODEL>(t, y, p, dy); }
};

template <int MODEL, int NS, int NP>
__global__ __launch_bounds__(64) void k_ode_step(int64_t n, double t0, double t1, double rtol, double atol, int max_steps,
                                                 double* __restrict__ states, double* __restrict__ params,
                                                 double* __restrict__ hstore, int* __restrict__ fail,
                                                 const uint8_t* __restrict__ stim_mask, StimArgs stim) {
    ode_dp5_step<NS, NP>(BuiltinRhs<MODEL>(), n, t0, t1, rtol, atol, max_steps, states, params, hstore, fail, stim_mask, stim);
}

template <int MODEL, int NS, int NP>
__global__ __launch_bounds__(64) void k_ode_step_stiff(int64_t n, double t0, double t1, double rtol, double atol, int max_steps,
                                                       double* __restrict__ states, double* __restrict__ params,
                                                       double* __restrict__ hstore, int* __restrict__ fail,
                                                       const uint8_t* __restrict__ stim_mask, StimArgs stim,
                                                       unsigned long long* __restrict__ stats) {
    ode_stiff_step<NS, NP>(BuiltinRhs<MODEL>(), n, t0, t1, rtol, atol, max_steps, states, params, hstore, fail, stim_mask, stim, stats);
}

// table[node][col] <- facet_field[facet[node]]   (PDE -> ODE, membrane.py:122-139)
__global__ void k_ode_from_facet(int64_t n, const int32_t* __restrict__ facet, const double* __restrict__ field, int stride,
                                 int col, double* __restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) table[i * stride + col] = field[facet[i]];
}
// facet_field[facet[node]] <- table[node][col]   (ODE -> PDE, membrane.py:141-162)
__global__ void k_ode_to_facet(int64_t n, const int32_t* __restrict__ facet, const double* __restrict__ table, int stride,
                               int col, double* __restrict__ field) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) field[facet[i]] = table[i * stride + col];
}

// the same for a list of columns in ONE launch (a membrane step moves V, E_k, K_e, Na_i in and V, I_ch_k out)
struct OdeOps { int n; int stride[ODE_MAX_OPS]; int col[ODE_MAX_OPS]; double* table[ODE_MAX_OPS]; double* field[ODE_MAX_OPS]; };
__global__ void k_ode_exchange_multi(int64_t n, const int32_t* __restrict__ facet, OdeOps ops, int to_facet) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int f = facet[i];
    for (int k = 0; k < ops.n; ++k) {
        double* t = ops.table[k] + i * ops.stride[k] + ops.col[k];
        if (to_facet) ops.field[k][f] = *t;
        else *t = ops.field[k][f];
    }
}

// `assert success` of membrane.py:113, deferred: knp_ode_step does not synchronise; the flag travels with the next status poll of
// a solve (krylov.hip: poll_status), a table download or knp_sync.  Call with the stream idle.
int ode_check_failed(knp_ctx* c) {
    int fail = 0;
    if (host_memcpy(c, &fail, c->status + KNP_ODE_FAIL_SLOT, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (!fail) return 0;
    hipMemset(c->status + KNP_ODE_FAIL_SLOT, 0, sizeof(int));
    c->err = "ODE integrator did not reach the end time";
    return 1;
}

// Wait for the stream, then check the ODE failure flag (knp_sync, the table transfers, a state save).  The flag rides to the host
// in front of the wait (status_look): one round trip.  KNP_SYNC_ONE_TRIP=0 (read per call): the wait, then ode_check_failed's
// blocking read of the word -- two.
int sync_check_ode(knp_ctx* c) {
    if (!env_flag("KNP_SYNC_ONE_TRIP", true)) {
        HIPCHK(c, host_stream_sync(c, c->stream));
        return ode_check_failed(c) ? -4 : 0;
    }
    int rc = status_look(c);
    if (rc) return rc;
    if (!((const int*)c->pinned)[KNP_ODE_FAIL_SLOT]) return 0;
    hipMemset(c->status + KNP_ODE_FAIL_SLOT, 0, sizeof(int));
    c->err = "ODE integrator did not reach the end time";
    return -4;
}

static OdeSet* get_set(knp_ctx* c, int handle) {
    if (!c->ode || handle < 0 || handle >= (int)c->ode->sets.size()) return nullptr;
    return &c->ode->sets[handle];
}

// state table of a handle for the recorder's state channels (record.hip): device pointer [n][ns]; false = no such handle.  The
// pointer stays valid until the context is destroyed: a later knp_ode_create may move the OdeSet records, never the device tables
// they point to.
bool ode_state_table(knp_ctx* c, int handle, const double** states, int64_t* n, int* ns) {
    const OdeSet* S = get_set(c, handle);
    if (!S) return false;
    *states = S->states; *n = S->n; *ns = S->ns;
    return true;
}

static void set_free(OdeSet& S) {
    hipFree(S.facet); hipFree(S.states); hipFree(S.params); hipFree(S.h); hipFree(S.stim_mask); hipFree(S.stats);
}

// checkpoint (state.hip): per model the state and parameter tables and the last accepted step size of every node, in the node order
// the model was created with (the caller's).  Block ids 1000 + 8 handle + {0, 1, 2}; the widths carry the model layout, so a snapshot
// of other models does not load.  The stimulus mask and values are configuration: the host sends them again.
int ode_state_blocks(knp_ctx* c, std::vector<StateBlk>& out) {
    if (!c->ode) return 0;
    for (size_t h = 0; h < c->ode->sets.size(); ++h) {
        OdeSet& S = c->ode->sets[h];
        void* dev[3] = {S.states, S.params, S.h};
        const int width[3] = {S.ns, S.np, 1};
        for (int q = 0; q < 3; ++q) {
            StateBlk b;
            b.id = 1000 + 8 * (int)h + q; b.kind = KNP_SK_MEMBRANE_FACET; b.type = KNP_ST_F64; b.count = S.n; b.width = width[q]; b.dev = dev[q];
            out.push_back(b);
        }
    }
    return 0;
}

void ode_destroy_all(knp_ctx* c) {
    if (!c->ode) return;
    if (!c->ode->rtc.empty()) host_stream_sync(c, c->stream);   // no launch of a registered kernel may still be in flight
    for (auto& R : c->ode->rtc)
        for (int q = 0; q < ODE_N_METHODS; ++q)
            if (R.mod[q]) hipModuleUnload(R.mod[q]);
    for (auto& S : c->ode->sets) set_free(S);
    delete c->ode;
    c->ode = nullptr;
}

extern "C" {

int knp_ode_create(knp_ctx* c, int model, int64_t n, const int32_t* facets, int ns, int np, const double* states,
                   const double* params) {
    if (!c) return -1;
    if (model >= ODE_RTC_ID0) {
        const RtcModel* R = rtc_model(c, model);
        if (!R) { c->err = "ode: model id not registered on this context (knp_ode_register)"; return -1; }
        if (ns != R->ns || np != R->np) { c->err = "ode: state / parameter counts differ from the registered kernel's"; return -1; }
    } else if (model < 1 || model > 6) { c->err = "ode: unknown device model id"; return -1; }
    if (model <= 3 && (ns != 4 || np != 17)) { c->err = "ode: HH models have 4 states and 17 parameters"; return -1; }
    if (model == 4 && (ns != 1 || np != 19)) { c->err = "ode: the glial model has 1 state and 19 parameters"; return -1; }
    if (model == 5 && (ns != 1 || np != 15)) { c->err = "ode: the leak model has 1 state and 15 parameters"; return -1; }
    if (model == 6 && (ns != 11 || np != 12)) { c->err = "ode: the calibration system has 11 states and 12 parameters"; return -1; }
    for (int64_t i = 0; i < n; ++i)
        if (facets[i] < 0 || facets[i] >= c->m.nf) { c->err = "ode: facet id out of range"; return -1; }
    OdeSet S;
    S.model = model; S.ns = ns; S.np = np; S.n = n;
    const size_t m = (size_t)(n ? n : 1);
    S.fail = c->status + KNP_ODE_FAIL_SLOT;
    auto fill = [&]() -> int {
        HIPCHK(c, hipMalloc((void**)&S.facet, m * sizeof(int32_t)));
        HIPCHK(c, hipMalloc((void**)&S.states, m * ns * sizeof(double)));
        HIPCHK(c, hipMalloc((void**)&S.params, m * np * sizeof(double)));
        HIPCHK(c, hipMalloc((void**)&S.h, m * sizeof(double)));
        HIPCHK(c, hipMalloc((void**)&S.stim_mask, m));
        HIPCHK(c, hipMemset(S.stim_mask, 0, m));
        HIPCHK(c, hipMemset(S.h, 0, m * sizeof(double)));
        HIPCHK(c, hipMalloc((void**)&S.stats, 4 * sizeof(unsigned long long)));
        HIPCHK(c, hipMemset(S.stats, 0, 4 * sizeof(unsigned long long)));
        if (n) {
            HIPCHK(c, host_memcpy(c, S.facet, facets, n * sizeof(int32_t), hipMemcpyHostToDevice));
            HIPCHK(c, host_memcpy(c, S.states, states, n * ns * sizeof(double), hipMemcpyHostToDevice));
            HIPCHK(c, host_memcpy(c, S.params, params, n * np * sizeof(double), hipMemcpyHostToDevice));
        }
        return 0;
    };
    if (const int rc = fill()) {                   // a partial set is released again: the context keeps no trace of it
        set_free(S);
        return rc;
    }
    std::vector<OdeSet>& sets = ode_make(c).sets;
    sets.push_back(S);
    return (int)sets.size() - 1;
}

// what: 0 = states, 1 = parameters
int knp_ode_table(knp_ctx* c, int handle, int what, int upload, double* host) {
    OdeSet* S = get_set(c, handle);
    if (!S || !host) return -1;
    double* dev = what == 0 ? S->states : S->params;
    const size_t bytes = (size_t)S->n * (what == 0 ? S->ns : S->np) * sizeof(double);
    { const int rc_ = sync_check_ode(c); if (rc_) return rc_; }
    if (bytes) HIPCHK(c, host_memcpy(c, upload ? (void*)dev : (void*)host, upload ? (void*)host : (void*)dev, bytes,
                                   upload ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return 0;
}

// ODE table column <- device facet field (offset = row * nf for multi-row fields), or the reverse
int knp_ode_exchange(knp_ctx* c, int handle, int what, int col, int field, int64_t offset, int to_facet) {
    OdeSet* S = get_set(c, handle);
    if (!S) return -1;
    int64_t nfld = 0;
    double* f = knp_field_ptr(c, field, &nfld);
    const int stride = what == 0 ? S->ns : S->np;
    if (!f || col < 0 || col >= stride || offset < 0 || offset + c->m.nf > nfld) { c->err = "ode_exchange: bad field / column"; return -1; }
    if (!S->n) return 0;
    double* table = what == 0 ? S->states : S->params;
    const dim3 g((unsigned)((S->n + 255) / 256)), b(256);
    if (to_facet) hipLaunchKernelGGL(k_ode_to_facet, g, b, 0, c->stream, S->n, S->facet, table, stride, col, f + offset);
    else hipLaunchKernelGGL(k_ode_from_facet, g, b, 0, c->stream, S->n, S->facet, f + offset, stride, col, table);
    HIPCHK(c, hipGetLastError());
    return 0;
}

int knp_ode_set_stimulus(knp_ctx* c, int handle, int n_entries, const int32_t* cols, const double* values, const uint8_t* mask) {
    OdeSet* S = get_set(c, handle);
    if (!S) return -1;
    if (n_entries < 0 || n_entries > ODE_MAX_STIM) { c->err = "ode_set_stimulus: at most 4 stimulus parameters"; return -1; }
    for (int e = 0; e < n_entries; ++e)
        if (cols[e] < 0 || cols[e] >= S->np) { c->err = "ode_set_stimulus: parameter column out of range"; return -1; }
    S->n_stim = n_entries;
    for (int e = 0; e < n_entries; ++e) { S->stim_col[e] = cols[e]; S->stim_val[e] = values[e]; }
    if (n_entries && S->n) {
        if (!mask) { c->err = "ode_set_stimulus: mask missing"; return -1; }
        HIPCHK(c, hipMemcpyAsync(S->stim_mask, mask, (size_t)S->n, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, host_stream_sync(c, c->stream));
    }
    return 0;
}

int knp_ode_exchange_multi(knp_ctx* c, int handle, int n, const int32_t* what, const int32_t* col, const int32_t* field,
                           const int64_t* offset, int to_facet) {
    OdeSet* S = get_set(c, handle);
    if (!S || n < 0 || (n && (!what || !col || !field || !offset))) return -1;
    for (int k0 = 0; k0 < n; k0 += ODE_MAX_OPS) {
        OdeOps ops;
        ops.n = (n - k0 < ODE_MAX_OPS) ? n - k0 : ODE_MAX_OPS;
        for (int k = 0; k < ops.n; ++k) {
            int64_t nfld = 0;
            double* f = knp_field_ptr(c, field[k0 + k], &nfld);
            const int stride = what[k0 + k] == 0 ? S->ns : S->np;
            if (!f || col[k0 + k] < 0 || col[k0 + k] >= stride || offset[k0 + k] < 0 || offset[k0 + k] + c->m.nf > nfld) {
                c->err = "ode_exchange: bad field / column";
                return -1;
            }
            ops.stride[k] = stride; ops.col[k] = col[k0 + k];
            ops.table[k] = what[k0 + k] == 0 ? S->states : S->params;
            ops.field[k] = f + offset[k0 + k];
        }
        if (!S->n || !ops.n) continue;
        hipLaunchKernelGGL(k_ode_exchange_multi, dim3((unsigned)((S->n + 255) / 256)), dim3(256), 0, c->stream, S->n, S->facet, ops, to_facet);
        HIPCHK(c, hipGetLastError());
    }
    return 0;
}

// Asynchronous: a node that cannot reach t0 + dt raises the context's ODE failure flag, reported (-4) by the next solve's status
// poll, table download or knp_sync -- no host round trip per membrane model and step.
int knp_ode_step(knp_ctx* c, int handle, double t0, double dt, double rtol, double atol) {
    OdeSet* S = get_set(c, handle);
    if (!S) return -1;
    if (!S->n) return 0;
    const dim3 g((unsigned)((S->n + 63) / 64)), b(64);
    const int max_steps = 100000;
    StimArgs st;
    st.n = S->n_stim;
    for (int e = 0; e < ODE_MAX_STIM; ++e) { st.col[e] = S->stim_col[e]; st.val[e] = S->stim_val[e]; }
    if (S->model >= ODE_RTC_ID0) {
        // a registered HIP_RHS kernel: same integrator text, block size, arguments and failure flag as k_ode_step
        const RtcModel* R = rtc_model(c, S->model);
        if (!R) { c->err = "ode_step: registered model is gone"; return -1; }
        if (!R->fn[S->method]) { c->err = "ode_step: the registered model has no kernel for the set's method"; return -1; }
        int64_t n = S->n;
        double t1 = t0 + dt;
        int ms = max_steps;
        const uint8_t* mask = S->stim_mask;
        void* args[] = {&n, &t0, &t1, &rtol, &atol, &ms, &S->states, &S->params, &S->h, &S->fail, &mask, &st, &S->stats};   // the last one: stiff only
        HIPCHK(c, hipModuleLaunchKernel(R->fn[S->method], g.x, 1, 1, b.x, 1, 1, 0, c->stream, args, nullptr));
        return 0;
    }
    if (S->method == 1) {
#define ODE_LAUNCH_STIFF(MODEL, NS, NP)                                                                                          \
    hipLaunchKernelGGL((k_ode_step_stiff<MODEL, NS, NP>), g, b, 0, c->stream, S->n, t0, t0 + dt, rtol, atol, max_steps, S->states, \
                       S->params, S->h, S->fail, (const uint8_t*)S->stim_mask, st, S->stats)
        if (S->model == 1) ODE_LAUNCH_STIFF(1, 4, 17);
        else if (S->model == 2) ODE_LAUNCH_STIFF(2, 4, 17);
        else if (S->model == 3) ODE_LAUNCH_STIFF(3, 4, 17);
        else if (S->model == 4) ODE_LAUNCH_STIFF(4, 1, 19);
        else if (S->model == 5) ODE_LAUNCH_STIFF(5, 1, 15);
        else ODE_LAUNCH_STIFF(6, 11, 12);
#undef ODE_LAUNCH_STIFF
        HIPCHK(c, hipGetLastError());
        return 0;
    }
#define ODE_LAUNCH(MODEL, NS, NP)                                                                                          \
    hipLaunchKernelGGL((k_ode_step<MODEL, NS, NP>), g, b, 0, c->stream, S->n, t0, t0 + dt, rtol, atol, max_steps, S->states, \
                       S->params, S->h, S->fail, (const uint8_t*)S->stim_mask, st)
    if (S->model == 1) ODE_LAUNCH(1, 4, 17);
    else if (S->model == 2) ODE_LAUNCH(2, 4, 17);
    else if (S->model == 3) ODE_LAUNCH(3, 4, 17);
    else if (S->model == 4) ODE_LAUNCH(4, 1, 19);
    else if (S->model == 5) ODE_LAUNCH(5, 1, 15);
    else ODE_LAUNCH(6, 11, 12);
#undef ODE_LAUNCH
    HIPCHK(c, hipGetLastError());
    return 0;
}

// hipRTC: the translation unit of knpemidg/ode_rtc.py -> a gfx950 code object.  Host only (no context, no device), so it can run on a
// worker thread while the context is being created.  Same code generation settings as build.py's hipcc line (-O3, and the floating-
// point contraction clang applies to HIP by default, stated explicitly), so a HIP_RHS identical to a built-in model's right-hand
// side gives the same instructions.  The log carries the compiler's resource-usage remarks (VGPRs, scratch) and any diagnostics.
int knp_ode_rtc_compile(const char* src, const char* name, void** code, size_t* size, char* log, size_t logcap) {
    if (log && logcap) log[0] = 0;
    if (!src || !code || !size) return -1;
    *code = nullptr;
    *size = 0;
    hiprtcProgram prog = nullptr;
    if (hiprtcCreateProgram(&prog, src, name ? name : "knp_ode_rtc.cpp", 0, nullptr, nullptr) != HIPRTC_SUCCESS) {
        if (log && logcap) snprintf(log, logcap, "hiprtcCreateProgram failed");
        return -2;
    }
    const char* opts[] = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast-honor-pragmas",
                          "-Rpass-analysis=kernel-resource-usage"};
    const hiprtcResult rc = hiprtcCompileProgram(prog, (int)(sizeof(opts) / sizeof(opts[0])), opts);
    size_t nlog = 0;
    if (log && logcap && hiprtcGetProgramLogSize(prog, &nlog) == HIPRTC_SUCCESS && nlog > 0) {
        std::string text(nlog, '\0');
        if (hiprtcGetProgramLog(prog, &text[0]) == HIPRTC_SUCCESS) {
            const size_t m = strnlen(text.c_str(), nlog) < logcap - 1 ? strnlen(text.c_str(), nlog) : logcap - 1;
            memcpy(log, text.data(), m);
            log[m] = 0;
        }
    }
    if (rc != HIPRTC_SUCCESS) {
        hiprtcDestroyProgram(&prog);
        return -3;
    }
    size_t n = 0;
    if (hiprtcGetCodeSize(prog, &n) != HIPRTC_SUCCESS || n == 0 || !(*code = malloc(n)) || hiprtcGetCode(prog, (char*)*code) != HIPRTC_SUCCESS) {
        free(*code);
        *code = nullptr;
        hiprtcDestroyProgram(&prog);
        if (log && logcap) snprintf(log, logcap, "hiprtcGetCode failed");
        return -4;
    }
    *size = n;
    hiprtcDestroyProgram(&prog);
    return 0;
}

void knp_ode_rtc_free(void* code) { free(code); }

// load a code object of knp_ode_rtc_compile on the context's device as the kernel of `method`; model < 0: of a new model, whose id
// (>= 1000, a model id for knp_ode_create) is returned; else of the registered model `model`, which has none for that method yet
static int rtc_register(knp_ctx* c, int model, int method, const void* code, size_t size, const char* kernel_name, int ns, int np) {
    if (!c) return -1;
    if (!code || !size || !kernel_name) { c->err = "ode_register: no code object / kernel name"; return -1; }
    if (ns < 1 || ns > 32 || np < 1 || np > 64) { c->err = "ode_register: 1..32 states and 1..64 parameters"; return -1; }
    if (method == 1 && ns > ODE_STIFF_MAX_STATES) { c->err = "ode_register: the stiff integrator takes at most 11 states"; return -1; }
    if (model >= 0) {
        const RtcModel* R = rtc_model(c, model);
        if (!R) { c->err = "ode_register: model id not registered on this context"; return -1; }
        if (R->ns != ns || R->np != np) { c->err = "ode_register: state / parameter counts differ from the registered model's"; return -1; }
        if (R->fn[method]) { c->err = "ode_register: the model already has a kernel for this method"; return -1; }
    }
    (void)size;                                      // hipModuleLoadData reads the ELF's own size
    HIPCHK(c, hipSetDevice(c->device));
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    if (const int rc = rtc_load_kernel(c, "ode_register", code, kernel_name, &mod, &fn)) return rc;
    auto& v = ode_make(c).rtc;
    if (model < 0) {
        RtcModel R;
        R.ns = ns;
        R.np = np;
        v.push_back(R);
        model = ODE_RTC_ID0 + (int)v.size() - 1;
    }
    v[model - ODE_RTC_ID0].mod[method] = mod;
    v[model - ODE_RTC_ID0].fn[method] = fn;
    return model;
}

int knp_ode_register(knp_ctx* c, const void* code, size_t size, const char* kernel_name, int ns, int np) {
    return rtc_register(c, -1, 0, code, size, kernel_name, ns, np);
}

// the kernel of one method (ode_rtc.source(ode, method)) for a registered model, or (model < 0) for a new one that has this kernel only
int knp_ode_register_method(knp_ctx* c, int model, int method, const void* code, size_t size, const char* kernel_name, int ns, int np) {
    if (!c) return -1;
    if (method < 0 || method >= ODE_N_METHODS) { c->err = "ode_register_method: 0 = DP5, 1 = stiff"; return -1; }
    return rtc_register(c, model, method, code, size, kernel_name, ns, np);
}

// 0 = Dormand-Prince 5(4), the default; 1 = stiff.  -1 and the set unchanged for anything else, or (with the context's error text) for a
// registered model that has no kernel of that method
int knp_ode_set_method(knp_ctx* c, int handle, int method) {
    OdeSet* S = get_set(c, handle);
    if (!S) return -1;
    if (method < 0 || method >= ODE_N_METHODS) { c->err = "ode_set_method: 0 = DP5, 1 = stiff"; return -1; }
    if (method == 1 && S->ns > ODE_STIFF_MAX_STATES) { c->err = "ode_set_method: the stiff integrator takes at most 11 states"; return -1; }
    if (S->model >= ODE_RTC_ID0) {
        const RtcModel* R = rtc_model(c, S->model);
        if (!R || !R->fn[method]) { c->err = "ode_set_method: the registered model has no kernel for this method"; return -1; }
    }
    S->method = method;
    return 0;
}

// counters of the stiff kernel since the set was created: accepted steps, rejected steps, right-hand-side calls, Jacobians (zeros under DP5)
int knp_ode_stats(knp_ctx* c, int handle, int64_t out[4]) {
    OdeSet* S = get_set(c, handle);
    if (!S || !out) return -1;
    { const int rc_ = sync_check_ode(c); if (rc_) return rc_; }
    unsigned long long v[4];
    HIPCHK(c, host_memcpy(c, v, S->stats, sizeof(v), hipMemcpyDeviceToHost));
    for (int q = 0; q < 4; ++q) out[q] = (int64_t)v[q];
    return 0;
}

}  // extern "C"
