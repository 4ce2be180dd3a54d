// Krylov scalars (device resident, one row of KS_N doubles per system) and work-vector bundle.
#pragma once
#include "knpemi_internal.hpp"

enum { KS_RHO = 0, KS_RHO_OLD, KS_ALPHA, KS_BETA, KS_OMEGA, KS_RES, KS_RES0, KS_BNORM, KS_TOL, KS_RNORM, KS_GM_T2, KS_GM_K, KS_N = 12 };   // KS_RNORM: ||b - A x|| in the cell-volume-weighted norm (PCG)
// PCG reuses the slots only BiCGStab / GMRES write (a system runs one method at a time; every *_INIT op rewrites its slots):
//   KS_CG_XA    ||x||_A^2: x0 . A x0 of the initial guess, raised to the sum of the steps' energies  sum_j alpha_j rho_j
//   KS_CG_EST   estimate of the energy-norm error ||x - x_k||_A of the CURRENT iterate (krylov.hip: OP_CG_BETA)
//   KS_CG_SUM   sum_j alpha_j rho_j = ||x_k - x_0||_A^2 + (cross terms vanish for x0 = 0): the Hestenes-Stiefel identity
//   KS_CG_RN0   the true residual norm of the initial guess in the norm of the residual target (reported as res[0])
enum { KS_CG_XA = KS_RHO_OLD, KS_CG_EST = KS_OMEGA, KS_CG_SUM = KS_GM_T2, KS_CG_RN0 = KS_GM_K };

// restarted GMRES (gmres_solve): per system the Hessenberg matrix (column-major, leading dimension m + 1), the Givens rotations, the
// rotated right-hand side g and the solution y of the small least-squares problem live behind the Krylov scalars in knp_ctx::scal
#define KNP_GM_MAX 30
// one system's GMRES state, H | cs | sn | g | y (+ 5 doubles of padding), seen through its base pointer (krylov_gm)
struct GmLayout {
    static constexpr int M = KNP_GM_MAX, LDH = M + 1;
    static constexpr int CS = LDH * M, SN = CS + M, G = SN + M, Y = G + M + 1, SIZE = Y + M + 5;
};
template <typename T> struct GmState : GmLayout {        // T = double, or const double in the kernels that only read it
    T* base;
    __host__ __device__ explicit GmState(T* b) : base(b) {}
    __host__ __device__ T& H(int i, int j) const { return base[i + LDH * j]; }
    __host__ __device__ T* cs() const { return base + CS; }
    __host__ __device__ T* sn() const { return base + SN; }
    __host__ __device__ T* g() const { return base + G; }
    __host__ __device__ T* y() const { return base + Y; }
    // PCG: running average of log beta (scalar_op: OP_CG_BETA).  It borrows H(0, 0), free in a PCG solve
    __host__ __device__ T& cg_log_beta() const { return base[0]; }
};
#define KNP_GM_STRIDE (GmLayout::SIZE)

// knp_ctx::scal: KS_N scalars per system | reduction results, KNP_MAX_RED per system (also the all-reduce scratch of comm.hip) | GMRES state
#define KNP_RED_OFFSET (KNP_MAX_SYS * KS_N)
#define KNP_GM_OFFSET (KNP_RED_OFFSET + KNP_MAX_SYS * KNP_MAX_RED)      // doubles in front of the GMRES state in knp_ctx::scal
#define KNP_SCAL_DOUBLES (KNP_GM_OFFSET + KNP_MAX_SYS * KNP_GM_STRIDE)  // the allocation (context.hip)
static_assert(KNP_GM_STRIDE == 1056 && KNP_GM_OFFSET == KNP_MAX_SYS * (KS_N + KNP_MAX_RED) &&
              KNP_SCAL_DOUBLES == KNP_MAX_SYS * (KS_N + KNP_MAX_RED + GmLayout::SIZE), "regions of knp_ctx::scal");
template <typename T> __host__ __device__ inline T* scal_row(T* scal, int s) { return scal + s * KS_N; }
template <typename T> __host__ __device__ inline T* scal_red(T* scal) { return scal + KNP_RED_OFFSET; }
template <typename T> __host__ __device__ inline T* scal_gm(T* scal, int s) { return scal + KNP_GM_OFFSET + s * KNP_GM_STRIDE; }
// A look (krylov.hip: status_look) copies the head of the status block to knp_ctx::pinned: the status words, then the scalar rows
// of every system -- what the solve loops test and what the solves' epilogues report
#define KNP_LOOK_BYTES (KNP_STATUS_BYTES + sizeof(double) * KNP_MAX_SYS * KS_N)
static_assert(KNP_STATUS_BYTES % sizeof(double) == 0 && KNP_LOOK_BYTES <= KNP_PINNED_BYTES, "head of the status block in the pinned mirror");
inline const int* look_status(const knp_ctx* c) { return (const int*)c->pinned; }
inline const double* look_scal(const knp_ctx* c, int s = 0) { return scal_row((const double*)((const char*)c->pinned + KNP_STATUS_BYTES), s); }
inline double* krylov_scal(const knp_ctx* c, int s = 0) { return scal_row(c->scal, s); }
inline double* krylov_red(const knp_ctx* c) { return scal_red(c->scal); }
inline double* krylov_gm(const knp_ctx* c, int s) { return scal_gm(c->scal, s); }

struct KrylovVecs {
    double *x, *b, *coef;                  // unknown, rhs, operator coefficient (kappa | dnphi)
    bjreal* binv;                          // block-Jacobi inverses (fp32 storage), [nsys][nc][nd*nd]
    const uint16_t* bj_idx = nullptr;      // KNP on structured meshes: per-cell entry of the inverse-block table (instead of binv)
    const bjreal* bj_tab = nullptr;        // [entries][nsys][nd*nd]
    double *r, *z, *p, *w;                 // PCG
    double *rhat, *v, *y;                  // BiCGStab extras (t aliases w)
    double* tmp = nullptr;                 // scratch of the Chebyshev block-Jacobi smoother (BiCGStab), or null
    double bj_lmax = 0.0;                  // > 0: lambda_max(Binv A) estimate -> two-step Chebyshev block-Jacobi
    const float* ivol = nullptr;           // [nc] 1 / cell volume: weights of the residual norms (see krylov.hip: weighted norms)
    bool d8 = false;                       // BiCGStab: stop on the order-8 norms of the residual / load densities (krylov.hip) instead of ||.||_w
    double* gm_V = nullptr;                // GMRES: Krylov basis [gm_m + 1][nsys][nc*nd]
    int gm_m = 0;                          // GMRES: restart length (<= KNP_GM_MAX)
    double r_abs = 0.0;                    // PCG: > 0 -> error-controlled stop on the true residual and the energy-norm error estimate (krylov.hip: cg_converged)
};

// the stopping test of one solve, by value into the reductions' scalar recurrences (krylov_scalar.hpp); rabs: the residual target
// of PCG (KrylovVecs::r_abs) or the early-stop factor of BiCGStab (knp_ctx::knp_early), norm8: order-8 density norms (VecDims::d8)
struct StopTest {
    double rtol, atol, rabs;
    int min_it, norm8;
};

// sums over the owned cells of the load measure of the stopping tests, per species (krylov.hip: residual_measure); not all-reduced
int load_measure(knp_ctx* c, const double* b, const float* ivol, bool d8, double* out);
int pcg_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int check_every, int* niter, double* res);
int knp_bj_lambda_max(knp_ctx* c, KrylovVecs& kv, int iters, double* out, bool emi = false);
int bicgstab_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every, int* niter,
                   double* res);
// right-preconditioned restarted GMRES(m) with the same preconditioner and the same stopping test on the true residual as bicgstab_solve
// (the reference's KNP solver is PETSc GMRES(30), solver.py:684-701)
int gmres_solve(knp_ctx* c, KrylovVecs& kv, double rtol, double atol, int maxit, int min_it, int check_every, int* niter, double* res);
